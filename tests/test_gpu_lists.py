"""List-level robustness on the GPU: ops.list_compare, ops.list_exposure and
ops.exposure_metrics against the numpy yardstick (tests/lists_ref.py), then
evaluate.list_robustness, evaluate.exposure and the CLI's .lists file end to end.

Bars.  overlap, jaccard, n_scored, the counts and total / coverage / gini / arp /
aplt are integers or one fp64 division of integers: compared with ==.  rbo and the
means: 1e-12 (at most 128 terms, each with <= d + 3 roundings, plus the sum: below
260 * 2^-53 ~ 3e-14 of a value <= 1).  entropy: (N + 64) * 2^-52 * max(ref, 1), the
summation bound for N positive terms plus a few ulps per log2."""
import glob
import importlib
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lists_ref

pytestmark = pytest.mark.gpu
PKG = "adversarial-collaborative-filtering_amd"


def _T(x, dev):
    return torch.tensor(np.ascontiguousarray(x), device=dev)


def _pairs(n, k, seed):
    """n pairs of lists of length k: the special rows first (cycled when n is small), random ones after."""
    rng = np.random.default_rng(seed)
    pool = 2 * k + 3

    def perm():
        return rng.permutation(pool)[:k].astype(np.int32)

    def cut(x, m):  # a -1 tail from position m
        x = x.copy()
        x[m:] = -1
        return x

    base = perm()
    swap = base.copy()
    if k > 1:
        swap[[0, 1]] = swap[[1, 0]]
    none = np.full(k, -1, np.int32)
    special = [(base, base.copy()), (base, base + pool), (base, base[::-1].copy()), (base, swap),
               (cut(base, k // 2), cut(perm(), k - k // 3)), (cut(perm(), 1), base), (none, base), (base, none),
               (none, none), (cut(base, k // 3), cut(base[::-1].copy(), k // 2))]
    rows = [special[(r + seed) % len(special)] if r < len(special) else (perm(), cut(perm(), int(rng.integers(0, k + 1))))
            for r in range(n)]
    return np.stack([a for a, _ in rows]), np.stack([b for _, b in rows])


@pytest.mark.parametrize("p", [0.5, 0.9, 0.98])
@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("k", [1, 7, 64, 65, 128])
def test_compare_matches_the_yardstick(ops, dev, k, n, p):
    cuts = tuple(sorted({1, (k + 1) // 2, k}))
    worst = 0.0
    for seed in (range(10) if n == 1 else (k + n,)):  # a single row: every special row in turn
        A, B = _pairs(n, k, seed)
        got = ops.list_compare(_T(A, dev), _T(B, dev), cuts, p)
        again = ops.list_compare(_T(A, dev), _T(B, dev), cuts, p)
        want_pu, want_mean, want_ns = lists_ref.compare(A, B, cuts, p)
        pu = got.per_user.cpu().numpy()
        assert got.cutoffs == cuts and pu.shape == (n, len(cuts), 3)
        assert np.array_equal(pu[:, :, 0], want_pu[:, :, 0]), "overlap"
        assert np.array_equal(pu[:, :, 1], want_pu[:, :, 1]), "jaccard"
        assert np.array_equal(got.n_scored.cpu().numpy(), want_ns)
        err = max(float(np.abs(pu[:, :, 2] - want_pu[:, :, 2]).max()),
                  float(np.abs(got.mean.cpu().numpy() - want_mean).max()))
        worst = max(worst, err)
        assert err <= 1e-12, err
        for a, b in ((got.per_user, again.per_user), (got.mean, again.mean), (got.n_scored, again.n_scored)):
            assert torch.equal(a, b)
    print(f"k={k} n={n} p={p}: max |rbo, mean - ref| = {worst:.3e}")


def test_compare_of_no_rows_and_unscored_rows(ops, dev):
    empty = torch.zeros((0, 9), dtype=torch.int32, device=dev)
    got = ops.list_compare(empty, empty, (1, 9))
    assert got.per_user.shape == (0, 2, 3) and not got.mean.any() and not got.n_scored.any()
    none = torch.full((3, 9), -1, dtype=torch.int32, device=dev)
    got = ops.list_compare(none, none, (1, 9))
    assert not got.per_user.any() and not got.mean.any() and got.n_scored.tolist() == [0, 0]


def _exposure_lists(n, k, num_items, seed):
    rng = np.random.default_rng(seed)
    lists = rng.integers(0, num_items + max(2, num_items // 8), (n, k)).astype(np.int32)  # some ids >= num_items
    for r in range(0, n, 3):
        lists[r, int(rng.integers(0, k + 1)):] = -1
    return lists


@pytest.mark.parametrize("num_items", [1, 63, 1000])
@pytest.mark.parametrize("n,k", [(1, 1), (5, 7), (257, 65), (130, 128)])
def test_exposure_counts_match_bincount(ops, dev, num_items, n, k):
    lists = _exposure_lists(n, k, num_items, n + k + num_items)
    cuts = tuple(sorted({1, (k + 1) // 2, k}))  # nested, checked together
    counts = ops.list_exposure(_T(lists, dev), num_items, cuts)
    assert counts.dtype == torch.int32 and counts.shape == (len(cuts), num_items)
    assert np.array_equal(counts.cpu().numpy(), lists_ref.exposure_counts(lists, num_items, cuts))


def test_exposure_when_every_user_holds_the_same_list(ops, dev):
    row = np.random.default_rng(3).permutation(63)[:40].astype(np.int32)
    lists = np.repeat(row[None, :], 257, axis=0)
    counts = ops.list_exposure(_T(lists, dev), 63, (1, 10, 40)).cpu().numpy()
    assert np.array_equal(counts, lists_ref.exposure_counts(lists, 63, (1, 10, 40)))
    assert set(counts[2].tolist()) == {0, 257} and counts[2].sum() == 257 * 40 and counts[0].max() == 257
    assert not ops.list_exposure(torch.zeros((0, 5), dtype=torch.int32, device=dev), 63, (5,)).any()


def _metric_cases():
    rng = np.random.default_rng(11)
    one = np.zeros(63, np.int64)
    one[17] = 5000
    return {
        "all zero": np.zeros((1, 63), np.int64),
        "one item holds everything": one[None, :],
        "uniform": np.full((1, 1000), 257, np.int64),
        "N = 1": np.array([[9]], np.int64),
        "N = 1, zero": np.array([[0]], np.int64),
        "random, N = 1000, three cutoffs": np.stack([rng.integers(0, 40, 1000) * (rng.random(1000) < f)
                                                     for f in (0.1, 0.5, 1.0)]).astype(np.int64),
        "random, N = 63": rng.integers(0, 1 << 20, (2, 63)),
    }


@pytest.mark.parametrize("name", list(_metric_cases()))
@pytest.mark.parametrize("with_pop", [True, False])
def test_exposure_metrics_match_the_yardstick(ops, dev, name, with_pop):
    counts = _metric_cases()[name]
    N = counts.shape[1]
    rng = np.random.default_rng(N)
    pop = rng.integers(0, 5000, N).astype(np.int32) if with_pop else None
    tail = (rng.random(N) < 0.8) if with_pop else None
    got = ops.exposure_metrics(_T(counts.astype(np.int32), dev), None if pop is None else _T(pop, dev),
                               None if tail is None else _T(tail.astype(np.uint8), dev))
    again = ops.exposure_metrics(_T(counts.astype(np.int32), dev), None if pop is None else _T(pop, dev),
                                 None if tail is None else _T(tail, dev))  # a bool tail is taken as well
    assert torch.equal(got, again)
    got = got.cpu().numpy()
    want = lists_ref.exposure_metrics(counts, pop, tail)
    assert got.shape == want.shape == (counts.shape[0], len(ops.EXPOSURE_METRICS))
    for m, col in enumerate(ops.EXPOSURE_METRICS):
        if col == "entropy":
            bar = (N + 64) * 2.0 ** -52 * np.maximum(want[:, m], 1.0)
            print(f"{name}: max |entropy - ref| = {np.abs(got[:, m] - want[:, m]).max():.3e} (bar {bar.min():.3e})")
            assert (np.abs(got[:, m] - want[:, m]) <= bar).all(), (got[:, m], want[:, m])
        else:
            assert np.array_equal(got[:, m], want[:, m]), (col, got[:, m], want[:, m])
    if not with_pop:
        assert not got[:, 4:].any()
    if name.startswith("all zero") or name == "N = 1, zero":
        assert not got.any()


# ---- end to end: a small MF, one epoch's triplets ---------------------------------------------------
U, I, D, K = 120, 200, 8, 20
CUTS = (1, 10, 20)
EPS_LIST = [0.0, 0.3]


@pytest.fixture(scope="module")
def world(acf, dev):
    """(model, dataset, triplets, list_robustness' rows): computed once, shared, left unchanged."""
    data = importlib.import_module(PKG + ".data")
    ds = data.synthetic_dataset(U, I, 3000, seed=5)
    args = SimpleNamespace(embed_size=D, lr=0.05, reg=0.0, dns=1, adv="grad", eps=0.5, adver=1, reg_adv=1.0, epochs=0,
                           seed=3)
    m = acf.MF(U, I, args).build_graph(device=dev)
    rng = np.random.default_rng(2)
    m.load_embeddings((rng.standard_normal((U + 1, D)) * 0.3).astype(np.float32),
                      (rng.standard_normal((I + 1, D)) * 0.3).astype(np.float32))
    u = rng.integers(0, U, 512).astype(np.int32)
    i = rng.integers(0, I, 512).astype(np.int32)
    j = rng.integers(0, I, 512).astype(np.int32)
    ep = acf.EpochTriplets(_T(u, dev), _T(i, dev), _T(j, dev), 64)
    keep = [t.clone() for t in (m.embedding_P, m.embedding_Q, m.delta_P, m.delta_Q)]
    rows = m.list_robustness(ds, ep, EPS_LIST, k=K, cutoffs=CUTS, modes=("grad", "random", "pgd"), p=0.9, seed=4,
                             iters=3)
    assert all(torch.equal(a, b) for a, b in zip(keep, (m.embedding_P, m.embedding_Q, m.delta_P, m.delta_Q)))
    return m, ds, ep, rows


def _close_rows(got, want):
    """rows (mode, eps, cutoff, jaccard, rbo, overlap, coverage, gini, entropy, arp, aplt) within the bars"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:3] == w[:3], (g, w)
        for col, (a, b) in enumerate(zip(g[3:], w[3:])):
            bar = 1e-12 if col < 3 else (I + 64) * 2.0 ** -52 * max(b, 1.0) if col == 5 else 0.0
            assert abs(a - b) <= bar, (g[:3], col, a, b)


def test_list_robustness_matches_the_rows_composed_by_hand(ops, dev, world):
    ev = importlib.import_module(PKG + ".evaluate")
    m, ds, ep, rows = world
    P, Q = m.embedding_P, m.embedding_Q
    users = np.arange(U, dtype=np.int32)
    off, ex = ev.train_exclusions(ds, users)
    pop, tail = ev.item_popularity(ds)

    def lists_of(Pa, Qa):
        return ops.recommend_topk(Pa, Qa, users, K, I, off, ex)[0].cpu().numpy()

    def rows_of(mode, eps, clean, lists):
        _, mean, _ = lists_ref.compare(clean, lists, CUTS, 0.9)
        expo = lists_ref.exposure_metrics(lists_ref.exposure_counts(lists, I, CUTS), pop, tail)
        return [(mode, eps, c, mean[x, 1], mean[x, 2], mean[x, 0], *expo[x, 1:]) for x, c in enumerate(CUTS)]

    clean = lists_of(P, Q)
    assert (clean >= 0).all()
    want = [(*r[:3], 1.0, 1.0, *r[5:]) for r in rows_of("clean", 0.0, clean, clean)]
    for mode in ("grad", "random"):
        nP, nQ = ops.adv_direction(P, Q, ep.user, ep.item_pos, ep.item_neg, adv=mode, seed=4, call=1, t=0)
        for eps in EPS_LIST:
            want += rows_of(mode, eps, clean, lists_of(ops.adv_apply(P, nP, eps), ops.adv_apply(Q, nQ, eps)))
    for eps in EPS_LIST:
        Pa, Qa = P, Q
        if eps > 0:
            dP, dQ, _ = ops.adv_pgd(P, Q, ep.user, ep.item_pos, ep.item_neg, eps, iters=3)
            Pa, Qa = ops.adv_apply(P, dP, 1.0), ops.adv_apply(Q, dQ, 1.0)
        want += rows_of("pgd", eps, clean, lists_of(Pa, Qa))
    _close_rows(rows, want)
    assert [(r[0], r[1]) for r in rows[::3]] == [("clean", 0.0)] + [(mo, e) for mo in ("grad", "random", "pgd")
                                                                   for e in EPS_LIST]
    # the clean rows: a list against itself, full lists
    for r, c in zip(rows[:3], CUTS):
        assert r[:6] == ("clean", 0.0, c, 1.0, 1.0, float(c))
    # eps = 0 moves nothing: every mode's eps = 0 rows are the clean rows
    for start in (3, 9, 15):
        _close_rows([("clean", *r[1:]) for r in rows[start:start + 3]], rows[:3])
    # the attack at eps = 0.3 does move the lists
    assert all(r[3] < 1.0 for r in rows[6:9]) and rows[8][5] < 20.0


def test_robustness_is_what_it_was_before_the_shared_loop(ops, dev, world):
    ev = importlib.import_module(PKG + ".evaluate")
    m, ds, ep, _ = world
    P, Q = m.embedding_P, m.embedding_Q
    plan = ev.init_eval_model(ds, SimpleNamespace(eval_mode="all"))
    rows = m.robustness(ds, plan, ep, EPS_LIST, modes=("grad", "random", "pgd"), seed=4, iters=3)

    def row(mode, eps, Pa, Qa):
        raw = ev.metrics_from_positions(ev.positions(Pa, Qa, plan).cpu().numpy(), plan.n_neg, plan.K)
        return (mode, eps, *raw.mean(axis=0)[:, -1].tolist())

    want = []
    for mode in ("grad", "random"):
        nP, nQ = ops.adv_direction(P, Q, ep.user, ep.item_pos, ep.item_neg, adv=mode, seed=4, call=1, t=0)
        want += [row(mode, eps, ops.adv_apply(P, nP, eps), ops.adv_apply(Q, nQ, eps)) for eps in EPS_LIST]
    for eps in EPS_LIST:
        Pa, Qa = P, Q
        if eps > 0:
            dP, dQ, _ = ops.adv_pgd(P, Q, ep.user, ep.item_pos, ep.item_neg, eps, iters=3)
            Pa, Qa = ops.adv_apply(P, dP, 1.0), ops.adv_apply(Q, dQ, 1.0)
        want.append(row("pgd", eps, Pa, Qa))
    assert rows == want
    (hr, ndcg, auc), _ = ev.evaluate(m, None, ds, plan, 0)
    assert rows[0][2:] == (hr[-1], ndcg[-1], auc[-1])


def test_exposure_matches_the_yardstick_on_recommends_lists(world):
    ev = importlib.import_module(PKG + ".evaluate")
    m, ds, _, _ = world
    pop, tail = ev.item_popularity(ds)
    for users, excl in ((None, True), (np.array([5, 3, 3, 119]), False)):
        rows = m.exposure(ds, users=users, k=K, cutoffs=(10, 20), exclude_train=excl)
        items, _ = ev.recommend(m, ds, users=users, k=K, exclude_train=excl)
        want = lists_ref.exposure_metrics(lists_ref.exposure_counts(items, I, (10, 20)), pop, tail)
        assert [r[0] for r in rows] == [10, 20]
        for r, w in zip(rows, want):
            for col, (a, b) in enumerate(zip(r[1:], w)):
                bar = (I + 64) * 2.0 ** -52 * max(b, 1.0) if col == 3 else 0.0
                assert abs(a - b) <= bar, (col, a, b)
        assert rows[1][1] == float(len(items) * K)


def test_cli_writes_lists_file(acf, tmp_path, monkeypatch):
    cli = importlib.import_module(PKG + ".cli")
    ev = importlib.import_module(PKG + ".evaluate")
    calls = []
    inner = ev.list_robustness

    def spy(*a, **kw):
        rows = inner(*a, **kw)
        calls.append((a, kw, rows))
        return rows
    monkeypatch.setattr(ev, "list_robustness", spy)
    monkeypatch.chdir(tmp_path)
    common = ["--path", str(tmp_path) + "/", "--dataset", "synthetic:300:200:8000", "--model", "apr", "--epochs", "1",
              "--adv_epoch", "1", "--verbose", "1", "--embed_size", "8", "--eval_mode", "all"]
    rc = cli.main(common + ["--opath", "t/", "--robust_eps", "0,0.5", "--robust_lists", "1,10", "--robust_iters", "2"])
    assert rc == 0 and len(calls) == 1
    files = glob.glob(str(tmp_path / "out" / "t" / "*.lists"))
    assert len(files) == 1 and len(glob.glob(str(tmp_path / "out" / "t" / "*.robust"))) == 1
    rows = cli.read_lists(files[0])
    a, kw, want = calls[0]
    assert rows == [tuple(r) for r in want] and kw["k"] == 10 and kw["cutoffs"] == [1, 10]
    assert rows == inner(*a, **kw)  # the same model, the same bits
    assert [(r[0], r[1], r[2]) for r in rows] == [(mo, e, c) for mo, es in (("clean", (0.0,)), ("grad", (0.0, 0.5)),
                                                                          ("random", (0.0, 0.5)), ("pgd", (0.0, 0.5)))
                                                  for e in es for c in (1, 10)]
    assert all(math.isfinite(x) for r in rows for x in r[3:])


def test_cli_robust_lists_needs_robust_eps(acf, tmp_path, monkeypatch, capsys):
    cli = importlib.import_module(PKG + ".cli")
    monkeypatch.chdir(tmp_path)
    rc = cli.main(["--path", str(tmp_path) + "/", "--opath", "u/", "--dataset", "synthetic:300:200:8000", "--model", "bpr",
                   "--epochs", "1", "--verbose", "1", "--embed_size", "8", "--robust_lists", "1,10"])
    assert rc == 0 and "--robust_lists" in capsys.readouterr().err
    assert not glob.glob(str(tmp_path / "out" / "u" / "*.lists"))
