"""All-items ranking for NeuMF on the GPU (acf_neumf_rank_all) against the
pair-list path: every exact comparison is with ctx.predict on the explicit pair
list users x [0, num_candidates), ordered on the host with
np.lexsort((ids, -scores)); items, score bits and positions must be equal."""
import functools
import importlib
import re

import numpy as np
import pytest
import torch

import neumf_oracle as N
from conftest import PKG

pytestmark = pytest.mark.gpu

U1, I1, NE = 37, 1003, 53  # user rows, item rows, entries of `users`
# The kernel's constants the two-strip case relies on (acf_neumf_rank.h): strips are cut
# down to RK_STRIP_MIN = 4,096 candidates while users x strips < RK_TARGET_WG = 1,024,
# and a block is MR = 16 candidates: 53 users x 5,003 candidates -> 2 strips of 2,512
# and 2,491 candidates, the last block of the second holding 11.
I1_STRIPS = 5003


@pytest.fixture(scope="module")
def nm(acf):
    return importlib.import_module(PKG + ".neumf")


@pytest.fixture(scope="module")
def native(acf):
    return importlib.import_module(PKG + "._native")


def _params(d, items=I1, seed=0):
    P = N.init_params(U1, items, d, seed + d)
    P["Wo"] = (P["Wo"] * 20).astype(np.float32)  # scores spread over (0, 1)
    return P


def _ctx(nm, P, dev):
    st = nm.NeuMFState(P["MF_U"].shape[0], P["MF_I"].shape[0], P["MF_U"].shape[1], dev)
    st.load(P)
    return nm.NeuMFContext(st, 64)


def _inputs(nc, items=I1, seed=1):
    """53 entries (shuffled, with repeats), their exclusion lists (unsorted, repeated,
    -1 and ids >= nc; entry 3 empty; entry 5 all but 3 items) and test items, each
    test item in its own list except for entry 3."""
    rng = np.random.default_rng(seed)
    users = np.concatenate([rng.permutation(U1), rng.integers(0, U1, NE - U1)]).astype(np.int32)
    rng.shuffle(users)
    tests = rng.integers(0, items, NE).astype(np.int32)
    lists = []
    for r in range(NE):
        li = rng.integers(0, items, int(rng.integers(1, 40))).tolist()
        li += [li[0], -1, nc, nc + 5, items + 3, int(tests[r])]
        rng.shuffle(li)
        lists.append(li)
    lists[3] = []
    lists[5] = [x for x in range(items) if x not in (7, 500, nc - 1)] + [int(tests[5])]
    off = np.zeros(NE + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return users, off, np.concatenate([np.asarray(x, np.int32) for x in lists]), tests, lists


def _pair_scores(ctx, users, nc):
    """ctx.predict on the explicit pair list users x [0, nc) -> float32 [n, nc]."""
    u = np.repeat(np.asarray(users, np.int32), nc)
    i = np.tile(np.arange(nc, dtype=np.int32), len(users))
    return ctx.predict(u, i).cpu().numpy().reshape(len(users), nc)


def _expected(S, lists, nc, k, tscore=None):
    n = S.shape[0]
    items = np.full((n, max(k, 1)), -1, np.int32)
    scores = np.full((n, max(k, 1)), -np.inf, np.float32)
    pos = np.zeros(n, np.int32)
    for r in range(n):
        keep = np.ones(nc, bool)
        ex = np.asarray([x for x in lists[r] if 0 <= x < nc], np.int64)
        keep[ex] = False
        ids = np.flatnonzero(keep)
        order = ids[np.lexsort((ids, -S[r, ids]))][:k]
        items[r, :len(order)] = order
        scores[r, :len(order)] = S[r, order]
        if tscore is not None:
            pos[r] = int((S[r, ids] >= tscore[r]).sum())
    return pos, items[:, :k], scores[:, :k]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _case(nm, dev, d, nc, items=I1):
    """One model, its inputs and the pair-list reference, shared by the tests."""
    ctx = _ctx(nm, _params(d, items), dev)
    users, off, ex, tests, lists = _inputs(nc, items)
    S = _pair_scores(ctx, users, nc)
    ts = ctx.predict(users, tests).cpu().numpy()
    for a in (S, ts):
        a.setflags(write=False)
    return ctx, users, off, ex, tests, lists, S, ts


def _check(got, want, k):
    pos, items, scores = got
    wpos, witems, wscores = want
    np.testing.assert_array_equal(items.cpu().numpy(), witems)
    np.testing.assert_array_equal(_bits(scores.cpu().numpy()), _bits(wscores))
    np.testing.assert_array_equal(pos.cpu().numpy(), wpos)
    assert items.shape == (len(wpos), k) and items.dtype == torch.int32 and pos.dtype == torch.int32


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("d", [8, 32, 64, 128])
def test_parity_with_predict(nm, dev, d, k):
    ctx, users, off, ex, tests, lists, S, ts = _case(nm, dev, d, I1)
    assert 0.0 < float(S.min()) and float(S.max()) < 1.0 and float(S.std()) > 1e-3  # spread, not saturated
    got = ctx.rank_all(users, k, None, off, ex, tests)
    _check(got, _expected(S, lists, I1, k, ts), k)
    tail = got[1][5].cpu().numpy()  # entry 5 has 3 candidates (fewer if its test item is one)
    assert (tail[3:] == -1).all() and bool(torch.isinf(got[2][5][3:]).all())


def test_fewer_candidates_than_item_rows(nm, dev):
    ctx, users, off, ex, tests, lists, S, ts = _case(nm, dev, 32, 1000)
    got = ctx.rank_all(users, 10, 1000, off, ex, tests)
    _check(got, _expected(S, lists, 1000, 10, ts), 10)
    assert int(got[1].max()) < 1000


@pytest.mark.parametrize("d,k", [(64, 10), (8, 128)])
def test_more_than_one_strip(nm, dev, d, k):
    ws = nm.rank_all_workspace(NE, I1_STRIPS, k)
    assert NE * 2 * k * 8 <= ws < NE * 3 * k * 8  # two partial lists per user
    ctx, users, off, ex, tests, lists, S, ts = _case(nm, dev, d, I1_STRIPS, I1_STRIPS)
    got = ctx.rank_all(users, k, None, off, ex, tests)
    _check(got, _expected(S, lists, I1_STRIPS, k, ts), k)
    assert int((got[1] >= 2512).sum()) > 0 and int((got[1] < 2512).sum()) > 0  # both strips contribute


def _permuted(nm, dev, d, order):
    P = _params(d)
    P["MF_I"], P["MLP_I"] = P["MF_I"][order].copy(), P["MLP_I"][order].copy()
    return _ctx(nm, P, dev)


def test_selection_under_pressure(nm, dev):
    """Scores rising with the id: every candidate beats the threshold and is
    appended (the most prunes); the reversed table gives the same scores."""
    d, u0 = 64, np.array([11], np.int32)
    base = _pair_scores(_ctx(nm, _params(d), dev), u0, I1)[0]
    order = np.argsort(base, kind="stable")
    up, down = _permuted(nm, dev, d, order), _permuted(nm, dev, d, order[::-1].copy())
    S = _pair_scores(up, u0, I1)
    assert (np.diff(S[0]) >= 0).all()
    got = up.rank_all(u0, 128, test_items=np.array([0], np.int32))
    _check(got, _expected(S, [[]], I1, 128, S[:, 0]), 128)
    assert int(got[0][0]) == I1
    rev = down.rank_all(u0, 128)
    np.testing.assert_array_equal(_bits(rev[2].cpu().numpy()), _bits(got[2].cpu().numpy()))
    _check((got[0], rev[1], rev[2]), _expected(_pair_scores(down, u0, I1), [[]], I1, 128, S[:, 0]), 128)


def test_ties_go_to_the_lower_id(nm, dev):
    d, u0 = 32, np.array([4], np.int32)
    P = _params(d)
    best = int(np.argmax(_pair_scores(_ctx(nm, P, dev), u0, I1)[0]))
    pool = np.setdiff1d(np.arange(I1), [best])
    ids = np.sort(np.r_[best, np.random.default_rng(5).choice(pool, 39, replace=False)])
    P["MF_I"][ids], P["MLP_I"][ids] = P["MF_I"][best], P["MLP_I"][best]
    ctx = _ctx(nm, P, dev)
    S = _pair_scores(ctx, u0, I1)
    t = int(ids[17])
    pos, items, scores = ctx.rank_all(u0, 128, None, np.array([0, 1]), np.array([t], np.int32), np.array([t], np.int32))
    others = ids[ids != t]
    np.testing.assert_array_equal(items[0, :39].cpu().numpy(), others)
    assert len(set(_bits(scores[0, :39].cpu().numpy()).tolist())) == 1
    assert int(pos[0]) == 39
    _check((pos, items, scores), _expected(S, [[t]], I1, 128, S[:, t]), 128)


def test_saturated_scores(nm, dev):
    P = _params(16)
    P["bo"][:] = 40.0
    ctx = _ctx(nm, P, dev)
    users, off, ex, tests, lists = _inputs(I1)
    S = _pair_scores(ctx, users, I1)
    assert (S == 1.0).all()
    pos, items, scores = ctx.rank_all(users, 10, None, off, ex, tests)
    want = _expected(S, lists, I1, 10, np.ones(NE, np.float32))
    _check((pos, items, scores), want, 10)
    for r in range(NE):
        cand = sorted(set(range(I1)) - set(lists[r]))
        assert items[r].cpu().tolist() == (cand[:10] + [-1] * 10)[:10] and int(pos[r]) == len(cand)


def test_deterministic_and_independent_of_the_other_users(nm, dev):
    ctx, users, off, ex, tests, lists, S, ts = _case(nm, dev, 64, I1)
    a = ctx.rank_all(users, 10, None, off, ex, tests)
    b = ctx.rank_all(users, 10, None, off, ex, tests)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for r in (0, 3, 5, 17, 52):
        li = np.asarray(lists[r], np.int32)
        one = ctx.rank_all(users[r:r + 1], 10, None, np.array([0, len(li)]), li, tests[r:r + 1])
        assert int(one[0][0]) == int(a[0][r]) and torch.equal(one[1][0], a[1][r])
        np.testing.assert_array_equal(_bits(one[2][0].cpu().numpy()), _bits(a[2][r].cpu().numpy()))
    # lists only and positions only agree with the combined call
    assert torch.equal(ctx.rank_all(users, 10, None, off, ex)[1], a[1])
    only = ctx.rank_all(users, 0, None, off, ex, tests)
    assert only[1] is None and only[2] is None and torch.equal(only[0], a[0])
    # no exclusion arguments: nothing is excluded
    free = ctx.rank_all(users, 10)
    _check((a[0], free[1], free[2]), (a[0].cpu().numpy(), *_expected(S, [[]] * NE, I1, 10)[1:]), 10)


@pytest.mark.parametrize("d", [8, 64, 128])
def test_scores_match_the_oracle(nm, dev, d):
    """Independent of predict: the CPU oracle's forward, at test_predict_matches_oracle's bar."""
    k = 10
    ctx, users, off, ex, tests, lists, S, ts = _case(nm, dev, d, I1)
    P = _params(d)
    _, items, scores = ctx.rank_all(users, k, None, off, ex, tests)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    for r in range(NE):
        want = N.predict(P, np.full(I1, users[r]), np.arange(I1)).reshape(-1)
        real = items[r] >= 0
        np.testing.assert_allclose(scores[r][real], want[items[r][real]], rtol=1e-5, atol=1e-7)
        cand = np.setdiff1d(np.arange(I1), [x for x in lists[r] if 0 <= x < I1])
        kth = np.sort(want[cand])[::-1][:k][-1]
        assert (want[items[r][real]] >= kth - 1e-6).all()
        assert set(items[r][real].tolist()) <= set(cand.tolist()) and real.sum() == min(k, len(cand))


def test_errors(nm, native, dev):
    ctx, users, off, ex, tests, lists, S, ts = _case(nm, dev, 8, I1)
    bad = users.copy()
    bad[9] = U1
    with pytest.raises(native.NativeIndexError, match="user"):
        ctx.rank_all(bad, 5, None, off, ex, tests)
    with pytest.raises(native.NativeIndexError, match="user"):
        ctx.rank_all(bad, 5)
    t = tests.copy()
    t[2] = -1
    with pytest.raises(native.NativeIndexError, match="item"):
        ctx.rank_all(users, 0, None, off, ex, t)
    s = ctx.state
    nbytes = nm.rank_all_workspace(NE, I1, 5)
    work = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    u = torch.as_tensor(users, device=dev)
    items = torch.empty((NE, 5), dtype=torch.int32, device=dev)
    scores = torch.empty((NE, 5), dtype=torch.float32, device=dev)
    args = [ctx._ptr, s.params.data_ptr(), u.data_ptr(), NE, I1, 0, 0, 0, 0, 5, items.data_ptr(),
            scores.data_ptr(), work.data_ptr()]
    with pytest.raises(native.NativeError, match="workspace") as e:
        native.call_neumf("acf_neumf_rank_all", *args, nbytes - 1, 0)
    assert e.value.code == 1
    for k, it, sc in ((0, 0, 0), (5, items.data_ptr(), 0)):  # nothing to compute; half an output
        with pytest.raises(native.NativeError) as e:
            native.call_neumf("acf_neumf_rank_all", *args[:9], k, it, sc, work.data_ptr(), nbytes, 0)
        assert e.value.code == 1
    native.call_neumf("acf_neumf_rank_all", *args, nbytes, 0)  # the context is usable after the errors
    torch.cuda.synchronize()
    assert torch.equal(items, ctx.rank_all(users, 5)[1])


@pytest.fixture(scope="module")
def run_ds(acf):
    rc = importlib.import_module(PKG + ".run_cli")
    return rc, rc.get_dataset("synthetic:40:300:2000", "", "all")


def test_evaluation_protocol(nm, acf, dev, run_ds):
    rc, ds = run_ds
    ev = importlib.import_module(PKG + ".evaluation")
    m = nm.NeuMF(ds.num_users, ds.num_items, 8, seed=0, device=dev)
    m.state.view("Wo").mul_(20.0)
    train = ds.trainMatrix
    for epoch in range(2):
        want = ev.evaluate_model(m, ds.testRatings, ds.testNegatives, 100)
        got = ev.evaluate_model_all(m, ds.testRatings, train, 100)
        assert got[0] == want[0] and got[1] == want[1] and len(got[0]) == ds.num_users - 1
        assert 0 < sum(got[0]) < len(got[0])  # neither all hits nor none: the ranks matter
        if epoch == 0:
            x, y = m.get_train_instances(train)
            m.train(x, y, 256)
    users = np.arange(1, ds.num_users)
    items, scores = m.recommend(users, 10, train)
    assert items.shape == (len(users), 10) and (items > 0).all()
    for u, row in zip(users.tolist(), items.tolist()):
        assert not set(row) & set(ds.trainSeq.get(u, []))
    np.testing.assert_array_equal(_bits(scores), _bits(m.rank(np.repeat(users, 10), items.reshape(-1)).reshape(-1, 10)))
    free, _ = m.recommend(users, 10)  # no train: nothing excluded
    assert free.shape == items.shape and (free >= 0).all()


def test_driver_writes_topk_and_evaluates_on_the_gpu(nm, dev, run_ds, tmp_path, monkeypatch):
    rc, ds = run_ds
    cli = importlib.import_module(PKG + ".cli")
    ev = importlib.import_module(PKG + ".evaluation")
    called = []
    real = ev.evaluate_model_all
    monkeypatch.setattr(ev, "evaluate_model_all", lambda *a: (called.append(1), real(*a))[1])
    path = str(tmp_path) + "/"
    res = rc.main(["--model", "neumf", "--data", "synthetic:40:300:2000", "--d", "8", "--epochs", "1", "--eval", "all",
                   "--topk", "5", "--path", path, "--opath", "t/", "--save_model", "0", "--bs", "256"], device=dev)
    assert len(called) == 2  # Init and the epoch: no pair list was scored
    topk = cli.read_topk(res["topk"])
    assert topk.shape == (ds.num_users - 1, 5) and (topk > 0).all()  # users 1 .. uNum - 1
    for u, row in enumerate(topk.tolist(), start=1):
        assert not set(row) & set(ds.trainSeq.get(u, []))
    text = open(path + "out/t/" + res["runName"] + ".out").read()
    init = re.search(r"Init: HR = ([0-9.]+), NDCG = ([0-9.]+)", text)
    m = nm.NeuMF(ds.num_users, ds.num_items, 8, seed=0, device=dev)
    hits, ndcgs = ev.evaluate_model(m, ds.testRatings, ds.testNegatives, 100)
    assert init.group(1) == "%f" % np.array(hits).mean() and init.group(2) == "%f" % np.array(ndcgs).mean()
