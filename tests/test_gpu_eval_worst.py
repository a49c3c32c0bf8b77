"""Certified worst-case positions on the GPU (ops.eval_positions_worst,
torch.ops.acf.eval_positions_worst, evaluate.certified, the CLI's --certify_eps).

The yardstick is evaluate.worst_positions_host's float64 restatement.  A count
is an integer, but the kernel decides m_c <= thr_c in fp32, so a candidate whose
float64 f_c = m_c - thr_c is within the rounding of the fp32 chains may fall on
either side.  With
  band_c = 2^-23 ((d + 2) |p| (|q_t| + |q_c|) + (d + 4) thr_c)
(twice the first-order rounding bound of the two seq_dot chains, the difference
chain, the square root and the product) every count must satisfy
  #{f_c < -band_c} <= worst <= #{f_c <= band_c}.
The exact checks need no band: the eps = 0 row is ops.eval_positions_all with t
added to the exclusions, rows do not decrease in eps, an entry alone gets the
count it gets among others, equal calls give equal bits."""
import functools
import importlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIDES = ("user", "item")
# sigma = 0.1 tables: a candidate flips at eps of the order of sigma on either side
EPS8 = (0.0, 0.005, 0.01, 0.025, 0.05, 0.1, 0.2, 0.4)


def _ops():
    return importlib.import_module(PKG + ".ops")


def _ev():
    return importlib.import_module(PKG + ".evaluate")


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return off, flat.astype(np.int32)


def worst(P, Q, users, tests, num_cand, elists, eps, side, check=True):
    eo, ef = csr(elists) if elists is not None else (None, None)
    got = _ops().eval_positions_worst(torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV),
                                      np.array(users, np.int32), np.array(tests, np.int32), num_cand, eo, ef,
                                      eps=eps, side=side, check=check)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(eps), len(users))
    return got.cpu().numpy()


def positions_all(P, Q, users, tests, num_cand, elists):
    """ops.eval_positions_all with every entry's test item added to its exclusions."""
    elists = elists if elists is not None else [[] for _ in users]
    off, flat = csr([list(e) + [t] for e, t in zip(elists, tests)])
    return _ops().eval_positions_all(torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV),
                                     np.array(users, np.int32), np.array(tests, np.int32), num_cand, off,
                                     flat).cpu().numpy()


def bracket(P, Q, users, tests, num_cand, elists, eps, side):
    """(lo, hi) int64 [n_eps, n]: the counts every correct fp32 evaluation lies between."""
    m, base, cand = _ev().worst_margins_host(P, Q, users, tests, num_cand, elists, side)
    d = P.shape[1]
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    pn = np.linalg.norm(P64[np.asarray(users)], axis=1)
    qn = np.linalg.norm(Q64, axis=1)
    scale = pn[:, None] * (qn[np.asarray(tests)][:, None] + qn[None, :num_cand])
    lo, hi = [], []
    for e in eps:
        thr = float(e) * base
        band = 2.0 ** -23 * ((d + 2) * scale + (d + 4) * thr)
        f = m - thr
        lo.append(((f < -band) & cand).sum(axis=1))
        hi.append(((f <= band) & cand).sum(axis=1))
    return np.stack(lo), np.stack(hi)


def check_case(P, Q, users, tests, num_cand, elists, eps, side):
    """The bracket, the eps = 0 row and monotonicity of one call; returns its counts."""
    assert eps[0] == 0.0
    got = worst(P, Q, users, tests, num_cand, elists, eps, side)
    lo, hi = bracket(P, Q, users, tests, num_cand, elists, eps, side)
    print(side, "d", P.shape[1], "cand", num_cand, "bracket width mean", float((hi - lo).mean()),
          "max", int((hi - lo).max()), "outside", int(((got < lo) | (got > hi)).sum()))
    assert (lo <= got).all() and (got <= hi).all(), (got - lo, hi - got)
    np.testing.assert_array_equal(got[0], positions_all(P, Q, users, tests, num_cand, elists))
    assert (np.diff(got, axis=0) >= 0).all()
    return got


# ---- mixed entries -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_case(d):
    """13 entries (not a multiple of 8; one user twice), 1,500 candidates of 1,507 item rows, sigma =
    0.1 tables.  Exclusion lists unsorted, with repeats, -1 and ids >= num_cand; entry 2 excludes its
    own test item; entry 5's test item is an item row but no candidate; row 9 of Q is a copy of entry
    0's test item (D = 0, m = 0: it counts at every eps)."""
    rng = np.random.default_rng(900 + d)
    U1, I1, num_cand = 40, 1507, 1500
    P = (0.1 * rng.standard_normal((U1, d))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((I1, d))).astype(np.float32)
    users = rng.permutation(U1)[:13].astype(np.int32)
    users[11] = users[3]
    tests = rng.choice(np.arange(20, num_cand), 13, replace=False).astype(np.int32)
    tests[5] = 1503
    Q[9] = Q[tests[0]]
    elists = []
    for r in range(13):
        e = rng.integers(20, num_cand, 20)
        e = np.concatenate([e, e[:4], [-1, num_cand + 5, num_cand]])
        elists.append(rng.permutation(e).astype(np.int32))
    elists[2] = np.concatenate([elists[2], [tests[2]]]).astype(np.int32)
    for a in (P, Q, users, tests):
        a.setflags(write=False)
    return P, Q, users, tests, num_cand, elists


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("d", [4, 8, 64, 100])
def test_mixed_entries(d, side):
    P, Q, users, tests, num_cand, elists = mixed_case(d)
    got = check_case(P, Q, users, tests, num_cand, elists, EPS8, side)
    assert got[-1].sum() > got[0].sum()  # the eps scale is the right one: counts move
    # NULL lists: nothing but the test item is left out
    none = check_case(P, Q, users, tests, num_cand, None, EPS8[:3], side)
    assert (none >= got[:3]).all()
    # the twin of entry 0's test item counts at every eps, 0 included
    twin = worst(P, Q, users[:1], tests[:1], num_cand, [list(elists[0]) + [9]], EPS8, side)
    np.testing.assert_array_equal(got[:, 0], twin[:, 0] + 1)
    # an entry alone gets the count it gets among others (tile position and neighbours do not matter)
    for r in (0, 5, 8, 12):
        alone = worst(P, Q, users[r:r + 1], tests[r:r + 1], num_cand, elists[r:r + 1], EPS8, side)
        np.testing.assert_array_equal(alone[:, 0], got[:, r])
    # equal calls give equal bits; one eps gives the matching row of eight
    np.testing.assert_array_equal(worst(P, Q, users, tests, num_cand, elists, EPS8, side), got)
    for e in (0, 4, 7):
        np.testing.assert_array_equal(worst(P, Q, users, tests, num_cand, elists, EPS8[e:e + 1], side)[0], got[e])


def test_item_side_with_a_large_eps_counts_every_candidate():
    P, Q, users, tests, num_cand, elists = mixed_case(8)
    _, _, cand = _ev().worst_margins_host(P, Q, users, tests, num_cand, elists, "item")
    got = worst(P, Q, users, tests, num_cand, elists, (0.0, 1e6), "item")
    np.testing.assert_array_equal(got[1], cand.sum(axis=1))
    assert (got[0] <= got[1]).all() and got[0].sum() < got[1].sum()


# ---- entry-tile edges, check=False ---------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_entry_tile_edges(n, side):
    """1, 7, 8 and 9 entries around the tile of 8: each column is the 13-entry call's column, byte for
    byte, so the tile's rows past the last entry leak into no live count."""
    P, Q, users, tests, num_cand, elists = mixed_case(8)
    eps = EPS8[::2]
    got = check_case(P, Q, users[:n], tests[:n], num_cand, elists[:n], eps, side)
    full = worst(P, Q, users, tests, num_cand, elists, eps, side)
    assert got.tobytes() == np.ascontiguousarray(full[:, :n]).tobytes()


@pytest.mark.parametrize("side", SIDES)
def test_unchecked_call_on_valid_input_gives_the_checked_bits(side):
    P, Q, users, tests, num_cand, elists = mixed_case(8)
    checked = worst(P, Q, users, tests, num_cand, elists, EPS8, side, check=True)
    assert worst(P, Q, users, tests, num_cand, elists, EPS8, side, check=False).tobytes() == checked.tobytes()


# ---- window edges, strips, large d ---------------------------------------------------
@pytest.mark.parametrize("num_cand", [1, 255, 256, 257, 2049, 2053])
def test_window_edges(num_cand):
    """The edges of the 256-candidate sweep window and of the 2,048-candidate bitmap; 1 is a single
    candidate (where it is the test item nothing counts), 2,049 one candidate in a second bitmap.
    Entry 2's test item is an item row outside the range and it excludes nothing inside, so every
    candidate is swept for it, the only one at num_cand = 1 too."""
    rng = np.random.default_rng(num_cand)
    P = (0.1 * rng.standard_normal((12, 8))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((num_cand + 3, 8))).astype(np.float32)
    users = rng.permutation(12)[:9].astype(np.int32)
    tests = rng.integers(0, num_cand, 9).astype(np.int32)
    tests[0], tests[1], tests[2] = num_cand - 1, 0, num_cand + 1
    elists = [np.concatenate([rng.integers(0, num_cand, 10), [num_cand - 1, num_cand, 0, -1]]).astype(np.int32)
              for _ in users]
    elists[3] = np.zeros(0, np.int32)
    elists[2] = np.array([-1, num_cand + 1], np.int32)
    Q[0] = Q[num_cand + 1]  # a twin of entry 2's test item: candidate 0 counts for it at every eps
    for side in SIDES:
        got = check_case(P, Q, users, tests, num_cand, elists, EPS8[::2], side)
        assert (got[:, 2] >= 1).all()


def test_strips():
    """3 entries x 70,000 candidates: many strips, the partial counts and the strip sum."""
    ops = _ops()
    rng = np.random.default_rng(73)
    n_cand = 70000
    P = (0.1 * rng.standard_normal((5, 8))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((n_cand, 8))).astype(np.float32)
    users, tests = [4, 0, 2], rng.integers(0, n_cand, 3).astype(np.int32)
    elists = [np.concatenate([rng.integers(0, n_cand, 50), [-1, n_cand + 5]]).astype(np.int32) for _ in users]
    eps = (0.0, 0.01, 0.05, 0.2)
    assert ops.eval_positions_worst_workspace(3, n_cand, len(eps)) >= 16 + 2 * len(eps) * 3 * 4
    for side in SIDES:
        got = check_case(P, Q, users, tests, n_cand, elists, eps, side)
        np.testing.assert_array_equal(worst(P, Q, users, tests, n_cand, elists, eps, side), got)
        np.testing.assert_array_equal(worst(P, Q, users[1:2], tests[1:2], n_cand, elists[1:2], eps[2:3], side)[0],
                                      got[2, 1:2])


def test_large_d():
    """d = 1,024: the tile of 4 entries (9 entries: three tiles, the last with one) within the LDS budget."""
    rng = np.random.default_rng(74)
    d, n_cand = 1024, 300
    P = (0.1 * rng.standard_normal((11, d))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((n_cand + 2, d))).astype(np.float32)
    users = rng.permutation(11)[:9].astype(np.int32)
    tests = rng.integers(0, n_cand, 9).astype(np.int32)
    elists = [np.concatenate([rng.integers(0, n_cand, 12), [-1, n_cand]]).astype(np.int32) for _ in users]
    for side in SIDES:
        got = check_case(P, Q, users, tests, n_cand, elists, (0.0, 0.05, 0.2, 1.0), side)
        alone = worst(P, Q, users[8:], tests[8:], n_cand, elists[8:], (0.0, 0.05, 0.2, 1.0), side)
        np.testing.assert_array_equal(alone[:, 0], got[:, 8])


@pytest.mark.parametrize("d", [512, 516])
def test_tile_threshold(d):
    """d = 512 is the last size with 8 entries per workgroup, 516 the first with 4."""
    rng = np.random.default_rng(d)
    n_cand = 260
    P = (0.1 * rng.standard_normal((10, d))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((n_cand, d))).astype(np.float32)
    users = np.arange(9, dtype=np.int32)
    tests = rng.integers(0, n_cand, 9).astype(np.int32)
    for side in SIDES:
        check_case(P, Q, users, tests, n_cand, None, (0.0, 0.1, 0.5), side)


# ---- range check, torch op ----------------------------------------------------------
def test_range_check():
    nat = importlib.import_module(PKG + "._native")
    P, Q, users, tests, num_cand, elists = mixed_case(8)
    for bad_u, bad_t in ((40, None), (-1, None), (None, 1507), (None, -2)):
        u, t = users.copy(), tests.copy()
        if bad_u is not None:
            u[4] = bad_u
        if bad_t is not None:
            t[4] = bad_t
        with pytest.raises(nat.NativeIndexError):
            worst(P, Q, u, t, num_cand, elists, (0.0, 0.1), "user")
        got = worst(P, Q, u, t, num_cand, elists, (0.0, 0.1), "user", check=False)  # read as row 0: no error
        u[4], t[4] = (0, t[4]) if bad_u is not None else (u[4], 0)
        np.testing.assert_array_equal(got, worst(P, Q, u, t, num_cand, elists, (0.0, 0.1), "user"))


def test_torch_op():
    ops = _ops()
    tops = importlib.import_module(PKG + ".torch_ops").load()
    P, Q, users, tests, num_cand, elists = mixed_case(8)
    tP, tQ = torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV)
    tu, tt = torch.tensor(users, device=DEV), torch.tensor(tests, device=DEV)
    eo, ef = csr(elists)
    teo, tef = torch.tensor(eo, device=DEV), torch.tensor(ef, device=DEV)
    for side in SIDES:
        want = ops.eval_positions_worst(tP, tQ, tu, tt, num_cand, teo, tef, eps=EPS8, side=side)
        got = tops.eval_positions_worst(tP, tQ, tu, tt, num_cand, teo, tef, list(EPS8), side)
        assert got.dtype == torch.int32 and torch.equal(got, want)
        none = tops.eval_positions_worst(tP, tQ, tu, tt, num_cand, teo[:0], tef[:0], [0.0, 0.1], side)
        assert torch.equal(none, ops.eval_positions_worst(tP, tQ, tu, tt, num_cand, eps=(0.0, 0.1), side=side))
    assert torch.equal(tops.eval_positions_worst(tP, tQ, tu, tt, num_cand, teo, tef, [0.05]),
                       ops.eval_positions_worst(tP, tQ, tu, tt, num_cand, teo, tef, eps=(0.05,)))
    with pytest.raises(IndexError):
        tops.eval_positions_worst(tP, tQ, tu + 1000, tt, num_cand, teo, tef, [0.1], "user")
    for bad in (dict(eps=[]), dict(eps=[-0.1]), dict(eps=[float("nan")]), dict(eps=[0.1] * 9), dict(side="both")):
        with pytest.raises(RuntimeError):
            tops.eval_positions_worst(tP, tQ, tu, tt, num_cand, teo, tef, bad.get("eps", [0.1]),
                                      bad.get("side", "user"))


# ---- end to end ---------------------------------------------------------------------
def test_certified_end_to_end(acf):
    ops, ev = _ops(), _ev()
    data = importlib.import_module(PKG + ".data")
    ds = data.get_dataset("synthetic:60:200:1500")
    plan = ev.init_eval_model(ds, Namespace(eval_mode="all"))
    n = len(plan.users)
    rng = np.random.default_rng(12)
    P = torch.tensor((0.1 * rng.standard_normal((ds.num_users, 16))).astype(np.float32), device=DEV)
    Q = torch.tensor((0.1 * rng.standard_normal((ds.num_items, 16))).astype(np.float32), device=DEV)
    tables = Namespace(embedding_P=P, embedding_Q=Q)
    eps, cuts = [0.0, 0.01, 0.05, 0.2], (10, plan.K)
    (hr, ndcg, auc), _ = ev.evaluate(tables, None, ds, plan)
    off, items = ds.sorted_lists()
    tu = np.repeat(np.arange(ds.num_users), 2).astype(np.int32)
    ti = items[np.minimum(off[tu], len(items) - 1)].astype(np.int32)
    tj = rng.integers(0, ds.num_items, len(tu)).astype(np.int32)
    for side in SIDES:
        rows = ev.certified((P, Q), plan, eps, side=side, cutoffs=cuts)
        assert [(r[0], r[1], r[2]) for r in rows] == [(side, e, K) for e in eps for K in cuts]
        by = {(r[1], r[2]): np.array(r[3:]) for r in rows}
        for K in cuts:
            # eps = 0 is evaluate()
            np.testing.assert_allclose(by[(0.0, K)], [hr[K - 1], ndcg[K - 1], auc[K - 1]], rtol=0, atol=1e-12)
            # lower bounds do not increase in eps
            for a, b in zip(eps, eps[1:]):
                assert (by[(b, K)] <= by[(a, K)]).all()
        assert by[(0.2, 10)][2] < by[(0.0, 10)][2]  # the budget bites at this scale
        # one particular attack of the same budget on the same side cannot do worse than the bound
        for mode in ("random", "grad"):
            nP, nQ = ops.adv_direction(P, Q, tu, ti, tj, adv=mode, seed=3)
            for e in eps:
                Pe = ops.adv_apply(P, nP, e) if side == "user" else P
                Qe = ops.adv_apply(Q, nQ, e) if side == "item" else Q
                pos = ev.positions(Pe, Qe, plan).cpu().numpy()
                attacked = ev.metrics_from_positions(pos, plan.n_neg, plan.K).mean(axis=0)  # [3, K]
                for K in cuts:
                    assert (by[(e, K)] <= attacked[:, K - 1] + 1.0 / n).all(), (side, mode, e, K)
    # the model layers
    args = Namespace(embed_size=16, lr=0.05, reg=0.0, dns=1, adv="grad", eps=0.5, adver=0, reg_adv=1.0,
                     epochs=1, seed=11)
    m = acf.MF(ds.num_users, ds.num_items, args).build_graph(device=torch.device(DEV))
    rows = m.certified(plan, [0.0, 0.01], side="item")
    assert [r[:3] for r in rows] == [("item", 0.0, plan.K), ("item", 0.01, plan.K)]
    (hr, ndcg, auc), _ = ev.evaluate(m, None, ds, plan)
    np.testing.assert_allclose(rows[0][3:], [hr[-1], ndcg[-1], auc[-1]], rtol=0, atol=1e-12)
    assert rows == acf.APR.certified.__get__(Namespace(_ensure=lambda: None, model=m))(plan, [0.0, 0.01], side="item")
    # more eps than one call takes: chunks of 8, same rows
    many = [0.0] + [0.01 * k for k in range(1, 10)]
    got = ev.certified((P, Q), plan, many, side="user")
    assert [r[1] for r in got] == many
    assert got[9] == ev.certified((P, Q), plan, many[9:], side="user")[0]


def test_cli_writes_certified_file(acf, tmp_path, monkeypatch):
    import glob
    cli = importlib.import_module(PKG + ".cli")
    monkeypatch.chdir(tmp_path)
    rc = cli.main(["--path", str(tmp_path) + "/", "--opath", "t/", "--dataset", "synthetic:300:200:8000",
                   "--model", "bpr", "--epochs", "1", "--verbose", "1", "--embed_size", "16",
                   "--certify_eps", "0,0.01,0.1", "--certify_side", "both"])
    assert rc == 0
    files = glob.glob(str(tmp_path / "out" / "t" / "*.certified"))
    assert len(files) == 1
    rows = cli.read_certified(files[0])
    assert [(r[0], r[1], r[2]) for r in rows] == [(s, e, 100) for s in SIDES for e in (0.0, 0.01, 0.1)]
    assert all(0.0 <= v <= 1.0 for r in rows for v in r[3:])
    assert rows[0][3:] == rows[3][3:]  # eps = 0 is the same ranking on either side
    for a, b in ((0, 1), (1, 2), (3, 4), (4, 5)):
        assert all(y <= x for x, y in zip(rows[a][3:], rows[b][3:]))
