"""Evaluation against several held-out items per user on the GPU
(ops.eval_positions_multi, ops.rank_metrics, evaluate.evaluate_multi).

Positions are integers, so every comparison of positions is exact equality.  The
yardstick is the existing ops.eval_positions_all with every entry repeated once
per test item and that item added to the entry's exclusions.  The device metrics
are held to evaluate.metrics_from_positions_multi (numpy, fp64) within rtol 1e-9:
both are fp64 sums of at most a few thousand terms in [0, 1], so their rounding
stays below 1e-12, while one changed position moves a metric by more than 1e-6 at
these sizes (asserted below)."""
import functools
import importlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUTS = (1, 5, 10, 100, 1024)


def _ops():
    return importlib.import_module(PKG + ".ops")


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return off, flat.astype(np.int32)


def yardstick(P, Q, users, tlists, num_cand, elists):
    """eval_positions_all on one entry per (entry, test item), exclusions = the entry's list + [t]."""
    ru, rt, rex = [], [], []
    for u, tl, el in zip(users, tlists, elists):
        for t in tl:
            ru.append(u)
            rt.append(t)
            rex.append(list(el) + [t])
    if not ru:
        return np.zeros(0, np.int32)
    off, flat = csr(rex)
    pos = _ops().eval_positions_all(torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV),
                                    np.asarray(ru, np.int32), np.asarray(rt, np.int32), num_cand, off, flat)
    return pos.cpu().numpy()


def multi(P, Q, users, tlists, num_cand, elists=None, check=True):
    to, tf = csr(tlists)
    eo, ef = csr(elists) if elists is not None else (None, None)
    pos = _ops().eval_positions_multi(torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV),
                                      np.asarray(users, np.int32), to, tf, num_cand, eo, ef, check=check)
    assert pos.dtype == torch.int32 and tuple(pos.shape) == (len(tf),)
    return pos.cpu().numpy()


# ---- the small grid ---------------------------------------------------------------
GRID_LENS = (0, 1, 2, 7, 300, 1, 2, 7, 0, 3, 5, 2, 1)  # 300 = one LDS chunk (256) + 44


@functools.lru_cache(maxsize=None)
def grid_case(d):
    """13 entries (not a multiple of 8; one user twice), 1,000 candidates of 1,010 item rows (not a
    multiple of 256), sigma = 0.1 tables; exclusion lists unsorted, with repeats, -1 and num_cand + 5."""
    rng = np.random.default_rng(700 + d)
    U1, I1, num_cand = 40, 1010, 1000
    P = (0.1 * rng.standard_normal((U1, d))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((I1, d))).astype(np.float32)
    users = rng.permutation(U1)[:13].astype(np.int32)
    users[11] = users[3]
    tlists = [rng.choice(num_cand, m, replace=False).astype(np.int32) for m in GRID_LENS]
    tlists[5][0] = 1004  # a test item that is an item row but no candidate
    elists = []
    for _ in users:
        e = rng.integers(0, num_cand, 20)
        e = np.concatenate([e, e[:4], [-1, num_cand + 5]])
        elists.append(rng.permutation(e).astype(np.int32))
    want = yardstick(P, Q, users, tlists, num_cand, elists)
    want.setflags(write=False)
    return P, Q, users, tlists, num_cand, elists, want


@pytest.mark.parametrize("d", [8, 64, 132])
def test_small_grid(d):
    P, Q, users, tlists, num_cand, elists, want = grid_case(d)
    got = multi(P, Q, users, tlists, num_cand, elists)
    np.testing.assert_array_equal(got, want)
    assert len(got) == sum(GRID_LENS)
    # without exclusions too (NULL lists)
    np.testing.assert_array_equal(multi(P, Q, users, tlists, num_cand),
                                  yardstick(P, Q, users, tlists, num_cand, [[] for _ in users]))


@functools.lru_cache(maxsize=None)
def long_case():
    """One user with 1,500 test items over 2,000 candidates, d = 8: six chunks, the metrics' any-m path."""
    rng = np.random.default_rng(71)
    P = (0.1 * rng.standard_normal((3, 8))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((2000, 8))).astype(np.float32)
    tlists = [rng.choice(2000, 1500, replace=False).astype(np.int32)]
    elists = [rng.integers(0, 2000, 30).astype(np.int32)]
    want = yardstick(P, Q, [2], tlists, 2000, elists)
    want.setflags(write=False)
    return P, Q, tlists, elists, want


def test_one_long_list():
    P, Q, tlists, elists, want = long_case()
    np.testing.assert_array_equal(multi(P, Q, [2], tlists, 2000, elists), want)


def test_strips():
    ops = _ops()
    rng = np.random.default_rng(72)
    n_cand = 70000
    P = (0.1 * rng.standard_normal((5, 8))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((n_cand, 8))).astype(np.float32)
    users = [4, 0, 2]
    tlists = [rng.choice(n_cand, 5, replace=False).astype(np.int32) for _ in users]
    elists = [np.concatenate([rng.integers(0, n_cand, 50), [-1, n_cand + 5]]).astype(np.int32) for _ in users]
    # more than one strip: the workspace holds more than the flag and one strip's 15 counts
    assert ops.eval_positions_multi_workspace(3, 15, n_cand) >= 16 + 2 * 15 * 4
    np.testing.assert_array_equal(multi(P, Q, users, tlists, n_cand, elists),
                                  yardstick(P, Q, users, tlists, n_cand, elists))


def test_ties_on_equal_bits():
    rng = np.random.default_rng(73)
    P = (0.1 * rng.standard_normal((4, 16))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((600, 16))).astype(np.float32)
    Q[50:60] = Q[10]    # ten more candidates with item 10's bits
    Q[300:303] = Q[200]
    users = [1, 3]
    tlists = [np.array([10, 55, 200, 7], np.int32), np.array([301, 10, 9], np.int32)]
    elists = [np.array([52, 400], np.int32), np.array([], np.int32)]
    got = multi(P, Q, users, tlists, 600, elists)
    np.testing.assert_array_equal(got, yardstick(P, Q, users, tlists, 600, elists))
    # items 10 and 55 tie: each sees the other and the 8 remaining copies (52 is excluded), and the same rest
    assert got[0] == got[1] and got[0] >= 9


def test_test_item_excluded_and_repeated():
    P, Q, users, _, num_cand, elists, _ = grid_case(8)
    users, elists = users[:3], [e.copy() for e in elists[:3]]
    tlists = [np.array([5, 9, 5, 700, 5], np.int32), np.array([int(elists[1][0]), 3], np.int32),
              np.array([11], np.int32)]
    elists[2] = np.concatenate([elists[2], [11, 11]]).astype(np.int32)  # the test item excluded, twice
    got = multi(P, Q, users, tlists, num_cand, elists)
    np.testing.assert_array_equal(got, yardstick(P, Q, users, tlists, num_cand, elists))
    assert got[0] == got[2] == got[4]  # a repeated test item: the same position each time
    # excluded or not, a test item never counts itself
    plain = multi(P, Q, users[2:], tlists[2:], num_cand, [elists[2][:-2]])
    if 11 not in elists[2][:-2]:
        np.testing.assert_array_equal(plain, got[-1:])


def test_independence_and_determinism():
    ops = _ops()
    P, Q, users, tlists, num_cand, elists, want = grid_case(64)
    off, _ = csr(tlists)
    for r in (3, 4, 9):  # alone
        alone = multi(P, Q, users[r:r + 1], tlists[r:r + 1], num_cand, elists[r:r + 1])
        np.testing.assert_array_equal(alone, want[off[r]:off[r + 1]])
    perm = np.random.default_rng(5).permutation(len(users))
    got = multi(P, Q, users[perm], [tlists[r] for r in perm], num_cand, [elists[r] for r in perm])
    np.testing.assert_array_equal(got, np.concatenate([want[off[r]:off[r + 1]] for r in perm]))
    # a chunk boundary moves nothing: the long list split into two entries of the same user
    r = 4
    halves = multi(P, Q, users[[r, r]], [tlists[r][:100], tlists[r][100:]], num_cand, [elists[r], elists[r]])
    np.testing.assert_array_equal(halves, want[off[r]:off[r + 1]])
    a = multi(P, Q, users, tlists, num_cand, elists)
    ops.recommend_topk(torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV), users, 10)  # another kernel
    b = multi(P, Q, users, tlists, num_cand, elists)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, want)


def _raw_positions(P, Q, users, tlists, num_cand, elists, check, ws_slack=64):
    """acf_eval_positions_multi through ctypes with canaries around positions and after the workspace:
    (return code, positions, canaries intact)."""
    ops = _ops()
    native = importlib.import_module(PKG + "._native")
    lib = native.load()
    tP, tQ = torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV)
    to, tf = csr(tlists)
    eo, ef = csr(elists)
    tu = torch.tensor(np.asarray(users, np.int32), device=DEV)
    tto, ttf = torch.tensor(to, device=DEV), torch.tensor(tf, device=DEV)
    teo, tef = torch.tensor(eo, device=DEV), torch.tensor(ef, device=DEV)
    T, pad = len(tf), 32
    pos = torch.full((T + 2 * pad,), -77, dtype=torch.int32, device=DEV)
    need = ops.eval_positions_multi_workspace(len(users), T, num_cand)
    work = torch.full((need // 4 + ws_slack,), -77, dtype=torch.int32, device=DEV)
    rc = lib.acf_eval_positions_multi(tP.data_ptr(), tQ.data_ptr(), P.shape[0], Q.shape[0], P.shape[1],
                                      tu.data_ptr(), tto.data_ptr(), ttf.data_ptr(), len(users), T, num_cand,
                                      teo.data_ptr(), tef.data_ptr(), pos.data_ptr() + 4 * pad, work.data_ptr(),
                                      need, int(check), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pos, work = pos.cpu().numpy(), work.cpu().numpy()
    intact = bool((pos[:pad] == -77).all() and (pos[pad + T:] == -77).all() and (work[(need + 3) // 4:] == -77).all())
    return rc, pos[pad:pad + T], intact


def test_range_errors_and_canaries():
    ops = _ops()
    native = importlib.import_module(PKG + "._native")
    P, Q, users, tlists, num_cand, elists, want = grid_case(8)
    rc, pos, intact = _raw_positions(P, Q, users, tlists, num_cand, elists, check=1)
    assert rc == native.ACF_OK and intact
    np.testing.assert_array_equal(pos, want)
    bad_users = users.copy()
    bad_users[2], bad_users[7] = P.shape[0] + 3, -1
    bad_lists = [t.copy() for t in tlists]
    bad_lists[4][299], bad_lists[3][0] = Q.shape[0] + 7, -2
    off, _ = csr(tlists)
    for bu, bl in ((bad_users, tlists), (users, bad_lists), (bad_users, bad_lists)):
        rc, pos, intact = _raw_positions(P, Q, bu, bl, num_cand, elists, check=1)
        assert rc == native.ACF_E_RANGE and intact
        rc, pos, intact = _raw_positions(P, Q, bu, bl, num_cand, elists, check=0)
        assert rc == native.ACF_OK and intact
        # entries with good indices are untouched by their neighbours' bad ones
        np.testing.assert_array_equal(pos[off[12]:off[13]], want[off[12]:off[13]])
        with pytest.raises(IndexError):
            multi(P, Q, bu, bl, num_cand, elists)
    # a bad user reads row 0, a bad test item reads item 0
    as_zero = users.copy()
    as_zero[2], as_zero[7] = 0, 0
    rc, pos, _ = _raw_positions(P, Q, bad_users, tlists, num_cand, elists, check=0)
    np.testing.assert_array_equal(pos, multi(P, Q, as_zero, tlists, num_cand, elists))
    # the strips path keeps to its workspace as well
    rng = np.random.default_rng(74)
    Qb = (0.1 * rng.standard_normal((9000, 8))).astype(np.float32)
    rc, pos, intact = _raw_positions(P, Qb, [1, 2], [[5, 8000], [7]], 9000, [[3], []], check=1)
    assert rc == native.ACF_OK and intact
    assert ops.eval_positions_multi_workspace(2, 3, 9000) > 16
    np.testing.assert_array_equal(pos, yardstick(P, Qb, [1, 2], [[5, 8000], [7]], 9000, [[3], []]))


# ---- metrics ----------------------------------------------------------------------
def _n_neg(num_cand, tlists, elists):
    out = []
    for t, e in zip(tlists, elists):
        e = np.asarray(e)
        out.append(num_cand - len(set(e[(e >= 0) & (e < num_cand)].tolist()) - set(t.tolist())) - len(set(t.tolist())))
    return np.asarray(out, np.int32)


def _check_metrics(pos, off, n_neg, cuts):
    ops = _ops()
    ev = importlib.import_module(PKG + ".evaluate")
    want = ev.metrics_from_positions_multi(pos, off, n_neg, cuts)
    tp, tn = torch.tensor(pos, device=DEV), torch.tensor(n_neg, device=DEV)
    a = ops.rank_metrics(tp, off, tn, cuts)
    b = ops.rank_metrics(tp, torch.tensor(off, device=DEV), tn, cuts)
    for name in ("per_user", "per_user_free", "mean_cut", "mean_free"):
        got = getattr(a, name)
        assert got.dtype == torch.float64 and tuple(got.shape) == want[name].shape
        np.testing.assert_allclose(got.cpu().numpy(), want[name], rtol=1e-9, atol=0)
        assert torch.equal(got, getattr(b, name))  # equal bits on equal inputs
    assert a.n_scored.dtype == torch.int64 and int(a.n_scored.item()) == want["n_scored"]
    return a, want


def test_rank_metrics_small_grid():
    ev = importlib.import_module(PKG + ".evaluate")
    P, Q, users, tlists, num_cand, elists, pos = grid_case(8)
    off, _ = csr(tlists)
    n_neg = _n_neg(num_cand, tlists, elists)
    a, want = _check_metrics(np.array(pos), off, n_neg, CUTS)
    assert int(a.n_scored.item()) == sum(1 for m in GRID_LENS if m > 0)  # the empty lists are left out
    empty = [r for r, m in enumerate(GRID_LENS) if m == 0]
    assert (a.per_user[empty] == 0).all() and (a.per_user_free[empty] == 0).all()
    # the tolerance separates: one position moved by one changes a mean by more than 1e-6
    moved = np.array(pos)
    moved[off[3]] += 1
    other = ev.metrics_from_positions_multi(moved, off, n_neg, CUTS)
    assert np.abs(other["mean_free"] - want["mean_free"]).max() > 1e-6
    # no cutoffs, and all lists empty
    a, _ = _check_metrics(np.array(pos), off, n_neg, ())
    z = np.zeros(4, np.int64)
    a, _ = _check_metrics(np.zeros(0, np.int32), z, np.ones(3, np.int32), (10,))
    assert int(a.n_scored.item()) == 0 and (a.mean_cut == 0).all()


def test_rank_metrics_long_list_and_ties():
    P, Q, tlists, elists, pos = long_case()
    off, _ = csr(tlists)
    _check_metrics(np.array(pos), off, _n_neg(2000, tlists, elists), CUTS)
    # tied positions: j goes by index
    _check_metrics(np.array([1, 1, 0, 4, 4, 4, 2], np.int32), np.array([0, 2, 7], np.int64),
                   np.array([9, 20], np.int32), (1, 2, 3, 1024))


# ---- end to end -------------------------------------------------------------------
def test_evaluate_multi_end_to_end(acf):
    ops = _ops()
    ev = importlib.import_module(PKG + ".evaluate")
    data = importlib.import_module(PKG + ".data")
    ds = data.get_dataset("synthetic:60:200:1500")
    args = Namespace(embed_size=16, lr=0.05, reg=0.0, dns=1, adv="grad", eps=0.5, adver=0, reg_adv=1.0,
                     epochs=1, seed=11)
    m = acf.MF(ds.num_users, ds.num_items, args).build_graph(device=torch.device(DEV))
    off, items = ds.sorted_lists()
    lists = {u: items[off[u]:off[u + 1]][-3:].tolist() + [int(ds.test_items[u])] for u in range(0, 60, 2)}
    lists[7] = []
    plan = ev.init_eval_multi(ds, lists)
    cuts = (10, 50, 100)
    out, raw = m.evaluate_multi(plan, cutoffs=cuts, raw=True)
    assert list(out) == ev.metric_names(cuts)
    assert out["n_users"] == 30
    for k, v in out.items():
        if k != "n_users":
            assert 0.0 <= v <= 1.0, (k, v)
    assert out["recall@100"] >= out["recall@10"] and out["hit@100"] >= out["recall@100"]
    want = ev.metrics_from_positions_multi(raw["positions"], plan.test_off, plan.n_neg, cuts)
    np.testing.assert_allclose(raw["per_user"], want["per_user"], rtol=1e-9)
    assert out == acf.APR.evaluate_multi.__get__(Namespace(_ensure=lambda: None, model=m))(plan, cutoffs=cuts)
    # the positions are the yardstick's
    P, Q = m.embedding_P.cpu().numpy(), m.embedding_Q.cpu().numpy()
    tl = [plan.test_items[plan.test_off[k]:plan.test_off[k + 1]] for k in range(len(plan.users))]
    el = [plan.excl[plan.excl_off[k]:plan.excl_off[k + 1]] for k in range(len(plan.users))]
    np.testing.assert_array_equal(raw["positions"], yardstick(P, Q, plan.users, tl, plan.num_candidates, el))
    # the torch ops return what ops.* returns
    tops = importlib.import_module(PKG + ".torch_ops").load()
    u, to, t, eo, ex, nn = plan.device_arrays(m.embedding_P.device)
    pos = tops.eval_positions_multi(m.embedding_P, m.embedding_Q, u, to, t, plan.num_candidates, eo, ex)
    assert torch.equal(pos.cpu(), torch.tensor(raw["positions"]))
    none = tops.eval_positions_multi(m.embedding_P, m.embedding_Q, u, to, t, plan.num_candidates,
                                     eo[:0], ex[:0])
    assert torch.equal(none, ops.eval_positions_multi(m.embedding_P, m.embedding_Q, u, to, t, plan.num_candidates))
    got = tops.rank_metrics(pos, to, nn, list(cuts))
    ref = ops.rank_metrics(pos, to, nn, cuts)
    for g, name in zip(got, ("per_user", "per_user_free", "mean_cut", "mean_free", "n_scored")):
        assert torch.equal(g, getattr(ref, name))
    with pytest.raises(IndexError):
        tops.eval_positions_multi(m.embedding_P, m.embedding_Q, u + 1000, to, t, plan.num_candidates, eo, ex)


def test_cli_writes_multi_file(acf, tmp_path, monkeypatch):
    import glob
    cli = importlib.import_module(PKG + ".cli")
    monkeypatch.chdir(tmp_path)
    f = tmp_path / "held.rating"
    f.write_text("".join("%d\t%d\t1\t0\n" % (u, (7 * u + 3 * k) % 200) for u in range(0, 300, 3) for k in range(4)))
    rc = cli.main(["--path", str(tmp_path) + "/", "--opath", "t/", "--dataset", "synthetic:300:200:8000",
                   "--model", "bpr", "--epochs", "1", "--verbose", "1", "--embed_size", "16", "--eval_mode", "all",
                   "--test_multi", str(f), "--cutoffs", "5,20"])
    assert rc == 0
    files = glob.glob(str(tmp_path / "out" / "t" / "*.multi"))
    assert len(files) == 1
    got = cli.read_multi(files[0])
    ev = importlib.import_module(PKG + ".evaluate")
    assert list(got) == ev.metric_names((5, 20)) and got["n_users"] == 100
    assert all(0.0 <= v <= 1.0 for k, v in got.items() if k != "n_users")
