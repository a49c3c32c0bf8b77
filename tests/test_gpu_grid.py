"""Grid training (ops.grid_train / acf_apr_grid_train): M models over
one triplet stream in one call, against the CPU oracle per member, bit for bit
against itself (independence of M and of the member's position, repeatability,
one call of n batches == n calls), against the existing trainer, and through
MFGrid / training_grid.

Unless a case says otherwise: tables of 65 x 49 rows, B = 32, 3 batches (the shape
of tests/golden/oracle_tiny.npz), tables drawn at sigma = 0.3 as in
test_gpu_parity.py so that an update is far above the tolerance.

Tolerance: the project's rtol 1e-5 / atol 1e-6 (test_gpu_parity.py), rtol widened
to max(1e-5, 2 n u) as test_single_step_strict does: n = the most terms any row
of any batch sums (a user's occurrences x 2 for its pos and neg branch, an item's
occurrences), u = 2^-24 (two orders of an n-term fp32 sum differ by 2 gamma_n).
"""
import argparse
import importlib
import os

import numpy as np
import pytest
import torch

from apr_oracle import HParams
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6
U1, I1, B, NB = 65, 49, 32, 3
NAMES = ("P", "Q", "accP", "accQ")

# (adver 1, eps 0.5, lambda 1), (adver 1, eps 2, lambda 0.1, reg 0.01, lr 0.1), a BPR control
HPS3 = (dict(adver=1, eps=0.5, reg_adv=1.0), dict(adver=1, eps=2.0, reg_adv=0.1, reg=0.01, lr=0.1), dict(adver=0))


def _tables(seed, M, d, u1=U1, i1=I1, scale=0.3):
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((M, u1, d)) * scale).astype(np.float32)
    Q = (rng.standard_normal((M, i1, d)) * scale).astype(np.float32)
    return P, Q


def _triplets(seed, n, u1=U1, i1=I1):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, u1, n).astype(np.int32), rng.integers(0, i1, n).astype(np.int32),
            rng.integers(0, i1, n).astype(np.int32))


def _gpu(P, Q, dev):
    return [torch.tensor(P, device=dev), torch.tensor(Q, device=dev), torch.full(P.shape, 0.1, device=dev),
            torch.full(Q.shape, 0.1, device=dev)]


def _oracle_member(oracle, P, Q, u, i, j, batch, hp):
    """One member through oracle.apr_batch, batch by batch: (tables, loss_clean, loss_adv)."""
    rP, rQ = P.copy(), Q.copy()
    aP, aQ = np.full(P.shape, 0.1, np.float32), np.full(Q.shape, 0.1, np.float32)
    lcs, las = [], []
    for t in range(len(u) // batch):
        s = slice(t * batch, (t + 1) * batch)
        lc, la, _, _ = oracle.apr_batch(rP, rQ, aP, aQ, u[s], i[s], j[s], hp)
        lcs.append(lc)
        las.append(la)
    return (rP, rQ, aP, aQ), np.concatenate(lcs), np.concatenate(las)


def _rtol(u, i, j, batch):
    n_terms = 1
    for t in range(len(u) // batch):
        s = slice(t * batch, (t + 1) * batch)
        n_terms = max(n_terms, 2 * np.bincount(u[s]).max(), np.bincount(np.concatenate([i[s], j[s]])).max())
    return max(RTOL, 2 * n_terms * 2.0 ** -24)


def _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, batch, hps):
    """grid_train on (P, Q) [M, ...] under hps (dicts) vs the oracle per member, losses included."""
    tabs = _gpu(P, Q, dev)
    lc, la = ops.grid_train(*tabs, [ops.StepHParams(**h) for h in hps], torch.tensor(u, device=dev),
                            torch.tensor(i, device=dev), torch.tensor(j, device=dev), batch, losses=True)
    torch.cuda.synchronize()
    rtol = _rtol(u, i, j, batch)
    for m, h in enumerate(hps):
        want, lc_w, la_w = _oracle_member(oracle, P[m], Q[m], u, i, j, batch, HParams(**h))
        for g, w, n in zip(tabs, want, NAMES):
            np.testing.assert_allclose(g[m].cpu().numpy(), w, rtol=rtol, atol=ATOL, err_msg=f"member {m} {n}")
        np.testing.assert_allclose(lc[m].cpu().numpy(), lc_w, rtol=rtol, atol=ATOL, err_msg=f"member {m} loss_clean")
        if h.get("adver", 0):
            np.testing.assert_allclose(la[m].cpu().numpy(), la_w, rtol=rtol, atol=ATOL,
                                       err_msg=f"member {m} loss_adv")
    return tabs


# ---- 1. parity per member -------------------------------------------------------
@pytest.mark.parametrize("d", [8, 20, 64, 132, 256])  # LPR 2, a padded row-group, the headline, a padded wave, the wave
def test_parity_per_member(ops, oracle, dev, d):
    P, Q = _tables(d, 3, d)
    u, i, j = _triplets(100 + d, NB * B)
    _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, B, HPS3)


# ---- 2. independence, bit for bit -----------------------------------------------
def _hps16():
    return [dict(adver=int(k % 5 != 4), eps=0.1 + 0.2 * k, reg_adv=0.25 * (1 + k % 4), lr=0.02 + 0.01 * k,
                 reg=0.01 * (k % 3)) for k in range(16)]


@pytest.fixture(scope="module")
def grid16(ops, dev):
    """An M = 16 grid of 16 distinct hparams at d = 64, trained once: (inputs, outputs)."""
    d = 64
    P, Q = _tables(7, 16, d)
    u, i, j = (torch.tensor(x, device=dev) for x in _triplets(8, NB * B))
    hps = [ops.StepHParams(**h) for h in _hps16()]
    tabs = _gpu(P, Q, dev)
    lc, la = ops.grid_train(*tabs, hps, u, i, j, B, losses=True)
    torch.cuda.synchronize()
    return (P, Q, u, i, j, hps), tabs + [lc, la]


@pytest.mark.parametrize("k", [0, 7, 15])
def test_member_equals_single_model_call(ops, dev, grid16, k):
    (P, Q, u, i, j, hps), out = grid16
    tabs = _gpu(P[k:k + 1], Q[k:k + 1], dev)
    lc, la = ops.grid_train(*tabs, [hps[k]], u, i, j, B, losses=True)
    for x, y, n in zip(tabs + [lc, la], out, NAMES + ("loss_clean", "loss_adv")):
        assert torch.equal(x[0], y[k]), n


def test_permuting_members_permutes_outputs(ops, dev, grid16):
    (P, Q, u, i, j, hps), out = grid16
    perm = np.random.default_rng(3).permutation(16)
    tabs = _gpu(P[perm], Q[perm], dev)
    lc, la = ops.grid_train(*tabs, [hps[p] for p in perm], u, i, j, B, losses=True)
    for x, y, n in zip(tabs + [lc, la], out, NAMES + ("loss_clean", "loss_adv")):
        assert torch.equal(x, y[torch.tensor(perm, device=dev)]), n


def test_two_calls_are_bit_equal(ops, dev, grid16):
    (P, Q, u, i, j, hps), out = grid16
    tabs = _gpu(P, Q, dev)
    lc, la = ops.grid_train(*tabs, hps, u, i, j, B, losses=True)
    for x, y, n in zip(tabs + [lc, la], out, NAMES + ("loss_clean", "loss_adv")):
        assert torch.equal(x, y), n


# ---- 3. hot and degenerate rows -------------------------------------------------
def _case(name):
    if name == "hot_user":  # one user in all 512 triplets: 1,024 terms, four partial sums
        u, i, j = _triplets(31, 512)
        u[:] = 5
        return u, i, j, 512
    u, i, j = _triplets(32, B)
    if name == "pos_and_neg":  # item 3 positive in some triplets, negative in others
        i[:6] = 3
        j[10:15] = 3
    elif name == "pos_equals_neg":
        j[4] = i[4]
    elif name == "identical":
        u[:], i[:], j[:] = 9, 11, 13
    elif name == "all_unique":  # 16 users, 32 items, B = 16: every row once (49 item rows hold no 64)
        k = np.arange(16, dtype=np.int32)
        return k, k.copy(), k + 16, 16
    return u, i, j, B


@pytest.mark.parametrize("name", ["hot_user", "pos_and_neg", "pos_equals_neg", "identical", "all_unique"])
def test_hot_and_degenerate_rows(ops, oracle, dev, name):
    u, i, j, batch = _case(name)
    if name == "hot_user":
        assert np.bincount(u).max() == 512
    if name == "pos_and_neg":
        assert (i == 3).any() and (j == 3).any()
    if name == "all_unique":
        assert len(np.unique(u)) == 16 and len(np.unique(np.concatenate([i, j]))) == 32
    P, Q = _tables(40, 3, 64)
    _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, batch, HPS3)


# ---- 4. across batches ----------------------------------------------------------
def test_across_batches(ops, oracle, dev):
    """Three batches over 6 users and 10 items: every row updated in batch t is read
    in batch t + 1 by other rows' terms.  Against the oracle, and one call of 3
    batches == three calls of 1 batch, bit for bit."""
    rng = np.random.default_rng(50)
    n = NB * B
    u = rng.integers(0, 6, n).astype(np.int32)
    i = rng.integers(0, 10, n).astype(np.int32)
    j = rng.integers(0, 10, n).astype(np.int32)
    P, Q = _tables(51, 3, 64)
    one = _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, B, HPS3)
    hps = [ops.StepHParams(**h) for h in HPS3]
    three = _gpu(P, Q, dev)
    for t in range(NB):
        s = slice(t * B, (t + 1) * B)
        ops.grid_train(*three, hps, torch.tensor(u[s], device=dev), torch.tensor(i[s], device=dev),
                       torch.tensor(j[s], device=dev), B)
    for x, y, n_ in zip(one, three, NAMES):
        assert torch.equal(x, y), n_


# ---- 5. shape edges -------------------------------------------------------------
def test_five_members_37_rows(ops, oracle, dev):
    """M = 5 and 37 unique rows (10 users, 27 items): neither divides the 16
    row-groups of a workgroup at d = 64."""
    k = np.arange(B)
    u, i, j = (k % 10).astype(np.int32), (k % 13).astype(np.int32), (13 + k % 14).astype(np.int32)
    assert len(np.unique(u)) + len(np.unique(np.concatenate([i, j]))) == 37
    P, Q = _tables(60, 5, 64)
    hps = list(HPS3) + [dict(adver=1, eps=1.0, reg_adv=0.5), dict(adver=0, reg=0.01)]
    _check_against_oracle(ops, oracle, dev, P, Q, u, i, j, B, hps)


def test_no_batches_leaves_tables_untouched(ops, dev):
    P, Q = _tables(61, 2, 64)
    tabs = _gpu(P, Q, dev)
    before = [t.clone() for t in tabs]
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    ops.grid_train(*tabs, [ops.StepHParams(adver=1), ops.StepHParams()], e, e, e, B)
    torch.cuda.synchronize()
    for x, y in zip(tabs, before):
        assert torch.equal(x, y)


def test_out_of_range_item_raises_before_any_write(ops, dev):
    native = importlib.import_module(PKG + "._native")
    P, Q = _tables(62, 2, 64)
    u, i, j = _triplets(63, NB * B)
    j[2 * B + 5] = I1
    tabs = _gpu(P, Q, dev)
    before = [t.clone() for t in tabs]
    with pytest.raises(native.NativeIndexError):
        ops.grid_train(*tabs, [ops.StepHParams(adver=1), ops.StepHParams()], torch.tensor(u, device=dev),
                       torch.tensor(i, device=dev), torch.tensor(j, device=dev), B, check=True)
    torch.cuda.synchronize()
    for x, y in zip(tabs, before):
        assert torch.equal(x, y)


# ---- 6. agreement with the existing trainer -------------------------------------
@pytest.mark.parametrize("m", [0, 1, 2])
def test_agrees_with_the_existing_trainer(ops, dev, m):
    d = 64
    P, Q = _tables(70, 3, d)
    u, i, j = _triplets(71, NB * B)
    ut, it, jt = (torch.tensor(x, device=dev) for x in (u, i, j))
    tabs = _gpu(P, Q, dev)
    hps = [ops.StepHParams(**h) for h in HPS3]
    ops.grid_train(*tabs, hps, ut, it, jt, B)
    single = _gpu(P[m], Q[m], dev)
    ctx = ops.APRContext(U1, I1, d, B, NB, dev)
    ctx.plan(ut, it, jt, B)
    ctx.train_planned(single, hps[m])
    torch.cuda.synchronize()
    rtol = _rtol(u, i, j, B)
    for g, w, n in zip(tabs, single, NAMES):
        np.testing.assert_allclose(g[m].cpu().numpy(), w.cpu().numpy(), rtol=rtol, atol=ATOL, err_msg=n)


# ---- 7. the Python layer --------------------------------------------------------
def _args(**kw):
    a = argparse.Namespace(embed_size=16, lr=0.05, reg=0.0, dns=1, adv="grad", eps=0.5, adver=0, reg_adv=1.0,
                           epochs=1, seed=0, eval_mode="all", batch_size=512, verbose=1, ckpt=0, path="", opath="g/",
                           dataset="Video", model="apr", restore=None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_from_model_copies_the_source(acf, ops, dev):
    mf = acf.MF(40, 30, _args()).build_graph(device=dev)
    mf.accumulator_P.fill_(0.7)
    grid = acf.MFGrid.from_model(mf, acf.MFGrid.product(eps=[0.1, 1.0], reg_adv=[0.5, 1.0]))
    assert len(grid) == 4 and [h.adver for h in grid.hparams()] == [1] * 4
    for m in range(4):
        mem = grid.member(m)
        assert torch.equal(mem.embedding_P, mf.embedding_P) and torch.equal(mem.embedding_Q, mf.embedding_Q)
        assert float(mem.accumulator_P.min()) == float(mem.accumulator_P.max()) == pytest.approx(0.1)
        assert mem.embedding_P.data_ptr() == grid.embedding_P[m].data_ptr()  # a view: no storage of its own
    assert (grid.member(3).eps, grid.member(3).reg_adv) == (1.0, 1.0)


def test_member_evaluates_like_an_mf_on_a_copy(acf, ops, dev):
    ds = acf.synthetic_dataset(300, 200, 6000, seed=3)
    args = _args()
    plan = acf.init_eval_model(ds, args)
    grid = acf.MFGrid(ds.num_users, ds.num_items, args, [dict(seed=1), dict(seed=2), dict(seed=1, eps=1.0)],
                      device=dev)
    assert torch.equal(grid.embedding_P[0], grid.embedding_P[2])  # equal seeds: equal tables
    assert not torch.equal(grid.embedding_P[0], grid.embedding_P[1])
    ep = acf.DeviceSampler(ds, 64, dev, seed=0).epoch(0)
    grid.train_epoch(ep.user, ep.item_pos, ep.item_neg, 64)
    for m in (0, 1):
        mf = acf.MF(ds.num_users, ds.num_items, args).build_graph(device=dev)
        mf.embedding_P.copy_(grid.embedding_P[m])
        mf.embedding_Q.copy_(grid.embedding_Q[m])
        got, raw = grid.member(m).evaluate(ds, plan)
        want, raw_w = mf.evaluate(ds, plan)
        assert got == want and np.array_equal(raw, raw_w)
        items, _ = grid.member(m).recommend(np.arange(10), 5, ds)
        items_w, _ = mf.recommend(np.arange(10), 5, ds)
        assert np.array_equal(items, items_w)


def test_training_grid_epoch_on_video_subset(acf, dev, tmp_path):
    """One training_grid epoch on the first 1,500 users of the Video fixture: M .out
    files under the single-model run names, and the .grid table."""
    train = importlib.import_module(PKG + ".train")
    z = np.load(os.path.join(GOLDEN, "video_data.npz"))
    os.makedirs(tmp_path / "data")
    keep = z["train_u"] < 1500
    with open(tmp_path / "data" / "Video.train.rating", "w") as f:
        f.writelines(f"{u}\t{i}\t{r}\t1\n" for u, i, r in zip(z["train_u"][keep], z["train_i"][keep],
                                                              z["train_r"][keep]))
    n_items = int(z["train_i"][keep].max()) + 1  # the subset's item count: a held-out item beyond it is folded back
    keep = z["test_u"] < 1500
    with open(tmp_path / "data" / "Video.test.rating", "w") as f:
        f.writelines(f"{u}\t{i % n_items}\t1\t1\n" for u, i in zip(z["test_u"][keep], z["test_i"][keep]))
    args = _args(path=str(tmp_path) + "/", embed_size=64, adver=1)
    ds = acf.get_dataset("Video", args.path, seed=2019)
    grid = acf.MFGrid(ds.num_users, ds.num_items, args, acf.MFGrid.product(eps=[0.5, 1.0], reg_adv=[1.0]), device=dev)
    best = train.training_grid(grid, ds, args, "Video_apr_grid_ts", epoch_start=1, epoch_end=1, time_stamp="ts")
    out = tmp_path / "out" / "g"
    for eps in (0.5, 1.0):
        name = "Video_apr_d64_e%f_l%f_ts" % (eps, 1.0)
        text = open(out / (name + ".out")).read()
        assert "Epoch 1 [" in text and "Epoch 1 is the best epoch" in text and "K = 10: HR = " in text
        assert os.path.exists(out / (name + ".hr")) and os.path.exists(out / (name + ".ndcg"))
    rows = train.read_grid_table(out / "Video_apr_grid_ts.grid")
    assert [(r[0], r[1], r[2], r[5], r[7]) for r in rows] == [(0, 0.5, 1.0, 1, 1), (1, 1.0, 1.0, 1, 1)]
    assert all(0.0 <= r[8] <= 1.0 and r[8] == best[r[0]]["hr10"] for r in rows)
