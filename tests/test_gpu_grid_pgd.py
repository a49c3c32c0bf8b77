"""Grid training against a K-step inner attack on the GPU (ops.grid_train with
StepHParams.adv_iters = K > 1 / acf_apr_grid_train_pgd): per member
against the float64 reference of tests/grid_pgd_ref.py (tables, accumulators,
loss_clean, loss_adv, no element excluded), bit for bit against itself and against
acf_apr_grid_train, and through MFGrid / training_grid.  Inputs: grid_pgd_ref.parity_case
/ degenerate_case (tables of 65 x 49 rows at sigma = 0.3, B = 32, 3 batches unless the
case says otherwise).

Tolerance (grid_pgd_ref.tolerance): per case, rtol = max(test_gpu_grid._rtol, 4 x the
largest deviation of the fp32 plan-order restatement step32 from the fp64 reference over
the case's members and outputs), atol 1e-6; the deviation is the smallest rtol at which
step32 is inside atol + rtol |want| everywhere.  The factor 4 covers what step32 does not
model (the kernel's dot-product tree, rsqrt / rcp) through K normalisations.  Measured on
the CPU (test_grid_pgd_host.py prints them):
  parity d = 8 / 20 / 64 / 132 / 256: largest deviation 6.5e-08 / 1.8e-07 / 1.5e-07 /
      2.6e-07 / 1.5e-06 -> rtol 1e-5 (the project's floor) at every d;
  hot_user (B = 160, 320 terms): 1.5e-05 -> rtol 6.1e-05 (_rtol alone: 3.8e-05);
  hot_item 3.5e-07, pos_equals_neg 1.9e-07, clipped 0, eps_zero 9.2e-08 -> rtol 1e-5.
On an MI355X the largest error of any element of any case was 0.16 of its tolerance
(each comparison prints its own figure under pytest -s).
"""
import argparse
import importlib
import os

import numpy as np
import pytest
import torch

import grid_pgd_ref as ref
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
B, NB = ref.B, ref.NB
NAMES = ("P", "Q", "accP", "accQ", "loss_clean", "loss_adv")


def _gpu(P, Q, dev):
    return [torch.tensor(P, device=dev), torch.tensor(Q, device=dev), torch.full(P.shape, 0.1, device=dev),
            torch.full(Q.shape, 0.1, device=dev)]


def _train(ops, dev, P, Q, u, i, j, batch, hps, **kw):
    """grid_train on fresh tables: [P, Q, accP, accQ, loss_clean, loss_adv] on the device."""
    tabs = _gpu(P, Q, dev)
    hps = [h if isinstance(h, ops.StepHParams) else ops.StepHParams(**h) for h in hps]
    lc, la = ops.grid_train(*tabs, hps, torch.tensor(u, device=dev), torch.tensor(i, device=dev),
                            torch.tensor(j, device=dev), batch, losses=True, **kw)
    torch.cuda.synchronize()
    return tabs + [lc, la]


def _check(ops, dev, key, case):
    P, Q, u, i, j, batch, hps = case
    out = _train(ops, dev, P, Q, u, i, j, batch, hps)
    rtol, atol = ref.tolerance(key, case)
    for m, (want, lc, la, dev_m) in enumerate(ref.reference(key, case)):
        for g, w, n in zip(out, (*want, lc, la), NAMES):
            if n == "loss_adv" and not hps[m].get("adver", 0):
                assert not g[m].any()  # a BPR member's row is never written
                continue
            got = g[m].cpu().numpy()
            err = np.abs(got - w)
            print("%s member %d %-10s max |diff| %.3e, max diff/(atol + rtol |want|) %.3f (rtol %.3g)" % (
                key, m, n, err.max(), (err / (atol + rtol * np.abs(w))).max(), rtol))
            np.testing.assert_allclose(got, w, rtol=rtol, atol=atol, err_msg=f"{key} member {m} {n}")
    return out


# ---- 1. parity per member ---------------------------------------------------------------
@pytest.mark.parametrize("d", ref.PARITY_DIMS)
def test_parity_per_member(ops, dev, d):
    """K = 1, 2 (inside the ball), 3 (projected from step 2), 5 (reg != 0) and a BPR member in one grid."""
    _check(ops, dev, ("parity", d), ref.parity_case(d))


# ---- 2. degenerate and hot rows, every member at K = 3 ------------------------------------
@pytest.mark.parametrize("name", ref.DEGENERATE)
def test_degenerate_and_hot_rows(ops, dev, name):
    case = ref.degenerate_case(name)
    out = _check(ops, dev, ("degenerate", name), case)
    if name == "eps_zero":  # K = 3 at eps = 0, with and without a step, is the eps = 0 one-step member's bits
        for x, n in zip(out, NAMES):
            assert torch.equal(x[0], x[1]) and torch.equal(x[2], x[1]), n
    if name == "pos_equals_neg":  # rows that only i == j triplets touch: zero gradient, untouched tables
        P, Q, u, i, j = case[:5]
        assert np.array_equal(out[0][0].cpu().numpy()[56:64], P[0][56:64])
        assert np.array_equal(out[1][0].cpu().numpy()[40:48], Q[0][40:48])


# ---- 3. bit level -----------------------------------------------------------------------
def _hps16(iters=(1, 3, 5, 2)):
    return [dict(adver=int(k % 5 != 4), eps=0.1 + 0.2 * k, reg_adv=0.25 * (1 + k % 4), lr=0.02 + 0.01 * k,
                 reg=0.01 * (k % 3), adv_iters=iters[k % len(iters)], adv_step=None if k % 2 else 0.3)
            for k in range(16)]


@pytest.fixture(scope="module")
def grid16(ops, dev):
    """A mixed M = 16 grid (K = 1, 3, 5, 2 in turn, every fifth member BPR) at d = 64, trained once."""
    P, Q = ref.tables(7, 16, 64)
    u, i, j = ref.triplets(8, NB * B)
    return (P, Q, u, i, j), _train(ops, dev, P, Q, u, i, j, B, _hps16())


def test_one_step_member_through_the_new_entry_equals_the_old_entry(ops, dev, grid16):
    (P, Q, u, i, j), out = grid16
    hps = _hps16()
    ks = [k for k in range(16) if hps[k]["adv_iters"] == 1 or not hps[k]["adver"]]
    assert len(ks) >= 4 and any(hps[k]["adver"] for k in ks)
    # the same members with the attack fields left out: all one-step, acf_apr_grid_train
    old = _train(ops, dev, P[ks], Q[ks], u, i, j, B,
                 [{f: v for f, v in hps[k].items() if f not in ("adv_iters", "adv_step")} for k in ks])
    for x, y, n in zip(old, out, NAMES):
        assert torch.equal(x, y[torch.tensor(ks, device=dev)]), n


@pytest.mark.parametrize("k", [1, 5, 13])  # K = 3 members
def test_k3_member_equals_its_solo_call(ops, dev, grid16, k):
    (P, Q, u, i, j), out = grid16
    assert _hps16()[k]["adv_iters"] == 3 and _hps16()[k]["adver"]
    solo = _train(ops, dev, P[k:k + 1], Q[k:k + 1], u, i, j, B, [_hps16()[k]])
    for x, y, n in zip(solo, out, NAMES):
        assert torch.equal(x[0], y[k]), n


def test_position_and_neighbours_k_do_not_matter(ops, dev, grid16):
    (P, Q, u, i, j), out = grid16
    perm = np.random.default_rng(3).permutation(16)
    hps = _hps16()
    got = _train(ops, dev, P[perm], Q[perm], u, i, j, B, [hps[p] for p in perm])
    for x, y, n in zip(got, out, NAMES):
        assert torch.equal(x, y[torch.tensor(perm, device=dev)]), n
    # the K = 3 members keep their bits when every other member's K changes (and max K with it)
    other = _hps16(iters=(4, 3, 1, 7))
    assert all(a["adv_iters"] == 3 for a, b in zip(other, hps) if b["adv_iters"] == 3)
    got = _train(ops, dev, P, Q, u, i, j, B, other)
    k3 = torch.tensor([k for k in range(16) if hps[k]["adv_iters"] == 3], device=dev)
    for x, y, n in zip(got, out, NAMES):
        assert torch.equal(x[k3], y[k3]), n


def test_two_calls_are_bit_equal(ops, dev, grid16):
    (P, Q, u, i, j), out = grid16
    for x, y, n in zip(_train(ops, dev, P, Q, u, i, j, B, _hps16()), out, NAMES):
        assert torch.equal(x, y), n


def test_one_call_of_three_batches_equals_three_calls(ops, dev):
    """Over 6 users and 10 items every row written in batch t is read in batch t + 1."""
    rng = np.random.default_rng(50)
    u, i, j = (rng.integers(0, n, NB * B).astype(np.int32) for n in (6, 10, 10))
    P, Q = ref.tables(51, len(ref.HPS_PARITY), 64)
    one = _train(ops, dev, P, Q, u, i, j, B, ref.HPS_PARITY)
    hps = [ops.StepHParams(**h) for h in ref.HPS_PARITY]
    three = _gpu(P, Q, dev)
    for t in range(NB):
        s = slice(t * B, (t + 1) * B)
        ops.grid_train(*three, hps, torch.tensor(u[s], device=dev), torch.tensor(i[s], device=dev),
                       torch.tensor(j[s], device=dev), B)
    for x, y, n in zip(one, three, NAMES):
        assert torch.equal(x, y), n


# ---- 4. edges ---------------------------------------------------------------------------
def test_out_of_range_index_raises_before_any_write(ops, dev):
    native = importlib.import_module(PKG + "._native")
    P, Q = ref.tables(62, 2, 64)
    u, i, j = ref.triplets(63, NB * B)
    j[2 * B + 5] = ref.I1
    tabs = _gpu(P, Q, dev)
    before = [t.clone() for t in tabs]
    with pytest.raises(native.NativeIndexError):
        ops.grid_train(*tabs, [ops.StepHParams(adver=1, adv_iters=3), ops.StepHParams()], torch.tensor(u, device=dev),
                       torch.tensor(i, device=dev), torch.tensor(j, device=dev), B, check=True)
    torch.cuda.synchronize()
    for x, y in zip(tabs, before):
        assert torch.equal(x, y)


def test_no_batches_leaves_tables_untouched(ops, dev):
    P, Q = ref.tables(61, 2, 64)
    tabs = _gpu(P, Q, dev)
    before = [t.clone() for t in tabs]
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    ops.grid_train(*tabs, [ops.StepHParams(adver=1, adv_iters=5), ops.StepHParams()], e, e, e, B)
    torch.cuda.synchronize()
    for x, y in zip(tabs, before):
        assert torch.equal(x, y)


# ---- 5. the Python layer ------------------------------------------------------------------
def test_training_grid_epoch_with_adv_iters_axis(acf, dev, tmp_path):
    """One training_grid epoch on the first 1,500 users of the Video fixture with
    --grid_adv_iters "1,3": both members log under their names, the K = 3 one with _k3."""
    train = importlib.import_module(PKG + ".train")
    cli = importlib.import_module(PKG + ".cli")
    z = np.load(os.path.join(GOLDEN, "video_data.npz"))
    os.makedirs(tmp_path / "data")
    keep = z["train_u"] < 1500
    with open(tmp_path / "data" / "Video.train.rating", "w") as f:
        f.writelines(f"{u}\t{i}\t{r}\t1\n" for u, i, r in zip(z["train_u"][keep], z["train_i"][keep],
                                                              z["train_r"][keep]))
    n_items = int(z["train_i"][keep].max()) + 1
    keep = z["test_u"] < 1500
    with open(tmp_path / "data" / "Video.test.rating", "w") as f:
        f.writelines(f"{u}\t{i % n_items}\t1\t1\n" for u, i in zip(z["test_u"][keep], z["test_i"][keep]))
    args = cli.parse_args(["--path", str(tmp_path) + "/", "--opath", "g/", "--dataset", "Video", "--model", "apr",
                           "--embed_size", "64", "--epochs", "1", "--eval_mode", "all", "--ckpt", "0",
                           "--grid_adv_iters", "1,3"])
    args.adver = 1
    assert isinstance(args, argparse.Namespace) and cli.grid_of(args) == [dict(adv_iters=1), dict(adv_iters=3)]
    ds = acf.get_dataset("Video", args.path, seed=2019)
    grid = acf.MFGrid(ds.num_users, ds.num_items, args, cli.grid_of(args), device=dev)
    assert torch.equal(grid.embedding_P[0], grid.embedding_P[1])  # one seed: the members differ in K alone
    best = train.training_grid(grid, ds, args, "Video_apr_grid_ts", epoch_start=1, epoch_end=1, time_stamp="ts")
    assert not torch.equal(grid.embedding_P[0], grid.embedding_P[1])
    out = tmp_path / "out" / "g"
    base = "Video_apr_d64_e%f_l%f_ts" % (0.5, 1.0)
    for name in (base, base + "_k3"):
        text = open(out / (name + ".out")).read()
        assert "Epoch 1 [" in text and "Epoch 1 is the best epoch" in text and "K = 10: HR = " in text
        assert os.path.exists(out / (name + ".hr")) and os.path.exists(out / (name + ".ndcg"))
    rows = train.read_grid_table(out / "Video_apr_grid_ts.grid")
    assert [(r[0], r[1], r[5], r[7], r[10]) for r in rows] == [(0, 0.5, 1, 1, 1), (1, 0.5, 1, 1, 3)]
    assert rows[1][11] == pytest.approx(2.5 * 0.5 / 3)
    assert all(r[8] == best[r[0]]["hr10"] for r in rows)
    assert grid.member(1).hparams().adv_iters == 3


def test_cli_adv_iters_trains_a_single_run_through_a_grid_of_one(acf, tmp_path, monkeypatch):
    """--adv_iters 3 on a plain apr run: the APR phase is a one-member grid that logs, evaluates
    and checkpoints as a single run under <runName>_k3, and --robust_iters checks it."""
    import glob
    cli = importlib.import_module(PKG + ".cli")
    monkeypatch.chdir(tmp_path)
    z = np.load(os.path.join(GOLDEN, "video_data.npz"))
    os.makedirs(tmp_path / "data")
    with open(tmp_path / "data" / "Video.train.rating", "w") as f:
        f.writelines(f"{u}\t{i}\t{r}\t1\n" for u, i, r in zip(z["train_u"], z["train_i"], z["train_r"]))
    with open(tmp_path / "data" / "Video.test.rating", "w") as f:
        f.writelines(f"{u}\t{i}\t1\t1\n" for u, i in zip(z["test_u"], z["test_i"]))
    rc = cli.main(["--path", str(tmp_path) + "/", "--opath", "t/", "--dataset", "Video", "--model", "apr", "--epochs",
                   "2", "--adv_epoch", "1", "--verbose", "2", "--eval_mode", "all", "--embed_size", "16", "--ckpt",
                   "1", "--seed", "0", "--adv_iters", "3", "--robust_eps", "0.5", "--robust_iters", "3"], "ori")
    assert rc == 0
    out = tmp_path / "out" / "t"
    outs = glob.glob(str(out / "*.out"))
    assert len(outs) == 1 and outs[0].endswith("_k3.out") and not glob.glob(str(out / "*.grid"))
    text = open(outs[0]).read()
    assert "Initialize BPR" in text and "Initialize APR" in text and "Epoch 2 [" in text
    assert "Epoch 2 is the best epoch" in text
    robust = glob.glob(str(out / "*_k3.robust"))
    assert len(robust) == 1 and [r[0] for r in cli.read_robust(robust[0])] == ["grad", "random", "pgd"]
    assert glob.glob(str(tmp_path / "Pretrain" / "Video" / "APR" / "embed_16" / "*" / "weights-2.npz"))
