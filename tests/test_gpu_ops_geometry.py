"""The decomposed ops (torch.ops.acf.gather_bpr_fwd_bwd / row_segment_sum /
l2norm_perturb / sparse_adagrad_apply, csrc/acf_ops.hip) one by one, at every
row geometry OPS_GEOM dispatches and at their edges.

test_gpu_torch_ops.py runs the ops composed into one step at d = 8, 64 and 256
and at rtol 1e-5, where an error at one op's edge can hide.  Here each op is
held to its own reference (tests/ops_ref.py) at

    D_OPS = [4, 8, 12, 20, 48, 100, 132, 260, 516, 768, 772, 1024]

which reaches all ten (LPR, NV) of OPS_GEOM, eight of them padded (some lanes of
a row-group own no chunk: they must add exact zeros and stay out of every
store).  So k_seg_sum, k_l2norm_perturb and k_sparse_adagrad run at <1,1>,
<64,2>, <64,3>, <64,4> and at every padded geometry, and k_gather_bpr at NV > 1.
Tables of 61 x 47 rows, 96 triplets: the geometry is under test, not the size.

Bars: row_segment_sum is exact (bits).  l2norm_perturb: (d + 8) u |want|
(ops_ref.l2_bar).  sparse_adagrad_apply: 4 u relative on the accumulator (a
product and a sum of non-negative terms: 2 u, 1 u if hipcc contracts them into
an fma), 4 u (|w| + |lr g / sqrt(acc)|) on the row (lr * g, v_rsq_f32 on an
accumulator that is 2 u off, their product: under 5 u of the step in the worst
case, typically 2; the subtraction 1 u of the row).  gather_bpr_fwd_bwd: x
within the d-term dot products' d u sum|p q|; loss and value rows at
test_gather_bpr_with_bounds' bar.  The composed step: k (ATOL + RTOL |want|)
with k from the fp32 oracle's distance to float64 (_few_step_scale); measured
k = 1 and kd = 1 (delta tables) at every d of {12, 100, 260, 772, 1024}:
one batch of 64 keeps the oracle inside the project's bar even at d = 1024
(test_ops_ref_host.py pins this without a GPU).  The loss bar of
gather_bpr_fwd_bwd has k = 1 except at (d, bounds) = (260, default): 5.0 and
(1024, default): 5.2, where the oracle with its sums reordered is 1.3 bars from
float64; the value rows' k is 1 everywhere.

Measured on the MI355X: l2norm_perturb's largest error 0.20 of its bar, the
Adagrad accumulator's 1.8 u, the Adagrad row's 0.68 of its bar; the file's 127
cases take 9 s together, the slowest (gather_bpr_fwd_bwd at d = 1024, most of it
the oracle's five runs) 0.8 s."""
import importlib

import numpy as np
import pytest
import torch

import ops_ref as R
import saturation_fixture as sf
from test_gpu_step_geometry import ATOL, RTOL, _few_step_scale
from test_gpu_step_saturation import _check_losses

pytestmark = pytest.mark.gpu
U = R.U


@pytest.fixture(scope="module")
def acf_ops():
    return importlib.import_module("adversarial-collaborative-filtering_amd.torch_ops").load()


def _t(x, dev):
    return torch.tensor(x, device=dev)


# ---------------------------------------------------------------------------
# row_segment_sum: exact
def _check_segment_sum(acf_ops, dev, name, d):
    idx, vals, rows = R.seg_case(name, d)
    uq, sm, cnt = acf_ops.row_segment_sum(_t(idx, dev), _t(vals, dev), rows)
    want_u, want_c, want = R.segment_sum_exact(idx, vals)
    assert uq.dtype == torch.int32 and cnt.dtype == torch.int32 and sm.dtype == torch.float32
    assert tuple(uq.shape) == (len(want_u),) == tuple(cnt.shape) and tuple(sm.shape) == (len(want_u), d)
    np.testing.assert_array_equal(uq.cpu().numpy(), want_u)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want_c)
    np.testing.assert_array_equal(sm.cpu().numpy(), want)


@pytest.mark.parametrize("d", R.D_OPS)
def test_row_segment_sum_at_every_geometry(acf_ops, dev, d):
    """m = 300 over 40 rows: unique rows, counts and the sequential fp32 sums in
    input order, bit for bit."""
    _check_segment_sum(acf_ops, dev, "base", d)


@pytest.mark.parametrize("name", R.SEG_EXTRA)
@pytest.mark.parametrize("d", R.SEG_EXTRA_D)
def test_row_segment_sum_edges(acf_ops, dev, d, name):
    """m around the 256 threads of a workgroup and 0, 1, 2; one segment of 5,000
    (a 5,000-term sequential sum); all distinct; descending; num_rows 1, 2, 3,
    2^20 and 2^20 + 1 (the sort's bit count) with row num_rows - 1 present;
    int64 indices.  m = 0: three empty tensors of the right widths."""
    _check_segment_sum(acf_ops, dev, name, d)


# ---------------------------------------------------------------------------
# l2norm_perturb
@pytest.mark.parametrize("k", R.L2_K)
@pytest.mark.parametrize("d", R.D_OPS)
def test_l2norm_perturb(acf_ops, dev, d, k):
    """Every element within (d + 8) u |want| of float64 (no row lies within the
    sum's error of the 1e-12 floor: test_ops_ref_host.py); the zero row stays
    zero, the row whose sum of squares overflows gives zeros, the floored row is
    g * 1e6 * eps; a call on the first k - 1 rows gives those rows the same bits."""
    g = R.l2_fixture(d, k)
    tg = _t(g, dev)
    for eps in R.L2_EPS:
        got = acf_ops.l2norm_perturb(tg, eps).cpu().numpy()
        want = R.l2norm_perturb64(g, eps)
        err = np.abs(got.astype(np.float64) - want)
        ratio = float((err / np.maximum(R.l2_bar(d, want), 1e-300)).max())
        print(f"d {d} k {k} eps {eps}: largest error {ratio:.3f} of the bar")
        assert (err <= R.l2_bar(d, want)).all(), ratio
        if k < 7:
            continue
        assert not got[R.L2_ZERO].any() and not got[R.L2_OVERFLOW].any()
        floored = g[R.L2_BELOW].astype(np.float64) * 1e6 * eps
        assert (np.abs(got[R.L2_BELOW] - floored) <= R.l2_bar(d, floored)).all()
    full = acf_ops.l2norm_perturb(tg, 0.5)
    part = acf_ops.l2norm_perturb(tg[:k - 1].contiguous(), 0.5)
    assert tuple(part.shape) == (k - 1, d) and torch.equal(full[:k - 1], part)


# ---------------------------------------------------------------------------
# sparse_adagrad_apply
@pytest.mark.parametrize("d", R.D_OPS)
def test_sparse_adagrad_apply(acf_ops, dev, d):
    """k = 1, 7 and the rows of one workgroup -1 / +0 / +1 (unique, unsorted, rows
    0 and 60 among them) against float64; the other rows keep their bits in
    both tensors; k = 0 changes nothing."""
    for k in R.adagrad_ks(d):
        W, acc, idx, g = R.adagrad_fixture(d, k)
        tW, tA = _t(W, dev), _t(acc, dev)
        acf_ops.sparse_adagrad_apply(tW, tA, _t(idx, dev), _t(g, dev), 0.05)
        W64, A64 = R.adagrad64(W, acc, idx, g)
        gW, gA = tW.cpu().numpy(), tA.cpu().numpy()
        rows = idx.astype(np.int64)
        err_a = np.abs(gA[rows] - A64[rows])
        assert (err_a <= 4 * U * A64[rows]).all(), (k, float((err_a / A64[rows]).max() / U))
        step = R.LR * g.astype(np.float64) / np.sqrt(A64[rows])
        bar = 4 * U * (np.abs(W[rows].astype(np.float64)) + np.abs(step))
        err_w = np.abs(gW[rows] - W64[rows])
        print(f"d {d} k {k}: acc {float((err_a / A64[rows]).max() / U):.2f} u, W {float((err_w / bar).max()):.3f} of the bar")
        assert (err_w <= bar).all(), (k, float((err_w / bar).max()))
        assert (gW[rows] != W[rows]).any()
        rest = np.setdiff1d(np.arange(R.U1), rows)
        assert np.array_equal(gW[rest].view(np.int32), W[rest].view(np.int32)), k
        assert np.array_equal(gA[rest].view(np.int32), acc[rest].view(np.int32)), k
    W, acc, _, _ = R.adagrad_fixture(d, 1)
    tW, tA = _t(W, dev), _t(acc, dev)
    acf_ops.sparse_adagrad_apply(tW, tA, torch.zeros(0, dtype=torch.int32, device=dev),
                                 torch.zeros(0, d, device=dev), 0.05)
    assert torch.equal(tW, _t(W, dev)) and torch.equal(tA, _t(acc, dev))


# ---------------------------------------------------------------------------
# gather_bpr_fwd_bwd
@pytest.mark.parametrize("setting", list(sf.BOUNDS))
@pytest.mark.parametrize("d", R.D_OPS)
def test_gather_bpr_fwd_bwd(acf_ops, oracle, dev, d, setting):
    """96 triplets in every regime of the score, with i == j, x exactly on each
    bound and one float beyond it: x within d u sum|p q| of float64; the loss
    regime by regime against the oracle and the value rows against g * partner
    in float64, both as test_gather_bpr_with_bounds holds them; the index
    blocks, the negated blocks and the clipped triplets' zero rows exactly."""
    fx, at_bound, outside, equal = R.gather_fixture(d, setting)
    lo, hi, u, i, j = (fx[k] for k in ("lo", "hi", "u", "i", "j"))
    n = R.N
    k, ur = R.gather_loss_bars(oracle, fx, _few_step_scale)
    lc_w = sf.oracle_run(oracle, fx)[1]
    loss, xg, pI, pV, qI, qV = acf_ops.gather_bpr_fwd_bwd(*(_t(fx[a], dev) for a in ("P", "Q", "u", "i", "j")), lo, hi)
    loss, xg, pI, pV, qI, qV = (a.cpu().numpy() for a in (loss, xg, pI, pV, qI, qV))
    want = R.gather_bpr64(fx["P"], fx["Q"], u, i, j, lo, hi)
    err = np.abs(xg - fx["x"])
    assert (err <= d * U * fx["ax"]).all(), float((err / np.maximum(d * U * fx["ax"], 1e-300)).max())
    assert not xg[equal].any()
    assert np.array_equal(xg[at_bound + outside], fx["x"][at_bound + outside].astype(np.float32))
    if k > 1:
        print(f"loss bar scaled by {k:.1f}")
    _check_losses(fx, (loss, None), (lc_w, None), (k, ur), 0, f"gather_bpr d {d}", family="ops_geometry")
    # structure, exactly
    assert np.array_equal(pI, np.concatenate([u, u])) and np.array_equal(qI, np.concatenate([i, j]))
    assert pV.shape == qV.shape == (2 * n, d)
    assert np.array_equal(qV[n:], -qV[:n])
    assert np.array_equal(pV[n:][equal], -pV[:n][equal])
    clipped = want[6]
    assert clipped[outside].all() and not clipped[at_bound].any()
    both = np.concatenate([clipped, clipped])
    kv = _few_step_scale(R.gather_values32(fx), [want[3], want[5]])
    if kv > 1:
        print(f"value rows: bar scaled by {kv:.1f}")
    for got, w, name in ((pV, want[3], "p values"), (qV, want[5], "q values")):
        assert (got[both] == 0).all(), f"{name}: a clipped triplet has a gradient"
        assert got[~both].any()
        np.testing.assert_allclose(got[~both], w[~both], rtol=kv * RTOL, atol=kv * ATOL, err_msg=name)


# ---------------------------------------------------------------------------
# the ops composed into one step, and bpr_apr_step, at the new geometries
def _close(got, want, k, name):
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=k * RTOL, atol=k * ATOL, err_msg=name)


@pytest.mark.parametrize("d", R.D_COMPOSE)
def test_ops_compose_the_apr_step(acf_ops, oracle, dev, d):
    """test_decomposed_ops_compose_the_apr_step's composition at padded and
    multi-chunk geometries, B = 64, against oracle.apr_batch."""
    from apr_oracle import HParams
    hp = HParams(adver=1)
    P, Q, u, i, j = R.compose_problem(d)
    want, deltas, k, kd = R.compose_reference(oracle, d, _few_step_scale)
    if k > 1 or kd > 1:
        print(f"bar scaled by {k:.1f}, delta bar by {kd:.1f}: 4x the fp32 oracle's distance from float64")
    tP, tQ, tu, ti, tj = (_t(a, dev) for a in (P, Q, u, i, j))
    taP, taQ = torch.full_like(tP, 0.1), torch.full_like(tQ, 0.1)
    lc, _, pI, pV, qI, qV = acf_ops.gather_bpr_fwd_bwd(tP, tQ, tu, ti, tj)
    uP, gP, _ = acf_ops.row_segment_sum(pI, pV, R.U1)
    uQ, gQ, _ = acf_ops.row_segment_sum(qI, qV, R.I1)
    dP, dQ = torch.zeros_like(tP), torch.zeros_like(tQ)
    dP[uP.long()] = acf_ops.l2norm_perturb(gP, hp.eps)
    dQ[uQ.long()] = acf_ops.l2norm_perturb(gQ, hp.eps)
    la, _, pI2, pV2, qI2, qV2 = acf_ops.gather_bpr_fwd_bwd(tP + dP, tQ + dQ, tu, ti, tj)
    for W, acc, idx, vals, rows in ((tP, taP, torch.cat([pI, pI2]), torch.cat([pV, hp.reg_adv * pV2]), R.U1),
                                    (tQ, taQ, torch.cat([qI, qI2]), torch.cat([qV, hp.reg_adv * qV2]), R.I1)):
        uq, g, _ = acf_ops.row_segment_sum(idx, vals, rows)
        acf_ops.sparse_adagrad_apply(W, acc, uq, g, hp.lr)
    _close(dP, deltas[0], kd, "delta_P")
    _close(dQ, deltas[1], kd, "delta_Q")
    for g, w, name in zip((tP, tQ, taP, taQ, lc, la), want, R.COMPOSE_NAMES):
        _close(g, w, k, name)


@pytest.mark.parametrize("d", R.D_COMPOSE)
def test_bpr_apr_step_at_the_new_geometries(acf_ops, oracle, dev, d):
    P, Q, u, i, j = R.compose_problem(d)
    want, _, k, _ = R.compose_reference(oracle, d, _few_step_scale)
    tP, tQ, tu, ti, tj = (_t(a, dev) for a in (P, Q, u, i, j))
    taP, taQ = torch.full_like(tP, 0.1), torch.full_like(tQ, 0.1)
    loss_c, loss_a, n_corr = acf_ops.bpr_apr_step(tP, tQ, taP, taQ, tu, ti, tj)
    for g, w, name in zip((tP, tQ, taP, taQ), want, R.COMPOSE_NAMES):
        _close(g, w, k, name)
    for g, w, name in ((loss_c, want[4], "loss_clean"), (loss_a, want[5], "loss_adv")):
        s = float(w.astype(np.float64).sum())
        assert abs(float(g) - s) <= k * (ATOL + RTOL * abs(s)), name
    # the oracle's count, up to the scores whose sign the dot products' error bound leaves open
    x, ax = sf.scores64(P.astype(np.float64), Q.astype(np.float64), u, i, j, 0, -80.0, 1e8)[:2]
    unsure = int(((np.abs(x) <= d * U * ax) & (i != j)).sum())
    bc = oracle.bpr_forward(P.copy(), Q.copy(), u, i, j, R.B_COMPOSE)[1]
    assert abs(int(n_corr) - int(bc[0])) <= unsure


# ---------------------------------------------------------------------------
# rejections: no kernel runs, the tables keep their bits
def test_bad_shapes_are_rejected_before_any_launch(acf_ops, dev):
    W, acc, idx, g = R.adagrad_fixture(8, 7)
    ok_idx = _t(idx, dev)
    tri = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    for d in (6, 1028):
        tW, tA = torch.ones(R.U1, d, device=dev), torch.full((R.U1, d), 0.5, device=dev)
        rows = torch.ones(7, d, device=dev)
        with pytest.raises(RuntimeError):
            acf_ops.gather_bpr_fwd_bwd(tW, tW, tri, tri, tri)
        with pytest.raises(RuntimeError):
            acf_ops.row_segment_sum(ok_idx, rows, R.U1)
        with pytest.raises(RuntimeError):
            acf_ops.l2norm_perturb(rows, 0.5)
        with pytest.raises(RuntimeError):
            acf_ops.sparse_adagrad_apply(tW, tA, ok_idx, rows, 0.05)
        torch.cuda.synchronize()
        assert bool((tW == 1).all()) and bool((tA == 0.5).all())
    tW, tA, tg = _t(W, dev), _t(acc, dev), _t(g, dev)
    wide = torch.ones(7, 16, device=dev)
    with pytest.raises(RuntimeError):  # a non-contiguous vals
        acf_ops.row_segment_sum(ok_idx, wide[:, :8], R.U1)
    with pytest.raises(RuntimeError):  # a float64 table
        acf_ops.gather_bpr_fwd_bwd(tW.double(), tW.double(), tri, tri, tri)
    with pytest.raises(RuntimeError):
        acf_ops.sparse_adagrad_apply(tW.double(), tA.double(), ok_idx, tg.double(), 0.05)
    with pytest.raises(RuntimeError):
        acf_ops.sparse_adagrad_apply(tW, tA.double(), ok_idx, tg, 0.05)
    with pytest.raises(RuntimeError):
        acf_ops.l2norm_perturb(tg.double(), 0.5)
    with pytest.raises(RuntimeError):  # g_rows narrower and wider than W
        acf_ops.sparse_adagrad_apply(tW, tA, ok_idx, wide[:, :4].contiguous(), 0.05)
    with pytest.raises(RuntimeError):
        acf_ops.sparse_adagrad_apply(tW, tA, ok_idx, wide, 0.05)
    with pytest.raises(RuntimeError):  # fewer rows than indices
        acf_ops.sparse_adagrad_apply(tW, tA, ok_idx, tg[:6].contiguous(), 0.05)
    torch.cuda.synchronize()
    assert torch.equal(tW, _t(W, dev)) and torch.equal(tA, _t(acc, dev))
