"""The APR training step at every dispatched row geometry (LPR, NV).

A table row of d floats is held by LPR lanes with NV float4 chunks each
(geometry() in csrc/acf_host.h): LPR the smallest power of two >= d/4, at most
64; NV = ceil(d/4 / LPR).  test_gpu_parity.py runs the step only where d/4 is a
power of two, so it never runs <1,1>, <64,3>, <64,4>, nor a padded geometry:
one where some lanes of a row-group own no chunk (c * 4 >= d) and must add
exact zeros to the row sums and stay out of every store.  This file runs the
step tests of test_gpu_parity.py at

    D = [4, 12, 20, 48, 100, 132, 260, 516, 768, 772, 1024]

with tiny problems: the row geometry is under test, not the problem size.  The
bars are those of test_gpu_parity.py (rtol 1e-5 / atol 1e-6 for a few steps,
fp32_parity for hot shapes, the Higham-scaled rtol for sums of many terms).
<2,1> is reachable at d = 8 only and stays with test_gpu_parity.py; the CPU
guard at the end of this file checks that the two files cover the dispatch
table between them.
"""
import numpy as np
import pytest
import torch

import test_gpu_parity as parity
from apr_oracle import HParams
from test_gpu_parity import (ATOL, RTOL, _close, _fused_fraction, _gpu_tables, _oracle_run, _problem,
                             _sparse_stream)

gpu = pytest.mark.gpu

D = [4, 12, 20, 48, 100, 132, 260, 516, 768, 772, 1024]
D_STREAM = [4, 12, 20, 48, 100, 132, 252]  # 252: the largest padded d with one chunk per lane
NAMES = ("P", "Q", "accP", "accQ")


def _geometry(d):
    """geometry() of csrc/acf_host.h."""
    d4 = d // 4
    lpr = 1
    while lpr < d4 and lpr < 64:
        lpr <<= 1
    return lpr, (d4 + lpr - 1) // lpr


def _dev_triplets(u, i, j, dev):
    return tuple(torch.tensor(x, device=dev) for x in (u, i, j))


def _step64(P, Q, aP, aQ, u, i, j, adver, eps=0.5, lr=0.05, reg_adv=1.0, lo=-80.0, hi=1e8):
    """One batch of the step in float64 (reg = 0, gradient-mode delta, the
    defaults of HParams): the graph of oracle/apr_oracle.py:tf_graph_step with no
    fp32 rounding, so the order of its sums does not matter."""
    p, qi, qj = P[u], Q[i], Q[j]
    x = (p * qi).sum(1) - (p * qj).sum(1)
    r = np.clip(x, lo, hi)
    lc = np.logaddexp(0, -r)
    g = -1 / (np.exp(r) + 1) * ((x >= lo) & (x <= hi))
    GP, GQ = np.zeros_like(P), np.zeros_like(Q)
    for G, rows, v in ((GP, u, g[:, None] * qi), (GQ, i, g[:, None] * p), (GP, u, -g[:, None] * qj),
                       (GQ, j, -g[:, None] * p)):
        np.add.at(G, rows, v)
    la = np.zeros_like(lc)
    if adver:
        dP, dQ = (G / np.sqrt(np.maximum((G * G).sum(1, keepdims=True), 1e-12)) * eps for G in (GP, GQ))
        pa, qia, qja = p + dP[u], qi + dQ[i], qj + dQ[j]
        xa = (pa * qia).sum(1) - (pa * qja).sum(1)
        ra = np.clip(xa, lo, hi)
        la = np.logaddexp(0, -ra)
        ga = -reg_adv / (np.exp(ra) + 1) * ((xa >= lo) & (xa <= hi))
        for G, rows, v in ((GP, u, ga[:, None] * qia), (GQ, i, ga[:, None] * pa), (GP, u, -ga[:, None] * qja),
                           (GQ, j, -ga[:, None] * pa)):
            np.add.at(G, rows, v)
    for W, A, G, rows in ((P, aP, GP, np.unique(u)), (Q, aQ, GQ, np.unique(np.concatenate([i, j])))):
        A[rows] += G[rows] ** 2
        W[rows] -= lr * G[rows] / np.sqrt(A[rows])
    return lc, la


def _run64(P, Q, u, i, j, B, adver):
    """(P, Q, accP, accQ, loss_clean, loss_adv) of _oracle_run's batches in float64."""
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    aP, aQ = (np.full(x.shape, np.float64(np.float32(0.1))) for x in (P, Q))
    ls = [_step64(P, Q, aP, aQ, u[t:t + B], i[t:t + B], j[t:t + B], adver) for t in range(0, len(u), B)]
    return [P, Q, aP, aQ, np.concatenate([x[0] for x in ls]), np.concatenate([x[1] for x in ls])]


def _few_step_scale(oracle_out, f64_out):
    """k of a few-step case: its bar is |got - want| <= k (ATOL + RTOL |want|).
    k = 1, the project's bar, where the fp32 oracle itself holds that bar against
    float64 on every table and loss of the case; otherwise the reference cannot
    tell a right kernel from a wrong one at 1e-5, and k = 4x the oracle's own
    largest distance from float64 in units of the bar (the convention of
    tests/neumf_ref.py).  From the reference alone, never from the kernels."""
    r = max(float((np.abs(o.astype(np.float64) - w) / (ATOL + RTOL * np.abs(w))).max())
            for o, w in zip(oracle_out, f64_out))
    return 1.0 if r <= 1.0 else 4.0 * r


def _outliers(got, want):
    """fp32_parity's count: elements outside rtol 1e-5 / atol 1e-6."""
    return int((np.abs(got.astype(np.float64) - want) > ATOL + RTOL * np.abs(want)).sum())


def _parity_allowance(oracle_tabs, f64_tabs):
    """Elements fp32_parity lets lie outside 1e-5 in a table of a hot case:
    None = its own max(2, 1e-5 size), where the fp32 oracle holds that against
    float64 on all four tables; otherwise 4x the oracle's own largest count."""
    n = max(_outliers(o, w) for o, w in zip(oracle_tabs, f64_tabs))
    return None if n <= max(2, int(1e-5 * oracle_tabs[0].size)) else 4 * n


def _hot_rtol(u, i, j):
    n_terms = max(2 * np.bincount(u).max(), np.bincount(np.concatenate([i, j])).max())
    return max(RTOL, 2 * n_terms * 2.0 ** -24)  # Higham bound, as test_single_step_strict


def _hot_loss_scale(oracle, P, Q, u, i, j, B, adver, lc_w, la_w, f64_losses):
    """k of a hot case's loss bar |got - want| <= k (ATOL + rtol |want|), rtol the
    Higham-scaled one: 1 where the fp32 oracle holds that bar against float64 AND
    against itself with its sums reordered (four seeded reorderings: the table
    columns permuted, which reorders every dot product, and the triplets
    permuted inside each batch, which reorders every row's sum over its
    occurrences; neither changes the result in exact arithmetic); otherwise 4x
    the largest of those distances.  The bound counts the terms of a row's sum
    over its occurrences, not the d products of a dot."""
    rtol = _hot_rtol(u, i, j)

    def dist(got, want):
        return float((np.abs(got.astype(np.float64) - want) / (ATOL + rtol * np.abs(want))).max())
    r = max(dist(lc_w, f64_losses[0]), dist(la_w, f64_losses[1]))
    rng = np.random.default_rng(0)
    for _ in range(4):
        cols = rng.permutation(P.shape[1])
        tp = np.concatenate([t + rng.permutation(B) for t in range(0, len(u), B)])
        _, lc2, la2, _ = _oracle_run(oracle, np.ascontiguousarray(P[:, cols]), np.ascontiguousarray(Q[:, cols]),
                                     u[tp], i[tp], j[tp], B, HParams(adver=adver))
        inv = np.argsort(tp)
        r = max(r, dist(lc2[inv], lc_w), dist(la2[inv], la_w))
    return 1.0 if r <= 1.0 else 4.0 * r


_refs = {}


def _reference(oracle, d, adver):
    """The 61 x 47, B = 64, nb = 4 problem of tests 1 and 2, its oracle run and
    the scale k of its bar (_few_step_scale), computed once per (d, adver)."""
    key = (d, adver)
    if key not in _refs:
        U1, I1, B, nb = 61, 47, 64, 4
        P, Q, u, i, j = _problem(d * 10 + adver, U1, I1, d, B, nb, dup_items=True)
        want, lc_w, la_w, _ = _oracle_run(oracle, P, Q, u, i, j, B, HParams(adver=adver))
        k = _few_step_scale(list(want) + [lc_w, la_w], _run64(P, Q, u, i, j, B, adver))
        for x in (P, Q, u, i, j, lc_w, la_w) + tuple(want):
            x.setflags(write=False)
        _refs[key] = (U1, I1, B, nb, P, Q, u, i, j, (want, k), lc_w, la_w)
    return _refs[key]


def _check_step(ctx, tabs, want_k, lc_w, la_w, adver):
    want, k = want_k
    lc, la = ctx.losses()
    torch.cuda.synchronize()
    assert ctx.step_errors() == 0
    if k > 1:
        print(f"bar scaled by {k:.1f}: 4x the fp32 oracle's distance from float64")
    got = list(tabs) + [lc] + [la] * bool(adver)
    for g, w, n in zip(got, list(want) + [lc_w, la_w], NAMES + ("loss_clean", "loss_adv")):
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=k * RTOL, atol=k * ATOL, err_msg=n)


# ---------------------------------------------------------------------------
# 1. the two-kernel step vs the oracle at every geometry
@gpu
@pytest.mark.parametrize("mapping", ["wave", "group"])
@pytest.mark.parametrize("adver", [0, 1])
@pytest.mark.parametrize("d,graph", [(d, False) for d in D] + [(20, True), (772, True)])
def test_step_matches_oracle_at_every_geometry(ops, oracle, dev, d, graph, adver, mapping):
    """test_train_planned_matches_oracle at D, on the two-kernel schedule
    (set_stream(False)): one wave per row ("wave": k_clean / k_adv with a team of
    64 / LPR lane-groups) and one lane-group per row ("group": the hash plan's
    k_tri_* kernels).  Tables, Adagrad accumulators and both losses.

    d = 1024 with adver = 1 is held to 25.6x the bar (_few_step_scale): there the
    fp32 oracle, which sums a row's 1,024 products one after the other, is itself
    6.4 bars from float64 (P 6.2, Q 5.3, accP 4.3, accQ 6.4, loss_adv 2.9; 35 to
    190 elements per table), and the kernels are 5.3 bars from the oracle in Q
    (35 elements, all in two rows), 6.4 in accQ, 2.0 in accP, 2.9 in loss_adv,
    while 0.4 (Q) and 0.9 (accQ) from float64.  Every other case: k = 1."""
    U1, I1, B, nb, P, Q, u, i, j, want, lc_w, la_w = _reference(oracle, d, adver)
    tabs = _gpu_tables(P, Q, dev)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_slot_mapping(mapping)
    ctx.set_stream(False)
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    if mapping == "group":
        assert ctx.plan_kind() == "hash"  # triplet-centric: the case runs k_tri_*
    ctx.train_planned(tabs, ops.StepHParams(adver=adver), graph=graph)
    _check_step(ctx, tabs, want, lc_w, la_w, adver)


# ---------------------------------------------------------------------------
# 2. one lane-group per row without fusion, and the sort-planned triplet path
@gpu
@pytest.mark.parametrize("d", [12, 100, 260, 772])
def test_packed_slot_kernels_without_fusion(ops, oracle, dev, d):
    """k_clean / k_adv with TEAM = 1 (mapping "group", fusion off before the
    plan: 64 / LPR rows per wave, the sort plan) vs the oracle."""
    U1, I1, B, nb, P, Q, u, i, j, want, lc_w, la_w = _reference(oracle, d, 1)
    tabs = _gpu_tables(P, Q, dev)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_slot_mapping("group")
    ctx.set_fusion(False)
    ctx.set_stream(False)
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    assert ctx.plan_kind() == "sort"
    ctx.train_planned(tabs, ops.StepHParams(adver=1), graph=False)
    _check_step(ctx, tabs, want, lc_w, la_w, 1)


@gpu
@pytest.mark.parametrize("d", [20, 516])
def test_sort_planned_triplet_path(ops, oracle, dev, d):
    """Mapping "group" with fusion on and set_plan_mode("sort"): the triplet
    path on the device-wide sort plan instead of the hash plan."""
    U1, I1, B, nb, P, Q, u, i, j, want, lc_w, la_w = _reference(oracle, d, 1)
    tabs = _gpu_tables(P, Q, dev)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_slot_mapping("group")
    ctx.set_plan_mode("sort")
    ctx.set_stream(False)
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    assert ctx.plan_kind() == "sort"
    ctx.train_planned(tabs, ops.StepHParams(adver=1), graph=False)
    _check_step(ctx, tabs, want, lc_w, la_w, 1)


# ---------------------------------------------------------------------------
# 3. delta and split calls
@gpu
@pytest.mark.parametrize("reg", [0.0, 0.01])
@pytest.mark.parametrize("d", [12, 100, 260, 1024])
def test_split_calls_and_delta_at_padded_geometries(ops, oracle, dev, reg, d):
    """test_split_calls_and_delta_match_oracle: delta_update, delta_tables,
    optimizer_step batch by batch.  Each delta table equals the oracle's and is
    exactly zero outside the rows its batch touches."""
    U1, I1, B, nb = 61, 47, 48, 3
    P, Q, u, i, j = _problem(5 + d, U1, I1, d, B, nb)
    want, _, _, deltas = _oracle_run(oracle, P, Q, u, i, j, B, HParams(adver=1, reg=reg))
    tabs = _gpu_tables(P, Q, dev)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    hp = ops.StepHParams(adver=1, reg=reg)
    for t in range(nb):
        s = slice(t * B, (t + 1) * B)
        ctx.delta_update(tabs, hp, t)
        dP, dQ = ctx.delta_tables()
        _close(dP, deltas[t][0], f"delta_P batch {t}")
        _close(dQ, deltas[t][1], f"delta_Q batch {t}")
        idle_u = np.setdiff1d(np.arange(U1), u[s])
        idle_i = np.setdiff1d(np.arange(I1), np.concatenate([i[s], j[s]]))
        assert len(idle_u) and len(idle_i)
        assert float(dP[torch.tensor(idle_u, device=dev)].abs().max()) == 0.0
        assert float(dQ[torch.tensor(idle_i, device=dev)].abs().max()) == 0.0
        ctx.optimizer_step(tabs, hp, t)
    for g, w, n in zip(tabs, want, NAMES):
        _close(g, w, n)
    assert ctx.step_errors() == 0


# ---------------------------------------------------------------------------
# 4. random delta
@gpu
@pytest.mark.parametrize("stream", [False, True])
@pytest.mark.parametrize("d", [12, 132, 260])
def test_random_delta_at_padded_geometries(ops, oracle, dev, stream, d):
    """test_random_delta_matches_oracle and the norm check of
    test_random_delta_has_norm_eps.  random_delta zeroes the elements past d, so
    a padded lane that drew noise would change the row's norm: every touched
    delta row has norm eps, every other row is zero."""
    U1, I1, B, nb = 50, 90, 64, 4
    P, Q, u, i, j = _problem(8 + d, U1, I1, d, B, nb, dup_items=True)
    hp = ops.StepHParams(adver=1, adv="random", seed=77)
    tri = _dev_triplets(u, i, j, dev)
    # split calls, batch 0: delta tables
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.plan(*tri, B)
    tabs = _gpu_tables(P, Q, dev)
    ctx.delta_update(tabs, hp, 0)
    dP, dQ = ctx.delta_tables()
    rP, rQ = P.copy(), Q.copy()
    aP, aQ = np.full(P.shape, 0.1, np.float32), np.full(Q.shape, 0.1, np.float32)
    _, _, wdP, wdQ = oracle.apr_batch(rP, rQ, aP, aQ, u[:B], i[:B], j[:B],
                                      HParams(adver=1, adv="random", seed=77, call=1, t=0), want_delta=True)
    _close(dP, wdP, "random delta_P")
    _close(dQ, wdQ, "random delta_Q")
    for delta, rows, N in ((dP, np.unique(u[:B]), U1), (dQ, np.unique(np.concatenate([i[:B], j[:B]])), I1)):
        norms = torch.linalg.vector_norm(delta[torch.tensor(rows, device=dev)], dim=1).cpu().numpy()
        np.testing.assert_allclose(norms, hp.eps, rtol=1e-5)
        idle = np.setdiff1d(np.arange(N), rows)
        assert len(idle) and float(delta[torch.tensor(idle, device=dev)].abs().max()) == 0.0
    # whole calls: a fresh context, two calls over the same 4 batches (call counter 1, then 2)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_stream(stream)
    ctx.plan(*tri, B)
    tabs = _gpu_tables(P, Q, dev)
    rP, rQ = P.copy(), Q.copy()
    aP, aQ = np.full(P.shape, 0.1, np.float32), np.full(Q.shape, 0.1, np.float32)
    for call in (1, 2):
        ctx.train_planned(tabs, hp)
        oracle.apr_train(rP, rQ, aP, aQ, u, i, j, B, HParams(adver=1, adv="random", seed=77, call=call))
        for g, w, n in zip(tabs, (rP, rQ, aP, aQ), NAMES):
            _close(g, w, f"call {call} {n}")
    assert ctx.step_errors() == 0 and ctx.stream_recoveries() == 0


# ---------------------------------------------------------------------------
# 5. the streamed step, bit for bit, and it really streamed
def _stream_problem(shape, d):
    B, nb = {"hot": (64, 12), "sparse": (256, 8)}[shape]
    if shape == "hot":  # rows recur inside and across batches
        rng = np.random.default_rng(d + 3)
        U1, I1 = 40, 30
        u, i, j = (rng.integers(0, N, nb * B).astype(np.int32) for N in (U1, I1, I1))
    else:  # mostly fused triplets, in-place rows, a hot set
        U1, I1 = 6000, 5000
        u, i, j = _sparse_stream(d + 3, U1, I1, B, nb)
    rng = np.random.default_rng(d)
    P = (rng.standard_normal((U1, d)) * 0.2).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.2).astype(np.float32)
    return U1, I1, B, nb, P, Q, u, i, j


@gpu
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("shape", ["hot", "sparse"])
@pytest.mark.parametrize("d", D_STREAM)
def test_stream_bit_identical_at_padded_geometries(ops, dev, d, shape, fuse):
    """test_stream_bit_identical_to_two_kernels where d/4 is no power of two: a
    version row is component-major with stride d/4 (element 4c + e at granule
    e * d/4 + c), and a padded lane's check feeds a wave-wide vote.  A slip there
    does not change the result: the wait gives up and the call is replayed on
    the two-kernel schedule.  So beyond equal bits this asserts that no call was
    replayed and that the plan's launch sequence holds a k_stream launch."""
    U1, I1, B, nb, P, Q, u, i, j = _stream_problem(shape, d)
    hp = ops.StepHParams(adver=1, reg=0.01, seed=5)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_fusion(fuse)
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    whole, split = [(0, nb)], [(0, 1), (1, 2), (3, 4), (7, nb - 7)]
    if d in (20, 132):
        matrix = ((False, whole, True), (False, whole, False), (False, split, True), (True, whole, True),
                  (True, whole, False), (True, split, True), (True, split, False))
    else:
        matrix = ((False, whole, True), (True, whole, False), (True, split, True))
    runs = []
    for stream, pieces, graph in matrix:
        ctx.set_stream(stream)
        tabs = _gpu_tables(P, Q, dev)
        for first, n in pieces:
            ctx.train_planned(tabs, hp, first, n, graph=graph)
        lc, la = ctx.losses()
        runs.append(tabs + [lc.clone(), la.clone()])
        assert ctx.step_errors() == 0
    ctx.set_stream(True)
    tabs = _gpu_tables(P, Q, dev)
    kinds = {k: v[1] for k, v in ctx.time_kernels(tabs, hp).items()}  # trains as train_planned does
    lc, la = ctx.losses()
    runs.append(tabs + [lc.clone(), la.clone()])
    torch.cuda.synchronize()
    assert kinds["stream"] > 0 and kinds["clean"] == 0 and kinds["adv"] == 0, kinds
    assert ctx.step_errors() == 0
    assert ctx.stream_recoveries() == 0
    names = NAMES + ("loss_clean", "loss_adv")
    for k, other in enumerate(runs[1:]):
        for x, y, n in zip(runs[0], other, names):
            assert torch.equal(x, y), (k, n)


@gpu
def test_two_chunk_rows_fall_back_to_two_kernels(ops, oracle, dev):
    """d = 260 (two chunks in lane 0, one in lanes 1-63): k_stream holds one
    chunk per lane, so a context with streamed steps on runs the two-kernel
    schedule, and says so; the result equals the oracle."""
    d = 260
    U1, I1, B, nb, P, Q, u, i, j, want, lc_w, la_w = _reference(oracle, d, 1)
    hp = ops.StepHParams(adver=1)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_stream(True)
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    tabs = _gpu_tables(P, Q, dev)
    kinds = {k: v[1] for k, v in ctx.time_kernels(tabs, hp).items()}
    assert kinds["stream"] == 0 and kinds["clean"] == nb and kinds["adv"] == nb, kinds
    assert want[1] == 1  # the oracle holds the project's bar at d = 260
    for g, w, n in zip(tabs, want[0], NAMES):
        _close(g, w, f"time_kernels {n}")
    tabs = _gpu_tables(P, Q, dev)
    ctx.train_planned(tabs, hp)
    _check_step(ctx, tabs, want, lc_w, la_w, 1)
    assert ctx.stream_recoveries() == 0


# ---------------------------------------------------------------------------
# 6. fusion on vs off, bit for bit
@gpu
@pytest.mark.parametrize("d", [12, 100, 260, 772])
@pytest.mark.parametrize("adv", ["grad", "random"])
@pytest.mark.parametrize("mapping", ["wave", "group"])
def test_fused_triplets_bit_identical_at_padded_geometries(ops, dev, d, adv, mapping):
    """test_fused_triplets_bit_identical_to_slot_path on 1500 x 1200 tables,
    B = 128, nb = 4 (more than half of the triplets fused): fusion on vs off,
    one call and piecewise calls, identical bits."""
    U1, I1, B, nb = 1500, 1200, 128, 4
    u, i, j = _sparse_stream(d + 1, U1, I1, B, nb)
    assert _fused_fraction(u, i, j, B) > 0.5
    rng = np.random.default_rng(d)
    P = (rng.standard_normal((U1, d)) * 0.2).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.2).astype(np.float32)
    hp = ops.StepHParams(adver=1, adv=adv, reg=0.01, seed=5)
    tri = _dev_triplets(u, i, j, dev)
    runs = []
    # "random" draws fresh noise every call: piecewise calls only in gradient mode
    cases = ((False, [(0, nb)]), (True, [(0, nb)])) + ((True, [(0, 1), (1, 2), (3, 1)]),) * (adv == "grad")
    for fuse, pieces in cases:
        ctx = ops.APRContext(U1, I1, d, B, nb, dev)
        ctx.set_slot_mapping(mapping)
        ctx.set_fusion(fuse)  # before the plan: a triplet-centric plan updates rows in place
        ctx.plan(*tri, B)
        tabs = _gpu_tables(P, Q, dev)
        for first, n in pieces:
            ctx.train_planned(tabs, hp, first, n, graph=first == 0)
        lc, la = ctx.losses()
        assert ctx.step_errors() == 0
        runs.append(tabs + [lc.clone(), la.clone()])
    torch.cuda.synchronize()
    for other in runs[1:]:
        for x, y, n in zip(runs[0], other, NAMES + ("loss_clean", "loss_adv")):
            assert torch.equal(x, y), n


# ---------------------------------------------------------------------------
# 7. hot slots at small scale
def _hot_problem(d, adver):
    U1, I1, B, nb = 12, 9, 256, 2
    P, Q, u, i, j = _problem(23 + d + adver, U1, I1, d, B, nb)
    for t in range(nb):  # every row of both tables is a hot slot (> ACF_HOT_MIN = 8 occurrences) in every batch
        s = slice(t * B, (t + 1) * B)
        assert np.bincount(u[s], minlength=U1).min() > 8
        assert np.bincount(np.concatenate([i[s], j[s]]), minlength=I1).min() > 8
    return U1, I1, B, nb, P, Q, u, i, j


def _hot_reference(oracle, d, adver):
    """_hot_problem, its oracle run and _parity_allowance, once per (d, adver)."""
    key = ("hot", d, adver)
    if key not in _refs:
        U1, I1, B, nb, P, Q, u, i, j = _hot_problem(d, adver)
        want, lc_w, la_w, _ = _oracle_run(oracle, P, Q, u, i, j, B, HParams(adver=adver))
        f64 = _run64(P, Q, u, i, j, B, adver)
        allow = (_parity_allowance(want, f64[:4]),
                 _hot_loss_scale(oracle, P, Q, u, i, j, B, adver, lc_w, la_w, f64[4:]))
        for x in (P, Q, u, i, j, lc_w, la_w) + tuple(want):
            x.setflags(write=False)
        _refs[key] = (U1, I1, B, nb, P, Q, u, i, j, want, lc_w, la_w, allow)
    return _refs[key]


def _check_hot(ctx, tabs, want, lc_w, la_w, allow, u, i, j, adver, fp32_parity):
    allow, k = allow
    lc, la = ctx.losses()
    torch.cuda.synchronize()
    assert ctx.step_errors() == 0
    for g, w, n in zip(tabs, want, NAMES):
        if allow is None:
            fp32_parity(g, w, n)
            continue
        # fp32_parity with the count the reference's own error sets (_parity_allowance)
        g = g.cpu().numpy()
        err = np.abs(g.astype(np.float64) - w)
        assert float(err.max()) <= 1e-5 * max(1.0, float(np.abs(w).max())), f"{n}: max abs diff {err.max():.3e}"
        print(f"{n}: {_outliers(g, w)} elements outside 1e-5, {allow} allowed: 4x the fp32 oracle's count vs float64")
        assert _outliers(g, w) <= allow, f"{n}: {_outliers(g, w)} of {w.size} elements outside 1e-5, {allow} allowed"
    rtol = _hot_rtol(u, i, j)
    if k > 1:
        print(f"loss bar scaled by {k:.1f}: 4x the fp32 oracle's distance from itself reordered / float64")
    np.testing.assert_allclose(lc.cpu().numpy(), lc_w, rtol=k * rtol, atol=k * ATOL, err_msg="loss_clean")
    if adver:
        np.testing.assert_allclose(la.cpu().numpy(), la_w, rtol=k * rtol, atol=k * ATOL, err_msg="loss_adv")


@gpu
@pytest.mark.parametrize("adver", [0, 1])
@pytest.mark.parametrize("d", [12, 100, 260, 516, 772])
def test_hot_slots_at_padded_geometries(ops, oracle, dev, d, adver, fp32_parity):
    """12 x 9 tables, B = 256: every slot has well over ACF_HOT_MIN occurrences,
    so every row is summed as pieces plus a combine of the pieces (the
    red[NV * 256] reductions of k_tri_combine / k_tri_cadv).  Tables at
    fp32_parity, losses at the Higham-scaled rtol, and the combine really ran.

    fp32_parity lets 2 elements of a table lie outside 1e-5.  With 6,192 and
    9,264 elements per table the fp32 oracle itself has more than that outside
    1e-5 of float64: 3 at (d, adver) = (516, 1), 9 at (772, 0), 21 at (772, 1);
    those cases allow 4x that (_parity_allowance: 12, 36, 84).  Measured there:
    5, 6 and 20 (25 with one wave per row) against the oracle, none against
    float64.  The largest difference stays under fp32_parity's 1e-5 throughout.

    Losses at (772, 1): the Higham rtol counts a row's occurrences (129 terms,
    1.54e-5), not the 772 products of each dot.  The oracle moves by 1.32 bars in
    loss_adv when its own sums are reordered and is 0.98 bars from float64; the
    kernels are 1.06 bars from the oracle (one element of 512, one wave per row)
    and 0.18 from float64.  That case's loss bar is 4x 1.32 (_hot_loss_scale);
    every other case keeps the Higham bar."""
    U1, I1, B, nb, P, Q, u, i, j, want, lc_w, la_w, allow = _hot_reference(oracle, d, adver)
    tabs = _gpu_tables(P, Q, dev)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_slot_mapping("group")
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    assert ctx.plan_kind() == "hash"
    t = ctx.time_kernels(tabs, ops.StepHParams(adver=adver))
    assert t["hot"][1] > 0
    _check_hot(ctx, tabs, want, lc_w, la_w, allow, u, i, j, adver, fp32_parity)


@gpu
@pytest.mark.parametrize("d", [20, 772])
def test_hot_rows_one_wave_per_row_at_padded_geometries(ops, oracle, dev, d, fp32_parity):
    """The same shape with one wave per row: overflow records, many rounds per
    wave (test_hot_rows_many_occurrences)."""
    U1, I1, B, nb, P, Q, u, i, j, want, lc_w, la_w, allow = _hot_reference(oracle, d, 1)
    tabs = _gpu_tables(P, Q, dev)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_slot_mapping("wave")
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    ctx.train_planned(tabs, ops.StepHParams(adver=1))
    _check_hot(ctx, tabs, want, lc_w, la_w, allow, u, i, j, 1, fp32_parity)


# ---------------------------------------------------------------------------
# 8. degenerate batches
@gpu
@pytest.mark.parametrize("stream", [False, True])
@pytest.mark.parametrize("case", ["one_per_batch", "identical", "edge_rows"])
@pytest.mark.parametrize("d", [12, 260])
def test_degenerate_batches_at_padded_geometries(ops, oracle, dev, d, case, stream):
    """The one_per_batch, identical and edge_rows cases of
    test_degenerate_batches_match_oracle, with its bars."""
    U1, I1 = 37, 29
    rng = np.random.default_rng(len(case) + d)
    if case == "one_per_batch":
        B, nb = 1, 6
        u, i, j = rng.integers(0, U1, nb), rng.integers(0, I1, nb), rng.integers(0, I1, nb)
    elif case == "identical":
        B, nb = 256, 3
        u = np.full(nb * B, 3)
        i = np.full(nb * B, 5)
        j = np.full(nb * B, 7)
        j[:B] = 5
    else:
        B, nb = 64, 4
        u = rng.choice([0, U1 - 1], nb * B)
        i, j = rng.choice([0, I1 - 1], nb * B), rng.choice([0, I1 - 1], nb * B)
    u, i, j = (x.astype(np.int32) for x in (u, i, j))
    P = (rng.standard_normal((U1, d)) * 0.3).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.3).astype(np.float32)
    want, lc_w, la_w, _ = _oracle_run(oracle, P, Q, u, i, j, B, HParams(adver=1))
    tabs = _gpu_tables(P, Q, dev)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_stream(stream)
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    ctx.train_planned(tabs, ops.StepHParams(adver=1))
    lc, la = ctx.losses()
    torch.cuda.synchronize()
    assert ctx.step_errors() == 0 and ctx.stream_recoveries() == 0
    # a row's sum over n occurrences in another order: Higham's bound 2 n u, relative to the row's scale
    n_terms = max(2 * np.bincount(u[:B]).max(), np.bincount(np.concatenate([i[:B], j[:B]])).max())
    rtol = max(RTOL, 2 * n_terms * 2.0 ** -24)
    for g, w, n in zip(tabs, want, NAMES):
        atol = max(ATOL, rtol * float(np.abs(w).max()))
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=rtol, atol=atol, err_msg=n)
    np.testing.assert_allclose(lc.cpu().numpy(), lc_w, rtol=rtol, atol=ATOL)
    np.testing.assert_allclose(la.cpu().numpy(), la_w, rtol=rtol, atol=ATOL)


# ---------------------------------------------------------------------------
# 9. the launch sequence of the triplet-centric schedule
def _tri_problem(seed, U1, I1, d, B, nb):
    u, i, j = _sparse_stream(seed, U1, I1, B, nb, hot=16, p_hot=0.3)  # some slots exceed 8 occurrences
    rng = np.random.default_rng(d)
    P = (rng.standard_normal((U1, d)) * 0.2).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.2).astype(np.float32)
    return P, Q, u, i, j


def _bits(ctx, tabs):
    lc, la = ctx.losses()
    assert ctx.step_errors() == 0
    return tabs + [lc.clone(), la.clone()]


def _same_bits(base, other, what):
    torch.cuda.synchronize()
    for x, y, n in zip(base, other, NAMES + ("loss_clean", "loss_adv")):
        assert torch.equal(x, y), (what, n)


@gpu
@pytest.mark.parametrize("adver", [1, 0])
@pytest.mark.parametrize("d", [64, 20])
def test_sort_plan_triplet_launch_sequence(ops, dev, d, adver):
    """Mapping "group", B = 128, fusion on, set_plan_mode("sort") (left to
    itself the context builds a hash plan here too): a triplet-centric sort
    plan.  Per batch a triplet pass and a combine per phase (APR: two phases),
    one flush per call, no streamed launch; time_kernels, train_planned and the
    two-phase API batch by batch leave the same bits."""
    U1, I1, B, nb = 300, 200, 128, 3
    P, Q, u, i, j = _tri_problem(d + 9, U1, I1, d, B, nb)
    assert max(np.bincount(np.concatenate([i[t * B:(t + 1) * B], j[t * B:(t + 1) * B]])).max() for t in range(nb)) > 8
    hp = ops.StepHParams(adver=adver, reg=0.01)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.set_slot_mapping("group")
    ctx.set_plan_mode("sort")
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    assert ctx.plan_kind() == "sort"
    tabs = _gpu_tables(P, Q, dev)
    ctx.train_planned(tabs, hp, graph=False)
    base = _bits(ctx, tabs)
    tabs = _gpu_tables(P, Q, dev)
    kinds = {k: v[1] for k, v in ctx.time_kernels(tabs, hp).items()}
    want = ({"clean": nb, "hot": 2 * nb, "adv": nb, "flush": 1, "stream": 0} if adver else
            {"clean": nb, "hot": nb, "adv": 0, "flush": 1, "stream": 0})
    assert kinds == want, kinds
    _same_bits(base, _bits(ctx, tabs), "time_kernels")
    tabs = _gpu_tables(P, Q, dev)
    for t in range(nb):
        if adver:
            ctx.delta_update(tabs, hp, t)
        ctx.optimizer_step(tabs, hp, t)
    _same_bits(base, _bits(ctx, tabs), "two-phase API")


@gpu
def test_hash_plan_triplet_launch_sequence(ops, dev):
    """B = 4,096 (the smallest batch the auto mapping packs), d = 64: a hash
    plan.  A whole step is three launches per batch (k_tri_clean, k_tri_cadv =
    the clean combine + the adversarial pass, the second combine); the two-phase
    API on the same plan runs the four-launch batch and leaves the same bits."""
    U1, I1, d, B, nb = 30000, 20000, 64, 4096, 2
    P, Q, u, i, j = _tri_problem(4096, U1, I1, d, B, nb)
    hp = ops.StepHParams(adver=1, reg=0.01)
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    ctx.plan(*_dev_triplets(u, i, j, dev), B)
    assert ctx.plan_kind() == "hash"
    tabs = _gpu_tables(P, Q, dev)
    ctx.train_planned(tabs, hp, graph=False)
    base = _bits(ctx, tabs)
    tabs = _gpu_tables(P, Q, dev)
    kinds = {k: v[1] for k, v in ctx.time_kernels(tabs, hp).items()}
    assert kinds == {"clean": nb, "adv": nb, "hot": nb, "flush": 1, "stream": 0}, kinds
    _same_bits(base, _bits(ctx, tabs), "time_kernels")
    tabs = _gpu_tables(P, Q, dev)
    for t in range(nb):
        ctx.delta_update(tabs, hp, t)
        ctx.optimizer_step(tabs, hp, t)
    _same_bits(base, _bits(ctx, tabs), "two-phase API")


# ---------------------------------------------------------------------------
# 10. CPU guard: D still covers the dispatch table
def test_calibrated_bars_come_from_the_oracle_alone(oracle):
    """The float64 restatement agrees with the fp32 oracle within the project's
    bar wherever d < 1024, so those cases keep that bar; the two calibrated bars
    (see _few_step_scale, _parity_allowance) are pinned here, without a GPU."""
    for d in D:
        for adver in (0, 1):
            k = _reference(oracle, d, adver)[9][1]
            assert (k == 1.0) == ((d, adver) != (1024, 1)), (d, adver, k)
    assert 4.0 < _reference(oracle, 1024, 1)[9][1] <= 32.0
    for d in (12, 20, 100, 260, 516, 772):
        for adver in (0, 1):
            allow, k = _hot_reference(oracle, d, adver)[-1]
            assert (allow is None) == ((d, adver) not in ((516, 1), (772, 0), (772, 1))), (d, adver, allow)
            assert allow is None or allow <= 100
            assert (k == 1.0) == ((d, adver) != (772, 1)) and k <= 8.0, (d, adver, k)


DISPATCHED = {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4)}  # DISPATCH_GEOM
PADDED = [12, 20, 48, 100, 132, 260, 516, 772]


def _parity_dims(test):
    for m in test.pytestmark:
        if m.name == "parametrize" and m.args[0] == "d":
            return list(m.args[1])
    raise AssertionError("no parametrisation over d")


def test_dims_cover_the_dispatch_table():
    """geometry() restated: D maps onto every instantiation of DISPATCH_GEOM but
    <2,1>, which only d = 8 reaches and test_train_planned_matches_oracle runs
    (both mappings); with it all ten are run against the oracle.  Every padded d
    has idle lanes, and each lane width and each NV >= 2 appears padded."""
    assert all(d % 4 == 0 and 4 <= d <= 1024 for d in D + D_STREAM)
    assert {_geometry(d) for d in range(4, 1025, 4)} == DISPATCHED
    assert [d for d in range(4, 1025, 4) if _geometry(d) == (2, 1)] == [8]
    assert 8 in _parity_dims(parity.test_train_planned_matches_oracle)
    assert {_geometry(d) for d in D} == DISPATCHED - {(2, 1)}
    for d in D:
        lpr, nv = _geometry(d)
        assert (d // 4 < lpr * nv) == (d in PADDED), d
        assert d // 4 > lpr * (nv - 1), d  # the last chunk index is in use
    assert {_geometry(d) for d in PADDED} == {(4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4)}
    assert {_geometry(d) for d in D if d not in PADDED} >= {(1, 1), (64, 3), (64, 4)}
    # the streamed step holds one chunk per lane: every lane width 4-64 with idle lanes, and the full <1,1>
    assert all(_geometry(d)[1] == 1 for d in D_STREAM)
    assert {_geometry(d)[0] for d in D_STREAM if d // 4 < _geometry(d)[0]} == {4, 8, 16, 32, 64}
    assert _geometry(4) == (1, 1) and 4 in D_STREAM
    assert _geometry(252) == (64, 1) and _geometry(256) == (64, 1) and _geometry(260) == (64, 2)
