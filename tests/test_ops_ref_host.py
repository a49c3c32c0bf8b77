"""CPU checks of tests/ops_ref.py: the fixtures of test_gpu_ops_geometry.py and
test_gpu_grid_shapes.py hold what those files rely on, and the references are
sensitive to what the GPU tests are meant to catch.  No GPU."""
import numpy as np
import pytest

import ops_ref as R
import saturation_fixture as sf
from test_gpu_step_geometry import _few_step_scale


def test_dims_reach_the_whole_dispatch_table():
    assert all(d % 4 == 0 and 4 <= d <= 1024 for d in R.D_OPS)
    assert {R.geometry(d) for d in range(4, 1025, 4)} == R.DISPATCHED
    assert {R.geometry(d) for d in R.D_OPS} == R.DISPATCHED  # all ten entries of OPS_GEOM
    padded = [d for d in R.D_OPS if d // 4 < R.geometry(d)[0] * R.geometry(d)[1]]
    assert padded == R.PADDED == [12, 20, 48, 100, 132, 260, 516, 772]
    for d in R.D_OPS:
        lpr, nv = R.geometry(d)
        assert d // 4 > lpr * (nv - 1), d  # the last chunk index is in use
    # every NV >= 2 runs padded, and <64,2> .. <64,4> all run
    assert {R.geometry(d) for d in R.PADDED} >= {(64, 1), (64, 2), (64, 3), (64, 4)}
    assert set(R.SEG_EXTRA_D) <= set(R.PADDED) and {R.geometry(d)[1] for d in R.SEG_EXTRA_D} == {1, 2}
    assert set(R.D_COMPOSE) <= set(R.D_OPS)


def _seg_cases():
    return [("base", d) for d in R.D_OPS] + [(n, d) for d in R.SEG_EXTRA_D for n in R.SEG_EXTRA]


@pytest.mark.parametrize("name,d", _seg_cases())
def test_segment_sum_fixtures_tell_the_order_of_a_sum(name, d):
    """Exponents spread over 2^+-20; wherever a segment has more than two values
    (a + b == b + a), the sum in reversed input order differs in bits: a sort
    that is not stable cannot pass the bit test."""
    idx, vals, rows = R.seg_case(name, d)
    assert vals.shape == (len(idx), d) and vals.dtype == np.float32
    assert not idx.flags.writeable and not vals.flags.writeable
    if len(idx):
        assert 0 <= idx.min() and idx.max() < rows
        e = np.log2(np.abs(vals[vals != 0]))
        assert e.min() < -15 and e.max() > 15
    uq, cnt, fwd = R.segment_sum_exact(idx, vals)
    assert np.array_equal(uq, np.unique(idx)) and cnt.sum() == len(idx)
    if len(idx) and cnt.max() > 2:
        rev = R.segment_sum_exact(idx, vals, reverse=True)[2]
        assert not np.array_equal(fwd.view(np.int32), rev.view(np.int32))
        assert not np.array_equal(fwd[cnt > 2].view(np.int32), rev[cnt > 2].view(np.int32))
    if name.startswith("rows"):
        assert rows - 1 in idx and 0 in idx
    if name == "int64":
        assert idx.dtype == np.int64
    if name == "all_equal":
        assert cnt.tolist() == [5000]
    if name == "all_distinct":
        assert cnt.max() == 1 and len(uq) == 300
    if name == "descending":
        assert (np.diff(idx) <= 0).all() and cnt.max() > 2


def test_segment_sum_cases_are_the_issue_s():
    assert R.SEG_M == (0, 1, 2, 255, 256, 257, 5000)
    assert R.SEG_ROWS == (1, 2, 3, 2 ** 20, 2 ** 20 + 1)
    # a row count just above a power of two needs one more sort bit than the power itself
    for rows in R.SEG_ROWS[3:]:
        idx = R.seg_case(f"rows{rows}", 20)[0]
        assert int(idx.max()).bit_length() == (20 if rows == 2 ** 20 else 21)
        assert np.bincount(idx).max() > 2  # rows recur: a mis-sorted key shows in the sums too


@pytest.mark.parametrize("d", R.D_OPS)
def test_l2norm_fixture_plants_its_rows(d):
    for k in R.L2_K:
        g = R.l2_fixture(d, k)
        assert g.shape == (k, d) and g.dtype == np.float32 and not g.flags.writeable
        ss = (g.astype(np.float64) ** 2).sum(1)
        # no row within the sum's relative error of the floor: the bar leaves no row out
        assert (R.l2_floor_margin(g) > 2 * d * R.U).all()
        if k < 7:
            continue
        assert not g[R.L2_ZERO].any()
        assert 0 < ss[R.L2_TINY] < 1e-14
        assert 1e-12 * (1 - 16 * d * R.U) < ss[R.L2_BELOW] < 1e-12 < ss[R.L2_ABOVE] < 1e-12 * (1 + 16 * d * R.U)
        assert (g[R.L2_OVERFLOW] == np.float32(1e19)).all() and ss[R.L2_OVERFLOW] > R.FLT_MAX
        want = R.l2norm_perturb64(g, 0.5)
        assert not want[R.L2_ZERO].any() and not want[R.L2_OVERFLOW].any()
        np.testing.assert_allclose(want[R.L2_BELOW], g[R.L2_BELOW].astype(np.float64) * 1e6 * 0.5, rtol=1e-15)
        np.testing.assert_allclose(np.linalg.norm(want[R.L2_ABOVE]), 0.5, rtol=1e-12)
        assert np.linalg.norm(want[R.L2_BELOW]) < 0.5 < 0.5 * (1 + 1e-12)


@pytest.mark.parametrize("d", R.D_OPS)
def test_adagrad_fixture(d):
    lpr = R.geometry(d)[0]
    ks = R.adagrad_ks(d)
    assert {1, 7} <= set(ks) and max(ks) <= R.U1
    assert set(ks) >= {min(R.U1, 256 // lpr + s) for s in (-1, 0, 1)}
    for k in ks:
        W, acc, idx, g = R.adagrad_fixture(d, k)
        assert len(idx) == k == len(np.unique(idx)) and R.U1 - 1 in idx and (k == 1 or 0 in idx)
        assert k < 2 or (np.diff(idx) < 0).any()  # unsorted
        assert acc.min() >= np.float32(0.1) and acc.max() < 5 and g.shape == (k, d)
        W2, acc2 = R.adagrad64(W, acc, idx, g)
        rest = np.setdiff1d(np.arange(R.U1), idx)
        assert np.array_equal(W2[rest], W[rest]) and np.array_equal(acc2[rest], acc[rest])
        assert (acc2[idx] >= acc[idx]).all() and (W2[idx] != W[idx]).any()


@pytest.mark.parametrize("setting", list(sf.BOUNDS))
@pytest.mark.parametrize("d", R.D_OPS)
def test_gather_fixture(d, setting):
    fx, at_bound, outside, equal = R.gather_fixture(d, setting)
    lo, hi, x, ax, u, i, j = (fx[k] for k in ("lo", "hi", "x", "ax", "u", "i", "j"))
    assert len(u) == R.N and fx["P"].shape == (R.U1, d) and fx["Q"].shape == (R.I1, d)
    assert len(equal) == R.N_EQ and (i[equal] == j[equal]).all() and not x[equal].any()
    assert len(at_bound) == len(outside) == (1 if setting == "default" else 2)
    bounds = (lo,) if setting == "default" else (lo, hi)
    assert tuple(x[at_bound]) == tuple(float(np.float32(b)) for b in bounds)
    beyond = [np.nextafter(np.float32(b), np.float32(s * np.inf)) for b, s in zip(bounds, (-1, 1))]
    assert tuple(x[outside]) == tuple(float(b) for b in beyond)
    # every other triplet keeps the margin condition, so its regime is the kernel's
    rest = np.setdiff1d(np.arange(R.N), at_bound + outside)
    for b in (lo, hi):
        assert (np.abs(x[rest] - b) > sf.margin_bound(d, ax[rest])).all()
    r = sf.regimes(x, lo, hi)
    for k in sf.POPULATED[setting]:
        assert (r == k).sum() >= 2, (sf.REGIME_NAMES[k], int((r == k).sum()))
    assert x[r == sf.UPPER].max(initial=0) <= sf.UPPER_MAX
    # the exact rows serve their triplet alone
    for t in at_bound + outside:
        assert (u == u[t]).sum() == 1 and (np.concatenate([i, j]) == i[t]).sum() == 1
        assert (np.concatenate([i, j]) == j[t]).sum() == 1
    loss, x64, p_idx, p_val, q_idx, q_val, clipped = R.gather_bpr64(fx["P"], fx["Q"], u, i, j, lo, hi)
    assert np.array_equal(x64, x) and np.array_equal(loss, fx["lc"])
    assert clipped[outside].all() and not clipped[at_bound].any() and clipped.sum() >= 3
    both = np.concatenate([clipped, clipped])
    assert not p_val[both].any() and not q_val[both].any() and p_val[~both].any()
    assert np.array_equal(q_val[R.N:], -q_val[:R.N])
    assert np.array_equal(p_idx, np.concatenate([u, u])) and np.array_equal(q_idx, np.concatenate([i, j]))


def test_composition_bars_come_from_the_oracle_alone(oracle):
    """k of the composed step's bar per d: 1 wherever the fp32 oracle holds the
    project's bar against float64; pinned here, without a GPU.  One batch of 64
    keeps the oracle inside the bar even at d = 1024 (test_gpu_step_geometry.py's
    four batches there do not): k = kd = 1 at every d."""
    ks = {d: R.compose_reference(oracle, d, _few_step_scale)[2:] for d in R.D_COMPOSE}
    print({d: (round(k, 2), round(kd, 2)) for d, (k, kd) in ks.items()})
    for d, (k, kd) in ks.items():
        assert k == 1.0 and kd == 1.0, (d, k, kd)


@pytest.mark.parametrize("B", R.GRID_B)
def test_grid_plan_width_of_every_batch_size(B):
    ipt = R.grid_plan_ipt(B)
    want = 1 if B <= 64 else 4 if B <= 256 else 8 if B <= 512 else 16
    assert ipt == want and 4 * B <= R.GRID_WG * ipt
    assert ipt == 1 or 4 * B > R.GRID_WG * {4: 1, 8: 4, 16: 8}[ipt]
    u, i, j = R.grid_width_triplets(B)
    assert len(u) == len(i) == len(j) == 2 * B


def test_grid_fixtures():
    assert {R.grid_plan_ipt(B) for B in R.GRID_B} == {1, 4, 8, 16}  # the four regimes
    assert {64, 65, 256, 257, 513, 1024} <= set(R.GRID_B)  # both sides of every threshold but 512 | 513
    assert any(4 * B % R.GRID_WG and B & (B - 1) for B in R.GRID_B)  # padding keys beside real ones
    u, i, j = R.grid_hot_item_triplets()
    assert len(u) == 1024
    terms = np.bincount(np.concatenate([i, j]), minlength=R.GRID_I1)
    assert {k: int(terms[k]) for k in R.HOT_ITEMS} == R.HOT_ITEMS == {3: 600, 5: 256, 8: 257}
    assert terms[3] > 2 * R.GRID_CHUNK and terms[8] > R.GRID_CHUNK and terms[5] == R.GRID_CHUNK
    assert (i == 3).sum() == 300 and (j == 3).sum() == 300 and not ((i == 3) & (j == 3)).any()
    # item 3's sorted terms e (positives 2B + t, negatives 3B + t) in partial sums of 256:
    # 256 +g terms | 44 +g and 212 -g terms | 88 -g terms; the second sum mixes the signs
    e = np.sort(np.concatenate([2048 + np.nonzero(i == 3)[0], 3072 + np.nonzero(j == 3)[0]]))
    plus = [int((e[c:c + R.GRID_CHUNK] < 3072).sum()) for c in range(0, 600, R.GRID_CHUNK)]
    minus = [int((e[c:c + R.GRID_CHUNK] >= 3072).sum()) for c in range(0, 600, R.GRID_CHUNK)]
    assert (plus, minus) == ([256, 44, 0], [0, 212, 88])
    u, i, j = R.grid_last_term_triplets()
    assert len(u) == 1024
    assert (u == u[-1]).sum() == 1 and (np.concatenate([i, j]) == i[-1]).sum() == 1
    assert (np.concatenate([i, j]) == j[-1]).sum() == 1 and i[-1] != j[-1]
    hps = R.grid_hps64()
    assert len(hps) == 64 == len({tuple(sorted(h.items())) for h in hps})
    assert {h["adver"] for h in hps} == {0, 1} and hps[63]["adver"] == 1 and hps[0]["adver"] == 1
    u, i, j = R.grid_wide_triplets()
    for col in (u, i, j):
        assert set(R.WIDE_EDGE) <= set(col.tolist()) and col.max() < R.WIDE_ROWS
    assert R.WIDE_ROWS > 2 ** 16 and 2 * R.WIDE_ROWS > 2 ** 17


def test_grid_chunk_fixture_tells_the_chunk_length():
    """grid_chunk_triplets: batch A's 512 terms of item 3 are two identical runs
    of 256, batch B holds the first run alone.  Restated in float32 with the
    terms fl(g_t p_u) (g_t from float64), a sum in partial sums of 256 doubles
    exactly, fl((2 G)^2) == 4 fl(G^2) bit for bit, and with partial sums of 64,
    128, 512 or 1,024 it does not."""
    (u, i, j), (uB, iB, jB) = R.grid_chunk_triplets()
    X, Y = R.CHUNK_ITEM, R.CHUNK_OTHER
    assert len(u) == 1024 and (i != j).all() and (iB != jB).all()
    assert np.array_equal(np.nonzero(i == X)[0], np.arange(512)) and not (j == X).any()
    for a in (u, i, j):
        assert np.array_equal(a[256:512], a[:256])
    assert np.array_equal(np.nonzero(iB == X)[0], np.arange(256)) and not (jB == X).any()
    assert np.array_equal(np.nonzero(iB == Y)[0], np.arange(256, 512)) and not (jB == Y).any()
    assert not (i == Y).any() and not (j == Y).any()
    assert np.array_equal(uB, u) and np.array_equal(jB, j) and np.array_equal(iB[512:], i[512:])
    P, Q = R.grid_chunk_tables()
    p, qi, qj = (a.astype(np.float64) for a in (P[0][u[:512]], Q[0][i[:512]], Q[0][j[:512]]))
    g = -1 / (np.exp((p * qi).sum(1) - (p * qj).sum(1)) + 1)
    terms = (g.astype(np.float32)[:, None] * P[0][u[:512]]).astype(np.float32)
    G = R.chunked_sum32(terms[:256], 256)
    four = np.float32(4) * (G * G)
    assert np.isfinite(four).all() and (G * G > 0).all()
    two = R.chunked_sum32(terms, 256)
    assert np.array_equal((two * two).view(np.int32), four.view(np.int32))
    for chunk in (64, 128, 512, 1024):
        other = R.chunked_sum32(terms, chunk)
        assert not np.array_equal((other * other).view(np.int32), four.view(np.int32)), chunk
