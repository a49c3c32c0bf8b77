"""CPU restatements and fixtures for the decomposed ops (csrc/acf_ops.hip, the
torch.ops.acf.* ops of csrc/acf_torch.cpp) and for the shapes of grid training
(csrc/acf_grid.hip), shared by test_ops_ref_host.py, test_gpu_ops_geometry.py
and test_gpu_grid_shapes.py.  Nothing here needs a GPU.

  geometry(d)              geometry() of csrc/acf_host.h
  segment_sum_exact        row_segment_sum: unique rows ascending, each the
                           sequential fp32 sum of its values in input order
  gather_bpr64             gather_bpr_fwd_bwd in float64 (clip, gradient mask,
                           loss, the four IndexedSlices blocks in concat order)
  l2norm_perturb64         eps * g / sqrt(max(g.g, 1e-12)) in float64
  adagrad64                acc += g^2; w -= lr g / sqrt(acc) in float64
  seg_case, l2_fixture, adagrad_fixture, gather_fixture, compose_problem,
  grid_*                   seeded fixtures, arrays read-only, built once

u = 2^-24 is the unit roundoff of float32 throughout."""
import numpy as np

import saturation_fixture as sf
from test_gpu_step_geometry import _step64

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
D_OPS = [4, 8, 12, 20, 48, 100, 132, 260, 516, 768, 772, 1024]
PADDED = [12, 20, 48, 100, 132, 260, 516, 772]
DISPATCHED = {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4)}  # OPS_GEOM
U1, I1, N = 61, 47, 96  # the ops' tables and triplets

_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def geometry(d):
    """geometry() of csrc/acf_host.h: (lanes per row, float4 chunks per lane)."""
    d4 = d // 4
    lpr = 1
    while lpr < d4 and lpr < 64:
        lpr <<= 1
    return lpr, (d4 + lpr - 1) // lpr


# ---------------------------------------------------------------------------
# row_segment_sum
def segment_sum_exact(idx, vals, reverse=False):
    """(uniq, count, summed): unique rows ascending; each row the SEQUENTIAL fp32
    sum, from zero, of its values in input order (TF's unsorted_segment_sum).
    reverse: in reversed input order, which a stable sort must not produce."""
    idx = np.asarray(idx).astype(np.int64).ravel()
    order = np.argsort(idx, kind="stable")
    uniq, start, count = np.unique(idx[order], return_index=True, return_counts=True)
    out = np.zeros((len(uniq), vals.shape[1]), np.float32)
    for k, (a, c) in enumerate(zip(start, count)):
        pos = order[a:a + c]
        acc = np.zeros(vals.shape[1], np.float32)
        for x in (pos[::-1] if reverse else pos):
            acc = acc + vals[x]  # float32 + float32: one rounding per add
        out[k] = acc
    return uniq.astype(np.int32), count.astype(np.int32), out


def _spread(rng, m, d):
    """Values with exponents spread over about 2^+-20: the order of a sum matters."""
    return (rng.standard_normal((m, d)) * 2.0 ** rng.integers(-20, 21, (m, d))).astype(np.float32)


SEG_M = (0, 1, 2, 255, 256, 257, 5000)
SEG_ROWS = (1, 2, 3, 1 << 20, (1 << 20) + 1)
SEG_EXTRA = ([f"m{m}" for m in SEG_M] + ["all_equal", "all_distinct", "descending", "int64"] +
             [f"rows{r}" for r in SEG_ROWS])
SEG_EXTRA_D = (20, 260)


def seg_case(name, d):
    """(idx, vals, num_rows) of a row_segment_sum case.  "base": m = 300 over 40
    rows.  "m<M>": M values over 40 rows.  "all_equal": one segment of 5,000.
    "all_distinct": a permutation of 300 rows.  "descending": the base indices
    sorted downwards.  "int64": the base with int64 indices.  "rows<R>":
    num_rows = R with rows 0 and R - 1 present; above 3 rows the indices come
    from a pool of 12 rows spread over every bit of R - 1, so segments recur."""
    key = ("seg", name, d)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(sum(map(ord, name)) * 1031 + d)
    m, rows = 300, 40
    if name.startswith("m"):
        m = int(name[1:])
    elif name == "all_equal":
        m = 5000
    elif name == "all_distinct":
        rows = 300
    elif name.startswith("rows"):
        rows = int(name[4:])
    idx = rng.integers(0, min(rows, 40), m)
    if name == "all_equal":
        idx[:] = 7
    elif name == "all_distinct":
        idx = rng.permutation(rows)
    elif name == "descending":
        idx = np.sort(idx)[::-1]
    elif name.startswith("rows"):
        if rows > 3:
            pool = np.unique(np.concatenate([[0, 1, rows - 1, rows - 2, rows // 2, rows // 2 - 1, 65535, 65536],
                                             rng.integers(0, rows, 4)]))
            idx = pool[rng.integers(0, len(pool), m)]
        idx[m // 3], idx[m // 2] = rows - 1, 0
    idx = np.ascontiguousarray(idx).astype(np.int64 if name == "int64" else np.int32)
    _cache[key] = _frozen(idx, _spread(rng, m, d)) + (rows,)
    return _cache[key]


# ---------------------------------------------------------------------------
# l2norm_perturb
L2_K = (1, 7, 300)
L2_EPS = (0.0, 0.5, 2.0)
L2_ZERO, L2_TINY, L2_BELOW, L2_ABOVE, L2_OVERFLOW = range(5)  # the planted rows, for k >= 7


def l2norm_perturb64(g, eps):
    """eps * g / sqrt(max(g.g, 1e-12)) in float64.  A sum of squares beyond the
    float32 range is inf in float32 whatever the order of the sum (its terms are
    non-negative, so every order's partial sums reach the total): the row is
    g * rsqrt(inf) = 0."""
    g = g.astype(np.float64)
    ss = (g * g).sum(1, keepdims=True)
    ss[ss > FLT_MAX] = np.inf
    return float(np.float32(eps)) * g / np.sqrt(np.maximum(ss, 1e-12))


def l2_bar(d, want):
    """|got - want| <= (d + 8) u |want|: the d-term sum of non-negative products
    carries at most d u of relative error (d products and d - 1 adds, none
    cancelling), which the rsqrt halves; v_rsq_f32 (1 ulp = 2 u) and the two
    rounded products (g * inv, * eps) add 4 u; in all under (d / 2 + 5) u."""
    return (d + 8) * U * np.abs(want)


def l2_fixture(d, k):
    """g [k, d] float32: rows at scales 1e-3 .. 1e3; for k >= 7 rows 0-4 are an
    all-zero row, a row with 0 < g.g < 1e-12 (elements near 1e-10), rows with
    g.g = 1e-12 (1 -+ 8 d u) (norm just below and just above 1e-6) and a row of
    1e19s, whose sum of squares overflows for d >= 4."""
    key = ("l2", d, k)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(7000 + 3 * d + k)
    g = rng.standard_normal((k, d)) * 10.0 ** rng.integers(-3, 4, (k, 1))
    if k >= 7:
        g[L2_ZERO] = 0
        g[L2_TINY] = rng.standard_normal(d) * 1e-10
        for row, sign in ((L2_BELOW, -1), (L2_ABOVE, 1)):
            v = rng.standard_normal(d)
            g[row] = v * np.sqrt(1e-12 * (1 + sign * 8 * d * U) / (v * v).sum())
        g[L2_OVERFLOW] = 1e19
    _cache[key] = _frozen(g.astype(np.float32))[0]
    return _cache[key]


def l2_floor_margin(g):
    """|g.g / 1e-12 - 1| per row, in float64."""
    g = g.astype(np.float64)
    return np.abs((g * g).sum(1) / 1e-12 - 1)


# ---------------------------------------------------------------------------
# sparse_adagrad_apply
LR = float(np.float32(0.05))  # the op rounds lr to float32


def adagrad64(W, acc, idx, g, lr=LR):
    """(W, acc) after acc[idx] += g^2; W[idx] -= lr g / sqrt(acc[idx]), float64."""
    W, acc, g = W.astype(np.float64), acc.astype(np.float64), g.astype(np.float64)
    acc[idx] += g * g
    W[idx] -= lr * g / np.sqrt(acc[idx])
    return W, acc


def adagrad_ks(d):
    """k of the Adagrad cases: 1, 7 and the rows of one workgroup (256 / LPR),
    one less and one more, capped at the table's 61 rows."""
    rpw = 256 // geometry(d)[0]
    return sorted({1, 7} | {min(U1, rpw + s) for s in (-1, 0, 1)})


def adagrad_fixture(d, k):
    """(W, acc, idx, g): 61-row tables, acc in [0.1, 5); k unique unsorted rows
    with row 60 (k = 1) or rows 0 and 60 (k >= 2) among them."""
    key = ("ada", d, k)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(8000 + 5 * d + k)
    W = (rng.standard_normal((U1, d)) * 0.3).astype(np.float32)
    acc = rng.uniform(0.1, 5.0, (U1, d)).astype(np.float32)
    acc = np.maximum(acc, np.float32(0.1))
    rest = rng.permutation(np.arange(1, U1 - 1))
    idx = np.concatenate([[U1 - 1], rest[:max(0, k - 2)], [0] * (k >= 2)]).astype(np.int32)  # 60 first, 0 last
    g = (rng.standard_normal((k, d)) * 10.0 ** rng.integers(-2, 2, (k, 1))).astype(np.float32)
    _cache[key] = _frozen(W, acc, idx, g)
    return _cache[key]


# ---------------------------------------------------------------------------
# gather_bpr_fwd_bwd
N_EQ = 4  # triplets with i == j


def gather_bpr64(P, Q, u, i, j, lo, hi):
    """float64: (loss, x, p_idx, p_val, q_idx, q_val, clipped) of
    gather_bpr_fwd_bwd; the value blocks in concat order [pos branch; neg branch]."""
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    p, qi, qj = P[u], Q[i], Q[j]
    x = (p * qi).sum(1) - (p * qj).sum(1)
    clipped = (x < lo) | (x > hi)
    r = np.clip(x, lo, hi)
    loss = np.logaddexp(0, -r)
    g = -1 / (np.exp(r) + 1) * ~clipped
    return (loss, x, np.concatenate([u, u]), np.concatenate([g[:, None] * qi, -g[:, None] * qj]),
            np.concatenate([i, j]), np.concatenate([g[:, None] * p, -g[:, None] * p]), clipped)


def gather_fixture(d, setting):
    """(fx, at_bound, outside, equal): 96 triplets on 61 x 47 tables under
    sf.BOUNDS[setting], fx laid out as saturation_fixture.problem's with nb = 1
    and adver = 0.  The ordinary triplets are picked by regime with twice the
    margin condition (sf._pick_batch); then N_EQ triplets with i == j (x = 0
    exactly); the exact triplets of sf.exact_problem (rows with one non-zero
    element, products of small integers: x == bound, and the next float beyond
    it), on rows no other triplet uses; the two always-clipped triplets of
    sf.make_tables.  at_bound / outside / equal list triplet indices."""
    key = ("gather", d, setting)
    if key in _cache:
        return _cache[key]
    lo, hi = sf.BOUNDS[setting]
    f32 = np.float32
    if setting == "default":  # 8 * -10 = -80; 8 * nextafter(-10) = nextafter(-80)
        cases = ((f32(8), f32(-10), lo, True), (f32(8), np.nextafter(f32(-10), f32(-np.inf)), lo, False))
    else:
        cases = ((f32(1), f32(lo), lo, True), (f32(1), np.nextafter(f32(lo), f32(-np.inf)), lo, False),
                 (f32(1), f32(hi), hi, True), (f32(1), np.nextafter(f32(hi), f32(np.inf)), hi, False))
    n = len(cases)
    rng = np.random.default_rng(9100 + d + (setting == "tight"))
    P0, Q0 = sf.make_tables(rng, U1, I1, d)
    ou, oi = U1 - 2 - n, I1 - 4 - 2 * n  # ordinary rows first, then the exact rows, then the always-clipped rows
    u, i, j = sf._pick_batch(rng, P0.astype(np.float64), Q0.astype(np.float64), d, setting, ou, oi, N - 2 - n - N_EQ)
    equal = list(range(len(u), len(u) + N_EQ))
    eq_i = rng.integers(0, oi, N_EQ)
    u, i, j = np.append(u, rng.integers(0, ou, N_EQ)), np.append(i, eq_i), np.append(j, eq_i)
    at_bound, outside = [], []
    cols = (0, d - 1, 5 % d, d - 4)  # the first and the last chunk of the row among them
    for k, (pv, qv, bound, passes) in enumerate(cases):
        urow, ipos, ineg = ou + k, oi + 2 * k, oi + 2 * k + 1
        P0[urow], Q0[ipos], Q0[ineg] = 0, 0, 0
        P0[urow, cols[k]], Q0[ipos, cols[k]] = pv, qv
        assert f32(pv * qv) == (f32(bound) if passes else np.nextafter(f32(bound), f32(np.sign(qv) * np.inf)))
        (at_bound if passes else outside).append(len(u))
        u, i, j = np.append(u, urow), np.append(i, ipos), np.append(j, ineg)
    u, i, j = np.append(u, [U1 - 1, U1 - 2]), np.append(i, [I1 - 2, I1 - 4]), np.append(j, [I1 - 1, I1 - 3])
    perm = rng.permutation(N)  # the planted triplets anywhere in the batch
    inv = np.argsort(perm)
    u, i, j = (a[perm].astype(np.int32) for a in (u, i, j))
    at_bound, outside, equal = ([int(inv[t]) for t in ts] for ts in (at_bound, outside, equal))
    P, Q = P0.astype(np.float64), Q0.astype(np.float64)
    x, ax = sf.scores64(P, Q, u, i, j, 0, lo, hi)[:2]
    lc = np.logaddexp(0, -np.clip(x, lo, hi))
    fx = dict(d=d, setting=setting, adver=0, lo=lo, hi=hi, B=N, nb=1, U1=U1, I1=I1, P=P0, Q=Q0, u=u, i=i, j=j,
              x=x, ax=ax, xa=x, axa=ax, lc=lc, la=np.zeros(N))
    _frozen(*(v for v in fx.values() if isinstance(v, np.ndarray)))
    _cache[key] = (fx, at_bound, outside, equal)
    return _cache[key]


def gather_loss_bars(oracle, fx, few_step_scale):
    """(k, upper-tail rtol) of the loss bar of test_gather_bpr_with_bounds for
    fx, from the reference alone: the fp32 oracle and four runs of it with its
    sums reordered (sf.oracle_samples) against the float64 losses."""
    if "loss_bars" not in fx:
        smp = sf.oracle_samples(oracle, fx)
        fx["loss_bars"] = (few_step_scale([s[1] for s in smp], [fx["lc"]] * len(smp)), sf.upper_rtol(fx, smp))
    return fx["loss_bars"]


def gather_values32(fx):
    """g * partner restated in float32 with numpy's own dot products, exp and
    division (test_gather_bpr_with_bounds' restatement): [p values, q values]."""
    P, Q, u, i, j, lo, hi = (fx[k] for k in ("P", "Q", "u", "i", "j", "lo", "hi"))
    clipped = (fx["x"] < lo) | (fx["x"] > hi)
    x32 = (P[u] * Q[i]).sum(1, dtype=np.float32) - (P[u] * Q[j]).sum(1, dtype=np.float32)
    g32 = (np.float32(-1) / (np.exp(np.clip(x32, np.float32(lo), np.float32(hi))) + np.float32(1))) * ~clipped
    return [np.concatenate([g32[:, None] * Q[i], -g32[:, None] * Q[j]]),
            np.concatenate([g32[:, None] * P[u], -g32[:, None] * P[u]])]


# ---------------------------------------------------------------------------
# the ops composed into one APR step
D_COMPOSE = (12, 100, 260, 772, 1024)
B_COMPOSE = 64
COMPOSE_NAMES = ("P", "Q", "accP", "accQ", "loss_clean", "loss_adv")


def compose_problem(d):
    """(P, Q, u, i, j): 61 x 47 tables at sigma = 0.3, one batch of 64 triplets,
    every ninth with i == j."""
    key = ("compose", d)
    if key not in _cache:
        rng = np.random.default_rng(300 + d)
        P = (rng.standard_normal((U1, d)) * 0.3).astype(np.float32)
        Q = (rng.standard_normal((I1, d)) * 0.3).astype(np.float32)
        u, i, j = (rng.integers(0, n, B_COMPOSE).astype(np.int32) for n in (U1, I1, I1))
        j[::9] = i[::9]
        _cache[key] = _frozen(P, Q, u, i, j)
    return _cache[key]


def compose_reference(oracle, d, few_step_scale):
    """The oracle's step of compose_problem(d) with the defaults of HParams:
    (tables + losses, delta tables, k, kd).  k scales the bar of the tables and
    losses, kd that of the delta tables (few_step_scale = _few_step_scale of
    test_gpu_step_geometry.py: the fp32 oracle against float64, 1 where it holds
    the project's bar, else 4x its distance)."""
    key = ("compose_ref", d)
    if key not in _cache:
        from apr_oracle import HParams
        P, Q, u, i, j = compose_problem(d)
        rP, rQ = P.copy(), Q.copy()
        aP, aQ = np.full(P.shape, 0.1, np.float32), np.full(Q.shape, 0.1, np.float32)
        lc, la, dP, dQ = oracle.apr_batch(rP, rQ, aP, aQ, u, i, j, HParams(adver=1), want_delta=True)
        P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
        d64 = sf.scores64(P64, Q64, u, i, j, 1, -80.0, 1e8)[4:]
        a64 = [np.full(x.shape, np.float64(np.float32(0.1))) for x in (P, Q)]
        l64 = _step64(P64, Q64, a64[0], a64[1], u, i, j, 1)
        want = _frozen(rP, rQ, aP, aQ, lc, la)
        deltas = _frozen(dP, dQ)
        _cache[key] = (want, deltas, few_step_scale(want, [P64, Q64] + a64 + list(l64)),
                       few_step_scale(deltas, d64))
    return _cache[key]


# ---------------------------------------------------------------------------
# grid training: the shapes of test_gpu_grid_shapes.py
GRID_U1, GRID_I1 = 65, 49  # test_gpu_grid.py's tables
GRID_B = (64, 65, 100, 256, 257, 513, 1000, 1024)
GRID_WG, GRID_CHUNK = 256, 256
HOT_ITEMS = {3: 600, 5: 256, 8: 257}  # item -> terms in the hot batch


def grid_plan_ipt(B):
    """Items per thread of the k_grid_plan instantiation acf_apr_grid_train picks
    for batch size B: the first of 1, 4, 8, 16 whose 256 threads hold the 4B terms."""
    for ipt in (1, 4, 8, 16):
        if 4 * B <= GRID_WG * ipt:
            return ipt
    raise ValueError(f"batch size {B} is beyond ACF_GRID_MAX_BATCH")


def grid_width_triplets(B, nb=2):
    key = ("grid_w", B)
    if key not in _cache:
        rng = np.random.default_rng(500 + B)
        _cache[key] = _frozen(*(rng.integers(0, n, nb * B).astype(np.int32) for n in (GRID_U1, GRID_I1, GRID_I1)))
    return _cache[key]


def grid_hot_item_triplets():
    """One batch of 1,024: item 3 the positive of 300 triplets and the negative
    of 300 others (600 terms in three partial sums: 256 +g terms, 44 +g and
    212 -g terms, 88 -g terms), item 5 with exactly 256 terms (one full partial
    sum), item 8 with 257 (a partial sum of one term); the other item terms over
    the remaining rows."""
    key = "grid_hot"
    if key not in _cache:
        rng = np.random.default_rng(77)
        B = 1024
        others = np.setdiff1d(np.arange(GRID_I1), list(HOT_ITEMS))
        ij = others[rng.integers(0, len(others), 2 * B)]  # [0, B): positives, [B, 2B): negatives
        free = rng.permutation(B)
        ij[free[:300]] = 3
        ij[B + free[300:600]] = 3
        ij[free[600:728]], ij[B + free[600:728]] = 5, 5  # pos == neg in 128 triplets: 256 terms
        ij[free[728:900]] = 8
        ij[B + free[900:985]] = 8  # 172 + 85 = 257
        u = rng.integers(0, GRID_U1, B)
        _cache[key] = _frozen(u.astype(np.int32), ij[:B].astype(np.int32), ij[B:].astype(np.int32))
    return _cache[key]


CHUNK_ITEM, CHUNK_OTHER = 3, 4


def grid_chunk_triplets():
    """(A, B): two batches of 1,024 that hold GRID_CHUNK = 256 to the bit.  In A
    item 3 is the positive of triplets 0..511 and of no other, and triplet
    256 + t is a copy (u, i, j) of triplet t: the row's sorted terms are two
    identical runs of 256, so with partial sums of 256 terms its gradient is
    acc + acc = 2 G exactly.  B is A with item 4 as the positive of triplets
    256..511: the row's gradient is G.  A BPR member with reg 0 and accumulators
    at 0 leaves fl((2 G)^2) = 4 fl(G^2) and fl(G^2) in the item's Adagrad slot;
    with partial sums of any other length A's sum is no exact doubling.  No
    triplet has i == j, and item 4 occurs nowhere else."""
    key = "grid_chunk"
    if key not in _cache:
        rng = np.random.default_rng(80)
        B = 1024
        others = np.setdiff1d(np.arange(GRID_I1), [CHUNK_ITEM, CHUNK_OTHER])
        u = rng.integers(0, GRID_U1, B)
        i = others[rng.integers(0, len(others), B)]
        j = others[(np.searchsorted(others, i) + rng.integers(1, len(others), B)) % len(others)]  # j != i
        i[:512] = CHUNK_ITEM
        u[256:512], j[256:512] = u[:256], j[:256]
        iB = i.copy()
        iB[256:512] = CHUNK_OTHER
        u, i, j, iB = (a.astype(np.int32) for a in (u, i, j, iB))
        _cache[key] = (_frozen(u, i, j), _frozen(u.copy(), iB, j.copy()))
    return _cache[key]


def grid_chunk_tables(d=64):
    """Member-major tables [1, rows, d] at sigma = 0.3 for grid_chunk_triplets."""
    key = ("grid_chunk_tables", d)
    if key not in _cache:
        rng = np.random.default_rng(81)
        _cache[key] = _frozen((rng.standard_normal((1, GRID_U1, d)) * 0.3).astype(np.float32),
                              (rng.standard_normal((1, GRID_I1, d)) * 0.3).astype(np.float32))
    return _cache[key]


def chunked_sum32(terms, chunk):
    """k_grid_sum's order in float32: partial sums of `chunk` terms, each summed
    one term after the other from zero, added in order (the first one taken as it is)."""
    tot = None
    for c0 in range(0, len(terms), chunk):
        acc = np.zeros(terms.shape[1], np.float32)
        for v in terms[c0:c0 + chunk]:
            acc = acc + v
        tot = acc if tot is None else tot + acc
    return tot


def grid_last_term_triplets():
    """One batch of 1,024 in which user 64 and items 47 and 48 occur in triplet
    1,023 alone: term 1,023 heads and term 2,047 ends the user's slot, terms
    3,071 and 4,095 (the last value GRID_EBITS holds) are the sole terms of theirs."""
    key = "grid_last"
    if key not in _cache:
        rng = np.random.default_rng(78)
        B = 1024
        u, i, j = (rng.integers(0, n, B).astype(np.int32) for n in (GRID_U1 - 1, GRID_I1 - 2, GRID_I1 - 2))
        u[-1], i[-1], j[-1] = GRID_U1 - 1, GRID_I1 - 2, GRID_I1 - 1
        _cache[key] = _frozen(u, i, j)
    return _cache[key]


def grid_hps64():
    """64 distinct hyper-parameter sets: test_gpu_grid.py's _hps16 recipe, extended."""
    return [dict(adver=int(k % 5 != 4), eps=0.1 + 0.05 * k, reg_adv=0.25 * (1 + k % 4), lr=0.02 + 0.002 * k,
                 reg=0.01 * (k % 3)) for k in range(64)]


WIDE_ROWS = 70000
WIDE_EDGE = (0, 65535, 65536, WIDE_ROWS - 1)


def grid_wide_triplets():
    """One batch of 64 on 70,000 x 70,000 tables: rows 0, 65,535, 65,536 and
    69,999 as user, as positive and as negative; the rest anywhere."""
    key = "grid_wide"
    if key not in _cache:
        rng = np.random.default_rng(79)
        u, i, j = (rng.integers(0, WIDE_ROWS, 64).astype(np.int32) for _ in range(3))
        for k, col in enumerate((u, i, j)):
            col[rng.permutation(64)[:8]] = np.repeat(WIDE_EDGE, 2)[rng.permutation(8)] if k else np.repeat(WIDE_EDGE, 2)
        _cache[key] = _frozen(u, i, j)
    return _cache[key]
