"""The fixture test_step_saturation_host.py and test_gpu_step_saturation.py
share: tiny APR / BPR problems whose triplets sit in every regime of the score
x = u.i - u.j that bpr_term / bpr_clip / bpr_loss (csrc/acf_rows.h) tell apart,

    CENTRAL  |x| <= 13.942385        loss = log(e^-x + 1), g = -1 / (e^x + 1)
    UPPER    13.94 < x <= clip_hi    loss = e^-x, g tiny
    LOWER    clip_lo <= x < -13.94   loss = -x, g ~ -1
    BELOW    x < clip_lo             g = 0, loss = -clip_lo
    ABOVE    x > clip_hi             g = 0, loss = softplus(-clip_hi)

under two settings of the bounds: "default" (-80, 1e8) and "tight" (-2, 3).

The table rows are drawn at per-row scales 0.3 / 1.0 / 2.0 (times (64 / d)^(1/4),
so the spread of the scores is the same at every d), which spreads the scores
of the 35 x 25 x 25 ordinary triplets over +-150.  The triplets of a batch are
not drawn blindly: batch t is picked, by quota per regime, from the scores of
the float64 trajectory at the start of batch t (_step64 of
test_gpu_step_geometry.py, the yardstick), so every batch holds every regime
although the tables move.  Two triplets of every batch use rows of their own:

    (CL_U; CL_I)  x = -120: below clip_lo in both settings, in both passes
    (CH_U; CH_I)  x = +30:  above clip_hi under the tight bounds (upper tail otherwise)

Their rows are touched by clipped triplets only: zero gradient, zero delta
(through the 1e-12 floor of l2_normalize), adversarial score == clean score,
rows and Adagrad slots bit-identical after any number of steps.

Everything is a pure function of (d, setting, adver) and the seeds below, which
were chosen on the CPU so that conditions() holds and the fp32 reference is
within half a bar of float64 (SEEDS); nothing here needs a GPU."""
import numpy as np

from test_gpu_step_geometry import _step64

U1, I1, B, NB = 37, 29, 64, 3
DIMS = (16, 64, 100, 132)  # (LPR, NV) = (4, 1), (16, 1), (32, 1) padded, (64, 1) padded
DIMS_STREAM = (16, 64, 100)
BOUNDS = {"default": (-80.0, 1e8), "tight": (-2.0, 3.0)}
SCALES = (0.3, 1.0, 2.0)
T = float(np.float32(13.942385))  # ACF_SOFTPLUS_T
UPPER_MAX = 60.0  # e^-60 is a normal float; denormal flushing is not under test
EPS, LR = 0.5, 0.05  # the defaults of HParams / StepHParams

CENTRAL, UPPER, LOWER, BELOW, ABOVE = range(5)
REGIME_NAMES = ("central", "upper", "lower", "below_lo", "above_hi")
POPULATED = {"default": (CENTRAL, UPPER, LOWER, BELOW), "tight": (CENTRAL, BELOW, ABOVE)}

N_USERS, N_ITEMS = U1 - 2, I1 - 4  # the ordinary rows
CL_U, CL_I = U1 - 1, (I1 - 2, I1 - 1)
CH_U, CH_I = U1 - 2, (I1 - 4, I1 - 3)
X_CL, X_CH = -120.0, 30.0

# Seeds chosen on the CPU; key (d, setting, adver), 0 where not listed.  Each is the
# smallest seed at which conditions() holds and every oracle sample (the fp32
# oracle and four runs of it with its sums reordered: oracle_samples) lies within
# HALF a bar (rtol 1e-5 / atol 1e-6) of float64 on every table, Adagrad slot, loss
# and delta table.  Two right fp32 results that are each within half a bar of the
# exact result are within a bar of each other; where the reference itself strays
# further, the bar cannot tell a kernel that is as right as the oracle from a
# wrong one.  (Seed 0 of (64, tight, 1): oracle samples up to 0.90 bars from
# float64, the kernels 0.93, the two 1.2 bars apart in one Adagrad slot.)
SEEDS = {(100, "default", 1): 1, (64, "tight", 0): 5, (132, "default", 0): 1, (16, "tight", 1): 13,
         (64, "default", 1): 8, (100, "default", 0): 6, (64, "tight", 1): 16, (132, "default", 1): 13,
         (132, "tight", 0): 81, (100, "tight", 1): 131, (132, "tight", 1): 342}
LARGE_SEEDS = {}
HALF_BAR = 0.5


def regimes(x, lo, hi):
    r = np.full(x.shape, CENTRAL)
    r[x > T] = UPPER
    r[x < -T] = LOWER
    r[x < lo] = BELOW
    r[x > hi] = ABOVE
    return r


def margin_bound(d, abs_sum):
    """4x the Higham bound of an fp32 dot product of d terms in any order, for the
    difference of two of them: 4 * 2d * 2^-24 * (sum|p q_i| + sum|p q_j|)."""
    return 4.0 * 2 * d * 2.0 ** -24 * abs_sum


def _delta(G, eps):
    return G / np.sqrt(np.maximum((G * G).sum(1, keepdims=True), 1e-12)) * eps


def scores64(P, Q, u, i, j, adver, lo, hi, eps=EPS):
    """Clean and adversarial score of every triplet of one batch in float64, the
    sums of |products| their margins are measured in, and the delta tables: the
    first half of _step64, which does not return them."""
    p, qi, qj = P[u], Q[i], Q[j]
    x = (p * qi).sum(1) - (p * qj).sum(1)
    ax = np.abs(p * qi).sum(1) + np.abs(p * qj).sum(1)
    dP, dQ = np.zeros_like(P), np.zeros_like(Q)
    if not adver:
        return x, ax, x.copy(), ax.copy(), dP, dQ
    g = -1 / (np.exp(np.clip(x, lo, hi)) + 1) * ((x >= lo) & (x <= hi))
    for G, rows, v in ((dP, u, g[:, None] * qi), (dQ, i, g[:, None] * p), (dP, u, -g[:, None] * qj),
                       (dQ, j, -g[:, None] * p)):
        np.add.at(G, rows, v)
    dP, dQ = _delta(dP, eps), _delta(dQ, eps)
    pa, qia, qja = p + dP[u], qi + dQ[i], qj + dQ[j]
    xa = (pa * qia).sum(1) - (pa * qja).sum(1)
    axa = np.abs(pa * qia).sum(1) + np.abs(pa * qja).sum(1)
    return x, ax, xa, axa, dP, dQ


def make_tables(rng, nu, ni, d):
    """float32 tables with per-row scales; the last two user rows and the last
    four item rows are the rows of the two always-clipped triplets."""
    norm = (64.0 / d) ** 0.25
    P = rng.standard_normal((nu, d)) * (np.array(SCALES)[rng.integers(0, 3, nu)] * norm)[:, None]
    Q = rng.standard_normal((ni, d)) * (np.array(SCALES)[rng.integers(0, 3, ni)] * norm)[:, None]
    for urow, (ipos, ineg), x in ((nu - 1, (ni - 2, ni - 1), X_CL), (nu - 2, (ni - 4, ni - 3), X_CH)):
        v = rng.standard_normal(d) * norm
        P[urow] = v
        Q[ipos] = v * (x / 2 / (v * v).sum())
        Q[ineg] = -Q[ipos]
    return P.astype(np.float32), Q.astype(np.float32)


def _windows(setting):
    """(lowest x, highest x, triplets of 64) per quota.  Default bounds: the tails
    stop short of clip_lo and of UPPER_MAX so that the adversarial score of a
    lower-tail triplet rarely crosses; the tight bounds add four bands beside the
    bounds, whose triplets the adversarial pass carries across (it lowers x)."""
    if setting == "default":
        return ((-T, T, 22), (T, 40.0, 12), (-70.0, -T, 12), (-np.inf, -90.0, 8), (-70.0, 40.0, 8))
    lo, hi = BOUNDS[setting]
    return ((lo, hi, 14), (-np.inf, lo - 3, 10), (hi + 3, np.inf, 10), (lo, lo + 1.5, 8), (hi, hi + 1.5, 8),
            (lo - 1.5, lo, 6), (hi - 1.5, hi, 6))


def _pick_batch(rng, P, Q, d, setting, nu, ni, size, n_cand=None):
    """`size` ordinary triplets of the current float64 tables, by quota."""
    lo, hi = BOUNDS[setting]
    if n_cand is None:  # every ordinary triplet with i != j
        u, i, j = (a.ravel() for a in np.meshgrid(np.arange(nu), np.arange(ni), np.arange(ni), indexing="ij"))
    else:  # a sample; one in fifty of it among 16 hot rows of each table
        hot = rng.random(n_cand) < 0.02
        u, i, j = (np.where(hot, rng.integers(0, 16, n_cand), rng.integers(0, n, n_cand)) for n in (nu, ni, ni))
    keep = i != j
    u, i, j = u[keep], i[keep], j[keep]
    x, ax = scores64(P, Q, u, i, j, 0, lo, hi)[:2]
    m = 2 * margin_bound(d, ax)  # twice the condition: the float32 trajectories differ a little
    ok = (np.abs(x - lo) > m) & (np.abs(x - hi) > m)
    taken = np.zeros(len(x), bool)
    out = []
    wins = _windows(setting)
    total = sum(w[2] for w in wins)
    for a, b, n in wins:
        n = n * size // total
        idx = np.nonzero(ok & ~taken & (x >= a) & (x <= b))[0]
        idx = rng.choice(idx, min(n, len(idx)), replace=False)
        taken[idx] = True
        out.append(idx)
    out = np.concatenate(out)
    if len(out) < size:  # a thin window: fill up with central triplets
        idx = np.nonzero(ok & ~taken & (np.abs(x) <= min(T, -lo, hi)))[0]
        out = np.concatenate([out, rng.choice(idx, size - len(out), replace=False)])
    out = rng.permutation(out)
    return u[out], i[out], j[out]


def _build(d, setting, adver, seed, nu, ni, batch, nb, n_cand=None):
    lo, hi = BOUNDS[setting]
    rng = np.random.default_rng(seed)
    P0, Q0 = make_tables(rng, nu, ni, d)
    P, Q = P0.astype(np.float64), Q0.astype(np.float64)
    aP, aQ = (np.full(a.shape, np.float64(np.float32(0.1))) for a in (P, Q))
    cols = {k: [] for k in ("u", "i", "j", "x", "ax", "xa", "axa", "lc", "la")}
    deltas = []
    for _ in range(nb):
        u, i, j = _pick_batch(rng, P, Q, d, setting, nu - 2, ni - 4, batch - 2, n_cand)
        at = rng.permutation(batch)[:2]  # where the two always-clipped triplets sit
        for k, (urow, (ipos, ineg)) in zip(np.sort(at), ((nu - 1, (ni - 2, ni - 1)), (nu - 2, (ni - 4, ni - 3)))):
            u, i, j = np.insert(u, k, urow), np.insert(i, k, ipos), np.insert(j, k, ineg)
        x, ax, xa, axa, dP, dQ = scores64(P, Q, u, i, j, adver, lo, hi)
        lc, la = _step64(P, Q, aP, aQ, u, i, j, adver, eps=EPS, lr=LR, lo=lo, hi=hi)
        deltas.append((dP, dQ))
        for k, v in zip(cols, (u, i, j, x, ax, xa, axa, lc, la)):
            cols[k].append(v)
    fx = {k: np.concatenate(v) for k, v in cols.items()}
    for k in "uij":
        fx[k] = fx[k].astype(np.int32)
    fx.update(d=d, setting=setting, adver=adver, lo=lo, hi=hi, B=batch, nb=nb, U1=nu, I1=ni, P=P0, Q=Q0,
              f64=[P, Q, aP, aQ, fx["lc"], fx["la"]], deltas=deltas,
              clipped_users=(nu - 1,) + (nu - 2,) * (setting == "tight"),
              clipped_items=(ni - 2, ni - 1) + (ni - 4, ni - 3) * (setting == "tight"))
    for v in list(fx.values()) + fx["f64"] + [a for pair in deltas for a in pair]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


_cache = {}


def problem(d, setting, adver):
    """The 37 x 29, B = 64, nb = 3 problem of (d, setting, adver) with its float64
    trajectory: per triplet of every step the clean and adversarial score (x, xa),
    the sums of |products| behind them (ax, axa) and the float64 losses (lc, la);
    the final float64 tables (f64) and the delta tables of every batch."""
    key = (d, setting, adver)
    if key not in _cache:
        _cache[key] = _build(d, setting, adver, SEEDS.get(key, 0), U1, I1, B, NB)
    return _cache[key]


LARGE = dict(U1=3000, I1=2500, B=4096, nb=2, d=64)


def large_problem(adver):
    """B = 4,096 (the smallest batch the auto mapping packs: a hash plan, the
    triplet-centric kernels), 3,000 x 2,500 rows, default bounds; one in fifty of the candidate
    triplets among 16 hot rows of each table, so some slots are summed in pieces."""
    key = ("large", adver)
    if key not in _cache:
        L = LARGE
        _cache[key] = _build(L["d"], "default", adver, LARGE_SEEDS.get(adver, 0), L["U1"], L["I1"], L["B"], L["nb"],
                             n_cand=40 * L["B"])
    return _cache[key]


def conditions(fx):
    """Assert the fixture's conditions on the float64 trajectory alone; returns
    the figures: per batch and pass the regime populations, the crossings of the
    adversarial pass, the smallest margin to a bound in units of margin_bound."""
    lo, hi, batch, nb, d, setting, adver = (fx[k] for k in ("lo", "hi", "B", "nb", "d", "setting", "adver"))
    passes = (("clean", fx["x"], fx["ax"]),) + ((("adv", fx["xa"], fx["axa"]),) if adver else ())
    out = {"populations": {}, "crossings": [], "min_margin": np.inf}
    for name, x, ax in passes:
        r = regimes(x, lo, hi).reshape(nb, batch)
        pops = np.stack([(r == k).sum(1) for k in range(5)], 1)  # [batch, regime]
        out["populations"][name] = pops
        for k in POPULATED[setting]:
            assert pops[:, k].min() >= 2, (name, REGIME_NAMES[k], pops[:, k])
        up = r.ravel() == UPPER
        assert not up.any() or x[up].max() <= UPPER_MAX, (name, x[up].max())
        for bound in (lo, hi):
            ratio = np.abs(x - bound) / margin_bound(d, ax)
            out["min_margin"] = min(out["min_margin"], float(ratio.min()))
            # every triplet: the cap on left-out cases is zero
            assert ratio.min() > 1.0, (name, bound, float(ratio.min()))
    if adver and setting == "tight":
        inside, inside_a = ((v >= lo) & (v <= hi) for v in (fx["x"], fx["xa"]))
        for t in range(nb):
            s = slice(t * batch, (t + 1) * batch)
            out["crossings"].append((int((inside[s] & ~inside_a[s]).sum()), int((~inside[s] & inside_a[s]).sum())))
            assert min(out["crossings"][-1]) >= 2, (t, out["crossings"][-1])
    # rows that only clipped triplets touch, in both passes
    clipped = (fx["x"] < lo) | (fx["x"] > hi)
    if adver:
        clipped &= (fx["xa"] < lo) | (fx["xa"] > hi)
    for rows, cols in ((fx["clipped_users"], (fx["u"],)), (fx["clipped_items"], (fx["i"], fx["j"]))):
        assert len(rows) >= 1
        for row in rows:
            hit = np.zeros(len(clipped), bool)
            for c in cols:
                hit |= c == row
            assert hit.sum() >= nb and clipped[hit].all(), row
            if adver:
                assert np.array_equal(fx["xa"][hit], fx["x"][hit]), row  # zero delta: the same score
    return out


def oracle_run(oracle, fx):
    """(tables, loss_clean, loss_adv, deltas) of the fp32 oracle (oracle.apr_batch,
    HParams(clip_lo, clip_hi)) on fx's batches, computed once per fixture."""
    if "oracle" not in fx:
        from apr_oracle import HParams
        hp = HParams(adver=fx["adver"], clip_lo=fx["lo"], clip_hi=fx["hi"], eps=EPS, lr=LR)
        P, Q = fx["P"].copy(), fx["Q"].copy()
        aP, aQ = np.full(P.shape, 0.1, np.float32), np.full(Q.shape, 0.1, np.float32)
        lcs, las, deltas = [], [], []
        for t in range(fx["nb"]):
            s = slice(t * fx["B"], (t + 1) * fx["B"])
            lc, la, dP, dQ = oracle.apr_batch(P, Q, aP, aQ, fx["u"][s], fx["i"][s], fx["j"][s], hp, want_delta=True)
            lcs.append(lc)
            las.append(la)
            deltas.append((dP, dQ))
        out = ((P, Q, aP, aQ), np.concatenate(lcs), np.concatenate(las), deltas)
        for a in out[0] + out[1:3] + tuple(x for pair in deltas for x in pair):
            a.setflags(write=False)
        fx["oracle"] = out
    return fx["oracle"]


def oracle_samples(oracle, fx, n=4):
    """The oracle's run and n more with its sums taken in other orders, mapped
    back to fx's order: the table columns permuted (every dot product reordered)
    and the triplets permuted inside each batch (every row's sum over its
    occurrences reordered).  Neither changes the result in exact arithmetic; a
    kernel sums in yet another order, so the spread of these runs around float64
    is the reference's own error.  [(tables, loss_clean, loss_adv, deltas)]."""
    if "samples" not in fx:
        out = [oracle_run(oracle, fx)]
        rng = np.random.default_rng(1)
        B, d = fx["B"], fx["d"]
        for _ in range(n):
            cols = rng.permutation(d)
            tp = np.concatenate([t * B + rng.permutation(B) for t in range(fx["nb"])])
            fy = {k: fx[k] for k in ("adver", "lo", "hi", "nb", "B")}
            fy.update(P=np.ascontiguousarray(fx["P"][:, cols]), Q=np.ascontiguousarray(fx["Q"][:, cols]),
                      u=fx["u"][tp], i=fx["i"][tp], j=fx["j"][tp])
            tabs, lc, la, deltas = oracle_run(oracle, fy)
            back, inv = np.argsort(cols), np.argsort(tp)
            out.append((tuple(a[:, back] for a in tabs), lc[inv], la[inv],
                        [(a[:, back], b[:, back]) for a, b in deltas]))
        fx["samples"] = out
    return fx["samples"]


def upper_rtol(fx, samples):
    """rtol of the upper-tail losses (atol 0): 4x the fp32 oracle's own largest
    relative distance from float64 on those triplets (oracle_samples), floored at 1e-5."""
    r = 0.0
    for _, lc_o, la_o, _ in samples:
        for x, got, want in ((fx["x"], lc_o, fx["lc"]),) + (((fx["xa"], la_o, fx["la"]),) if fx["adver"] else ()):
            up = regimes(x, fx["lo"], fx["hi"]) == UPPER
            if up.any():
                r = max(r, float((np.abs(got[up].astype(np.float64) - want[up]) / want[up]).max()))
    return max(1e-5, 4.0 * r)


def bars(oracle, fx, few_step_scale, tables=True):
    """(k, kd, upper-tail rtol) of fx, from the reference alone: k of the project
    bar for the tables and losses (or the losses alone), kd for the delta tables
    (few_step_scale = _few_step_scale of test_gpu_step_geometry.py: 1 where every
    oracle sample holds the bar against float64, else 4x the largest distance)."""
    key = ("bars", tables)
    if key not in fx:
        smp = oracle_samples(oracle, fx)
        got = [a for tabs, lc, la, _ in smp for a in (list(tabs) if tables else []) + [lc, la]]
        k = few_step_scale(got, list(fx["f64"][0 if tables else 4:]) * len(smp))
        kd = 1.0
        if fx["adver"] and tables:
            kd = few_step_scale([a for s in smp for pair in s[3] for a in pair],
                                [a for pair in fx["deltas"] for a in pair] * len(smp))
        fx[key] = (k, kd, upper_rtol(fx, smp))
    return fx[key]


# ---------------------------------------------------------------------------
# the exact-bound case: one batch; a handful of triplets on rows with a single
# non-zero element each (a power of two in the user row), used by no other
# triplet, so the score is exact in any summation order
def exact_problem(d, setting):
    """(fx, at_bound, outside): fx as problem() with nb = 1 and adver = 1 (its
    clean pass is the BPR step's); at_bound / outside list (index of the triplet,
    bound) of the triplets with x == bound exactly, which pass gradient, and with
    x the next float outside it, which do not.  Default bounds: clip_lo only
    (x = clip_hi = 1e8 passes a gradient of zero)."""
    key = ("exact", d, setting)
    if key in _cache:
        return _cache[key]
    lo, hi = BOUNDS[setting]
    f32 = np.float32
    if setting == "default":  # 8 * -10 = -80; 8 * nextafter(-10) = nextafter(-80)
        cases = ((f32(8), f32(-10), lo, True), (f32(8), np.nextafter(f32(-10), f32(-np.inf)), lo, False))
    else:
        cases = ((f32(1), f32(lo), lo, True), (f32(1), np.nextafter(f32(lo), f32(-np.inf)), lo, False),
                 (f32(1), f32(hi), hi, True), (f32(1), np.nextafter(f32(hi), f32(np.inf)), hi, False))
    n = len(cases)
    nu, ni = U1, I1
    rng = np.random.default_rng(9000 + d + (setting == "tight"))
    P0, Q0 = make_tables(rng, nu, ni, d)
    # ordinary rows first, then the exact rows, then the always-clipped rows (make_tables)
    ou, oi = nu - 2 - n, ni - 4 - 2 * n
    u, i, j = _pick_batch(rng, P0.astype(np.float64), Q0.astype(np.float64), d, setting, ou, oi, B - 2 - n)
    at_bound, outside = [], []
    cols = (0, d - 1, 5, d - 4)  # the first and the last chunk of the row among them
    for k, (pv, qv, bound, passes) in enumerate(cases):
        urow, ipos, ineg = ou + k, oi + 2 * k, oi + 2 * k + 1
        P0[urow], Q0[ipos], Q0[ineg] = 0, 0, 0
        P0[urow, cols[k]], Q0[ipos, cols[k]] = pv, qv
        assert f32(pv * qv) == (f32(bound) if passes else np.nextafter(f32(bound), f32(np.sign(qv) * np.inf)))
        (at_bound if passes else outside).append((len(u), bound))
        u, i, j = np.append(u, urow), np.append(i, ipos), np.append(j, ineg)
    u, i, j = np.append(u, [nu - 1, nu - 2]), np.append(i, [ni - 2, ni - 4]), np.append(j, [ni - 1, ni - 3])
    P, Q = P0.astype(np.float64), Q0.astype(np.float64)
    aP, aQ = (np.full(a.shape, np.float64(np.float32(0.1))) for a in (P, Q))
    x, ax, xa, axa, dP, dQ = scores64(P, Q, u, i, j, 1, lo, hi)
    fx = dict(d=d, setting=setting, adver=1, lo=lo, hi=hi, B=B, nb=1, U1=nu, I1=ni, P=P0, Q=Q0,
              u=u.astype(np.int32), i=i.astype(np.int32), j=j.astype(np.int32), x=x, ax=ax, xa=xa, axa=axa)
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = (fx, at_bound, outside)
    return _cache[key]
