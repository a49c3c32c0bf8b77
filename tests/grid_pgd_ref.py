"""Reference of one grid member's batch step against a K-step inner attack
(ops.grid_train with StepHParams.adv_iters = K), written from the
semantics, not from the kernel:

  delta_0 = 0; for k = 1 .. K: g_k = the batch's BPR gradient per row at
  (P + delta_{k-1}, Q + delta_{k-1}); n_k = g_k / sqrt(max(g_k . g_k, 1e-12));
  v = delta_{k-1} + alpha * n_k; delta_k = v if |v| <= eps else v * (eps / |v|).
  K = 1 is APR's delta = eps * n_1.  Then G = G0 (clean, unperturbed tables) + the reg
  term + reg_adv * G_adv(delta_K), Adagrad on the batch's rows; loss_adv is the
  per-triplet loss at delta_K.  alpha None: 2.5 * eps / K.

step64: float64 numpy, the yardstick; its delta loop is evaluate.pgd_host, the fp64
yardstick of ops.adv_pgd.  step32: the same step in float32 with every row's terms
summed in the plan's order (a user row: its pos-branch terms in triplet order, then
its neg-branch terms; an item row: its terms as a positive, then as a negative; 256
terms per partial sum, partial sums added in order) and every product rounded before
it is added.  step32 models the fp32 rounding of the step, not the kernel's dot-product
tree; the distance between the two is what the GPU tests' tolerance is derived from
(deviation).
"""
import importlib

import numpy as np

from conftest import PKG

DEFAULTS = dict(lr=0.05, eps=0.5, reg=0.0, reg_adv=1.0, adver=0, clip_lo=-80.0, clip_hi=1e8, adv_iters=1,
                adv_step=None)
CHUNK = 256


def hparams(hp):
    """hp (a dict of StepHParams fields) with the defaults filled in and alpha resolved."""
    h = dict(DEFAULTS, **hp)
    if h["adv_step"] is None:
        h["adv_step"] = 2.5 * h["eps"] / h["adv_iters"]
    return h


# ---- float64 ------------------------------------------------------------------------
def _terms64(P, Q, u, i, j, lo, hi):
    """(g, loss) per triplet and the per-row gradient sums (gP, gQ) at the given tables."""
    p, qi, qj = P[u], Q[i], Q[j]
    x = (p * qi).sum(1) - (p * qj).sum(1)
    xc = np.clip(x, lo, hi)
    g = -1.0 / (np.exp(xc) + 1.0) * ((x >= lo) & (x <= hi))
    gP, gQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(gP, u, g[:, None] * qi)
    np.add.at(gP, u, -g[:, None] * qj)
    np.add.at(gQ, i, g[:, None] * p)
    np.add.at(gQ, j, -g[:, None] * p)
    return np.logaddexp(0.0, -xc), gP, gQ


def _unit64(t):
    return t / np.sqrt(np.maximum((t * t).sum(1, keepdims=True), 1e-12))


def delta64(P, Q, u, i, j, h):
    """(delta_P, delta_Q) of the batch, dense float64 (rows outside the batch stay 0)."""
    K, eps = h["adv_iters"], h["eps"]
    if K == 1:
        _, gP, gQ = _terms64(P, Q, u, i, j, h["clip_lo"], h["clip_hi"])
        return _unit64(gP) * eps, _unit64(gQ) * eps
    pgd_host = importlib.import_module(PKG + ".evaluate").pgd_host
    dP, dQ, _ = pgd_host(P, Q, u, i, j, eps, iters=K, alpha=h["adv_step"], lo=h["clip_lo"], hi=h["clip_hi"])
    return dP, dQ


def gradient64(P, Q, u, i, j, h):
    """(loss_clean, loss_adv, G_P, G_Q, delta_P, delta_Q) of one batch, float64."""
    B, d = len(u), P.shape[1]
    lc, GP, GQ = _terms64(P, Q, u, i, j, h["clip_lo"], h["clip_hi"])
    la, dP, dQ = np.zeros(B), np.zeros_like(P), np.zeros_like(Q)
    if h["reg"]:
        coef = 2.0 * h["reg"] / (B * d) * (2.0 if h["adver"] else 1.0)
        GP += coef * np.bincount(u, minlength=len(P))[:, None] * P
        GQ += coef * (np.bincount(i, minlength=len(Q)) + np.bincount(j, minlength=len(Q)))[:, None] * Q
    if h["adver"]:
        dP, dQ = delta64(P, Q, u, i, j, h)
        la, aP, aQ = _terms64(P + dP, Q + dQ, u, i, j, h["clip_lo"], h["clip_hi"])
        GP += h["reg_adv"] * aP
        GQ += h["reg_adv"] * aQ
    return lc, la, GP, GQ, dP, dQ


def step64(P, Q, accP, accQ, u, i, j, hp):
    """One batch on float64 tables, in place: (loss_clean, loss_adv)."""
    h = hparams(hp)
    u, i, j = (np.asarray(x, dtype=np.int64) for x in (u, i, j))
    lc, la, GP, GQ, _, _ = gradient64(P, Q, u, i, j, h)
    for W, A, G, rows in ((P, accP, GP, np.unique(u)), (Q, accQ, GQ, np.unique(np.concatenate([i, j])))):
        A[rows] += G[rows] * G[rows]
        W[rows] -= h["lr"] * G[rows] / np.sqrt(A[rows])
    return lc, la


# ---- float32, plan order --------------------------------------------------------------
f32 = np.float32


def _dot32(a, b):
    return (a * b).sum(dtype=f32)


def _bpr32(x, lo, hi):
    xc = min(max(x, lo), hi)
    with np.errstate(over="ignore"):
        g = -f32(1) / (np.exp(xc) + f32(1)) if lo <= x <= hi else f32(0)
        loss = f32(np.logaddexp(f32(0), -xc))
    return f32(g), loss


def _sums32(P, Q, dP, dQ, u, i, j, lo, hi):
    """Per unique row of the batch its gradient sum at (P + dP, Q + dQ) in the plan's
    order: ({row: sum} for users, {row: sum} for items, per-triplet loss)."""
    B = len(u)
    g, loss, rows3 = np.zeros(B, f32), np.zeros(B, f32), []
    for t in range(B):
        p, qi, qj = P[u[t]] + dP[u[t]], Q[i[t]] + dQ[i[t]], Q[j[t]] + dQ[j[t]]
        g[t], loss[t] = _bpr32(_dot32(p, qi) - _dot32(p, qj), lo, hi)
        rows3.append((p, qi, qj))

    def total(terms):  # [(coefficient, vector)] in plan order, 256 per partial sum
        tot = None
        for c0 in range(0, len(terms), CHUNK):
            acc = np.zeros_like(terms[0][1])
            for c, x in terms[c0:c0 + CHUNK]:
                acc = acc + c * x
            tot = acc if tot is None else tot + acc
        return tot

    sP = {r: total([(g[t], rows3[t][1]) for t in range(B) if u[t] == r] +
                   [(-g[t], rows3[t][2]) for t in range(B) if u[t] == r]) for r in np.unique(u)}
    sQ = {r: total([(g[t], rows3[t][0]) for t in range(B) if i[t] == r] +
                   [(-g[t], rows3[t][0]) for t in range(B) if j[t] == r]) for r in np.unique(np.concatenate([i, j]))}
    return sP, sQ, loss


def _unit32(g):
    return g * (f32(1) / np.sqrt(np.maximum(_dot32(g, g), f32(1e-12))))


def step32(P, Q, accP, accQ, u, i, j, hp):
    """One batch on float32 tables, in place, in the plan's order: (loss_clean, loss_adv)."""
    h = hparams(hp)
    u, i, j = (np.asarray(x, dtype=np.int64) for x in (u, i, j))
    B, d = len(u), P.shape[1]
    lo, hi, eps, alpha = f32(h["clip_lo"]), f32(h["clip_hi"]), f32(h["eps"]), f32(h["adv_step"])
    zP, zQ = np.zeros_like(P), np.zeros_like(Q)
    GP, GQ, lc = _sums32(P, Q, zP, zQ, u, i, j, lo, hi)
    la = np.zeros(B, f32)
    cu, ci = np.bincount(u, minlength=len(P)), np.bincount(np.concatenate([i, j]), minlength=len(Q))
    coef = (f32(2) * f32(h["reg"]) / (f32(B) * f32(d))) * f32(2 if h["adver"] else 1)
    if h["adver"]:
        dP, dQ = zP.copy(), zQ.copy()
        sP, sQ = GP, GQ
        for k in range(h["adv_iters"]):
            if k:
                sP, sQ, _ = _sums32(P, Q, dP, dQ, u, i, j, lo, hi)
            for dl, sums in ((dP, sP), (dQ, sQ)):
                for r, g in sums.items():
                    if h["adv_iters"] == 1:
                        dl[r] = _unit32(g) * eps
                        continue
                    v = dl[r] + alpha * _unit32(g)
                    s = np.sqrt(_dot32(v, v))
                    dl[r] = v if s <= eps else v * (eps / s)
        aP, aQ, la = _sums32(P, Q, dP, dQ, u, i, j, lo, hi)
    for W, A, G, cnt, adv in ((P, accP, GP, cu, aP if h["adver"] else None),
                              (Q, accQ, GQ, ci, aQ if h["adver"] else None)):
        for r, g in G.items():
            if h["reg"]:
                g = g + (coef * f32(cnt[r])) * W[r]
            if adv is not None:
                g = g + f32(h["reg_adv"]) * adv[r]
            A[r] = A[r] + g * g
            W[r] = W[r] - (f32(h["lr"]) * g) * (f32(1) / np.sqrt(A[r]))
    return lc, la


# ---- a member over a stream of batches, and the tolerance ------------------------------
def run_member(step, P, Q, u, i, j, batch, hp, dtype):
    """A member's tables through every batch of the stream by `step`:
    ((P, Q, accP, accQ), loss_clean, loss_adv), accumulators from 0.1."""
    P, Q = P.astype(dtype), Q.astype(dtype)
    aP, aQ = np.full(P.shape, 0.1, dtype), np.full(Q.shape, 0.1, dtype)
    lcs, las = [], []
    for t in range(len(u) // batch):
        s = slice(t * batch, (t + 1) * batch)
        lc, la = step(P, Q, aP, aQ, u[s], i[s], j[s], hp)
        lcs.append(lc)
        las.append(la)
    return (P, Q, aP, aQ), np.concatenate(lcs), np.concatenate(las)


def deviation(got, want, atol):
    """The smallest rtol at which every element of got is within atol + rtol * |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    over = np.maximum(np.abs(got - want) - atol, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(over > 0, over / np.abs(want), 0.0)
    return float(r.max()) if r.size else 0.0


# ---- the inputs of the GPU tests (tests/test_gpu_grid_pgd.py), shared with the CPU tests ---
RTOL, ATOL = 1e-5, 1e-6       # the project's single-step tolerance: the floor
U1, I1, B, NB = 65, 49, 32, 3  # the shape of tests/test_gpu_grid.py

# K = 1, K = 2 with alpha = eps / (2K) (the iterates stay inside the ball), K = 3 with
# alpha = eps (the projection engages from step 2), K = 5 with reg != 0, a BPR member
HPS_PARITY = (dict(adver=1, eps=0.5), dict(adver=1, eps=0.5, adv_iters=2, adv_step=0.125),
              dict(adver=1, eps=1.0, adv_iters=3, adv_step=1.0, reg_adv=0.5),
              dict(adver=1, eps=2.0, adv_iters=5, reg=0.01, lr=0.1, reg_adv=0.1), dict(adver=0))
HPS_K3 = (dict(adver=1, eps=0.5, adv_iters=3), dict(adver=1, eps=1.0, adv_iters=3, adv_step=1.0, reg=0.01))
PARITY_DIMS = (8, 20, 64, 132, 256)
DEGENERATE = ("hot_user", "hot_item", "pos_equals_neg", "clipped", "eps_zero")


def tables(seed, M, d, u1=U1, i1=I1, scale=0.3):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((M, u1, d)) * scale).astype(np.float32),
            (rng.standard_normal((M, i1, d)) * scale).astype(np.float32))


def triplets(seed, n, u1=U1, i1=I1):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, u1, n).astype(np.int32), rng.integers(0, i1, n).astype(np.int32),
            rng.integers(0, i1, n).astype(np.int32))


def parity_case(d):
    """(P, Q, u, i, j, batch, hps) of the parity test at dim d."""
    P, Q = tables(d, len(HPS_PARITY), d)
    return (P, Q, *triplets(100 + d, NB * B), B, HPS_PARITY)


def degenerate_case(name):
    """(P, Q, u, i, j, batch, hps) of a degenerate / hot-row case, every member at K = 3, d = 64."""
    hps, batch = HPS_K3, B
    u, i, j = triplets(32, NB * B)
    if name == "hot_user":  # one user in all 160 triplets of a batch: 320 terms, two partial sums
        batch = 160
        u, i, j = triplets(31, 2 * batch)
        u[:] = 5
    elif name == "hot_item":  # one item as every positive
        i[:] = 7
        j[j == 7] = 8
    elif name == "pos_equals_neg":  # 8 triplets per batch with i == j on users and items nothing else touches
        u, i, j = triplets(33, NB * B, u1=56, i1=40)
        for b in range(NB):
            t = np.arange(b * B, b * B + 8)
            u[t], i[t], j[t] = 56 + t % 8, 40 + t % 8, 40 + t % 8
    elif name == "clipped":  # a clip of +-0.5 around scores of spread ~1: most terms are zero
        hps = tuple(dict(h, clip_lo=-0.5, clip_hi=0.5) for h in HPS_K3)
    elif name == "eps_zero":  # K = 3, K = 1 and K = 3 with a step, all at eps = 0, on equal tables
        hps = (dict(adver=1, eps=0.0, adv_iters=3), dict(adver=1, eps=0.0),
               dict(adver=1, eps=0.0, adv_iters=3, adv_step=0.3))
    else:
        raise ValueError(name)
    P, Q = tables(40, len(hps), 64)
    if name == "eps_zero":
        P[1:], Q[1:] = P[0], Q[0]
    return P, Q, u, i, j, batch, hps


def base_rtol(u, i, j, batch):
    """test_gpu_grid._rtol: max(1e-5, 2 n u), n the most terms any row of any batch sums."""
    n_terms = 1
    for t in range(len(u) // batch):
        s = slice(t * batch, (t + 1) * batch)
        n_terms = max(n_terms, 2 * np.bincount(u[s]).max(), np.bincount(np.concatenate([i[s], j[s]])).max())
    return max(RTOL, 2 * n_terms * 2.0 ** -24)


_CACHE = {}


def reference(key, case):
    """Per member of a case: the fp64 result and the deviation of the fp32 plan-order
    restatement from it, computed once per key: [(want, lc, la, deviation)]."""
    if key not in _CACHE:
        P, Q, u, i, j, batch, hps = case
        out = []
        for m, hp in enumerate(hps):
            want = run_member(step64, P[m], Q[m], u, i, j, batch, hp, np.float64)
            got = run_member(step32, P[m], Q[m], u, i, j, batch, hp, np.float32)
            dev = max([deviation(g, w, ATOL) for g, w in zip(got[0], want[0])] +
                      [deviation(got[1], want[1], ATOL), deviation(got[2], want[2], ATOL)])
            out.append((*want, dev))
        _CACHE[key] = out
    return _CACHE[key]


def tolerance(key, case):
    """(rtol, atol) of GPU against fp64 for a case: 4 x the largest measured deviation of
    the fp32 restatement over the case's members, never below base_rtol / 1e-6."""
    dev = max(r[3] for r in reference(key, case))
    return max(base_rtol(*case[2:6]), 4.0 * dev), ATOL
