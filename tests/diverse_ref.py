"""The numpy yardstick of ops.list_similarity and ops.rerank_mmr: the contract of
include/acf_apr.h restated with np.float32 operations for the chains (one IEEE
rounding per operation, as tests/nbr_ref.py does, so the bits are the kernel's)
and np.float64 for the ILS sums.  Shared by test_diverse_host.py (which checks it
against brute force) and test_gpu_diverse.py (which holds the GPU to it)."""
import numpy as np

METRICS = ("dot", "cosine", "euclid")
F0 = np.float32(0.0)


def _rows(T, ids):
    """T's rows for an id array of any shape: negative and out-of-range ids read row 0."""
    T = np.asarray(T, np.float32)
    ids = np.asarray(ids, np.int64)
    return T[np.where((ids < 0) | (ids >= T.shape[0]), 0, ids)]


def pair_sims(T, ids, metric):
    """[n, m, m] f32: sim(T[ids[r, a]], T[ids[r, b]]) for every pair of positions,
    section 4h's arithmetic (k ascending from +0.0, every operation rounded)."""
    R = _rows(T, ids)  # [n, m, d]
    n, m, d = R.shape
    acc = np.zeros((n, m, m), np.float32)
    with np.errstate(all="ignore"):
        if metric == "euclid":
            for k in range(d):
                diff = R[:, :, None, k] - R[:, None, :, k]
                acc = acc + diff * diff
            return F0 - acc
        for k in range(d):
            acc = acc + R[:, :, None, k] * R[:, None, :, k]
        if metric == "dot":
            return acc
        assert metric == "cosine", metric
        n2 = np.zeros((n, m), np.float32)
        for k in range(d):
            n2 = n2 + R[:, :, k] * R[:, :, k]
        nrm = np.sqrt(n2)
        den = nrm[:, :, None] * nrm[:, None, :]
        quot = acc / np.where(den > 0, den, np.float32(1.0))
        return np.where(den > 0, quot + F0, F0).astype(np.float32)


def tree_mean(values, flags):
    """The mean of values[flags] as k_div_means adds it: thread t of 256 adds rows
    t, t + 256, ... ascending, a halving tree adds the 256 sums, one division."""
    part = np.zeros(256, np.float64)
    cnt = 0
    for r in range(len(values)):
        if flags[r]:
            part[r % 256] = part[r % 256] + np.float64(values[r])
            cnt += 1
    off = 128
    while off > 0:
        part[:off] = part[:off] + part[off:2 * off]
        off >>= 1
    return part[0] / np.float64(cnt) if cnt else np.float64(0.0)


def list_similarity(T, lists, cutoffs, metric, sims=None):
    """(ils f64 [n, n_cut], means f64 [n_cut])."""
    lists = np.asarray(lists, np.int64)
    n, k = lists.shape
    kmax = max(cutoffs)
    valid = lists >= 0
    sims = pair_sims(T, lists[:, :kmax], metric) if sims is None else sims
    c = np.zeros((n, kmax), np.float64)  # c_b: a ascending, fp64
    pos = np.arange(kmax)
    for a in range(kmax):
        take = valid[:, a, None] & valid[:, :kmax] & (pos[None, :] > a)
        c = c + np.where(take, sims[:, a, :kmax].astype(np.float64), 0.0)
    ils = np.zeros((n, len(cutoffs)), np.float64)
    flags = np.zeros((n, len(cutoffs)), bool)
    for q, K in enumerate(cutoffs):
        S = np.zeros(n, np.float64)
        for b in range(K):  # b ascending
            S = S + np.where(valid[:, b], c[:, b], 0.0)
        L = valid[:, :K].sum(axis=1)
        flags[:, q] = L >= 2
        pairs = (L * (L - 1) // 2).astype(np.float64)
        ils[:, q] = np.where(flags[:, q], S / np.where(flags[:, q], pairs, 1.0), 0.0)
    means = np.array([tree_mean(ils[:, q], flags[:, q]) for q in range(len(cutoffs))], np.float64)
    return ils, means


def rerank_mmr(T, cand, rel, k_out, lam, metric, sims=None):
    """(items i32 [n, k_out], rel f32 [n, k_out], obj f32 [n, k_out])."""
    cand = np.asarray(cand, np.int32)
    rel = np.asarray(rel, np.float32)
    n, m = cand.shape
    sims = pair_sims(T, cand, metric) if sims is None else sims
    lam = np.float32(lam)
    oml = np.float32(1.0) - lam
    items = np.full((n, k_out), -1, np.int32)
    rel_out = np.full((n, k_out), -np.inf, np.float32)
    obj = np.full((n, k_out), -np.inf, np.float32)
    with np.errstate(all="ignore"):
        for r in range(n):
            open_ = (cand[r] >= 0) & np.isfinite(rel[r])
            a = lam * rel[r]
            pen = np.zeros(m, np.float32)
            for j in range(k_out):
                if not open_.any():
                    break
                o = a if j == 0 else a - oml * pen
                idx = np.nonzero(open_)[0]
                best = idx[np.argmax(o[idx])]  # the first of the largest: ties to the lower position
                items[r, j], rel_out[r, j], obj[r, j] = cand[r, best], rel[r, best], o[best]
                open_[best] = False
                s = sims[r, :, best]
                pen = s.copy() if j == 0 else np.maximum(pen, s)
    return items, rel_out, obj
