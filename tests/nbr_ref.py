"""The numpy yardstick of ops.neighbors_topk (acf_neighbors_topk): the contract of
include/acf_apr.h restated in fp32 with every operation rounded on its own.
numpy's float32 +, -, *, / and sqrt are IEEE correctly rounded, one rounding per
operation, so the bits are the kernel's.  Shared by test_neighbors_host.py (which
checks it against fp64) and test_gpu_neighbors.py (which holds the GPU to it)."""
import numpy as np

METRICS = ("dot", "cosine", "euclid")
F0 = np.float32(0.0)


def seq_dot(A, B):
    """[n, m] f32: s = s + A[:, k] * B[:, k] for k ascending from +0.0."""
    s = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k in range(A.shape[1]):
        s = s + A[:, k, None] * B[None, :, k]
    return s


def row_norms(A):
    """[n] f32: sqrt of the same chain over A[:, k]^2."""
    s = np.zeros(A.shape[0], np.float32)
    for k in range(A.shape[1]):
        s = s + A[:, k] * A[:, k]
    return np.sqrt(s)


def nbr_scores(T, X, queries, metric, num_cand=None, check=False):
    """[n, num_cand] f32 scores of rows X[queries] against T[:num_cand].  A query
    outside X is read as row 0 (check: IndexError instead)."""
    T = np.asarray(T, np.float32)
    X = T if X is None else np.asarray(X, np.float32)
    num_cand = T.shape[0] if num_cand is None else num_cand
    q = np.asarray(queries, np.int64).reshape(-1)
    bad = (q < 0) | (q >= X.shape[0])
    if check and bad.any():
        raise IndexError("query outside the query table")
    q = np.where(bad, 0, q)
    A, B = X[q], T[:num_cand]
    with np.errstate(all="ignore"):
        if metric == "euclid":
            d2 = np.zeros((len(q), num_cand), np.float32)
            for k in range(T.shape[1]):
                diff = A[:, k, None] - B[None, :, k]
                d2 = d2 + diff * diff
            return F0 - d2
        s = seq_dot(A, B)
        if metric == "dot":
            return s
        assert metric == "cosine", metric
        den = row_norms(A)[:, None] * row_norms(B)[None, :]
        quot = s / np.where(den > 0, den, np.float32(1.0))
        return np.where(den > 0, quot + F0, F0).astype(np.float32)


def nbr_reference(T, X, queries, metric, k, num_cand=None, exclude_self=True, lists=None, check=False):
    """(items int32 [n, k], scores f32 [n, k]): per query the candidates [0,
    num_cand) minus the SET of lists[j] (out-of-range entries ignored) minus, with
    exclude_self, the id of the query (0 for a query outside X), ordered by score
    descending then id ascending; -1 / -inf past the last candidate."""
    T = np.asarray(T, np.float32)
    num_cand = T.shape[0] if num_cand is None else num_cand
    rows = (T if X is None else np.asarray(X)).shape[0]
    q = np.asarray(queries, np.int64).reshape(-1)
    scores = nbr_scores(T, X, q, metric, num_cand, check)
    q = np.where((q < 0) | (q >= rows), 0, q)
    items = np.full((len(q), k), -1, np.int32)
    out = np.full((len(q), k), -np.inf, np.float32)
    for j in range(len(q)):
        keep = np.ones(num_cand, bool)
        if lists is not None:
            ex = np.asarray(lists[j], np.int64)
            keep[ex[(ex >= 0) & (ex < num_cand)]] = False
        if exclude_self and q[j] < num_cand:
            keep[q[j]] = False
        ids = np.nonzero(keep)[0]
        s = scores[j, ids]
        sel = ids[np.lexsort((ids, -s))][:k]
        items[j, :len(sel)] = sel
        out[j, :len(sel)] = scores[j, sel]
    return items, out


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return off, flat.astype(np.int32)
