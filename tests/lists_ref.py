"""The numpy yardstick of the list-level robustness ops (ops.list_compare,
ops.list_exposure, ops.exposure_metrics): the definitions of include/acf_apr.h
restated plainly, in fp64 and Python ints, one row at a time."""
import math

import numpy as np


def compare_row(a, b, cutoffs, p):
    """[(overlap, jaccard, rbo) per cutoff] of one pair of lists, and whether the row is scored."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    la, lb = sum(x >= 0 for x in a), sum(x >= 0 for x in b)
    depth = [len({x for x in a[:d] if x >= 0} & {x for x in b[:d] if x >= 0}) for d in range(1, len(a) + 1)]
    out = []
    for K in cutoffs:
        D = min(int(K), max(la, lb))
        if D == 0:
            out.append((0.0, 0.0, 0.0))
            continue
        X = depth[:D]  # X_d, d = 1..D
        pw, total = 1.0, 0.0
        for d in range(1, D + 1):  # d ascending, p^d by repeated multiplication
            pw *= p
            total += (X[d - 1] / d) * pw
        rbo = (X[-1] / D) * pw + ((1.0 - p) / p) * total
        out.append((float(X[-1]), X[-1] / (min(la, D) + min(lb, D) - X[-1]), rbo))
    return out, max(la, lb) > 0


def compare(A, B, cutoffs, p):
    """per_user [n, n_cut, 3], mean [n_cut, 3] over the scored rows, n_scored [n_cut]."""
    A, B = np.asarray(A), np.asarray(B)
    n, nc = A.shape[0], len(cutoffs)
    per_user, scored = np.zeros((n, nc, 3)), np.zeros(n, bool)
    for r in range(n):
        rows, scored[r] = compare_row(A[r], B[r], cutoffs, p)
        per_user[r] = rows
    ns = int(scored.sum())
    mean = np.array([[math.fsum(per_user[scored, c, m]) / ns if ns else 0.0 for m in range(3)] for c in range(nc)])
    return per_user, mean.reshape(nc, 3), np.full(nc, ns, np.int64)


def exposure_counts(lists, num_items, cutoffs):
    """counts int64 [n_cut, num_items] by np.bincount."""
    lists = np.asarray(lists)
    out = []
    for K in cutoffs:
        ids = lists[:, :K].reshape(-1)
        ids = ids[(ids >= 0) & (ids < num_items)]
        out.append(np.bincount(ids, minlength=num_items))
    return np.stack(out).astype(np.int64)


def exposure_metrics_row(counts, pop=None, tail=None):
    """(total, coverage, gini, entropy, arp, aplt) of one row of counts: Python ints, one division each."""
    c = [int(x) for x in np.asarray(counts)]
    N, T = len(c), sum(c)
    if T == 0:
        return (0.0,) * 6
    s = [int(x) for x in np.sort(np.asarray(counts))]
    G = sum((2 * j - N - 1) * s[j - 1] for j in range(1, N + 1))
    entropy = -math.fsum((x / T) * math.log2(x / T) for x in c if x > 0)
    arp = sum(x * int(q) for x, q in zip(c, pop)) / T if pop is not None else 0.0
    aplt = sum(x for x, t in zip(c, tail) if t) / T if tail is not None else 0.0
    return (float(T), sum(x > 0 for x in c) / N, G / (N * T), entropy + 0.0, arp, aplt)


def exposure_metrics(counts, pop=None, tail=None):
    return np.array([exposure_metrics_row(row, pop, tail) for row in np.asarray(counts)])
