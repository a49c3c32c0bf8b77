"""The fixture test_adv_pgd_host.py and test_gpu_adv_pgd.py share: 37 user rows x
53 item rows, sigma = 0.1 tables and 1,400 triplets that hit every path of the
whole-stream direction (csrc/acf_adv.h):
  user row 3    300 triplets = 600 terms: three chunks of ADV_CHUNK = 256
  item row 7    exactly 256 terms (200 as the positive, 56 as the negative): one full chunk
  item row 11   a single term
  user row 36 and item row 52 (and whatever the draw leaves out): no term at all
Everything is a pure function of (d, seed); nothing here needs a GPU."""
import numpy as np

U1, I1, N = 37, 53, 1400
DIMS = (8, 64, 100)  # row geometries (LPR, NV) = (2, 1), (16, 1), (32, 1)
HOT_USER, FULL_ITEM, ONCE_ITEM, FREE_USER, FREE_ITEM = 3, 7, 11, 36, 52
EPS, ITERS = 0.2, 5
MIX_SEED = 5  # start table of the mixed projection case: see mixed_start


def problem(d, seed=0):
    rng = np.random.default_rng(1000 * seed + d)
    P = (rng.standard_normal((U1, d)) * 0.1).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.1).astype(np.float32)
    users = np.setdiff1d(np.arange(U1), [HOT_USER, FREE_USER])
    items = np.setdiff1d(np.arange(I1), [FULL_ITEM, ONCE_ITEM, FREE_ITEM])
    u = rng.choice(users, N).astype(np.int32)
    i = rng.choice(items, N).astype(np.int32)
    j = rng.choice(items, N).astype(np.int32)
    u[:300] = HOT_USER
    i[300:500] = FULL_ITEM
    j[500:556] = FULL_ITEM
    i[600] = ONCE_ITEM
    return P, Q, u, i, j


def term_counts(u, i, j):
    """Terms per user row and per item row (two per triplet for the user, one per item occurrence)."""
    return 2 * np.bincount(u, minlength=U1), np.bincount(i, minlength=I1) + np.bincount(j, minlength=I1)


def mixed_start(d, eps=EPS, seed=MIX_SEED):
    """Start tables whose row norms are spread over [0, 2 eps]: with a small step
    some rows stay inside the ball and some are projected."""
    rng = np.random.default_rng(77 * seed + d)
    out = []
    for rows in (U1, I1):
        x = rng.standard_normal((rows, d))
        x *= (rng.uniform(0.0, 2.0 * eps, rows) / np.linalg.norm(x, axis=1))[:, None]
        out.append(x.astype(np.float32))
    return out


def pre_projection_norms(pgd_host, P, Q, u, i, j, alpha, start, side="both"):
    """|delta + alpha n| per row of (P, Q) by the float64 restatement: one step in a
    ball that is never left."""
    dP, dQ, _ = pgd_host(P, Q, u, i, j, 1e30, 1, alpha, side, start)
    return np.linalg.norm(dP, axis=1), np.linalg.norm(dQ, axis=1)


def branches(norms, eps):
    """(projected, skipped) per row: rows within 1e-5 eps of the ball's edge are skipped."""
    return norms > eps, np.abs(norms - eps) <= 1e-5 * eps


def loo_plan(seed=3):
    """A 37-entry leave-one-out plan over all 53 items: (users, tests, excl_off, excl,
    excl_lists); every list holds its user's test item, as init_eval_model's do."""
    rng = np.random.default_rng(seed)
    users = np.arange(U1, dtype=np.int32)
    tests = rng.integers(0, I1, U1).astype(np.int32)
    lists = [np.union1d(rng.integers(0, I1, 5), [t]).astype(np.int32) for t in tests]
    off = np.zeros(U1 + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return users, tests, off, np.concatenate(lists), lists
