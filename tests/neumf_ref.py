"""The float64 yardstick of the NeuMF gradient: torch-CPU autograd of the graph
oracle/neumf_oracle.py restates in fp32 (the adversarial delta included), the bar
GPU gradients are held to, and the problems of test_gpu_neumf_batches.py.  Shared
by test_neumf_oracle.py (which checks the fp32 oracle and the bar against it
without a GPU) and the GPU modules.

The bar (check_grads), per tensor n:  |got - want| <= 1e-4 |want| + k max|want_n|.
It has no absolute floor: the gradients carry 1/B, and an embedding table's
largest element is ~1e-5 at B in the thousands, so a fixed atol of 1e-6 would let
most of a table pass as zero.  k comes from the reference alone (calibrate): 4x the
fp32 numpy oracle's largest distance from float64, in units of max|want_n|, over a
module's cases.  4x because the GPU adds the same fp32 terms in another fixed order
(split-K over the weight-gradient slots), the room tests/test_gpu_plan.py gives
free-running parity over the oracle's own sensitivity."""
import functools

import numpy as np
import torch

import neumf_oracle as N

TABLES = ("MF_U", "MF_I", "MLP_U", "MLP_I")
RTOL = 1e-4
K_MAX = 1e-4  # calibrate refuses a looser bar than this, whatever the seeds give


def torch_grads_losses(P, u, i, y, hp):
    """(gradients float64 per tensor, clean loss, adversarial loss) by autograd."""
    T = {n: torch.tensor(P[n], dtype=torch.float64, requires_grad=True) for n in N.NAMES}
    ut, it = torch.tensor(u), torch.tensor(i)
    yt = torch.tensor(y, dtype=torch.float64)

    def loss_fn(delta=None):
        mu, mi, lu, li = T["MF_U"][ut], T["MF_I"][it], T["MLP_U"][ut], T["MLP_I"][it]
        if delta is not None:
            mu, mi, lu, li = mu + delta["MF_U"], mi + delta["MF_I"], lu + delta["MLP_U"], li + delta["MLP_I"]
        a1 = torch.relu(torch.cat([lu, li], 1) @ T["W1"] + T["b1"])
        a2 = torch.relu(a1 @ T["W2"] + T["b2"])
        p = torch.sigmoid(torch.cat([mu * mi, a2], 1) @ T["Wo"] + T["bo"])[:, 0]
        pc = torch.clamp(p, 1e-7, 1 - 1e-7)
        return -(yt * torch.log(pc) + (1 - yt) * torch.log(1 - pc)).mean()

    lc = loss_fn()
    total = lc
    la = 0.0
    if hp.adver:
        G = torch.autograd.grad(lc, [T[n] for n in TABLES], retain_graph=True)
        delta = {}
        for n, g in zip(TABLES, G):
            idx = ut if n.endswith("_U") else it
            r = g[idx]
            delta[n] = (hp.eps * r / torch.sqrt(torch.clamp((r * r).sum(1, keepdim=True), min=1e-12))).detach()
        la = loss_fn(delta)
        total = lc + hp.reg_adv * la
    grads = torch.autograd.grad(total, [T[n] for n in N.NAMES])
    return {n: g.numpy() for n, g in zip(N.NAMES, grads)}, float(lc.detach()), float(torch.as_tensor(la).detach())


def _torch_grads(P, u, i, y, hp):
    grads, lc, _ = torch_grads_losses(P, u, i, y, hp)
    return grads, lc


def bar(want, k):
    """The elementwise bound of check_grads for one tensor."""
    want = np.asarray(want, np.float64)
    return RTOL * np.abs(want) + k * np.abs(want).max()


def check_grads(got, want64, k, what=""):
    """Every tensor of `got` (name -> array) within the bar of the float64 gradient;
    a tensor whose reference gradient is all zero checks nothing and is refused."""
    for n in N.NAMES:
        want = np.asarray(want64[n], np.float64)
        g = np.asarray(got[n], np.float64)
        assert g.shape == want.shape, f"{what}{n}: shape {g.shape} != {want.shape}"
        top = float(np.abs(want).max())
        assert top > 0, f"{what}{n}: the reference gradient is all zero"
        err = np.abs(g - want)
        over = err > bar(want, k)
        if over.any() or not np.isfinite(g).all():
            w = np.unravel_index(np.argmax(err - bar(want, k)), err.shape)
            raise AssertionError(f"{what}{n}: {int(over.sum())} of {want.size} elements outside rtol {RTOL:g} + "
                                 f"{k:.3g} max|want| (max|want| {top:.3e}); worst at {w}: got {g[w]:.9e}, "
                                 f"want {want[w]:.9e}")


def oracle_distance(oracle_g, want64):
    """name -> max|oracle - want| / max|want| of the fp32 oracle's gradient."""
    return {n: float(np.abs(np.asarray(oracle_g[n], np.float64) - want64[n]).max() / np.abs(want64[n]).max())
            for n in N.NAMES}


def calibrate(distances):
    """k of check_grads from the oracle's distances (dicts of oracle_distance) of a
    module's cases: 4x the largest; a bar looser than K_MAX is refused."""
    k = 4.0 * max(max(d.values()) for d in distances)
    assert 0 < k <= K_MAX, f"calibrated k = {k:.3e} outside (0, {K_MAX:g}]"
    return k


# ---- the problems of test_gpu_neumf_batches.py -------------------------------
EPS, REG_ADV = 0.5, 0.7
SPARE = 13  # the row that takes the places a planted row must not have

# (B, d, U1, I1): one gradient each, adver 0 and 1
GRAD_CASES = (
    (1040, 16, 500, 300),    # the first block count past the in-line limit
    (2064, 8, 500, 300),     # two staging rounds of k_nmf_rows, wgrad_group<false>
    (2064, 64, 500, 300),    # two staging rounds
    (4112, 64, 500, 300),    # 257 blocks: workgroup 0 runs a second, full block (d = DFAST)
    (4100, 36, 500, 300),    # a workgroup's second block is short (nt = 4), partial panels
    (5000, 128, 2000, 3000),  # weights read from global, 313 blocks
    (8200, 64, 500, 300),    # three blocks for the first workgroups
)
LIMIT_CASES = ((1024, 16, 500, 300), (1040, 16, 500, 300))  # both sides of FR_MAXB
DIM_CASES = tuple((B, d, 41, 37) for d in (4, 12, 36, 100) for B in (96, 300))


def all_cases():
    seen = []
    for c in GRAD_CASES + LIMIT_CASES + DIM_CASES:
        for adver in (0, 1):
            if (c, adver) not in seen:
                seen.append((c, adver))
    return seen


def case_id(c):
    return "B%d-d%d" % (c[0], c[1])


def _fill(rng, B, rows, draws, fixed, first_at, only):
    """draws with every row present (when the free places allow), then the planted
    places: fixed {position: row}; first_at {row: position of its first
    occurrence}; only: rows with no occurrence but their fixed one."""
    x = np.asarray(draws, np.int64).copy()
    free = np.setdiff1d(np.arange(B), np.fromiter(fixed, np.int64, len(fixed)))
    if len(free) >= rows:
        x[rng.permutation(free)[:rows]] = np.arange(rows)
    for r, p in first_at.items():
        head = x[:p]
        head[head == r] = SPARE
    for r in only:
        x[x == r] = SPARE
    for p, r in fixed.items():
        x[p] = r
    return x.astype(np.int32)


def plants(B):
    """The planted places of a batch of B >= 2,064 (RCH = 2,048 indices per staging
    round of k_nmf_rows, blocks of 16): (user side, item side), each (fixed,
    first_at, only).  Users: row 7 at 0, 2047, 2048 and B-1 (one owner summing
    across the rounds and into the last block).  Items: row 9 first at 2048 (an
    owner whose first occurrence is in round two) and row 11 at B-1 only (one
    occurrence alone in the last, short block).  Position 2048 and B-1 hold user
    row 7, so the same two shapes on the user side sit one place off: row 9 first
    at 2049, row 11 at B-2 only."""
    if B < 2064:
        return ({}, {}, ()), ({}, {}, ())
    users = ({0: 7, 2047: 7, 2048: 7, B - 1: 7, 2049: 9, B - 2: 11}, {9: 2049}, (11,))
    items = ({2048: 9, B - 1: 11}, {9: 2048}, (11,))
    return users, items


def problem(B, d, U1=500, I1=300, seed=0):
    """(P, u, i, y): uniform users, Zipf items, every row of a table of <= B rows
    present, the planted rows of plants(B)."""
    P = N.init_params(U1, I1, d, 100 + seed)
    rng = np.random.default_rng(1000 * seed + B + d)
    pu, pi = plants(B)
    u = _fill(rng, B, U1, rng.integers(0, U1, B), *pu)
    i = _fill(rng, B, I1, (rng.zipf(1.3, B) - 1) % I1, *pi)
    y = (rng.random(B) < 0.5).astype(np.float32)
    return P, u, i, y


def hparams(adver):
    return N.NeuMFHParams(adver=adver, eps=EPS, reg_adv=REG_ADV)


@functools.lru_cache(maxsize=None)
def reference(case, adver):
    """One case's problem, float64 gradient and losses, and the fp32 oracle's
    distance from them -- computed once per process, never written to."""
    B, d, U1, I1 = case
    P, u, i, y = problem(B, d, U1, I1, seed=adver)
    hp = hparams(adver)
    want, lc, la = torch_grads_losses(P, u.astype(np.int64), i.astype(np.int64), y, hp)
    og, olc, ola = N.grad_step(P, u, i, y, hp)
    for a in list(P.values()) + [u, i, y] + list(want.values()) + list(og.values()):
        a.setflags(write=False)
    return dict(P=P, u=u, i=i, y=y, want=want, lc=lc, la=la, oracle=og, oracle_losses=(olc, ola),
                dist=oracle_distance(og, want))


@functools.lru_cache(maxsize=None)
def batches_k():
    """k of test_gpu_neumf_batches.py: calibrated over all its gradient cases."""
    return calibrate([reference(c, a)["dist"] for c, a in all_cases()])
