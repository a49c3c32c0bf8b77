"""The fixture test_flat_saturation_host.py and test_gpu_flat_saturation.py share:
small FastAdversarialMF and Keras BPR problems that sit OFF the Keras
initialisation, in every regime k_amf_inst / k_kbpr_inst (csrc/acf_keras_mf.hip)
tell apart.  numpy only; nothing here needs a GPU.

AMF (amf_problem): tables of 50 x 40 rows, batches of 37.  D_u's W2 is all
positive and D_i's all negative ("plus"; "minus" mirrors it), so the pre-sigmoid
z of a row has one sign per table and grows with the row's scale.  Rows 0..19 of
each table are reserved for the adversarial gathers ua / ia:

    rows 0..6   scaled so that z = +-(4, 13.5, 14.5, 19, 30, 60, 100)
                  |z| <= 14.5: inside the BCE clip [1e-7, 1 - 1e-7], large magnitude
                  |z| >= 19:   outside (s above the clip for z > 0, below for z < 0):
                               zero gradient, clipped loss; e^100 overflows float32
    row  7      all zeros: h = b1, EXACTLY 0 on the even units (b1 is 0 there)
    rows 8..19  left at the init scale

b1 is U(-0.2, 0.2) on the odd units and 0 on the even ones, b2 = +0.3 (D_u) /
-0.3 (D_i), and the scales are solved with both in place.  Unit 3 is dead for every
row (its column of W1 is 0 and its b1 -0.1), so its column of W1's gradient and its
elements of b1's and W2's are exactly 0; about half of the other units are dead per row.  u and i come from rows
>= 20 so the MSE stays O(1), but for instance 0 of every batch: u[0] = ua[0] (the
|z| = 19 row: no discriminator gradient, an MSE contribution) and i[0] = ia[0]
(row 8).  With hot > 0 the |z| = 14.5 row is gathered `hot` more times, spread over
the batch, so the ballot sweep of k_amf_rows crosses a 64-lane boundary on it.

No |z| of a gathered row may lie in NO_GO = [15.5, 17.5]: float64 clips at
|z| = ln(1e7) = 16.12, float32 at z = 16.64 on the high side (1 + e^-z rounds to
1 from there on), and one ulp of expf flips `inside` in between.  Likewise no
non-zero h of a gathered row may be closer to 0 than any float32 summation order
can move it (relu_margin >= d 2^-24 of the sum of the absolute terms); the seed
is the first for which that holds.

KBPR (kbpr_problem): tables of 40 x 30 rows, 37 triplets.  Eleven triplets on rows
of their own have the positive row parallel to the user row (no cancellation inside
x = u.p - u.n; the negative row stays at the init scale), both scaled by the same
factor so that x = (3, 8, 20, 40, 80, 87, -8, -20, -40, -80, -87): from x = 20 on
sigmoid(x) rounds to 1 (gradient exactly 0), at x = -87 it is 1.6e-38, the last
normal floats.  overflow=True adds x = (-95, -120): e^-x is inf, sigmoid 0, the loss
inf and the gradient (-1/B * inf) * 0 = NaN.  The other triplets are
ordinary init-scale ones on other rows, with j == i ties and one hot item.
"""
from types import SimpleNamespace

import numpy as np

import amf_oracle as A

F = np.float32
DIMS = (4, 12, 64, 132)

# -- AMF ---------------------------------------------------------------------
AMF_U, AMF_I, AMF_B = 50, 40, 37
RESERVED = 20
Z_TARGETS = (4.0, 13.5, 14.5, 19.0, 30.0, 60.0, 100.0)
ZERO_ROW, PLAIN_ROW = 7, 8
ROW_19, ROW_14_5 = 3, 2
DEAD_UNIT = 3
NO_GO = (15.5, 17.5)
INSIDE, OUT_HIGH, OUT_LOW = range(3)


def _solve_scale(e0, W1, b1, W2, b2, target):
    """c with relu(c e0 W1 + b1) . W2 + b2 == target (float64).  W2 has one sign, so
    sign(W2) z is convex and piecewise linear in c: Newton from the right of the
    largest root walks down to it in finitely many steps."""
    a = e0 @ W1
    c = 1e9
    for _ in range(200):
        act = c * a + b1 > 0
        val = np.maximum(c * a + b1, 0) @ W2 + b2
        if abs(val - target) < 1e-10 * abs(target):
            return c
        c -= (val - target) / (a[act] @ W2[act])
    raise AssertionError("scale did not converge")


def _amf_build(d, sign, n, batch, hot, seed):
    rng = np.random.default_rng(1000 * d + seed)
    buf = A.init_params(AMF_U, AMF_I, d, seed)
    P, Q, Du, Di = A.unflatten(buf, AMF_U, AMF_I, d)
    signs = (sign, -sign)
    for D, sg, b2 in ((Du, signs[0], 0.3), (Di, signs[1], -0.3)):
        D["W2"][:] = sg * np.abs(D["W2"])
        D["b1"][1::2] = rng.uniform(-0.2, 0.2, d // 2)
        D["b2"][0] = b2
        D["W1"][:, DEAD_UNIT], D["b1"][DEAD_UNIT] = 0, -0.1  # h = -0.1 whatever the row
    for E, D, sg in ((P, Du, signs[0]), (Q, Di, signs[1])):
        W = {k: D[k].astype(np.float64) for k in A.DISC}
        for r, zt in enumerate(Z_TARGETS):
            e0 = E[r].astype(np.float64)
            if np.maximum(e0 @ W["W1"], 0) @ np.abs(W["W2"]) < np.maximum(-e0 @ W["W1"], 0) @ np.abs(W["W2"]):
                e0 = -e0  # the half-space where the live units weigh more
            E[r] = e0 * _solve_scale(e0, W["W1"], W["b1"], W["W2"], W["b2"][0], sg * zt)
        E[ZERO_ROW] = 0
    inst = [np.zeros(n, np.int32) for _ in range(4)] + [np.zeros(n, F) for _ in range(5)]
    u, i, ua, ia, y, tu, ti, du, di = inst
    for o in range(0, n, batch):
        m = min(batch, n - o)
        s = slice(o, o + m)
        u[s] = rng.integers(RESERVED, AMF_U, m)
        i[s] = rng.integers(RESERVED, AMF_I, m)
        u[o + 2: o + m: 9] = u[o + 2]  # a hot MSE row
        for x, first in ((ua, ROW_19), (ia, PLAIN_ROW)):
            x[s] = rng.integers(0, RESERVED, m)
            head = [first] + [r for r in range(PLAIN_ROW + 1) if r != first]
            x[o: o + min(m, len(head))] = head[:m]
        if hot:
            pos = o + len(head) + rng.choice(m - len(head), hot, replace=False)
            ua[pos] = ROW_14_5
            ia[pos] = ROW_14_5
        u[o], i[o] = ua[o], ia[o]
    y[:] = rng.integers(0, 2, n)
    tu[:] = rng.integers(0, 2, n)
    ti[:] = rng.integers(0, 2, n)
    du[:], di[:] = 1 - tu, 1 - ti
    return buf, [u, i, y, ua, ia, tu, ti, du, di]


def _amf_regimes(buf, d, ua, ia):
    """Per discriminator: z (float64), the regime of every instance and whether some
    unit of it has h == 0 exactly, as the fp32 restatement sees them; the relu margin."""
    P, Q, Du, Di = A.unflatten(buf, AMF_U, AMF_I, d)
    z64, regime, zero_h, dead, margin = [], [], [], [], np.inf
    for E, D, idx in ((P, Du, ua), (Q, Di, ia)):
        h, _, s = A.disc_forward(D, E[idx])
        regime.append(np.where(s > F(1) - A.CLIP, OUT_HIGH, np.where(s < A.CLIP, OUT_LOW, INSIDE)))
        zero_h.append((h == 0).any(1))
        dead.append(float((h <= 0).mean()))
        W = {k: D[k].astype(np.float64) for k in A.DISC}
        e = E[idx].astype(np.float64)
        h64 = e @ W["W1"] + W["b1"]
        z64.append(np.maximum(h64, 0) @ W["W2"] + W["b2"][0])
        mag = np.abs(e) @ np.abs(W["W1"]) + np.abs(W["b1"])
        nz = h64 != 0
        assert ((h == 0) == ~nz).all()
        margin = min(margin, float((np.abs(h64[nz]) / mag[nz]).min()))
    return z64, regime, zero_h, dead, margin


_AMF = {}


def amf_problem(d, case="plus", n=AMF_B, batch=AMF_B, hot=0):
    """case: "plus" (D_u's W2 > 0, D_i's < 0) or "minus" (mirrored); n instances in
    batches of `batch`; hot: extra gathers of the |z| = 14.5 rows per batch.  Returns a
    namespace: buf (the flat float32 parameters), inst = [u, i, y, ua, ia, tu, ti, du,
    di] (the order of amf_oracle.grad_step), uNum, iNum, d, and per discriminator
    z64 / regime / zero_h / dead (the dead-unit fraction), relu_margin, seed."""
    key = (d, case, n, batch, hot)
    if key not in _AMF:
        for seed in range(64):
            buf, inst = _amf_build(d, 1 if case == "plus" else -1, n, batch, hot, seed)
            z64, regime, zero_h, dead, margin = _amf_regimes(buf, d, inst[3], inst[4])
            if margin >= d * 2.0 ** -24:
                break
        else:
            raise AssertionError("no seed keeps every pre-activation clear of 0")
        buf.setflags(write=False)
        for x in inst:
            x.setflags(write=False)
        _AMF[key] = SimpleNamespace(buf=buf, inst=inst, uNum=AMF_U, iNum=AMF_I, d=d, z64=z64, regime=regime,
                                    zero_h=zero_h, dead=dead, relu_margin=margin, seed=seed)
    return _AMF[key]


def amf_segments(d):
    """The flat buffer's segments: name -> slice (P, Q, D_u, D_i)."""
    o, blk = (AMF_U + AMF_I) * d, A.disc_block(d)
    return {"P": slice(0, AMF_U * d), "Q": slice(AMF_U * d, o), "D_u": slice(o, o + blk),
            "D_i": slice(o + blk, o + 2 * blk)}


# -- KBPR --------------------------------------------------------------------
KB_U, KB_I, KB_B = 40, 30, 37
X_FINITE = (3.0, 8.0, 20.0, 40.0, 80.0, 87.0, -8.0, -20.0, -40.0, -80.0, -87.0)
X_OVERFLOW = (-95.0, -120.0)
X_MIN_FINITE = -88.0
ORDINARY, TAIL, OVERFLOW = range(3)


def kbpr_x32(params, d, u, i, j):
    """x = u.p - u.n as kbpr_oracle.kbpr_grad rounds it."""
    P, Q = params[: KB_U * d].reshape(KB_U, d), params[KB_U * d:].reshape(KB_I, d)
    return ((P[u] * Q[i]).sum(1, dtype=F) - (P[u] * Q[j]).sum(1, dtype=F)).astype(F)


_KB = {}


def kbpr_problem(d, overflow=False):
    """Returns a namespace: params (flat float32 [uEmb | iEmb]), u, i, j (int32, 37
    triplets), U1, I1, d, x32 (the restatement's x), regime per triplet (ORDINARY: init
    scale; TAIL: a finite softplus tail; OVERFLOW) and targets (the x aimed at, NaN
    for the ordinary triplets)."""
    key = (d, overflow)
    if key not in _KB:
        rng = np.random.default_rng(77 + d)
        params = rng.uniform(-0.05, 0.05, (KB_U + KB_I) * d).astype(F)
        P, Q = params[: KB_U * d].reshape(KB_U, d), params[KB_U * d:].reshape(KB_I, d)
        xs = X_FINITE + (X_OVERFLOW if overflow else ())
        ns, slots = len(xs), len(X_FINITE) + len(X_OVERFLOW)
        u, i, j = (np.zeros(KB_B, np.int32) for _ in range(3))
        targets = np.full(KB_B, np.nan)
        for k, x in enumerate(xs):  # user 1 + k, positive 1 + k, negative 1 + slots + k
            ru, rp, rn = 1 + k, 1 + k, 1 + slots + k
            e = P[ru].astype(np.float64)
            un, uu = e @ Q[rn].astype(np.float64), e @ e
            # rows a e and +-a e: x = +-a^2 |e|^2 - a e.n, the positive root
            sg = 1.0 if x > 0 else -1.0
            a = (sg * un + np.sqrt(un * un + 4 * uu * abs(x))) / (2 * uu)
            P[ru], Q[rp] = a * e, sg * a * e
            u[k], i[k], j[k], targets[k] = ru, rp, rn, x
        # ordinary triplets on the other rows: items 0 and 27..29, item 28 hot
        m = KB_B - ns
        u[ns:] = rng.integers(1 + slots, KB_U, m)
        pool = np.array([0] + list(range(1 + 2 * slots, KB_I)), np.int32)
        i[ns:] = pool[rng.integers(0, len(pool), m)]
        j[ns:] = pool[rng.integers(0, len(pool), m)]
        i[ns::3] = pool[-2]
        j[ns + 1:: 7] = i[ns + 1:: 7]  # ties: x == 0 exactly
        u[ns + 2] = u[ns + 5]          # a user with two triplets
        order = rng.permutation(KB_B)  # the tails anywhere in the batch
        u, i, j, targets = u[order], i[order], j[order], targets[order]
        x32 = kbpr_x32(params, d, u, i, j)
        regime = np.where(np.isnan(targets), ORDINARY, np.where(targets < X_MIN_FINITE, OVERFLOW, TAIL))
        for arr in (params, u, i, j):
            arr.setflags(write=False)
        _KB[key] = SimpleNamespace(params=params, u=u, i=i, j=j, U1=KB_U, I1=KB_I, d=d, x32=x32, regime=regime,
                                   targets=targets)
    return _KB[key]
