"""flat_saturation_fixture.py on the CPU: the fixture reaches every regime it claims
at every d, and the two fp32 restatements (oracle/amf_oracle.py, oracle/kbpr_oracle.py)
agree with float64 torch autograd there -- the yardsticks test_gpu_flat_saturation.py
holds the kernels of csrc/acf_keras_mf.hip to.  No kernel runs."""
import numpy as np
import pytest
import torch

import amf_oracle as A
import flat_saturation_fixture as X
from kbpr_oracle import kbpr_grad
from test_amf_oracle import _autograd

AMF_CASES = [(d, case) for d in X.DIMS for case in ("plus", "minus")]


def kbpr_autograd(p):
    """float64 gradient of mean(1 + softplus(-x)) (== 1 - log(sigmoid(x)), finite for
    every x) and the per-triplet losses."""
    t = torch.tensor(p.params.astype(np.float64), requires_grad=True)
    P, Q = t[: p.U1 * p.d].view(p.U1, p.d), t[p.U1 * p.d:].view(p.I1, p.d)
    u, i, j = (torch.as_tensor(x.astype(np.int64)) for x in (p.u, p.i, p.j))
    x = (P[u] * Q[i]).sum(1) - (P[u] * Q[j]).sum(1)
    loss = 1 + torch.nn.functional.softplus(-x)
    G = torch.autograd.grad(loss.mean(), t)[0]
    return G.numpy(), loss.detach().numpy()


def kbpr_overflow_rows(p):
    """Mask over the flat buffer: the rows that an overflowing triplet gathers."""
    mask = np.zeros((p.U1 + p.I1, p.d), bool)
    for b in np.flatnonzero(p.regime == X.OVERFLOW):
        mask[p.u[b]] = mask[p.U1 + p.i[b]] = mask[p.U1 + p.j[b]] = True
    return mask.reshape(-1)


# -- H1 ------------------------------------------------------------------------
@pytest.mark.parametrize("d,case", AMF_CASES + [(64, "hot")])
def test_amf_fixture_hits_every_regime(d, case):
    p = X.amf_problem(64, "plus", n=130, batch=130, hot=75) if case == "hot" else X.amf_problem(d, case)
    u, i, y, ua, ia, *_ = p.inst
    pos = (0, 1) if case in ("plus", "hot") else (1, 0)  # the discriminator with z > 0, the one with z < 0
    rows = (ua, ia)
    for k in range(2):
        z = np.abs(p.z64[k])
        assert not ((z >= X.NO_GO[0]) & (z <= X.NO_GO[1])).any()
        # every target reached, with its sign, by the row that aims at it
        sign = 1.0 if k == pos[0] else -1.0
        for r, zt in enumerate(X.Z_TARGETS):
            got = p.z64[k][rows[k] == r]
            assert len(got) and np.allclose(got, sign * zt, rtol=1e-5)
        assert (p.regime[k][z <= 14.6] == X.INSIDE).all() and (z <= 14.6).sum() >= 4
        assert (p.regime[k][z >= 18.9] == (X.OUT_HIGH if k == pos[0] else X.OUT_LOW)).all()
        assert (z >= 18.9).sum() >= 4
        assert p.zero_h[k][rows[k] == X.ZERO_ROW].all() and (rows[k] == X.ZERO_ROW).any()
        assert 0.25 <= p.dead[k] <= 0.75
        assert (rows[k] < X.RESERVED).all()
    assert p.relu_margin >= p.d * 2.0 ** -24
    assert u[0] == ua[0] == X.ROW_19 and i[0] == ia[0] == X.PLAIN_ROW
    assert (u[1:] >= X.RESERVED).all() and (i[1:] >= X.RESERVED).all()
    if case == "hot":
        assert (ua == X.ROW_14_5).sum() >= 70 and (ia == X.ROW_14_5).sum() >= 70
        # the row's occurrences span more than one 64-lane sweep of k_amf_rows
        assert np.ptp(np.flatnonzero(ua == X.ROW_14_5)) > 64 and np.ptp(np.flatnonzero(ia == X.ROW_14_5)) > 64


@pytest.mark.parametrize("d", X.DIMS)
def test_kbpr_fixture_hits_every_regime(d):
    fin, ovf = X.kbpr_problem(d), X.kbpr_problem(d, overflow=True)
    for p, xs in ((fin, X.X_FINITE), (ovf, X.X_FINITE + X.X_OVERFLOW)):
        tail = ~np.isnan(p.targets)
        assert sorted(p.targets[tail]) == sorted(xs)
        np.testing.assert_allclose(p.x32[tail], p.targets[tail], rtol=1e-4)
        assert (np.abs(p.x32[~tail]) < 0.1).all()
        # the tails' rows are their own
        for arr in (p.u, p.i, p.j):
            assert len(set(arr[tail])) == tail.sum()
        assert not set(p.i[tail]) & set(p.j[tail])
        assert not (set(p.u[tail]) & set(p.u[~tail])) and not (set(p.i[tail]) | set(p.j[tail])) & (
            set(p.i[~tail]) | set(p.j[~tail]))
        assert (p.i[~tail] == p.j[~tail]).any() and np.bincount(p.i[~tail]).max() >= 5
    assert (fin.regime != X.OVERFLOW).all() and fin.x32.min() >= X.X_MIN_FINITE
    assert (ovf.regime == X.OVERFLOW).sum() == len(X.X_OVERFLOW)
    assert (ovf.x32[ovf.regime == X.OVERFLOW] < -88.8).all()
    assert ovf.x32[ovf.regime != X.OVERFLOW].min() >= X.X_MIN_FINITE


# -- H2 ------------------------------------------------------------------------
@pytest.mark.parametrize("d,case", AMF_CASES + [(64, "hot")])
def test_amf_restatement_matches_float64(d, case):
    p = X.amf_problem(64, "plus", n=130, batch=130, hot=75) if case == "hot" else X.amf_problem(d, case)
    with np.errstate(over="ignore"):
        G, loss, parts = A.grad_step(p.buf, p.uNum, p.iNum, d, *p.inst)
    W, wl = _autograd(p.buf, p.uNum, p.iNum, d, *map(np.array, p.inst))
    np.testing.assert_allclose(G, W, rtol=1e-4, atol=1e-7)
    assert ((G == 0) == (W == 0)).all()
    # the loss: float64 clips at 1e-7 and 1 - 1e-7, float32 at their roundings (1 - 1e-7 is
    # 1 - 2^-23 there, 0.18 apart in the log), so the float64 loss takes float32's bounds
    lo, hi = float(A.CLIP), float(np.float32(1) - A.CLIP)
    u, i, y, ua, ia, tu, ti, *_ = p.inst
    P, Q, _, _ = A.unflatten(p.buf.astype(np.float64), p.uNum, p.iNum, d)
    want, atol = [(((P[u] * Q[i]).sum(1) - y) ** 2).mean()], [1e-7]
    for z, t, regime in ((p.z64[0], tu, p.regime[0]), (p.z64[1], ti, p.regime[1])):
        s = np.clip(1 / (1 + np.exp(-z)), lo, hi)
        want.append((-(t * np.log(s) + (1 - t) * np.log1p(-s))).mean())
        # inside the clip a float32 s near 1 is 2^-23 off at most (1 + e^-z rounded, then
        # the quotient), which log(1 - s) magnifies by 1 / (1 - s): 0.1 at z = 14.5
        atol.append(1e-7 + ((regime == X.INSIDE) * (1 - t) * 2.0 ** -23 / (1 - s)).mean())
    for k in range(3):
        np.testing.assert_allclose(parts[k], want[k], rtol=1e-5, atol=atol[k])
    assert wl > 0 and np.isfinite(wl)
    seg = X.amf_segments(d)
    o = seg["D_u"].start
    for k in range(2):  # out-of-clip and dead units leave exact zeros in W1's and b1's gradients
        blk = G[o + k * A.disc_block(d):][: A.disc_block(d)]
        assert not blk[: d * d].reshape(d, d)[:, X.DEAD_UNIT].any() and blk[: d * d].any()
        assert blk[d * d + X.DEAD_UNIT] == 0 and blk[d * d + d + X.DEAD_UNIT] == 0
    # the |z| = 19 row's gradient is the MSE's alone; the rows past it in the clip get none
    GP, GQ = G[seg["P"]].reshape(-1, d), G[seg["Q"]].reshape(-1, d)
    assert GP[X.ROW_19].any() and not GP[4:7].any() and not GQ[3:7].any()


@pytest.mark.parametrize("d", X.DIMS)
def test_kbpr_restatement_matches_float64(d):
    p = X.kbpr_problem(d)
    G, loss = kbpr_grad(p.params, p.U1, d, p.u, p.i, p.j)
    W, wl = kbpr_autograd(p)
    assert np.isfinite(G).all() and np.isfinite(loss).all()
    np.testing.assert_allclose(G, W, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(loss, wl, rtol=1e-5, atol=1e-7)
    sat = p.targets >= 20  # sigmoid rounds to 1: the gradient is exactly 0, the loss exactly 1
    assert (loss[sat] == 1).all() and not G.reshape(-1, d)[p.u[sat]].any()


# -- H3 ------------------------------------------------------------------------
@pytest.mark.parametrize("d", X.DIMS)
def test_kbpr_overflow_is_contained(d):
    p = X.kbpr_problem(d, overflow=True)
    with np.errstate(all="ignore"):
        G, loss = kbpr_grad(p.params, p.U1, d, p.u, p.i, p.j)
    W, wl = kbpr_autograd(p)
    ovf = p.regime == X.OVERFLOW
    bad = kbpr_overflow_rows(p)
    assert (~np.isfinite(G) == bad).all() and np.isnan(G[bad]).all()
    assert np.isposinf(loss[ovf]).all() and np.isfinite(wl).all()
    np.testing.assert_allclose(G[~bad], W[~bad], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(loss[~ovf], wl[~ovf], rtol=1e-5, atol=1e-7)
