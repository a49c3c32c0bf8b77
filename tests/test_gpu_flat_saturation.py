"""Keras BPR (acf_kbpr_*) and FastAdversarialMF (acf_amf_*) of csrc/acf_keras_mf.hip OFF
the Keras initialisation and across train() calls, on flat_saturation_fixture.py:

  A1  acf_amf_grad where the BCE clip, its `inside` flag and the relu mask (h == 0
      exactly) all act, b1 / b2 non-zero: against the fp32 restatement (sharp) and
      float64 autograd (independent)
  A2  acf_amf_train over three such batches
  B1  BPR.train in the softplus tails (|x| up to 87), per-triplet losses included
  B2  three consecutive train() calls: Adam's iteration count and moments carry over
  B3  BPR with its own lr / beta1 / beta2 / adam_eps
  B4  x < -88.7: the loss overflows and the gradient is NaN, in the
      gathered rows only
  C   the native context: rank before train, re-created for a larger batch, reused
      for a smaller one

test_flat_saturation_host.py checks the fixture and the restatements on the CPU."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import amf_oracle as A
import flat_saturation_fixture as X
from conftest import PKG
from kbpr_oracle import kbpr_epoch, kbpr_grad, keras_adam
from test_amf_oracle import _autograd
from test_flat_saturation_host import kbpr_autograd, kbpr_overflow_rows

pytestmark = pytest.mark.gpu

GPU_DIMS = X.DIMS + (256,)


def _native():
    return importlib.import_module(PKG + "._native")


def _amf_model(p, dev, buf=None):
    FM = importlib.import_module(PKG + ".fast_adversarial_mf").FastAdversarialMF
    r = FM(p.uNum, p.iNum, p.d, seed=1, device=dev)
    r.params.copy_(torch.as_tensor(np.array(p.buf if buf is None else buf)))
    return r


def _bpr_model(p, dev, **adam):
    r = importlib.import_module(PKG + ".keras_bpr").BPR(p.U1, p.I1, p.d, seed=3, device=dev, **adam)
    r.params.copy_(torch.as_tensor(np.array(p.params)))
    return r


def _amf_case(d, case):
    return X.amf_problem(64, "plus", n=130, batch=130, hot=75) if case == "hot" else X.amf_problem(d, case)


@functools.lru_cache(maxsize=None)
def _amf_reference(d, case):
    """(fp32 restatement's gradient, its loss parts, float64 autograd's gradient), read-only."""
    p = _amf_case(d, case)
    with np.errstate(over="ignore"):
        G, _, parts = A.grad_step(p.buf, p.uNum, p.iNum, d, *p.inst)
    W, _ = _autograd(p.buf, p.uNum, p.iNum, d, *map(np.array, p.inst))
    G.setflags(write=False)
    W.setflags(write=False)
    return G, parts, W


def _seg_close(got, want, d, rtol, atol, what):
    """assert_allclose per segment of the flat buffer, atol scaled by max(1, max|want|) of the segment."""
    for name, sl in X.amf_segments(d).items():
        scale = max(1.0, float(np.abs(want[sl]).max()))
        np.testing.assert_allclose(got[sl], want[sl], rtol=rtol, atol=atol * scale, err_msg=f"{what} {name}")


# -- A1 ------------------------------------------------------------------------
@pytest.mark.parametrize("d,case", [(d, c) for d in GPU_DIMS for c in ("plus", "minus")] + [(64, "hot")])
def test_amf_grad_off_init(dev, d, case):
    """Sharp: the fp32 restatement at rtol 1e-4 and, per segment, atol 1e-7 max(1, max|G|),
    with its exact zeros.  Independent: float64 autograd W, where the kernel's max|G - W| /
    max|W| per segment may be 4x the restatement's (two fp32 summation orders differ by about
    as much as either does from exact).  Measured on an MI355X (table in DESIGN.md §11): both
    ratios 1.6e-7 .. 7.1e-7, the kernel's at most 1.5x the restatement's."""
    p = _amf_case(d, case)
    G, parts, W = _amf_reference(d, case)
    r = _amf_model(p, dev)
    loss = r.grad_batch(*[torch.as_tensor(np.array(x)).to(dev) for x in p.inst])
    got = r.grad.cpu().numpy()
    _seg_close(got, G, d, 1e-4, 1e-7, "grad")
    assert not got[G == 0].any()  # out-of-clip instances, dead units: exact zeros
    np.testing.assert_allclose(loss.double().mean(0).cpu().numpy(), parts, rtol=1e-5, atol=1e-7)
    for name, sl in X.amf_segments(d).items():
        top = float(np.abs(W[sl]).max())
        e_gpu, e_ref = float(np.abs(got[sl] - W[sl]).max()) / top, float(np.abs(G[sl] - W[sl]).max()) / top
        print(f"A1 d={d} {case} {name}: max|G|={np.abs(G[sl]).max():.3e} gpu/f64={e_gpu:.3e} fp32/f64={e_ref:.3e}")
        assert e_gpu <= max(4 * e_ref, 1e-6), (name, e_gpu, e_ref)


# -- A2 ------------------------------------------------------------------------
@pytest.mark.parametrize("d", [12, 64])
def test_amf_train_off_init(dev, d):
    """acf_amf_train over 37 + 37 + 20 instances of the fixture stream."""
    n, B = 2 * X.AMF_B + 20, X.AMF_B
    p = X.amf_problem(d, "plus", n=n)
    r = _amf_model(p, dev)
    T = [torch.as_tensor(np.array(x)).to(dev).contiguous() for x in p.inst]
    losses = torch.empty(n, 3, device=dev)
    _native().call_neumf("acf_amf_train", r._context(B), r.params.data_ptr(), r.grad.data_ptr(), r.m.data_ptr(),
                         r.v.data_ptr(), *[t.data_ptr() for t in T], n, B, 1, ctypes.byref(r.hp),
                         losses.data_ptr(), torch.cuda.current_stream().cuda_stream)
    buf = p.buf.copy()
    m, v = np.zeros_like(buf), np.zeros_like(buf)
    with np.errstate(over="ignore"):
        want = A.train_epoch(buf, m, v, 1, p.uNum, p.iNum, d, p.inst, B)
    np.testing.assert_allclose(r.params.cpu().numpy(), buf, rtol=1e-5, atol=2e-6)
    _seg_close(r.m.cpu().numpy(), m, d, 1e-4, 1e-9, "m")
    np.testing.assert_allclose(r.v.cpu().numpy(), v, rtol=1e-4, atol=1e-12)
    got = [float(losses[o: o + B].double().sum(1).mean()) for o in range(0, n, B)]
    np.testing.assert_allclose(got, want, rtol=1e-5)
    assert not r.grad.any()


# -- B1 ------------------------------------------------------------------------
def _bpr_check(r, params, m, v, where=None):
    """The tolerances of test_gpu_keras_bpr.test_epoch_matches_oracle (and the AMF train test's for v)."""
    sel = slice(None) if where is None else where
    np.testing.assert_allclose(r.params.cpu().numpy()[sel], params[sel], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(r.m.cpu().numpy()[sel], m[sel], rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(r.v.cpu().numpy()[sel], v[sel], rtol=1e-4, atol=1e-12)


def _bpr_losses(r, p):
    """acf_kbpr_train over the fixture as one batch; the per-triplet losses.  Steps r."""
    T = [torch.as_tensor(np.array(x)).to(r.device).contiguous() for x in (p.u, p.i, p.j)]
    losses = torch.empty(len(p.u), device=r.device)
    _native().call_neumf("acf_kbpr_train", r._context(len(p.u)), r.params.data_ptr(), r.grad.data_ptr(),
                         r.m.data_ptr(), r.v.data_ptr(), *[t.data_ptr() for t in T], len(p.u), len(p.u), 1,
                         ctypes.byref(r.hp), losses.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return losses.cpu().numpy()


def _loss_atol(p):
    """2 d 2^-24 (|u| |p| + |u| |n|): what two float32 summation orders of x can differ by."""
    P, Q = p.params[: p.U1 * p.d].reshape(p.U1, p.d).astype(np.float64), p.params[p.U1 * p.d:].reshape(
        p.I1, p.d).astype(np.float64)
    nu, np_, nn = (np.linalg.norm(x, axis=1) for x in (P[p.u], Q[p.i], Q[p.j]))
    return 2 * p.d * 2.0 ** -24 * (nu * np_ + nu * nn)


@pytest.mark.parametrize("d", GPU_DIMS)
def test_bpr_epoch_in_the_tails(dev, d):
    p = X.kbpr_problem(d)
    n, batch = len(p.u), 16  # 16 + 16 + 5
    r = _bpr_model(p, dev)
    r._rng = np.random.RandomState(5)
    perm = np.random.RandomState(5).permutation(n)
    loss = r.train([p.u, p.i, p.j], np.ones(n), batch)
    params = p.params.copy()
    m, v = np.zeros_like(params), np.zeros_like(params)
    want_l = kbpr_epoch(params, m, v, 1, p.U1, d, p.u[perm], p.i[perm], p.j[perm], batch)
    _bpr_check(r, params, m, v)
    assert abs(loss - float(want_l.astype(np.float64).mean())) <= 1e-5 * abs(loss)
    assert r.t == 3 and np.isfinite(r.params.cpu().numpy()).all()
    # the per-triplet losses at the fixture's own parameters: one batch from a fresh model
    got = _bpr_losses(_bpr_model(p, dev), p)
    _, l32 = kbpr_grad(p.params, p.U1, d, p.u, p.i, p.j)
    _, l64 = kbpr_autograd(p)
    atol = _loss_atol(p)
    for want in (l32, l64):
        err = np.abs(got - want)
        print(f"B1 d={d}: loss max err {err.max():.3e}, largest err / bound {(err / (1e-5 * np.abs(want) + atol)).max():.3f}")
        assert (err <= 1e-5 * np.abs(want) + atol).all()
    assert (got[p.targets >= 20] == 1).all()  # sigmoid rounds to 1


# -- B2 ------------------------------------------------------------------------
def test_bpr_resume(dev):
    """Three train() calls == one oracle run with t and the moments carried over, and
    is told apart from a run whose t restarts at 1 with every call."""
    p = X.kbpr_problem(16)
    n, batch = len(p.u), 16
    r = _bpr_model(p, dev)
    r._rng, rs = np.random.RandomState(5), np.random.RandomState(5)
    good, bad = p.params.copy(), p.params.copy()
    gm, gv, bm, bv = (np.zeros_like(good) for _ in range(4))
    for call in range(3):
        r.train([p.u, p.i, p.j], np.ones(n), batch)
        perm = rs.permutation(n)
        kbpr_epoch(good, gm, gv, 1 + 3 * call, p.U1, p.d, p.u[perm], p.i[perm], p.j[perm], batch)
        kbpr_epoch(bad, bm, bv, 1, p.U1, p.d, p.u[perm], p.i[perm], p.j[perm], batch)
        _bpr_check(r, good, gm, gv)
        assert r.t == 3 * (call + 1)
    apart = np.abs(good - bad)
    assert (apart > 100 * (2e-6 + 1e-5 * np.abs(good))).mean() > 0.25


def _amf_stream(seed, uNum, iNum, n):
    rng = np.random.default_rng(seed)
    users = rng.integers(0, uNum, n)
    items = (rng.zipf(1.5, n) % iNum).astype(np.int64)
    users[::6] = users[0]
    return users, items, rng.integers(0, 2, n).astype(np.float32)


def _amf_epoch_inputs(rs, users, items, y, pop_percent):
    """What FastAdversarialMF.train feeds acf_amf_train, drawn from rs as train draws from
    its own RandomState: adversarial_instances, then the shuffle."""
    n, h = len(y), len(y) // 2
    assert n == 2 * h

    def draw(x):
        pop, rare = A.popularity_split(x, pop_percent)
        ids = np.concatenate([pop[rs.randint(0, len(pop), h)], rare[rs.randint(0, len(rare), h)]])
        return ids, np.concatenate([np.ones(h), np.zeros(h)]).astype(np.float32)

    ux, tu = draw(users)
    ix, ti = draw(items)
    perm = rs.permutation(n)
    return [np.asarray(x)[perm] for x in (users, items, y, ux, ix, tu, ti, tu[::-1], ti[::-1])]


def _amf_check(r, buf, m, v):
    np.testing.assert_allclose(r.params.cpu().numpy(), buf, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(r.m.cpu().numpy(), m, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(r.v.cpu().numpy(), v, rtol=1e-4, atol=1e-12)


def test_amf_resume(dev):
    FM = importlib.import_module(PKG + ".fast_adversarial_mf").FastAdversarialMF
    uNum, iNum, d, n, batch = 60, 45, 16, 150, 64
    users, items, y = _amf_stream(11, uNum, iNum, n)
    r = FM(uNum, iNum, d, seed=2, device=dev)
    good = r.params.cpu().numpy().copy()
    bad = good.copy()
    gm, gv, bm, bv = (np.zeros_like(good) for _ in range(4))
    r._rng, rs = np.random.RandomState(5), np.random.RandomState(5)
    for call in range(3):
        loss = r.train([users, items], y, batch)
        inst = _amf_epoch_inputs(rs, users, items, y, r.pop_percent)
        want = A.train_epoch(good, gm, gv, 1 + 3 * call, uNum, iNum, d, inst, batch)
        A.train_epoch(bad, bm, bv, 1, uNum, iNum, d, inst, batch)
        _amf_check(r, good, gm, gv)
        sizes = [min(batch, n - o) for o in range(0, n, batch)]
        assert abs(loss - np.dot(want, sizes) / n) <= 1e-5 * abs(loss)
        assert r.t == 3 * (call + 1)
    apart = np.abs(good - bad)
    assert (apart > 100 * (2e-6 + 1e-5 * np.abs(good))).mean() > 0.25


# -- B3 ------------------------------------------------------------------------
def test_bpr_adam_hyperparameters(dev):
    hp = dict(lr=0.01, beta1=0.8, beta2=0.99, adam_eps=1e-5)
    p = X.kbpr_problem(12)
    n, batch = len(p.u), 16
    r = _bpr_model(p, dev, **hp)
    r._rng, rs = np.random.RandomState(5), np.random.RandomState(5)
    params, dflt = p.params.copy(), p.params.copy()
    m, v, dm, dv = (np.zeros_like(params) for _ in range(4))
    t = 1
    for _ in range(2):
        r.train([p.u, p.i, p.j], np.ones(n), batch)
        perm = rs.permutation(n)
        u, i, j = p.u[perm], p.i[perm], p.j[perm]
        kbpr_epoch(dflt, dm, dv, t, p.U1, p.d, u, i, j, batch)
        for o in range(0, n, batch):
            G, _ = kbpr_grad(params, p.U1, p.d, u[o: o + batch], i[o: o + batch], j[o: o + batch])
            keras_adam(params, G, m, v, t, hp["lr"], hp["beta1"], hp["beta2"], hp["adam_eps"])
            t += 1
    _bpr_check(r, params, m, v)
    assert (np.abs(params - dflt) > 100 * (2e-6 + 1e-5 * np.abs(params))).mean() > 0.25  # the defaults are far off


# -- B4 ------------------------------------------------------------------------
@pytest.mark.parametrize("d", [12, 64])
def test_bpr_overflow_is_contained(dev, d):
    p = X.kbpr_problem(d, overflow=True)
    r = _bpr_model(p, dev)
    got_l = _bpr_losses(r, p)
    params = p.params.copy()
    m, v = np.zeros_like(params), np.zeros_like(params)
    with np.errstate(all="ignore"):
        want_l = kbpr_epoch(params, m, v, 1, p.U1, d, p.u, p.i, p.j, len(p.u))
    bad = kbpr_overflow_rows(p)
    for got, want in ((r.params, params), (r.m, m), (r.v, v)):
        assert (~np.isfinite(want) == bad).all()
        assert (~np.isfinite(got.cpu().numpy()) == bad).all()
    _bpr_check(r, params, m, v, where=~bad)
    ovf = p.regime == X.OVERFLOW
    assert np.isposinf(want_l[ovf]).all() and np.isposinf(got_l[ovf]).all()
    assert (np.abs(got_l[~ovf] - want_l[~ovf]) <= 1e-5 * np.abs(want_l[~ovf]) + _loss_atol(p)[~ovf]).all()
    clean = ~ovf
    sc = r.rank(p.u[clean], p.i[clean]).reshape(-1)
    P, Q = params[: p.U1 * d].reshape(p.U1, d), params[p.U1 * d:].reshape(p.I1, d)
    assert np.isfinite(sc).all()
    np.testing.assert_allclose(sc, (P[p.u[clean]] * Q[p.i[clean]]).sum(1), rtol=1e-5, atol=1e-6)


# -- C -------------------------------------------------------------------------
def _rank_check(r, users, items):
    got = r.rank(users[:40], items[:40]).reshape(-1)
    P, Q = r.uEmb.cpu().numpy(), r.iEmb.cpu().numpy()
    np.testing.assert_allclose(got, (P[users[:40]] * Q[items[:40]]).sum(1), rtol=1e-5, atol=1e-6)


def test_bpr_context_grows_and_is_reused(dev):
    KB = importlib.import_module(PKG + ".keras_bpr")
    U1, I1, d, n = 40, 30, 8, 150
    rng = np.random.default_rng(4)
    u = rng.integers(1, U1, n).astype(np.int32)
    i = (rng.zipf(1.3, n) % (I1 - 1) + 1).astype(np.int32)
    j = rng.integers(1, I1, n).astype(np.int32)
    r = KB.BPR(U1, I1, d, seed=3, device=dev)
    _rank_check(r, u, i)  # before any train: a context of its own
    assert r._ctx_batch == 1
    params = r.params.cpu().numpy().copy()
    m, v = np.zeros_like(params), np.zeros_like(params)
    r._rng, rs = np.random.RandomState(5), np.random.RandomState(5)
    t = 1
    for batch, ctx_batch in ((16, 16), (64, 64), (16, 64)):  # re-created twice, then the larger one reused
        r.train([u, i, j], np.ones(n), batch)
        assert r._ctx_batch == ctx_batch
        perm = rs.permutation(n)
        kbpr_epoch(params, m, v, t, U1, d, u[perm], i[perm], j[perm], batch)
        t += (n + batch - 1) // batch
        _bpr_check(r, params, m, v)
        _rank_check(r, u, i)
    assert r.t == t - 1


def test_amf_context_grows_and_is_reused(dev):
    FM = importlib.import_module(PKG + ".fast_adversarial_mf").FastAdversarialMF
    uNum, iNum, d, n = 60, 45, 8, 150
    users, items, y = _amf_stream(12, uNum, iNum, n)
    r = FM(uNum, iNum, d, seed=2, device=dev)
    _rank_check(r, users, items)
    assert r._ctx_batch == 1
    buf = r.params.cpu().numpy().copy()
    m, v = np.zeros_like(buf), np.zeros_like(buf)
    r._rng, rs = np.random.RandomState(5), np.random.RandomState(5)
    t = 1
    for batch, ctx_batch in ((16, 16), (64, 64), (16, 64)):
        r.train([users, items], y, batch)
        assert r._ctx_batch == ctx_batch
        A.train_epoch(buf, m, v, t, uNum, iNum, d, _amf_epoch_inputs(rs, users, items, y, r.pop_percent), batch)
        t += (n + batch - 1) // batch
        _amf_check(r, buf, m, v)
        _rank_check(r, users, items)
    assert r.t == t - 1
