"""libacf_neumf.so above 1,024 instances per batch and at the dims that are no
power of two, against the float64 autograd of the same graph (tests/neumf_ref.py).

The regimes (thresholds in csrc/acf_neumf_step.h):
  B <= 1,024 (FR_MAXB)   rows in line (k_nmf_step / k_nmf_inst<.., true>)
  B >  1,024             k_nmf_inst<0>, k_nmf_rows, k_nmf_inst<1> with the clean
                         pass's weight-gradient workgroups, k_nmf_rows; the second
                         activation buffer at max_batch * 2 * d
  B >  2,048 (RCH)       k_nmf_rows stages the indices in more than one round: a
                         row's owner may sit in an earlier round than occurrences
                         it sums, or find its first occurrence in a later one
  B >  4,096 (16 * 256)  inst_block and wgrad_group loop over blocks; the next
                         block's gather is in flight while one computes; a short
                         last block can be a workgroup's second
Planted rows (neumf_ref.plants) at every B >= 2,064: user row 7 at 0, 2047, 2048
and B-1; item row 9 first at 2048, item row 11 at B-1 only; user row 9 first at
2049 and user row 11 at B-2 only (2048 and B-1 are row 7's on the user side).

The bar is neumf_ref.check_grads: |got - want64| <= 1e-4 |want64| + k max|want64|
per tensor, no absolute floor.  k is measured from the reference alone, at run
time: 4x the fp32 numpy oracle's largest distance from float64 over this module's
cases (neumf_ref.all_cases), refused above 1e-4.  Measured: k = 1.336e-5.  The
oracle's worst per-tensor distance, in units of max|want64| (adver 0 / 1):
  B 1040 d 16    7.5e-7 (W2)  / 6.8e-7 (b1)      B 96  d 4     4.1e-7 (Wo) / 2.1e-7 (W1)
  B 2064 d 8     1.5e-6 (W1)  / 6.9e-7 (b1)      B 300 d 4     6.5e-7 (bo) / 3.2e-7 (b1)
  B 2064 d 64    1.1e-6 (b2)  / 8.4e-7 (MLP_I)   B 96  d 12    2.6e-7 (W1) / 2.7e-7 (W2)
  B 4112 d 64    3.3e-6 (b2)  / 1.4e-6 (b1)      B 300 d 12    3.9e-7 (b1) / 2.4e-7 (b2)
  B 4100 d 36    1.3e-6 (b2)  / 1.3e-6 (MF_I)    B 96  d 36    3.0e-7 (MLP_I) / 2.9e-7 (W1)
  B 5000 d 128   1.7e-6 (b1)  / 1.5e-6 (b2)      B 300 d 36    4.2e-7 (W2) / 7.3e-7 (W2)
  B 8200 d 64    2.8e-6 (b1)  / 2.3e-6 (b2)      B 96  d 100   4.2e-7 (Wo) / 5.3e-7 (W1)
  B 1024 d 16    8.7e-7 (b2)  / 5.2e-7 (W2)      B 300 d 100   9.4e-7 (Wo) / 5.0e-7 (b2)
test_neumf_oracle.py::test_batches_bar_is_met_by_the_oracle_alone checks the bar
itself without a GPU.  Losses: rtol 1e-5 against float64."""
import numpy as np
import pytest
import torch

import neumf_oracle as N
import neumf_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nm(acf):
    import importlib
    from conftest import PKG
    return importlib.import_module(PKG + ".neumf")


def _state(nm, P, dev):
    U1, d = P["MF_U"].shape
    st = nm.NeuMFState(U1, P["MF_I"].shape[0], d, dev)
    st.load(P)
    return st


def _reset(st, P):
    st.load(P)
    for buf in (st.grad, st.m, st.v):
        buf.zero_()
    st.t = 0


def _grad(nm, dev, ref, adver, max_batch=None, rows_in_line=True):
    """(gradient per tensor, [clean, adversarial] loss, flat gradient) of one ctx.grad."""
    st = _state(nm, {n: a.copy() for n, a in ref["P"].items()}, dev)  # (the shared reference is read-only)
    ctx = nm.NeuMFContext(st, max_batch or len(ref["u"]))
    if not rows_in_line:
        ctx.set_rows_in_line(False)
    loss = torch.zeros(2, device=dev)
    hp = ctx.hparams(adver=adver, eps=R.EPS, reg_adv=R.REG_ADV)
    ctx.grad(ref["u"].copy(), ref["i"].copy(), ref["y"].copy(), hp, loss)
    torch.cuda.synchronize()
    return {n: st.view(n, st.grad).cpu().numpy() for n in N.NAMES}, loss.cpu().numpy(), st.grad.clone()


def _check(got, loss, ref, adver, what):
    R.check_grads(got, ref["want"], R.batches_k(), what)
    np.testing.assert_allclose(loss[:1 + adver], [ref["lc"], ref["la"]][:1 + adver], rtol=1e-5, err_msg=what)
    if not adver:
        assert loss[1] == 0.0


@pytest.mark.parametrize("adver", [0, 1])
@pytest.mark.parametrize("case", R.GRAD_CASES, ids=R.case_id)
def test_grad_matches_float64(nm, dev, case, adver):
    """One gradient per batch regime (see the module docstring) against float64."""
    ref = R.reference(case, adver)
    got, loss, _ = _grad(nm, dev, ref, adver)
    _check(got, loss, ref, adver, f"{R.case_id(case)} adver={adver} ")


@pytest.mark.parametrize("adver", [0, 1])
def test_grad_below_max_batch(nm, dev, adver):
    """A batch shorter than the context's max_batch: the adversarial pass's second
    activation buffer starts at max_batch * 2 * d, not at B * 2 * d."""
    case = R.GRAD_CASES[3]
    ref = R.reference(case, adver)
    got, loss, _ = _grad(nm, dev, ref, adver, max_batch=6000)
    _check(got, loss, ref, adver, f"{R.case_id(case)} of 6000 adver={adver} ")


@pytest.mark.parametrize("adver", [0, 1])
def test_in_line_limit_from_both_sides(nm, dev, adver):
    """B = 1,024 (the largest batch summed in line) and B = 1,040 (the smallest on
    the k_nmf_rows path), each on a default context and on one with rows in line
    switched off, all four against float64; the two paths give the same bits at
    1,024, and the switch changes nothing at 1,040."""
    for case in R.LIMIT_CASES:
        ref = R.reference(case, adver)
        what = f"{R.case_id(case)} adver={adver} "
        got_a, loss_a, flat_a = _grad(nm, dev, ref, adver)
        got_b, loss_b, flat_b = _grad(nm, dev, ref, adver, rows_in_line=False)
        _check(got_a, loss_a, ref, adver, what + "(default) ")
        _check(got_b, loss_b, ref, adver, what + "(rows kernel) ")
        assert torch.equal(flat_a, flat_b) and np.array_equal(loss_a, loss_b), what


@pytest.mark.parametrize("case", R.DIM_CASES, ids=R.case_id)
def test_dims_grad_matches_float64(nm, dev, case):
    """d = 4, 12, 36, 100 (check_dims takes every multiple of 4 up to 128; d % 16 != 0
    is wgrad_group<false> and partial MFMA panels) at B = 96 and 300, in line and
    on the k_nmf_rows path."""
    for adver in (0, 1):
        ref = R.reference(case, adver)
        for in_line in (True, False):
            got, loss, _ = _grad(nm, dev, ref, adver, rows_in_line=in_line)
            _check(got, loss, ref, adver, f"{R.case_id(case)} adver={adver} in_line={in_line} ")


def _epoch(batch, n, d, U1, I1, seed):
    P = N.init_params(U1, I1, d, seed)
    rng = np.random.default_rng(seed + 9)
    u = rng.integers(0, U1, n).astype(np.int32)
    i = ((rng.zipf(1.3, n) - 1) % I1).astype(np.int32)
    y = (rng.random(n) < 0.5).astype(np.float32)
    return P, u, i, y


def _stepwise(ctx, st, u, i, y, batch, hp, losses):
    for k, o in enumerate(range(0, len(u), batch)):
        e = min(o + batch, len(u))
        ctx.grad(u[o:e], i[o:e], y[o:e], hp, losses[k])
        ctx.adam(hp)


@pytest.mark.parametrize("batch,n,d,U1,I1", [
    (1500, 3500, 64, 500, 300),   # k_nmf_rows batches, then a tail of 500 in line
    (2064, 4129, 16, 500, 300),   # two staging rounds, then a tail of one instance
    (4112, 9000, 64, 500, 300),   # looping workgroups, then a tail of 776 in line
    (96, 1000, 12, 41, 37),       # d % 16 != 0
    (96, 1000, 100, 41, 37),      # d > 64 and no multiple of 16
])
def test_train_equals_stepwise(nm, dev, batch, n, d, U1, I1):
    """acf_neumf_train == grad + dense adam per batch, bit for bit (parameters,
    moments, losses), where one call mixes the k_nmf_rows path with an in-line
    tail, and at the odd dims.  At (1500, 3500, 64) the three Adam steps are also
    held to the oracle's (test_training_steps_match_oracle's tolerance)."""
    P, u, i, y = _epoch(batch, n, d, U1, I1, 21)
    nb = (n + batch - 1) // batch
    for adver in (0, 1):
        a, b = _state(nm, P, dev), _state(nm, P, dev)
        ca, cb = nm.NeuMFContext(a, batch), nm.NeuMFContext(b, batch)
        hp = ca.hparams(adver=adver, eps=R.EPS, reg_adv=R.REG_ADV)
        la = ca.train(u, i, y, batch, hp)
        lb = torch.zeros_like(la)
        _stepwise(cb, b, u, i, y, batch, hp, lb)
        torch.cuda.synchronize()
        assert a.t == b.t == nb and la.shape == (nb, 2)
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
        assert torch.equal(la, lb) and bool((la[:, 0] > 0).all()) and bool((la[:, 1] > 0).all()) == bool(adver)
        assert not a.grad.any() and not b.grad.any()
        if (batch, n) == (1500, 3500):
            hp_o = R.hparams(adver)
            Po = {k: v.copy() for k, v in P.items()}
            m = {k: np.zeros_like(v) for k, v in P.items()}
            v = {k: np.zeros_like(v) for k, v in P.items()}
            for t, o in enumerate(range(0, n, batch), 1):
                g, *_ = N.grad_step(Po, u[o:o + batch], i[o:o + batch], y[o:o + batch], hp_o)
                N.adam(Po, g, m, v, t, hp_o)
            for name in N.NAMES:
                np.testing.assert_allclose(a.view(name).cpu().numpy(), Po[name], rtol=1e-4, atol=2e-6, err_msg=name)


@pytest.mark.parametrize("max_batch", [64, 8192])
@pytest.mark.parametrize("n", [4112, 70001])
def test_predict_matches_oracle(nm, dev, n, max_batch):
    """Prediction takes any n on any context: 257 blocks on 257 workgroups, and
    4,376 blocks (the last of one instance) on 512 looping workgroups."""
    P, u, i, _ = _epoch(512, n, 64, 500, 300, 3)
    ctx = nm.NeuMFContext(_state(nm, P, dev), max_batch)
    got = ctx.predict(u, i).cpu().numpy()
    np.testing.assert_allclose(got, N.predict(P, u, i), rtol=1e-5, atol=1e-7)


def test_give_up_in_the_tail_replays_exactly(nm, dev):
    """batch 1,500 over 2,000 instances: the full batch takes k_nmf_rows, the tail
    of 500 runs in line.  Spin limit 0 makes the tail's waits give up at once (a
    designed error code).  With the failsafe on the call is replayed on the
    row-sum path: the bits of set_rows_in_line(False), one recovery, and the
    arrival counters are zeroed (the next call at the default limit matches too).
    With the failsafe off the call raises, and the one after it is sound."""
    batch, n, d = 1500, 2000, 64
    P, u, i, y = _epoch(batch, n, d, 500, 300, 47)
    for adver in (1, 0):
        a, b = _state(nm, P, dev), _state(nm, P, dev)
        ca, cb = nm.NeuMFContext(a, batch), nm.NeuMFContext(b, batch)
        cb.set_rows_in_line(False)
        hp = ca.hparams(adver=adver, eps=R.EPS, reg_adv=R.REG_ADV)

        def same():
            ta, tb = ca.train(u, i, y, batch, hp), cb.train(u, i, y, batch, hp)
            torch.cuda.synchronize()
            assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
            assert torch.equal(ta, tb) and a.t == b.t

        ca.set_spin_limit(0)
        same()
        assert ca.recoveries() == 1
        ca.set_spin_limit(1 << 22)  # the default: the tail runs in line again, on zeroed counters
        same()
        assert ca.recoveries() == 1
        ca.set_failsafe(False)
        ca.set_spin_limit(0)
        with pytest.raises(RuntimeError, match="timed out"):
            ca.train(u, i, y, batch, hp)
        assert ca.recoveries() == 1
        # what the failed call wrote is undefined: start both over; the context itself is sound
        ca.set_spin_limit(1 << 22)
        _reset(a, P)
        _reset(b, P)
        same()
