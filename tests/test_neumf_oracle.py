"""The NeuMF oracle (oracle/neumf_oracle.py) against torch-CPU autograd (float64)
of the same graph: gradients of the clean and the adversarial objective, the
delta, and the Keras Adam update.  Parity with the reference's own adversarial
NeuMF is unpinned (it does not run: NeuMF.py:131); the clean NeuMF graph follows
NeuMF.py:10-52."""
import numpy as np
import pytest
import torch

import neumf_oracle as N
import neumf_ref as R
from neumf_ref import _torch_grads

U1, I1, D, B = 23, 19, 8, 40


def _problem(seed):
    P = N.init_params(U1, I1, D, seed)
    rng = np.random.default_rng(seed + 1)
    u = rng.integers(0, U1, B)
    i = rng.integers(0, I1, B)
    u[:5] = 3  # duplicated rows
    i[3:9] = 7
    y = (rng.random(B) < 0.5).astype(np.float32)
    return P, u, i, y


@pytest.mark.parametrize("adver", [0, 1])
def test_oracle_grads_match_autograd(adver):
    P, u, i, y = _problem(3 + adver)
    hp = N.NeuMFHParams(adver=adver, eps=0.5, reg_adv=1.0)
    g, lc, la = N.grad_step(P, u, i, y, hp)
    want, lc_t = _torch_grads(P, u, i, y, hp)
    assert abs(lc - lc_t) < 1e-5
    for n in N.NAMES:
        np.testing.assert_allclose(g[n], want[n], rtol=2e-4, atol=2e-7, err_msg=n)
    if adver:
        assert la > 0


def test_untouched_rows_have_zero_gradient():
    P, u, i, y = _problem(5)
    g, *_ = N.grad_step(P, u, i, y, N.NeuMFHParams(adver=1))
    untouched = np.setdiff1d(np.arange(U1), u)
    assert np.all(g["MF_U"][untouched] == 0) and np.all(g["MLP_U"][untouched] == 0)


def test_adam_matches_keras_formula():
    """Keras 2.2 Adam: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); dense update, so a
    parameter with zero gradient still moves when its moment is non-zero."""
    hp = N.NeuMFHParams()
    P = {n: np.ones(s, np.float32) for n, s in N.shapes(3, 3, 4).items()}
    m = {n: np.zeros_like(P[n]) for n in N.NAMES}
    v = {n: np.zeros_like(P[n]) for n in N.NAMES}
    g = {n: np.full_like(P[n], 0.5) for n in N.NAMES}
    N.adam(P, g, m, v, 1, hp)
    lr_t = 0.001 * np.sqrt(1 - 0.999) / (1 - 0.9)
    want = 1 - lr_t * (0.1 * 0.5) / (np.sqrt(0.001 * 0.25) + 1e-7)
    np.testing.assert_allclose(P["W1"], want, rtol=1e-6)
    g0 = {n: np.zeros_like(P[n]) for n in N.NAMES}
    before = P["W1"].copy()
    N.adam(P, g0, m, v, 2, hp)
    assert np.all(P["W1"] < before)  # momentum keeps moving it


@pytest.mark.parametrize("adver", [0, 1])
@pytest.mark.parametrize("case", R.GRAD_CASES + R.LIMIT_CASES[:1] + R.DIM_CASES, ids=R.case_id)
def test_batches_bar_is_met_by_the_oracle_alone(case, adver):
    """The bar test_gpu_neumf_batches.py holds the GPU to (neumf_ref.check_grads with
    the calibrated k) checked without a GPU, per case: the fp32 oracle is within a
    quarter of it; it has teeth (no tensor would pass as all zero, and no touched
    row of MF_U or MF_I would pass as a zero row, which is what a kernel that
    lost a row's owner leaves; the MLP rows travel with them); every row
    of the small tables is in the batch, and the planted rows are where
    neumf_ref.plants says."""
    B, d, U1, I1 = case
    ref = R.reference(case, adver)
    k = R.batches_k()
    assert k <= R.K_MAX
    worst = max(ref["dist"], key=ref["dist"].get)
    print(f"{R.case_id(case)} adver={adver}: oracle worst {ref['dist'][worst]:.2e} ({worst}); k = {k:.3e}")
    assert 4 * ref["dist"][worst] <= k
    want, u, i = ref["want"], ref["u"], ref["i"]
    for n in N.NAMES:
        quarter = R.bar(want[n], k) / 4
        err = np.abs(ref["oracle"][n].astype(np.float64) - want[n])
        assert (err <= quarter).all(), f"{n}: the oracle is {float((err / quarter).max()):.2f} quarter-bars off"
    zeros = {n: np.zeros_like(want[n]) for n in N.NAMES}
    for n in N.NAMES:
        with pytest.raises(AssertionError, match=n + ":"):
            R.check_grads({**zeros, **{m: want[m] for m in N.NAMES if m != n}}, want, k)
    for n in ("MF_U", "MF_I"):  # (an MLP row can have next to no gradient: dead relus)
        touched = np.unique(u if n.endswith("_U") else i)
        row_top = np.abs(want[n][touched]).max(1)
        floor = k * np.abs(want[n]).max() / (1 - R.RTOL)  # |w| <= rtol |w| + k max: passes as zero
        assert (row_top > floor).all(), f"{n}: {int((row_top <= floor).sum())} touched rows would pass as zero rows"
    if U1 <= B and I1 <= B:
        assert len(np.unique(u)) == U1 and len(np.unique(i)) == I1
    if B >= 2064:
        assert list(np.nonzero(u == 7)[0][[0, -1]]) == [0, B - 1] and u[2047] == u[2048] == 7
        assert np.nonzero(u == 9)[0][0] == 2049 and list(np.nonzero(u == 11)[0]) == [B - 2]
        assert np.nonzero(i == 9)[0][0] == 2048 and list(np.nonzero(i == 11)[0]) == [B - 1]
    np.testing.assert_allclose(ref["oracle_losses"], [ref["lc"], ref["la"]], rtol=2e-6)
