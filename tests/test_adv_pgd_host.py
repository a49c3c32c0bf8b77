"""The iterated attack without a GPU: evaluate.pgd_host (the float64 restatement
the GPU tests measure against) on the shared fixture, the fixture's own
guarantees, argument validation of ops.adv_pgd / evaluate.robustness("pgd"),
the C-ABI declarations and the CLI flags."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import pgd_fixture as F
from conftest import PKG, REPO


@pytest.fixture(scope="module")
def native():
    mod = importlib.import_module(PKG + "._native")
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


@pytest.fixture(scope="module")
def ops(native):
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def ev(native):
    return importlib.import_module(PKG + ".evaluate")


@pytest.fixture(scope="module")
def solved(ev):
    """pgd_host on the d = 8 fixture, once."""
    P, Q, u, i, j = F.problem(8)
    return (P, Q, u, i, j), ev.pgd_host(P, Q, u, i, j, F.EPS, F.ITERS)


def test_fixture_has_the_row_shapes_it_promises():
    for d in F.DIMS:
        P, Q, u, i, j = F.problem(d)
        assert P.shape == (F.U1, d) and Q.shape == (F.I1, d) and len(u) == len(i) == len(j) == F.N
        cu, ci = F.term_counts(u, i, j)
        assert 512 < cu[F.HOT_USER] <= 768  # three chunks
        assert ci[F.FULL_ITEM] == 256 and ci[F.ONCE_ITEM] == 1
        assert cu[F.FREE_USER] == 0 and ci[F.FREE_ITEM] == 0


def test_projection_keeps_every_row_in_the_ball(solved):
    _, (dP, dQ, losses) = solved
    for t in (dP, dQ):
        assert (np.linalg.norm(t, axis=1) <= F.EPS * (1 + 1e-12)).all()
    assert losses.shape == (F.ITERS + 1,) and np.isfinite(losses).all()
    # the default step 2.5 eps / iters walks every touched row to the edge within the five steps
    assert np.isclose(np.linalg.norm(dP[F.HOT_USER]), F.EPS) and not dP[F.FREE_USER].any()


def test_zero_step_is_a_no_op(ev, solved):
    (P, Q, u, i, j), (dP, dQ, _) = solved
    sP, sQ = (x.astype(np.float64) for x in F.mixed_start(8, eps=F.EPS / 2))  # row norms in [0, eps)
    aP, aQ, losses = ev.pgd_host(P, Q, u, i, j, F.EPS, 3, 0.0, "both", (sP, sQ))
    assert np.array_equal(aP, sP) and np.array_equal(aQ, sQ)
    assert losses[0] == losses[-1]
    # rows already on the edge: projecting again moves them by a rounding error at the most
    aP, aQ, _ = ev.pgd_host(P, Q, u, i, j, F.EPS, 3, 0.0, "both", (dP, dQ))
    np.testing.assert_allclose(aP, dP, rtol=1e-14, atol=0)
    np.testing.assert_allclose(aQ, dQ, rtol=1e-14, atol=0)


def test_user_side_leaves_the_item_delta_at_its_start(ev, solved):
    (P, Q, u, i, j), _ = solved
    sP, sQ = F.mixed_start(8, eps=F.EPS / 2)  # inside the ball or not: the still side is not projected either
    dP, dQ, _ = ev.pgd_host(P, Q, u, i, j, F.EPS, 2, None, "user", (sP, sQ))
    assert np.array_equal(dQ, sQ.astype(np.float64)) and not np.array_equal(dP, sP.astype(np.float64))
    dP, dQ, _ = ev.pgd_host(P, Q, u, i, j, F.EPS, 2, None, "item", (sP, sQ))
    assert np.array_equal(dP, sP.astype(np.float64)) and not np.array_equal(dQ, sQ.astype(np.float64))


def test_eps_zero_gives_zeros(ev, solved):
    (P, Q, u, i, j), _ = solved
    dP, dQ, losses = ev.pgd_host(P, Q, u, i, j, 0.0, 3, 0.1)
    assert not dP.any() and not dQ.any()
    assert losses[0] == losses[-1]


@pytest.mark.parametrize("d", F.DIMS)
def test_the_attack_raises_the_loss_on_the_fixture(ev, d):
    """What test_gpu_adv_pgd.py asserts of the GPU holds for the restatement alone."""
    P, Q, u, i, j = F.problem(d)
    losses = ev.pgd_host(P, Q, u, i, j, F.EPS, F.ITERS)[2]
    assert losses[-1] > losses[0] * 1.01 and (np.diff(losses) > 0).all(), losses


@pytest.mark.parametrize("d", F.DIMS)
def test_projection_cases_skip_at_most_two_rows(ev, d):
    """The three cases of the GPU's branch test, on the restatement: with a small
    step from zero no row leaves the ball, with alpha = 2 eps every touched row
    does, the mixed start has rows of both kinds; at most 2 rows lie within 1e-5
    eps of the edge."""
    P, Q, u, i, j = F.problem(d)
    cu, ci = F.term_counts(u, i, j)
    for alpha, start, want in ((F.EPS / 20, None, "none"), (2 * F.EPS, None, "touched"),
                               (F.EPS / 20, F.mixed_start(d), "mixed")):
        nu, ni = F.pre_projection_norms(ev.pgd_host, P, Q, u, i, j, alpha, start)
        skipped = 0
        for norms, cnt in ((nu, cu), (ni, ci)):
            proj, skip = F.branches(norms, F.EPS)
            skipped += int(skip.sum())
            if want == "none":
                assert not proj.any()
            elif want == "touched":
                assert np.array_equal(proj, cnt > 0)
            else:
                assert proj.sum() >= 5 and (~proj).sum() >= 5
        assert skipped <= 2, (d, want, skipped)


def test_header_and_binding_declare_the_entry_points(native):
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    fns = set(re.findall(r"^\s*int\s+(acf_\w+)\s*\(", text, re.M))
    want = {"acf_adv_plan_workspace", "acf_adv_plan", "acf_adv_direction_planned", "acf_adv_pgd_workspace",
            "acf_adv_pgd"}
    assert want <= fns and want <= set(native.SIGNATURES) and want <= native.exported_symbols()


def test_workspace_queries_are_host_only(native, ops):
    pb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    native.call("acf_adv_plan_workspace", 1400, 37, 53, ctypes.byref(pb), ctypes.byref(wb))
    assert pb.value >= 4 * 1400 * 4 + (37 + 53 + 1) * 4 + 4 and wb.value >= 4 * 4 * 1400 * 4
    direction = ops.adv_direction_workspace(1400, 37, 53, 64)
    pgd = ops.adv_pgd_workspace(1400, 37, 53, 64)
    assert pgd >= direction + pb.value + 2 * (37 + 53) * 64 * 4
    assert ops.adv_pgd_workspace(0, 37, 53, 64) >= 2 * (37 + 53) * 64 * 4
    with pytest.raises(native.NativeError):
        native.call("acf_adv_plan_workspace", 1 << 29, 37, 53, ctypes.byref(pb), ctypes.byref(wb))
    with pytest.raises(ValueError, match="n must lie"):
        ops.adv_pgd_workspace(-1, 37, 53, 64)


def test_native_pgd_rejects_bad_arguments_before_any_launch(native):
    """Every refusal below comes before the first HIP call: the pointers are never used."""
    one = ctypes.c_void_p(256)  # aligned, never dereferenced

    def pgd(eps=0.5, alpha=0.1, iters=3, side=0, ws_bytes=1 << 40):
        return native.load().acf_adv_pgd(one, one, 37, 53, 8, one, one, one, 10, -80.0, 1e8, None, 0, eps, alpha,
                                         iters, side, None, None, one, one, one, one, ws_bytes, 0, None)
    for kw in (dict(iters=0), dict(iters=1025), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(alpha=-0.1), dict(alpha=float("nan")), dict(side=3), dict(side=-1), dict(ws_bytes=16)):
        assert pgd(**kw) == native.ACF_E_INVALID, kw


def _cpu_problem():
    P, Q = torch.zeros(4, 8), torch.zeros(6, 8)
    u = torch.zeros(5, dtype=torch.int32)
    return P, Q, u


def test_adv_pgd_validates_before_any_native_call(ops, monkeypatch):
    for mod in (ops._native, ops):
        monkeypatch.setattr(mod, "call", lambda *a, **k: pytest.fail("a native call was made"))
    P, Q, u = _cpu_problem()
    for iters in (0, 1025):
        with pytest.raises(ValueError, match="iters must lie"):
            ops.adv_pgd(P, Q, u, u, u, 0.5, iters=iters)
    with pytest.raises(TypeError, match="iters"):
        ops.adv_pgd(P, Q, u, u, u, 0.5, iters=2.5)
    for eps in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps must be"):
            ops.adv_pgd(P, Q, u, u, u, eps)
    for alpha in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="alpha must be"):
            ops.adv_pgd(P, Q, u, u, u, 0.5, alpha=alpha)
    with pytest.raises(ValueError, match="side must be"):
        ops.adv_pgd(P, Q, u, u, u, 0.5, side="rows")
    with pytest.raises(ValueError, match="equal lengths"):
        ops.adv_pgd(P, Q, u, u[:4], u, 0.5)
    with pytest.raises(ValueError, match="table's shape"):
        ops.adv_pgd(P, Q, u, u, u, 0.5, start=(torch.zeros(4, 8), torch.zeros(5, 8)))
    with pytest.raises(ValueError, match="table's shape"):
        ops.adv_pgd(P, Q, u, u, u, 0.5, start=(torch.zeros(4, 4), torch.zeros(6, 8)))
    with pytest.raises(ValueError, match="start must be"):
        ops.adv_pgd(P, Q, u, u, u, 0.5, start="zeros")
    with pytest.raises(TypeError, match="start must be"):
        ops.adv_pgd(P, Q, u, u, u, 0.5, start=torch.zeros(4, 8))
    with pytest.raises(ValueError, match="HIP device"):  # CPU tensors: there is no CPU path
        ops.adv_pgd(P, Q, u, u, u, 0.5)
    with pytest.raises(TypeError, match="AdvPlan"):
        ops.adv_direction(P, Q, u, u, u, plan=object())
    with pytest.raises(ValueError, match="HIP device"):
        ops.adv_plan(u, u, u, 4, 6)
    with pytest.raises(ValueError, match="equal lengths"):
        ops.adv_plan(u, u[:3], u, 4, 6)


def test_robustness_pgd_validates_before_any_native_call(ops, ev, monkeypatch):
    for mod in (ops._native, ops):
        monkeypatch.setattr(mod, "call", lambda *a, **k: pytest.fail("a native call was made"))
    trip = ([np.zeros(5, np.int32)],) * 3

    def run(eps=(0.5,), triplets=trip, **kw):
        return ev.robustness(None, None, None, triplets, eps, modes=("pgd",), **kw)
    for iters in (0, 1025):
        with pytest.raises(ValueError, match="iters must lie"):
            run(iters=iters)
    with pytest.raises(ValueError, match="eps must be"):
        run(eps=(0.5, -1.0))
    with pytest.raises(ValueError, match="eps must be"):
        run(eps=(float("nan"),))
    for step in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="alpha must be"):
            run(step=step)
    with pytest.raises(ValueError, match="side must be"):
        run(side="rows")
    with pytest.raises(ValueError, match="equal lengths"):
        run(triplets=([np.zeros(5, np.int32)], [np.zeros(4, np.int32)], [np.zeros(5, np.int32)]))
    with pytest.raises(ValueError, match="at least one triplet"):
        run(triplets=([], [], []))
    with pytest.raises(ValueError, match="mode must be"):
        ev.robustness(None, None, None, trip, [0.5], modes=("fgsm",))


def test_surface_passes_the_keywords_through(acf):
    import inspect
    for fn in (acf.robustness, acf.MF.robustness, acf.APR.robustness):
        params = inspect.signature(fn).parameters
        assert (params["iters"].default, params["step"].default, params["side"].default) == (10, None, "both")
        assert params["modes"].default == ("grad", "random")
    tops = importlib.import_module(PKG + ".torch_ops")
    assert "adv_pgd" in tops.OPS and hasattr(tops.load(), "adv_pgd")


@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_cli_flags_default_to_off(flavor):
    cli = importlib.import_module(PKG + ".cli")
    a = cli.parse_args([], flavor)
    assert a.robust_iters == 0 and a.robust_step is None
    a = cli.parse_args(["--robust_eps", "0.5", "--robust_iters", "3", "--robust_step", "0.25"], flavor)
    assert a.robust_iters == 3 and a.robust_step == 0.25 and a.robust_eps == [0.5]
    for bad in (["--robust_iters", "-1"], ["--robust_iters", "1025"], ["--robust_iters", "x"],
                ["--robust_step", "-0.1"], ["--robust_step", "nan"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad, flavor)
