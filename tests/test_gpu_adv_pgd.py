"""The iterated attack on the GPU: the kept plan and the planned
direction (ops.adv_plan, ops.adv_direction(plan=...)), the projected step and its
loop (ops.adv_pgd), evaluate.robustness's "pgd" mode and the CLI's --robust_iters.

The yardstick is evaluate.pgd_host (float64 numpy) on the fixture of
pgd_fixture.py; test_adv_pgd_host.py shows on the CPU that the restatement alone
meets what is asserted of the GPU here."""
import glob
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pgd_fixture as F
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6  # the project's single-step bar


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".evaluate")


@pytest.fixture(scope="module", params=F.DIMS)
def case(request, ops, dev):
    """The fixture at one d: host arrays, device tensors, one plan."""
    host = F.problem(request.param)
    T = tuple(torch.tensor(x, device=dev) for x in host)
    plan = ops.adv_plan(T[2], T[3], T[4], F.U1, F.I1)
    return SimpleNamespace(d=request.param, host=host, T=T, plan=plan)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _bits64(a, b):
    return a.dtype == b.dtype == torch.float64 and bool((a.view(torch.int64) == b.view(torch.int64)).all())


def _np(t):
    return t.cpu().numpy()


# ---- the plan and the planned direction -------------------------------------------
def test_planned_direction_gives_the_unplanned_bits(ops, dev, case):
    P, Q, u, i, j = case.T
    a = ops.adv_direction(P, Q, u, i, j)
    b = ops.adv_direction(P, Q, u, i, j, plan=case.plan)
    assert _bits(a[0], b[0]) and _bits(a[1], b[1])
    ops.recommend_topk(P, Q, torch.arange(8, dtype=torch.int32, device=dev), 10)  # another kernel in between
    c = ops.adv_direction(P, Q, u, i, j, plan=case.plan)
    assert _bits(a[0], c[0]) and _bits(a[1], c[1])
    assert not a[0][F.FREE_USER].any() and not a[1][F.FREE_ITEM].any() and bool(a[0][F.HOT_USER].any())


def test_one_plan_serves_two_table_pairs(ops, case):
    P, Q, u, i, j = case.T
    P2, Q2 = (torch.tensor(x, device=P.device) for x in F.problem(case.d, seed=1)[:2])
    for A, B in ((P, Q), (P2, Q2), (P, Q)):
        want = ops.adv_direction(A, B, u, i, j)
        got = ops.adv_direction(A, B, u, i, j, plan=case.plan)
        assert _bits(want[0], got[0]) and _bits(want[1], got[1])
    assert not _bits(ops.adv_direction(P, Q, u, i, j)[0], ops.adv_direction(P2, Q2, u, i, j)[0])
    with pytest.raises(ValueError, match="plan was built for"):
        ops.adv_direction(P[:-1].contiguous(), Q, u, i, j, plan=case.plan)
    with pytest.raises(ValueError, match="plan was built for"):
        ops.adv_direction(P, Q, u[:-1], i[:-1], j[:-1], plan=case.plan)


# ---- one step against the restatement ------------------------------------------------
def test_single_steps_match_the_restatement(ops, ev, case):
    """Teacher-forced: step k starts from the GPU's own delta_k on both sides, so
    only one step's rounding is compared.  Rows no triplet touches keep their bits."""
    Ph, Qh, uh, ih, jh = case.host
    P, Q, u, i, j = case.T
    cu, ci = F.term_counts(uh, ih, jh)
    alpha = 2.5 * F.EPS / F.ITERS
    dP, dQ = torch.zeros_like(P), torch.zeros_like(Q)
    for k in range(5):
        nP, nQ, _ = ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=1, alpha=alpha, start=(dP, dQ), plan=case.plan)
        wP, wQ, _ = ev.pgd_host(Ph, Qh, uh, ih, jh, F.EPS, 1, alpha, "both", (_np(dP), _np(dQ)))
        for name, got, want, cnt, old in (("P", nP, wP, cu, dP), ("Q", nQ, wQ, ci, dQ)):
            err = np.abs(_np(got).astype(np.float64) - want)
            print(f"d {case.d} step {k} delta_{name}: max abs error {err.max():.3e}")
            np.testing.assert_allclose(_np(got)[cnt > 0], want[cnt > 0], rtol=RTOL, atol=ATOL,
                                       err_msg=f"step {k} delta_{name}")
            free = torch.as_tensor(np.flatnonzero(cnt == 0), device=P.device)
            assert _bits(got[free], old[free]), f"step {k}: untouched rows of delta_{name} moved"
        dP, dQ = nP, nQ


@pytest.mark.parametrize("which", ["none", "touched", "mixed"])
def test_projection_takes_the_restatements_branch(ops, ev, case, which):
    """Small step from zero: no row leaves the ball.  alpha = 2 eps: every touched
    row is projected.  Mixed start: both kinds.  The restatement says which branch
    a row takes; a row the GPU projected ends on the edge, one it kept ends where
    the restatement's unprojected row does.  Rows within 1e-5 eps of the edge are
    skipped, at most 2 of them (test_adv_pgd_host.py: the fixture meets the cap)."""
    Ph, Qh, uh, ih, jh = case.host
    P, Q, u, i, j = case.T
    alpha = 2 * F.EPS if which == "touched" else F.EPS / 20
    start_h = F.mixed_start(case.d) if which == "mixed" else None
    start = tuple(torch.tensor(x, device=P.device) for x in start_h) if start_h else None
    dP, dQ, _ = ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=1, alpha=alpha, start=start, plan=case.plan)
    wP, wQ, _ = ev.pgd_host(Ph, Qh, uh, ih, jh, F.EPS, 1, alpha, "both", start_h)
    nu, ni = F.pre_projection_norms(ev.pgd_host, Ph, Qh, uh, ih, jh, alpha, start_h)
    skipped = 0
    for name, got, want, norms in (("P", dP, wP, nu), ("Q", dQ, wQ, ni)):
        proj, skip = F.branches(norms, F.EPS)
        skipped += int(skip.sum())
        g = np.linalg.norm(_np(got).astype(np.float64), axis=1)
        on_edge = g > F.EPS * (1 - 5e-6)  # a kept row's norm is below eps (1 - 1e-5) up to fp32 rounding
        keep = ~skip
        assert np.array_equal(on_edge[keep], proj[keep]), (name, np.flatnonzero(on_edge != proj))
        np.testing.assert_allclose(_np(got)[keep], want[keep], rtol=RTOL, atol=ATOL, err_msg=f"delta_{name}")
        if which == "mixed":
            assert proj[keep].any() and (~proj[keep]).any()
    assert skipped <= 2


# ---- the loop ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five(ops, case):
    P, Q, u, i, j = case.T
    return ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=F.ITERS, plan=case.plan)


def test_five_iterations_equal_five_chained_calls(ops, case, five):
    P, Q, u, i, j = case.T
    alpha = 2.5 * F.EPS / F.ITERS
    dP = dQ = None
    losses = []
    for k in range(F.ITERS):
        dP, dQ, ls = ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=1, alpha=alpha, start=None if k == 0 else (dP, dQ))
        assert not losses or _bits64(losses[-1][1:], ls[:1])
        losses.append(ls)
    assert _bits(dP, five[0]) and _bits(dQ, five[1])
    chained = torch.cat([ls[:1] for ls in losses] + [losses[-1][1:]])
    assert _bits64(chained, five[2])


def test_equal_calls_give_equal_bits(ops, case, five):
    P, Q, u, i, j = case.T
    again = ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=F.ITERS)  # plans inside the call
    assert _bits(again[0], five[0]) and _bits(again[1], five[1]) and _bits64(again[2], five[2])
    acf_ops = importlib.import_module(PKG + ".torch_ops").load()
    op = acf_ops.adv_pgd(P, Q, u, i, j, F.EPS, F.ITERS)
    assert _bits(op[0], five[0]) and _bits(op[1], five[1]) and _bits64(op[2], five[2])


def test_every_row_stays_in_the_ball(ops, case, five):
    P, Q, u, i, j = case.T
    runs = [five[:2], ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=2, alpha=2 * F.EPS, start="random", seed=9)[:2],
            ops.adv_pgd(P, Q, u, i, j, 0.0, iters=2, alpha=0.1)[:2]]
    for (dP, dQ), eps in zip(runs, (F.EPS, F.EPS, 0.0)):
        for t in (dP, dQ):
            norms = np.linalg.norm(_np(t).astype(np.float64), axis=1)
            assert (norms <= eps * (1 + 1e-6)).all(), norms.max()
    # the random start puts every row on the edge, touched or not
    assert np.linalg.norm(_np(runs[1][0])[F.FREE_USER].astype(np.float64)) == pytest.approx(F.EPS, rel=1e-5)


def test_sides_leave_the_other_delta_at_its_start(ops, case):
    P, Q, u, i, j = case.T
    sP, sQ = (torch.tensor(x, device=P.device) for x in F.mixed_start(case.d, eps=F.EPS / 2))
    dP, dQ, _ = ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=2, side="user", start=(sP, sQ), plan=case.plan)
    assert _bits(dQ, sQ) and not _bits(dP, sP)
    dP, dQ, _ = ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=2, side="item", start=(sP, sQ), plan=case.plan)
    assert _bits(dP, sP) and not _bits(dQ, sQ)
    dP, dQ, _ = ops.adv_pgd(P, Q, u, i, j, F.EPS, iters=2, side="user", plan=case.plan)
    assert not dQ.any() and bool(dP.any())


def test_losses_start_clean_and_rise(ops, ev, case, five):
    Ph, Qh, uh, ih, jh = case.host
    P, Q, u, i, j = case.T
    losses = _np(five[2])
    clean = float(ops.bpr_forward(P, Q, u, i, j, 100)[0].double().sum())  # 14 fp32 batch sums, added in fp64
    want = ev.pgd_host(Ph, Qh, uh, ih, jh, F.EPS, F.ITERS)[2]
    print(f"d {case.d} losses {losses.tolist()} (restatement {want.tolist()}), bpr_forward {clean}")
    assert losses[0] == pytest.approx(clean, rel=1e-6)
    assert losses[-1] > losses[0]
    np.testing.assert_allclose(losses, want, rtol=1e-5)


def test_no_triplets_project_the_start(ops, case):
    P, Q, u, i, j = case.T
    sP, sQ = (torch.tensor(x, device=P.device) for x in F.mixed_start(case.d))
    dP, dQ, losses = ops.adv_pgd(P, Q, u[:0], i[:0], j[:0], F.EPS, iters=3, start=(sP, sQ))
    assert not losses.any() and losses.shape == (4,)
    for got, s in ((dP, sP), (dQ, sQ)):
        n0 = np.linalg.norm(_np(s).astype(np.float64), axis=1)
        want = _np(s).astype(np.float64) * np.minimum(1.0, F.EPS / n0)[:, None]
        np.testing.assert_allclose(_np(got), want, rtol=RTOL, atol=ATOL)
        inside = torch.as_tensor(np.flatnonzero(n0 < F.EPS * (1 - 1e-5)), device=P.device)
        assert _bits(got[inside], s[inside])


def test_out_of_range_index_is_an_index_error(ops, case):
    native = importlib.import_module(PKG + "._native")
    P, Q, u, i, j = case.T
    bad = j.clone()
    bad[40] = F.I1
    with pytest.raises(native.NativeIndexError, match="item"):
        ops.adv_pgd(P, Q, u, i, bad, F.EPS, iters=1, check=True)
    with pytest.raises(native.NativeIndexError, match="item"):
        ops.adv_plan(u, i, bad, F.U1, F.I1)
    lax = ops.adv_plan(u, i, bad, F.U1, F.I1, check=False)  # the word stays in the plan
    with pytest.raises(native.NativeIndexError, match="item"):
        ops.adv_pgd(P, Q, u, i, bad, F.EPS, iters=1, plan=lax, check=True)


# ---- against the certificate ----------------------------------------------------------
def _loo(dev):
    users, tests, off, ex, _ = F.loo_plan()
    return (torch.tensor(users, device=dev), torch.tensor(tests, device=dev), torch.tensor(off, device=dev),
            torch.tensor(ex, device=dev))


@pytest.mark.parametrize("eps", [0.05, 0.2])
def test_attack_never_beats_the_certificate(ops, case, eps):
    """The certified worst-case position bounds every attack within the budget, this
    one included; 0.1 % of slack on eps covers the projection's rounding."""
    P, Q, u, i, j = case.T
    users, tests, off, ex = _loo(P.device)
    dP, _, _ = ops.adv_pgd(P, Q, u, i, j, eps, iters=F.ITERS, side="user", plan=case.plan)
    Pa = ops.adv_apply(P, dP, 1.0)
    pos = _np(ops.eval_positions_all(Pa, Q, users, tests, F.I1, off, ex))
    worst = _np(ops.eval_positions_worst(P, Q, users, tests, F.I1, off, ex, eps=(1.001 * eps,), side="user"))[0]
    clean = _np(ops.eval_positions_all(P, Q, users, tests, F.I1, off, ex))
    print(f"d {case.d} eps {eps}: mean position clean {clean.mean():.2f}, attacked {pos.mean():.2f}, "
          f"certified worst {worst.mean():.2f}")
    assert len(pos) == F.U1 and (pos <= worst).all(), np.flatnonzero(pos > worst)


# ---- evaluate.robustness and the CLI --------------------------------------------------------
def test_robustness_pgd_rows(ops, ev, case):
    """One step of size eps from zero is the single-step attack up to the projection's
    rounding: the "pgd" rows rank as the "grad" rows do on all but one user at the most,
    and the "grad" rows are what adv_direction + adv_apply + positions give."""
    P, Q, u, i, j = case.T
    users, tests, off, ex, lists = F.loo_plan()
    n_neg = np.array([F.I1 - len(x) for x in lists], np.int64)
    plan = ev.EvalPlan("all", users.astype(np.int64), tests.astype(np.int64), n_neg, 10, excl_off=off, excl=ex,
                       num_candidates=F.I1)
    model = SimpleNamespace(embedding_P=P, embedding_Q=Q)
    trip = SimpleNamespace(user=u, item_pos=i, item_neg=j)
    metrics = lambda pos: tuple(ev.metrics_from_positions(pos, n_neg, 10).mean(axis=0)[:, -1].tolist())  # noqa: E731
    nP, nQ = ops.adv_direction(P, Q, u, i, j)
    for eps in (0.05, 0.2):
        rows = ev.robustness(model, None, plan, trip, [0.0, eps], modes=("grad", "pgd"), iters=1, step=eps)
        assert [(r[0], r[1]) for r in rows] == [("grad", 0.0), ("grad", eps), ("pgd", 0.0), ("pgd", eps)]
        assert rows[2][2:] == rows[0][2:]
        for e, row in ((0.0, rows[0]), (eps, rows[1])):
            pos_g = _np(ev.positions(ops.adv_apply(P, nP, e), ops.adv_apply(Q, nQ, e), plan))
            assert row[2:] == metrics(pos_g)
        dP, dQ, _ = ops.adv_pgd(P, Q, u, i, j, eps, iters=1, alpha=eps)
        pos_p = _np(ev.positions(ops.adv_apply(P, dP, 1.0), ops.adv_apply(Q, dQ, 1.0), plan))
        assert len(pos_p) == F.U1 and int((pos_p != pos_g).sum()) <= 1
        assert rows[3][2:] == metrics(pos_p)
    assert [r[0] for r in ev.robustness(model, None, plan, trip, [0.05])] == ["grad", "random"]


def _video_run(cli, work, extra):
    os.makedirs(os.path.join(work, "data"), exist_ok=True)
    z = np.load(os.path.join(GOLDEN, "video_data.npz"))
    with open(os.path.join(work, "data", "Video.train.rating"), "w") as f:
        f.writelines(f"{u}\t{i}\t{r}\t1\n" for u, i, r in zip(z["train_u"], z["train_i"], z["train_r"]))
    with open(os.path.join(work, "data", "Video.test.rating"), "w") as f:
        f.writelines(f"{u}\t{i}\t1\t1\n" for u, i in zip(z["test_u"], z["test_i"]))
    rc = cli.main(["--path", work + "/", "--opath", "t/", "--dataset", "Video", "--model", "apr", "--epochs", "2",
                   "--adv_epoch", "1", "--verbose", "2", "--eval_mode", "all", "--embed_size", "16", "--ckpt", "0",
                   "--seed", "0", "--robust_eps", "0.5", *extra], "ori")
    assert rc == 0
    files = glob.glob(os.path.join(work, "out", "t", "*.robust"))
    assert len(files) == 1
    return open(files[0]).read(), cli.read_robust(files[0])


def test_cli_writes_pgd_rows_only_when_asked(acf, tmp_path, monkeypatch):
    cli = importlib.import_module(PKG + ".cli")
    monkeypatch.chdir(tmp_path)
    text, rows = _video_run(cli, str(tmp_path / "with"), ["--robust_iters", "3"])
    assert [(r[0], r[1]) for r in rows] == [("grad", 0.5), ("random", 0.5), ("pgd", 0.5)]
    assert all(0.0 <= x <= 1.0 for r in rows for x in r[2:])
    plain, rows0 = _video_run(cli, str(tmp_path / "without"), [])
    assert [(r[0], r[1]) for r in rows0] == [("grad", 0.5), ("random", 0.5)]
    # the same seed trains the same model: without the flag the file is the first two lines, byte for byte
    assert plain == "".join(text.splitlines(keepends=True)[:2])
