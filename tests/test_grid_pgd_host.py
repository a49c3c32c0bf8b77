"""Grid training against a K-step inner attack, without a GPU: the
reference of tests/grid_pgd_ref.py against torch autograd and the oracle, the fp32
restatement's distance from it on every input of the GPU tests (the source of their
tolerance), the workspace query and the refusals of acf_apr_grid_pgd_workspace /
acf_apr_grid_train_pgd before any launch, ops.grid_train's validation, MFGrid.product's
order, the run names and .grid files with and without the new axis, the CLI flags,
and the refusal of every one-step trainer."""
import argparse
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import grid_pgd_ref as ref
from apr_oracle import HParams
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
def cli():
    return importlib.import_module(PKG + ".cli")


# ---- the reference ---------------------------------------------------------------------
def _autograd(P, Q, u, i, j, h):
    """(delta_P, delta_Q, G_P, G_Q) of one batch by torch autograd in float64."""
    P, Q = torch.tensor(P, dtype=torch.float64), torch.tensor(Q, dtype=torch.float64)
    u, i, j = (torch.tensor(x, dtype=torch.int64) for x in (u, i, j))
    B, d = len(u), P.shape[1]

    def loss(Pa, Qa):
        x = (Pa[u] * Qa[i]).sum(1) - (Pa[u] * Qa[j]).sum(1)
        return torch.nn.functional.softplus(-x.clamp(h["clip_lo"], h["clip_hi"])).sum()

    def unit(g):
        return g / (g * g).sum(1, keepdim=True).clamp_min(1e-12).sqrt()
    dP, dQ = torch.zeros_like(P), torch.zeros_like(Q)
    for _ in range(h["adv_iters"]):
        a, b = dP.clone().requires_grad_(), dQ.clone().requires_grad_()
        gP, gQ = torch.autograd.grad(loss(P + a, Q + b), (a, b))
        if h["adv_iters"] == 1:
            dP, dQ = unit(gP) * h["eps"], unit(gQ) * h["eps"]
            break
        out = []
        for dl, g in ((dP, gP), (dQ, gQ)):
            v = dl + h["adv_step"] * unit(g)
            s = (v * v).sum(1, keepdim=True).sqrt()
            out.append(torch.where(s <= h["eps"], v, v * (h["eps"] / s.clamp_min(1e-300))))
        dP, dQ = out
    Pg, Qg = P.clone().requires_grad_(), Q.clone().requires_grad_()
    reg = h["reg"] * 2.0 / (B * d) * ((Pg[u] ** 2).sum() + (Qg[i] ** 2).sum() + (Qg[j] ** 2).sum())
    total = loss(Pg, Qg) + reg + h["reg_adv"] * loss(Pg + dP, Qg + dQ)  # adver = 1: reg counts twice
    GP, GQ = torch.autograd.grad(total, (Pg, Qg))
    return [t.numpy() for t in (dP, dQ, GP, GQ)]


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_reference_equals_autograd(m):
    P, Q, u, i, j, batch, hps = ref.parity_case(20)
    h = ref.hparams(hps[m])
    s = slice(0, batch)
    P64, Q64 = P[m].astype(np.float64), Q[m].astype(np.float64)
    _, _, GP, GQ, dP, dQ = ref.gradient64(P64, Q64, u[s].astype(np.int64), i[s].astype(np.int64),
                                          j[s].astype(np.int64), h)
    for got, want, n in zip((dP, dQ, GP, GQ), _autograd(P64, Q64, u[s], i[s], j[s], h),
                            ("delta_P", "delta_Q", "G_P", "G_Q")):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-10, err_msg=n)
    if h["adv_iters"] == 3:  # alpha = eps: the projection has engaged, every moved row is on the sphere
        norms = np.sqrt((dP * dP).sum(1))[np.unique(u[s])]
        np.testing.assert_allclose(norms, h["eps"], rtol=1e-12)
    if h["adv_iters"] == 2:  # alpha = eps / (2K): inside the ball
        assert np.sqrt((dP * dP).sum(1)).max() <= 0.5 * h["eps"] * (1 + 1e-12)


@pytest.mark.parametrize("hp", [dict(adver=1, eps=0.5), dict(adver=1, eps=2.0, reg_adv=0.1, reg=0.01, lr=0.1),
                                dict(adver=0, reg=0.01)])
def test_reference_at_one_step_equals_the_oracle(oracle, hp):
    P, Q = ref.tables(64, 1, 64)
    u, i, j = ref.triplets(164, ref.NB * ref.B)
    want, lc, la = ref.run_member(ref.step64, P[0], Q[0], u, i, j, ref.B, hp, np.float64)
    oP, oQ = P[0].copy(), Q[0].copy()
    aP, aQ = np.full(oP.shape, 0.1, np.float32), np.full(oQ.shape, 0.1, np.float32)
    for t in range(ref.NB):
        s = slice(t * ref.B, (t + 1) * ref.B)
        olc, ola, _, _ = oracle.apr_batch(oP, oQ, aP, aQ, u[s], i[s], j[s], HParams(**hp))
        np.testing.assert_allclose(olc, lc[s], rtol=ref.RTOL, atol=ref.ATOL)
        if hp["adver"]:
            np.testing.assert_allclose(ola, la[s], rtol=ref.RTOL, atol=ref.ATOL)
    for got, w, n in zip((oP, oQ, aP, aQ), want, "P Q accP accQ".split()):
        np.testing.assert_allclose(got, w, rtol=ref.RTOL, atol=ref.ATOL, err_msg=n)


def _cases():
    return [(("parity", d), ref.parity_case(d)) for d in ref.PARITY_DIMS] + \
           [(("degenerate", n), ref.degenerate_case(n)) for n in ref.DEGENERATE]


def test_fp32_restatement_stays_inside_the_tolerance_on_every_gpu_input(capsys):
    """The tolerance of the GPU tests is 4 x this deviation (floor: the project's), so
    the restatement is inside it by a factor of 4 where the floor does not apply; the
    figures are printed (pytest -s) and recorded in test_gpu_grid_pgd.py's docstring."""
    with capsys.disabled():
        for key, case in _cases():
            devs = [r[3] for r in ref.reference(key, case)]
            rtol, atol = ref.tolerance(key, case)
            print("\n%s: deviation %s, rtol %.3g atol %.0e" % (key, " ".join("%.2e" % x for x in devs), rtol, atol),
                  end="")
            assert np.isfinite(devs).all() and max(devs) <= rtol and rtol >= ref.RTOL and atol == ref.ATOL
            assert rtol <= 1e-4  # a seed whose restatement drifts further is changed, not tolerated


def test_degenerate_cases_are_what_they_claim():
    _, _, u, i, j, batch, _ = ref.degenerate_case("hot_user")
    assert batch == 160 and 2 * np.bincount(u[:batch]).max() == 320 > ref.CHUNK
    _, _, u, i, j, batch, _ = ref.degenerate_case("hot_item")
    assert (i == 7).all() and not (j == 7).any()
    P, Q, u, i, j, batch, hps = ref.degenerate_case("pos_equals_neg")
    assert (i[:8] == j[:8]).all() and not np.isin(u[8:batch], u[:8]).any() and not np.isin(i[8:batch], i[:8]).any()
    h = ref.hparams(hps[0])
    _, _, GP, GQ, dP, dQ = ref.gradient64(P[0].astype(np.float64), Q[0].astype(np.float64), u[:batch].astype(int),
                                          i[:batch].astype(int), j[:batch].astype(int), h)
    assert not GP[u[:8]].any() and not dP[u[:8]].any() and not dQ[i[:8]].any()  # zero gradient: delta stays 0
    P, Q, u, i, j, batch, hps = ref.degenerate_case("clipped")
    x = ((P[0][u] * Q[0][i]).sum(1) - (P[0][u] * Q[0][j]).sum(1))[:batch]
    assert (np.abs(x) > 0.5).sum() >= batch // 2 and (np.abs(x) < 0.5).any()


# ---- the C-ABI -------------------------------------------------------------------------
def _query(native, name, M=4, B=512, nb=8, U1=100, I1=80, d=64, out=True):
    size = ctypes.c_size_t()
    rc = getattr(native.load(), name)(M, B, nb, U1, I1, d, ctypes.byref(size) if out else None)
    return rc, size.value


def test_header_and_binding_declare_the_entry_points(native):
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    fns = set(re.findall(r"^\s*int\s+(acf_\w+)\s*\(", text, re.M))
    want = {"acf_apr_grid_pgd_workspace", "acf_apr_grid_train_pgd"}
    assert want <= fns and want <= set(native.SIGNATURES) and want <= native.exported_symbols()
    assert re.search(r"#define\s+ACF_GRID_MAX_ADV_ITERS\s+32\b", text)
    assert re.search(r"#define\s+ACF_APR_ABI_VERSION\s+2\b", text)


@pytest.mark.parametrize("kw", [dict(), dict(M=7, B=160, d=20), dict(M=64, B=1024, d=256, nb=1), dict(nb=0)])
def test_workspace_grows_by_exactly_the_second_delta_buffer(native, ops, kw):
    (rc0, base), (rc1, pgd) = _query(native, "acf_apr_grid_workspace", **kw), \
        _query(native, "acf_apr_grid_pgd_workspace", **kw)
    assert rc0 == rc1 == native.ACF_OK
    a = dict(dict(M=4, B=512, nb=8, U1=100, I1=80, d=64), **kw)
    assert pgd - base == (a["M"] * 3 * a["B"] * a["d"] * 4 + 255) // 256 * 256
    assert ops.grid_pgd_workspace(a["M"], a["B"], a["nb"], a["U1"], a["I1"], a["d"]) == pgd


def test_workspace_query_rejects_bad_shapes_without_a_device(native):
    for kw in (dict(M=0), dict(M=65), dict(d=2), dict(d=6), dict(d=260), dict(B=0), dict(B=1025), dict(nb=-1),
               dict(out=False)):
        assert _query(native, "acf_apr_grid_pgd_workspace", **kw)[0] == native.ACF_E_INVALID, kw


def test_native_train_rejects_bad_arguments_before_any_launch(native):
    """Every refusal below comes before the first HIP call: the pointers are never used."""
    one = ctypes.c_void_p(256)  # aligned, never dereferenced
    lib = native.load()

    def train(M=2, nb=3, iters=(1, 3), step=(0.0, 0.25), null=None, P=one, ws=one, ws_bytes=1 << 40, **field):
        hps = (native.HParams * 64)()
        for h in hps:
            h.lr, h.eps, h.reg_adv, h.clip_lo, h.clip_hi, h.adver = 0.05, 0.5, 1.0, -80.0, 1e8, 1
        for k, v in field.items():
            setattr(hps[1], k, v)
        K = None if null == "iters" else (ctypes.c_int32 * 64)(*iters)
        A = None if null == "step" else (ctypes.c_float * 64)(*step)
        return lib.acf_apr_grid_train_pgd(P, one, one, one, M, 65, 49, 64, hps, K, A, one, one, one, 32, nb, None,
                                          None, ws, ws_bytes, 0, None)
    for kw in (dict(iters=(1, 0)), dict(iters=(1, 33)), dict(iters=(-1, 3)), dict(step=(0.0, -0.5)),
               dict(step=(0.0, float("nan"))), dict(step=(float("inf"), 0.1)), dict(null="iters"), dict(null="step"),
               dict(M=0), dict(M=65), dict(P=None), dict(ws=None), dict(ws_bytes=16), dict(adv_mode=1),
               dict(zero_delta=1)):
        assert train(**kw) == native.ACF_E_INVALID, kw
    # the one-step query's bytes are too few for the K-step entry
    size = ctypes.c_size_t()
    assert lib.acf_apr_grid_workspace(2, 32, 3, 65, 49, 64, ctypes.byref(size)) == native.ACF_OK
    assert train(ws_bytes=size.value) == native.ACF_E_INVALID
    assert train(nb=0) == native.ACF_OK and train(nb=0, iters=(32, 1)) == native.ACF_OK  # nothing to do: no launch


# ---- ops.grid_train --------------------------------------------------------------------
def test_grid_train_validates_the_attack_before_any_native_call(ops, monkeypatch):
    for mod in (ops._native, ops):
        monkeypatch.setattr(mod, "call", lambda *a, **k: pytest.fail("a native call was made"))
    hp = ops.StepHParams(adver=1)
    tabs = [torch.zeros(2, 65, 8), torch.zeros(2, 49, 8), torch.zeros(2, 65, 8), torch.zeros(2, 49, 8)]
    u = torch.zeros(64, dtype=torch.int32)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match=r"adv_iters must lie in \[1, 32\]"):
            ops.grid_train(*tabs, [hp, ops.StepHParams(adver=1, adv_iters=bad)], u, u, u, 32)
    for bad in (2.0, True, "3"):
        with pytest.raises(TypeError, match="adv_iters must be an int"):
            ops.grid_train(*tabs, [hp, ops.StepHParams(adver=1, adv_iters=bad)], u, u, u, 32)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="adv_step must be finite"):
            ops.grid_train(*tabs, [hp, ops.StepHParams(adver=1, adv_iters=3, adv_step=bad)], u, u, u, 32)
    with pytest.raises(ValueError, match="adv_step must be finite"):  # the default step of eps = nan
        ops.grid_train(*tabs, [hp, ops.StepHParams(adver=1, adv_iters=3, eps=float("nan"))], u, u, u, 32)
    with pytest.raises(ValueError, match="HIP device"):  # valid K and alpha: the next refusal is the tensors'
        ops.grid_train(*tabs, [hp, ops.StepHParams(adver=1, adv_iters=32, adv_step=0.0)], u, u, u, 32)
    assert ops.grid_pgd_arguments(ops.StepHParams(eps=0.5, adv_iters=5)) == (5, 0.25)
    assert ops.grid_pgd_arguments(ops.StepHParams(eps=0.5, adv_iters=5, adv_step=0.1)) == (5, 0.1)


def test_step_hparams_keeps_its_c_struct(ops, native):
    a, b = ops.StepHParams(adver=1, eps=0.7).to_c(), ops.StepHParams(adver=1, eps=0.7, adv_iters=3, adv_step=0.2)._struct()
    assert ctypes.sizeof(a) == ctypes.sizeof(native.HParams) and bytes(a) == bytes(b)
    assert (ops.StepHParams().adv_iters, ops.StepHParams().adv_step) == (1, None)


# ---- one-step trainers refuse --------------------------------------------------------------
def _args(**kw):
    a = argparse.Namespace(embed_size=16, lr=0.05, reg=0.0, dns=1, adv="grad", eps=0.5, adver=1, reg_adv=1.0,
                           epochs=1, seed=0, eval_mode="all", batch_size=512, verbose=1, ckpt=0, path="", opath="g/",
                           dataset="Video", model="apr", restore=None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_stepwise_and_sharded_trainers_raise_on_k_steps(ops, native):
    model = importlib.import_module(PKG + ".model")
    distributed = importlib.import_module(PKG + ".distributed")
    hp = ops.StepHParams(adver=1, adv_iters=3)
    with pytest.raises(ValueError, match="one-step delta only"):
        hp.to_c()
    ctx = object.__new__(ops.APRContext)  # no device: the refusal comes before any native call
    ctx._tables = lambda *a: None
    ctx._ptr, ctx.device = None, torch.device("cpu")
    t = (None,) * 4
    for fn in (lambda: ctx.delta_update(t, hp, 0), lambda: ctx.optimizer_step(t, hp, 0),
               lambda: ctx.train_planned(t, hp, 0, 1),
               lambda: object.__new__(distributed.ShardedAPR).train(None, None, None, hp)):
        with pytest.raises(ValueError, match="one-step delta only"):
            fn()
    mf = model.MF(10, 10, _args(adv_iters=3))
    assert mf.hparams().adv_iters == 3 and mf.hparams(adver=0).adv_iters == 1  # a BPR step has no attack
    for fn in (lambda: mf.context(32, 1), lambda: mf.pipeline(32)):
        with pytest.raises(ValueError, match="one-step delta only"):
            fn()
    assert model.MF(10, 10, _args()).hparams().adv_iters == 1


# ---- MFGrid, names, .grid files ------------------------------------------------------------
def test_product_puts_adv_iters_outermost_and_is_unchanged_without_it(native):
    MFGrid = importlib.import_module(PKG + ".model").MFGrid
    g = MFGrid.product(eps=[0.1, 0.5], reg_adv=[0.5, 1.0], adv_iters=[1, 3])
    assert g == [dict(adv_iters=k, eps=e, reg_adv=r) for k in (1, 3) for e in (0.1, 0.5) for r in (0.5, 1.0)]
    assert MFGrid.product(adv_iters=[2, 5], adv_step=0.1) == [dict(adv_iters=2, adv_step=0.1),
                                                               dict(adv_iters=5, adv_step=0.1)]
    assert MFGrid.product(eps=[0.5], lr=[0.01, 0.05], seeds=2) == \
        [dict(eps=0.5, lr=lr, seed=s) for lr in (0.01, 0.05) for s in (0, 1)]  # the pinned order, no new key
    with pytest.raises(ValueError, match="empty"):
        MFGrid.product(adv_iters=[])


def test_members_carry_the_fields(native):
    model = importlib.import_module(PKG + ".model")
    grid = model.MFGrid(10, 10, _args(), model.MFGrid.product(eps=[0.5, 1.0], adv_iters=[1, 3], adv_step=0.2),
                        _init=False)
    assert [(h.adv_iters, h.adv_step, h.eps) for h in grid.hparams()] == \
        [(1, 0.2, 0.5), (1, 0.2, 1.0), (3, 0.2, 0.5), (3, 0.2, 1.0)]
    assert [(a.adv_iters, a.adv_step) for a in grid.member_args] == [(1, 0.2)] * 2 + [(3, 0.2)] * 2
    plain = model.MFGrid(10, 10, _args(), [dict(eps=0.5)], _init=False)
    assert [(h.adv_iters, h.adv_step) for h in plain.hparams()] == [(1, None)]
    assert model.MFGrid(10, 10, _args(adv_iters=4), [dict()], _init=False).hparams()[0].adv_iters == 4
    assert model.argparse_like(model.MF(10, 10, _args(adv_iters=3, adv_step=0.1))).adv_iters == 3


def test_run_names_and_grid_files(native, cli, tmp_path):
    model = importlib.import_module(PKG + ".model")
    train = importlib.import_module(PKG + ".train")
    base = ["--dataset", "Video", "--model", "apr", "--embed_size", "64", "--grid_eps", "0.1,0.5"]
    best = [dict(epoch=3, hr10=0.25, ndcg10=0.125), {}, dict(epoch=1, hr10=0.5, ndcg10=0.25), {}]
    # without the axis: the single-run names and the ten-column file, byte for byte
    args = cli.parse_args(base)
    args.adver = 1
    grid = model.MFGrid(10, 10, args, cli.grid_of(args), _init=False)
    single = ["%s_%s_d%d_e%f_l%f_%s" % ("Video", "apr", 64, e, 1.0, "TS") for e in (0.1, 0.5)]
    assert train.grid_run_names(grid, args, "TS") == single
    train.write_grid_table(str(tmp_path), "a.grid", grid, best[:2])
    assert open(tmp_path / "a.grid").read() == \
        "0\t0.1\t1.0\t0.05\t0.0\t1\t0\t3\t0.25\t0.125\n1\t0.5\t1.0\t0.05\t0.0\t1\t0\t-1\tnan\tnan\n"
    rows = train.read_grid_table(tmp_path / "a.grid")
    assert len(rows) == 2 and len(rows[0]) == 10 and rows[0][:8] == (0, 0.1, 1.0, 0.05, 0.0, 1, 0, 3)
    # with it: K = 1 members keep their names, K = 3 members get _k3; two trailing columns on every line
    args = cli.parse_args(base + ["--grid_adv_iters", "1,3"])
    args.adver = 1
    grid = model.MFGrid(10, 10, args, cli.grid_of(args), _init=False)
    assert train.grid_run_names(grid, args, "TS") == single + [n + "_k3" for n in single]
    train.write_grid_table(str(tmp_path), "b.grid", grid, best)
    lines = open(tmp_path / "b.grid").read().splitlines()
    assert lines[0] == "0\t0.1\t1.0\t0.05\t0.0\t1\t0\t3\t0.25\t0.125\t1\t0.25"
    rows = train.read_grid_table(tmp_path / "b.grid")
    assert [r[10:] for r in rows] == [(1, 2.5 * 0.1), (1, 2.5 * 0.5), (3, 2.5 * 0.1 / 3), (3, 2.5 * 0.5 / 3)]
    assert [r[:7] for r in rows[2:]] == [(2, 0.1, 1.0, 0.05, 0.0, 1, 0), (3, 0.5, 1.0, 0.05, 0.0, 1, 0)]
    with open(tmp_path / "c.grid", "w") as f:
        f.write("0\t0.1\t1.0\n")
    with pytest.raises(ValueError, match="expected 10 or 12"):
        train.read_grid_table(tmp_path / "c.grid")


# ---- the CLI -------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_cli_flags(cli, flavor):
    a = cli.parse_args(["--model", "apr"], flavor)
    assert (a.grid_adv_iters, a.adv_iters, a.adv_step) == ([], 1, None)
    assert cli.grid_of(a) is None and cli.single_adv_iters(a) == 0  # the defaults change nothing
    a = cli.parse_args(["--model", "apr", "--grid_adv_iters", "1,3,5"], flavor)
    assert a.grid_adv_iters == [1, 3, 5] and cli.grid_of(a) == [dict(adv_iters=k) for k in (1, 3, 5)]
    a = cli.parse_args(["--model", "apr", "--grid_adv_iters", "1,3", "--grid_eps", "0.5,1", "--adv_step", "0.1"],
                       flavor)
    assert cli.grid_of(a) == [dict(adv_iters=k, eps=e, adv_step=0.1) for k in (1, 3) for e in (0.5, 1.0)]
    a = cli.parse_args(["--model", "apr", "--adv_iters", "4", "--adv_step", "0.2"], flavor)
    assert (a.adv_iters, a.adv_step) == (4, 0.2) and cli.grid_of(a) is None and cli.single_adv_iters(a) == 4
    a = cli.parse_args(["--model", "apr", "--adv_iters", "4", "--grid_eps", "0.5"], flavor)
    assert cli.single_adv_iters(a) == 0 and a.adv_iters == 4  # the grid's members inherit K from args
    for bad in (["--model", "bpr", "--adv_iters", "3"], ["--model", "bpr", "--grid_adv_iters", "1,3"],
                ["--model", "apr", "--adv_iters", "0"], ["--model", "apr", "--adv_iters", "33"],
                ["--model", "apr", "--adv_iters", "x"], ["--model", "apr", "--grid_adv_iters", "1,40"],
                ["--model", "apr", "--adv_step", "0.1"], ["--model", "apr", "--adv_iters", "3", "--adv_step", "-1"],
                ["--model", "apr", "--adv_iters", "3", "--adv", "random"],
                ["--model", "apr", "--grid_adv_iters", "1,3", "--topk", "5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad, flavor)
