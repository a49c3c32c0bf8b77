"""Grid training without a GPU: the workspace query and the refusals of
acf_apr_grid_workspace / acf_apr_grid_train that come before any launch, the C-ABI
declarations, MFGrid.product's order, the members' run names, the --grid_* flags and
the argument validation of ops.grid_train."""
import ctypes
import importlib
import os
import re

import pytest
import torch

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


def _query(native, M=4, B=512, nb=8, U1=100, I1=80, d=64, out=True):
    size = ctypes.c_size_t()
    rc = native.load().acf_apr_grid_workspace(M, B, nb, U1, I1, d, ctypes.byref(size) if out else None)
    return rc, size.value


def test_header_and_binding_declare_the_entry_points(native):
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    fns = set(re.findall(r"^\s*int\s+(acf_\w+)\s*\(", text, re.M))
    want = {"acf_apr_grid_workspace", "acf_apr_grid_train"}
    assert want <= fns and want <= set(native.SIGNATURES) and want <= native.exported_symbols()
    assert re.search(r"#define\s+ACF_GRID_MAX_MODELS\s+64\b", text)


def test_workspace_grows_with_members_batch_and_batches(native, ops):
    rc, base = _query(native)
    assert rc == native.ACF_OK
    # the two scratch tables alone: 2 x M x 3B x d floats
    assert base >= 2 * 4 * 3 * 512 * 64 * 4
    assert _query(native, M=8)[1] > base
    assert _query(native, B=1024)[1] > base
    assert _query(native, nb=16)[1] > base
    assert _query(native, nb=0)[0] == native.ACF_OK
    assert ops.grid_workspace(4, 512, 8, 100, 80, 64) == base


def test_workspace_query_rejects_bad_shapes_without_a_device(native):
    for kw in (dict(M=0), dict(M=65), dict(d=2), dict(d=6), dict(d=260), dict(B=0), dict(B=1025), dict(nb=-1),
               dict(out=False)):
        assert _query(native, **kw)[0] == native.ACF_E_INVALID, kw
    for d in (4, 8, 20, 256):
        assert _query(native, d=d)[0] == native.ACF_OK


def test_native_train_rejects_bad_arguments_before_any_launch(native):
    """Every refusal below comes before the first HIP call: the pointers are never used."""
    one = ctypes.c_void_p(256)  # aligned, never dereferenced
    lib = native.load()

    def train(M=2, d=64, B=32, nb=3, hp=None, P=one, user=one, ws=one, ws_bytes=1 << 40, **field):
        hps = (native.HParams * 64)()
        for h in hps:
            h.lr, h.eps, h.reg_adv, h.clip_lo, h.clip_hi, h.adver = 0.05, 0.5, 1.0, -80.0, 1e8, 1
        for k, v in field.items():
            setattr(hps[1], k, v)
        return lib.acf_apr_grid_train(P, one, one, one, M, 65, 49, d, hps if hp is None else hp, user, one, one, B,
                                      nb, None, None, ws, ws_bytes, 0, None)
    for kw in (dict(M=0), dict(M=65), dict(d=2), dict(d=6), dict(d=260), dict(B=0), dict(B=1025), dict(nb=-1),
               dict(P=None), dict(user=None), dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(ws_bytes=16),
               dict(adv_mode=1), dict(zero_delta=1)):
        assert train(**kw) == native.ACF_E_INVALID, kw
    assert lib.acf_apr_grid_train(one, one, one, one, 2, 65, 49, 64, None, one, one, one, 32, 3, None, None, one,
                                  1 << 40, 0, None) == native.ACF_E_INVALID
    assert train(nb=0) == native.ACF_OK  # nothing to do: no launch


def test_product_order_is_eps_then_reg_adv_then_lr_then_seed(native):
    MFGrid = importlib.import_module(PKG + ".model").MFGrid
    g = MFGrid.product(eps=[0.1, 0.5], reg_adv=[0.5, 1.0, 2.0])
    assert g == [dict(eps=e, reg_adv=r) for e in (0.1, 0.5) for r in (0.5, 1.0, 2.0)]
    g = MFGrid.product(eps=[0.5], lr=[0.01, 0.05], seeds=2)
    assert g == [dict(eps=0.5, lr=lr, seed=s) for lr in (0.01, 0.05) for s in (0, 1)]
    assert MFGrid.product(seeds=[7, 9]) == [dict(seed=7), dict(seed=9)]
    with pytest.raises(ValueError, match="empty"):
        MFGrid.product(eps=[])


def test_member_run_names_equal_the_single_model_names(native, cli):
    model = importlib.import_module(PKG + ".model")
    train = importlib.import_module(PKG + ".train")
    args = cli.parse_args(["--dataset", "Video", "--model", "apr", "--embed_size", "64", "--grid_eps", "0.1,0.5",
                           "--grid_reg_adv", "1,2"])
    args.adver = 1
    grid = model.MFGrid(10, 10, args, cli.grid_of(args), _init=False)
    names = train.grid_run_names(grid, args, "TS")
    single = ["%s_%s_d%d_e%f_l%f_%s" % ("Video", "apr", 64, e, l, "TS") for e in (0.1, 0.5) for l in (1.0, 2.0)]
    assert names == single  # cli.main's format for one apr run at that (eps, reg_adv)
    assert [(h.eps, h.reg_adv, h.adver) for h in grid.hparams()] == [(e, l, 1) for e in (0.1, 0.5) for l in (1.0, 2.0)]
    # lr or seeds in the grid: a suffix keeps the names apart
    args = cli.parse_args(["--dataset", "Video", "--model", "apr", "--grid_eps", "0.5", "--grid_lr", "0.01,0.05",
                           "--grid_seeds", "2"])
    grid = model.MFGrid(10, 10, args, cli.grid_of(args), _init=False)
    names = train.grid_run_names(grid, args, "TS")
    assert len(set(names)) == 4 and all(n.startswith(single[2][:-3]) for n in names)
    with pytest.raises(ValueError, match="unknown grid keys"):
        model.MFGrid(10, 10, args, [dict(embed_size=8)], _init=False)


@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_grid_flags(cli, flavor):
    a = cli.parse_args([], flavor)
    assert a.grid_eps == [] and a.grid_reg_adv == [] and a.grid_lr == [] and a.grid_seeds == 0
    assert cli.grid_of(a) is None  # without a --grid_* flag nothing changes
    a = cli.parse_args(["--grid_eps", "0.1,0.5,1", "--grid_reg_adv", "0.5,1"], flavor)
    assert a.grid_eps == [0.1, 0.5, 1.0] and a.grid_reg_adv == [0.5, 1.0] and len(cli.grid_of(a)) == 6
    a = cli.parse_args(["--grid_lr", "0.01,0.05", "--grid_seeds", "3"], flavor)
    assert cli.grid_of(a) == [dict(lr=lr, seed=s) for lr in (0.01, 0.05) for s in range(3)]
    for bad in (["--grid_eps", "x"], ["--grid_eps", "-1"], ["--grid_lr", "0"], ["--grid_seeds", "65"],
                ["--grid_seeds", "-1"], ["--grid_eps", "0.5", "--topk", "5"],
                ["--grid_eps", ",".join(["0.5"] * 9), "--grid_reg_adv", ",".join(["1"] * 9)]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad, flavor)


def test_grid_train_validates_before_any_native_call(ops, monkeypatch):
    for mod in (ops._native, ops):
        monkeypatch.setattr(mod, "call", lambda *a, **k: pytest.fail("a native call was made"))
    hp = ops.StepHParams(adver=1)

    def tabs(M=2, u1=65, i1=49, d=8):
        return [torch.zeros(M, u1, d), torch.zeros(M, i1, d), torch.zeros(M, u1, d), torch.zeros(M, i1, d)]
    u = torch.zeros(64, dtype=torch.int32)
    with pytest.raises(ValueError, match="1 to 64 members"):
        ops.grid_train(*tabs(), [], u, u, u, 32)
    with pytest.raises(ValueError, match="1 to 64 members"):
        ops.grid_train(*tabs(65), [hp] * 65, u, u, u, 32)
    with pytest.raises(TypeError, match="StepHParams"):
        ops.grid_train(*tabs(), [hp, dict(eps=1.0)], u, u, u, 32)
    with pytest.raises(ValueError, match="not grid modes"):
        ops.grid_train(*tabs(), [hp, ops.StepHParams(adver=1, adv="random")], u, u, u, 32)
    with pytest.raises(ValueError, match="not grid modes"):
        ops.grid_train(*tabs(), [hp, ops.StepHParams(adver=1, zero_delta=1)], u, u, u, 32)
    with pytest.raises(ValueError, match=r"\[M = 2, rows, d\]"):  # three members' tables, two hparams
        ops.grid_train(*tabs(3), [hp, hp], u, u, u, 32)
    with pytest.raises(ValueError, match=r"\[M = 2, rows, d\]"):
        ops.grid_train(torch.zeros(65, 8), *tabs()[1:], [hp, hp], u, u, u, 32)
    t = tabs()
    t[2] = torch.zeros(2, 64, 8)
    with pytest.raises(ValueError, match="accumulator shapes"):
        ops.grid_train(*t, [hp, hp], u, u, u, 32)
    t = tabs()
    t[1], t[3] = torch.zeros(2, 49, 16), torch.zeros(2, 49, 16)
    with pytest.raises(ValueError, match="dims differ"):
        ops.grid_train(*t, [hp, hp], u, u, u, 32)
    for d in (6, 260):
        with pytest.raises(ValueError, match="multiple of 4"):
            ops.grid_train(*tabs(d=d), [hp, hp], u, u, u, 32)
    with pytest.raises(TypeError, match="float32"):
        ops.grid_train(tabs()[0].double(), *tabs()[1:], [hp, hp], u, u, u, 32)
    for B in (0, 1025):
        with pytest.raises(ValueError, match="batch_size must lie"):
            ops.grid_train(*tabs(), [hp, hp], u, u, u, B)
    with pytest.raises(ValueError, match="equal lengths"):
        ops.grid_train(*tabs(), [hp, hp], u, u[:32], u, 32)
    with pytest.raises(ValueError, match="not a multiple"):
        ops.grid_train(*tabs(), [hp, hp], u[:40], u[:40], u[:40], 32)
    with pytest.raises(ValueError, match="HIP device"):  # CPU tensors: there is no CPU path
        ops.grid_train(*tabs(), [hp, hp], u, u, u, 32)
