"""Robustness evaluation without a GPU: the C-ABI declarations, the host-only
workspace query, argument validation of ops.adv_direction / ops.adv_apply, the
CLI's --robust_eps flag with its writer / reader, the exports, and the build
hash covering csrc/acf_adv.h."""
import ctypes
import importlib
import os
import re
import shutil

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


def test_header_declares_the_entry_points(native):
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    fns = set(re.findall(r"^\s*int\s+(acf_\w+)\s*\(", text, re.M))
    want = {"acf_adv_direction_workspace", "acf_adv_direction", "acf_adv_apply"}
    assert want <= fns
    assert want <= set(native.SIGNATURES) and want <= native.exported_symbols()


def _workspace(native, n, U1, I1, d):
    size = ctypes.c_size_t(0)
    native.call("acf_adv_direction_workspace", n, U1, I1, d, ctypes.byref(size))
    return size.value


def test_workspace_query_is_monotone(native, ops):
    sizes = [_workspace(native, n, 6041, 3707, 64) for n in (0, 1, 63, 1000, 4096, 993_792, 10_000_000)]
    assert sizes[0] >= 0
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # eight 4-byte words per term (keys and values, twice) and the coefficient at least
    assert sizes[5] >= 993_792 * (4 * 16 + 4)
    assert sizes[5] < 256 << 20  # ml-1m's whole stream: well under 256 MiB
    rows = [_workspace(native, 1000, U1, I1, 64) for U1, I1 in ((10, 10), (1000, 10), (1000, 5000), (10**6, 10**6))]
    assert rows == sorted(rows) and rows[-1] > rows[0]
    dims = [_workspace(native, 100_000, 100, 100, d) for d in (8, 64, 512)]
    assert dims == sorted(dims)
    assert ops.adv_direction_workspace(1000, 33, 29, 64) == _workspace(native, 1000, 33, 29, 64)


def test_workspace_query_rejects_bad_arguments(native, ops):
    for args in ((-1, 10, 10, 64), (1 << 29, 10, 10, 64), (10, 0, 10, 64), (10, 10, 10, 6), (10, 1 << 31, 10, 64)):
        with pytest.raises(native.NativeError):
            _workspace(native, *args)
    with pytest.raises(native.NativeError):
        native.call("acf_adv_direction_workspace", 10, 10, 10, 64, None)
    with pytest.raises(ValueError, match="n must lie"):
        ops.adv_direction_workspace(-1, 10, 10, 64)


def test_adv_direction_validates_before_any_launch(ops):
    P, Q = torch.zeros(4, 8), torch.zeros(6, 8)
    u = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(ValueError, match="adv must be"):
        ops.adv_direction(P, Q, u, u, u, adv="fgsm")
    with pytest.raises(ValueError, match="equal lengths"):
        ops.adv_direction(P, Q, u, u[:4], u)
    with pytest.raises(ValueError, match="equal lengths"):
        ops.adv_direction(P, Q, u, u, [0, 1])
    with pytest.raises(ValueError, match="HIP device"):  # CPU tensors: there is no CPU path
        ops.adv_direction(P, Q, u, u, u)
    with pytest.raises(TypeError):
        ops.adv_direction(P.double(), Q, u, u, u)
    with pytest.raises(TypeError):
        ops.adv_direction([[0.0] * 8], Q, u, u, u)


def test_adv_apply_validates_before_any_launch(ops):
    W, N = torch.zeros(4, 8), torch.zeros(4, 8)
    with pytest.raises(ValueError, match="HIP device"):
        ops.adv_apply(W, N, 0.5)
    with pytest.raises(TypeError):
        ops.adv_apply(W.double(), N, 0.5)
    with pytest.raises(TypeError):
        ops.adv_apply(None, N, 0.5)


@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_parse_args_robust_eps(flavor):
    cli = importlib.import_module(PKG + ".cli")
    assert cli.parse_args([], flavor).robust_eps == []  # off
    assert cli.parse_args(["--robust_eps", "0.5,1,2"], flavor).robust_eps == [0.5, 1.0, 2.0]
    assert cli.parse_args(["--robust_eps", " 0 , 0.25 "], flavor).robust_eps == [0.0, 0.25]
    assert cli.parse_args(["--robust_eps", ""], flavor).robust_eps == []
    for bad in ("0.5,-1", "x", "1,nan", "inf"):
        with pytest.raises(SystemExit):
            cli.parse_args(["--robust_eps", bad], flavor)


def test_robust_file_round_trip(tmp_path):
    cli = importlib.import_module(PKG + ".cli")
    rows = [("grad", 0.0, 0.7123456789012345, 0.41, 0.93), ("grad", 0.5, 0.1, 1 / 3, 0.5),
            ("random", 2.0, 0.0, 0.0, 1.0)]
    cli.write_robust(str(tmp_path / "out" / "t"), "run.robust", rows)
    lines = open(tmp_path / "out" / "t" / "run.robust").read().splitlines()
    assert len(lines) == 3 and lines[0].split("\t")[:2] == ["grad", "0.0"]
    assert all(len(x.split("\t")) == 5 for x in lines)
    assert cli.read_robust(tmp_path / "out" / "t" / "run.robust") == rows


def test_surface_exports(acf):
    ev = importlib.import_module(PKG + ".evaluate")
    tr = importlib.import_module(PKG + ".train")
    assert callable(ev.robustness) and callable(tr.adv_update)
    assert callable(acf.robustness) and callable(acf.adv_update)
    for cls in (acf.MF, acf.APR):
        assert callable(getattr(cls, "robustness")) and callable(getattr(cls, "adv_update"))
    with pytest.raises(ValueError, match="mode must be"):
        ev.robustness(None, None, None, ([], [], []), [0.5], modes=("pgd",))
    with pytest.raises(ValueError, match="eps must be"):
        ev.robustness(None, None, None, ([], [], []), [-0.5])


def test_triplet_arrays_accepts_what_training_batch_returns(acf):
    import numpy as np
    ev = importlib.import_module(PKG + ".evaluate")
    ep = acf.EpochTriplets(torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32),
                           torch.full((4,), 2, dtype=torch.int32), 2)
    u, i, j = ev.triplet_arrays(ep)
    assert u is ep.user and i is ep.item_pos and j is ep.item_neg
    lists = ([np.array([[1], [2]]), np.array([[3], [4]])], [np.array([[5], [6]]), np.array([[7], [8]])],
             [np.array([[9], [1]]), np.array([[2], [3]])])
    u, i, j = ev.triplet_arrays(lists)
    assert u.dtype == np.int32 and u.tolist() == [1, 2, 3, 4] and i.tolist() == [5, 6, 7, 8]
    assert j.tolist() == [9, 1, 2, 3]
    assert ev.triplet_arrays((lists[0], lists[1], None, lists[2]))[2].tolist() == [9, 1, 2, 3]
    with pytest.raises(ValueError):
        ev.triplet_arrays((lists[0], lists[1]))


def test_build_hash_covers_the_new_header(tmp_path):
    bn = importlib.import_module(PKG + ".build_native")
    rel = f"{PKG}/csrc/acf_adv.h"
    assert rel in bn.LIBS["apr"]["headers"]
    spec = bn.LIBS["apr"]
    for r in [*spec["srcs"], *spec["headers"]]:
        dst = tmp_path / r
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copyfile(os.path.join(bn.REPO, r), dst)
    h0 = bn.source_hash("apr", str(tmp_path))
    assert h0 == bn.source_hash("apr")
    hdr = tmp_path / rel
    hdr.write_text(hdr.read_text() + "\n// edited\n")
    assert bn.source_hash("apr", str(tmp_path)) != h0
