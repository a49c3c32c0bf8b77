"""Top-K recommendation lists without a GPU: the C-ABI declarations, the
host-only workspace query, argument validation of ops.recommend_topk, the
exclusion-CSR helper, and the CLI's --topk flag with its writer / reader."""
import ctypes
import importlib
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import PKG, REPO

MiB = 1 << 20


@pytest.fixture(scope="module")
def native():
    mod = importlib.import_module(PKG + "._native")
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


def test_header_declares_both_functions():
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    fns = set(re.findall(r"^\s*int\s+(acf_\w+)\s*\(", text, re.M))
    assert {"acf_recommend_topk", "acf_recommend_topk_workspace"} <= fns


def _workspace(native, n, num_cand, k, kernel):
    size = ctypes.c_size_t(0)
    native.call("acf_recommend_topk_workspace", n, num_cand, k, kernel, ctypes.byref(size))
    return size.value


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_workspace_is_far_below_a_score_matrix(native, kernel):
    """The two conditions of the feature: ml-1m (a 89 MB score matrix) and 64
    users x 5M items (1.28 GB) both need less than 64 MiB."""
    a = _workspace(native, 6040, 3706, 100, kernel)
    b = _workspace(native, 64, 5_000_000, 100, kernel)
    assert 0 < a < 64 * MiB
    assert 0 < b < 64 * MiB
    # the partial lists hold at least one list of k entries per user
    assert a >= 6040 * 100 * 8 and b >= 64 * 100 * 8


def test_workspace_grid_matches_the_recorded_bytes(native):
    """The strip cut is ABI: every byte count equals the one recorded before the
    sweeps shared one strip function (tests/golden/make_sweep_strips.py)."""
    with open(os.path.join(REPO, "tests", "golden", "sweep_strips.json")) as f:
        want = json.load(f)["topk"]
    assert len(want) == 8 * 7 * 3 * 3
    got = {key: _workspace(native, *map(int, key.split(","))) for key in want}
    assert got == want


def test_workspace_rejects_bad_arguments(native):
    for k in (0, 129, -1):
        with pytest.raises(native.NativeError, match="k must be"):
            _workspace(native, 10, 10, k, 0)
    with pytest.raises(native.NativeError, match="kernel"):
        _workspace(native, 10, 10, 10, 3)
    with pytest.raises(native.NativeError):
        native.call("acf_recommend_topk_workspace", 10, 10, 10, 0, None)
    assert _workspace(native, 10, 0, 128, 0) > 0  # no candidates: still room for the padding
    ops = importlib.import_module(PKG + ".ops")
    assert ops.recommend_topk_workspace(6040, 3706, 100, "mfma") == _workspace(native, 6040, 3706, 100, 1)


def test_recommend_topk_validates_before_any_launch(native):
    ops = importlib.import_module(PKG + ".ops")
    P, Q = torch.zeros(4, 8), torch.zeros(6, 8)
    u = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HIP device"):
        ops.recommend_topk(P, Q, u, 3)
    for k in (0, 129, -2, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            ops.recommend_topk(P, Q, u, k)
    with pytest.raises(ValueError, match="kernel must be"):
        ops.recommend_topk(P, Q, u, 3, kernel="gemm")
    with pytest.raises(TypeError):
        ops.recommend_topk(P.double(), Q, u, 3)


def _toy_dataset():
    """4 users; user 2 has no train item; lists unsorted with a repeat."""
    lists = [[5, 1, 3, 1], [0], [], [7, 2]]
    off = np.zeros(5, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    data = importlib.import_module(PKG + ".data")
    ds = data._DatasetBase()
    ds.num_users, ds.num_items = 4, 8
    ds.list_off, ds.list_items = off, np.concatenate([np.asarray(x, np.int32) for x in lists])
    return ds


def test_train_exclusions_csr():
    ev = importlib.import_module(PKG + ".evaluate")
    ds = _toy_dataset()
    off, items = ev.train_exclusions(ds, [3, 2, 0, 0, 1])
    assert off.dtype == np.int64 and items.dtype == np.int32
    np.testing.assert_array_equal(off, [0, 2, 2, 5, 8, 9])
    np.testing.assert_array_equal(items, [2, 7, 1, 3, 5, 1, 3, 5, 0])
    # a user past the train lists has nothing to exclude; no users: an empty CSR
    off, items = ev.train_exclusions(ds, [9, 1])
    np.testing.assert_array_equal(off, [0, 0, 1])
    np.testing.assert_array_equal(items, [0])
    off, items = ev.train_exclusions(ds, [])
    np.testing.assert_array_equal(off, [0])
    assert items.size == 0


def test_topk_file_round_trip(tmp_path):
    cli = importlib.import_module(PKG + ".cli")
    items = np.array([[4, 2, 9], [7, -1, -1], [-1, -1, -1], [0, 1, 2]], np.int32)
    cli.write_topk(str(tmp_path / "out" / "t"), "run.topk", items)
    text = open(tmp_path / "out" / "t" / "run.topk").read()
    assert text == "0\t4,2,9\n1\t7\n2\t\n3\t0,1,2\n"
    np.testing.assert_array_equal(cli.read_topk(tmp_path / "out" / "t" / "run.topk"), items)
    got = cli.read_topk(tmp_path / "out" / "t" / "run.topk", k=2)
    np.testing.assert_array_equal(got, items[:, :2])


@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_parse_args_accepts_topk(flavor):
    cli = importlib.import_module(PKG + ".cli")
    assert cli.parse_args([], flavor).topk == 0
    assert cli.parse_args(["--topk", "25"], flavor).topk == 25


def test_model_layer_exposes_recommend(acf):
    assert callable(getattr(acf.MF, "recommend")) and callable(getattr(acf.APR, "recommend"))
    m = SimpleNamespace(embedding_P=torch.zeros(4, 8), embedding_Q=torch.zeros(9, 8))
    ev = importlib.import_module(PKG + ".evaluate")
    with pytest.raises(ValueError, match="HIP device"):  # reaches the op with the helper's CSR; no CPU path
        ev.recommend(m, _toy_dataset(), k=3)
