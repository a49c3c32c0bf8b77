"""All-items ranking for NeuMF without a GPU: the C-ABI declarations and bindings,
the host-only workspace query, argument validation of NeuMFContext.rank_all
before any launch, run.py's --topk flag, the lazy --eval all negatives and
evaluate_model_all against evaluate_model."""
import ctypes
import importlib
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import PKG, REPO

YELP = (25_677, 25_816)  # users, item rows of the benchmarked yelp shape


@pytest.fixture(scope="module")
def native():
    mod = importlib.import_module(PKG + "._native")
    if not os.path.exists(mod.NEUMF_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return mod


def test_header_declares_both_functions():
    text = open(os.path.join(REPO, "include", "acf_neumf.h")).read()
    fns = set(re.findall(r"^\s*int\s+(acf_\w+)\s*\(", text, re.M))
    assert {"acf_neumf_rank_all", "acf_neumf_rank_all_workspace"} <= fns


def test_native_binds_both_functions(native):
    assert {"acf_neumf_rank_all", "acf_neumf_rank_all_workspace"} <= set(native.NEUMF_SIGNATURES)
    assert {"acf_neumf_rank_all", "acf_neumf_rank_all_workspace"} <= native.neumf_exported_symbols()
    bn = importlib.import_module(PKG + ".build_native")
    for lib in ("apr", "neumf"):  # the shared selection header is part of both hashes
        assert any(h.endswith("acf_topk_select.h") for h in bn.LIBS[lib]["headers"])


def _workspace(native, n, nc, k):
    size = ctypes.c_size_t(0)
    native.call_neumf("acf_neumf_rank_all_workspace", n, nc, k, ctypes.byref(size))
    return size.value


def test_workspace_query_is_host_only_and_small(native):
    """No device is touched (this test runs without one); at the yelp shape with
    K = 100 the workspace is below one eighth of the score array, and it holds at
    least one list of k keys per user."""
    n, nc = YELP
    got = _workspace(native, n, nc, 100)
    assert n * 100 * 8 <= got < n * nc * 4 // 8
    assert _workspace(native, 0, 10, 0) > 0 and _workspace(native, 5, 1, 128) > 0
    # few users: more strips (to fill the device), still far below the score array
    assert _workspace(native, 1, nc, 128) < nc * 4
    nm = importlib.import_module(PKG + ".neumf")
    assert nm.rank_all_workspace(n, nc, 100) == got


def test_workspace_rejects_bad_arguments(native):
    for args in ((10, 10, 129), (10, 10, -1), (-1, 10, 10), (10, 0, 10), (10, -3, 10)):
        with pytest.raises(native.NativeError) as e:
            _workspace(native, *args)
        assert e.value.code == 1  # ACF_E_INVALID
    with pytest.raises(native.NativeError):
        native.call_neumf("acf_neumf_rank_all_workspace", 10, 10, 10, None)


@pytest.fixture()
def stub_ctx(native, monkeypatch):
    """A NeuMFContext over a CPU state whose native layer refuses every call: what
    rank_all rejects, it rejects before any launch."""
    nm = importlib.import_module(PKG + ".neumf")
    calls = []

    def refuse(name, *a):
        calls.append(name)
        raise AssertionError("native call " + name)
    monkeypatch.setattr(native, "call_neumf", refuse)
    ctx = object.__new__(nm.NeuMFContext)
    ctx.state = SimpleNamespace(U1=6, I1=9, d=8, device=torch.device("cpu"), params=torch.zeros(4))
    ctx.max_batch, ctx._ptr = 16, None
    return ctx, calls


def test_rank_all_validates_before_any_launch(stub_ctx):
    ctx, calls = stub_ctx
    u = np.arange(4)
    for k in (-1, 129, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            ctx.rank_all(u, k)
    with pytest.raises(ValueError, match="nothing to compute"):
        ctx.rank_all(u, 0)
    with pytest.raises(TypeError, match="users"):
        ctx.rank_all(np.zeros(4, np.float32), 3)
    with pytest.raises(TypeError, match="test_items"):
        ctx.rank_all(u, 0, test_items=torch.zeros(4))
    with pytest.raises(TypeError, match="excl_items"):
        ctx.rank_all(u, 3, excl_off=np.zeros(5, np.int64), excl_items=np.zeros(2, np.float64))
    with pytest.raises(ValueError, match="users"):
        ctx.rank_all(np.zeros((2, 2), np.int32), 3)
    with pytest.raises(ValueError, match="test_items must have"):
        ctx.rank_all(u, 0, test_items=np.arange(3))
    for nc in (0, 10):
        with pytest.raises(ValueError, match="num_candidates"):
            ctx.rank_all(u, 3, num_candidates=nc)
    with pytest.raises(ValueError, match="go together"):
        ctx.rank_all(u, 3, excl_off=np.zeros(5, np.int64))
    with pytest.raises(ValueError, match=r"len\(users\) \+ 1"):
        ctx.rank_all(u, 3, excl_off=np.zeros(4, np.int64), excl_items=np.zeros(1, np.int32))
    with pytest.raises(ValueError, match="non-decreasing"):  # a list running past excl_items
        ctx.rank_all(u, 3, excl_off=np.array([0, 1, 2, 3, 4]), excl_items=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="non-decreasing"):
        ctx.rank_all(u, 3, excl_off=np.array([0, 2, 1, 3, 3]), excl_items=np.zeros(3, np.int32))
    assert calls == []


def test_model_layer_exposes_recommend_and_positions(acf):
    nm = importlib.import_module(PKG + ".neumf")
    for cls in (nm.NeuMF, nm.AdversarialNeuMF):
        assert callable(getattr(cls, "recommend")) and callable(getattr(cls, "positions_all"))


def test_exclusion_csr_reuses_train_exclusions():
    """Item 0, the train items (unique, ascending) and the test item per user, in
    the order of `users` (repeats allowed), from a dok-like train matrix."""
    nm = importlib.import_module(PKG + ".neumf")
    train = {(1, 4): 1.0, (1, 2): 1.0, (3, 7): 1.0, (1, 4.0): 1.0, (2, 5): 1.0}
    m = object.__new__(nm.NeuMF)
    m.uNum, m.iNum = 5, 9
    off, items = m._exclusions([3, 1, 4, 1], train, [6, 8, 1, 3])
    np.testing.assert_array_equal(off, [0, 3, 7, 9, 13])
    np.testing.assert_array_equal(items, [7, 0, 6, 2, 4, 0, 8, 0, 1, 2, 4, 0, 3])
    off, items = m._exclusions([2, 2], train)
    np.testing.assert_array_equal(off, [0, 2, 4])
    np.testing.assert_array_equal(items, [5, 0, 5, 0])
    assert off.dtype == np.int64 and items.dtype == np.int32


def _run_cli():
    return importlib.import_module(PKG + ".run_cli")


def test_parse_args_accepts_topk_and_refuses_129(capsys):
    rc = _run_cli()
    assert rc.parse_args([]).topk == 0
    assert rc.parse_args(["--topk", "128"]).topk == 128
    for bad in ("129", "-1"):
        with pytest.raises(SystemExit):
            rc.parse_args(["--topk", bad])
    assert "--topk must lie in" in capsys.readouterr().err


def test_topk_is_refused_for_other_models():
    with pytest.raises(SystemExit, match="--topk"):
        _run_cli().main(["--model", "bpr", "--data", "synthetic:30:50:600", "--topk", "5"])


def _eager_negatives(ds):
    """The construction RunDataset used before the lists became lazy."""
    every = np.arange(1, ds.num_items)
    out = [[]] * ds.num_users
    for x in range(1, ds.num_users):
        keep = np.ones(ds.num_items, bool)
        keep[0] = False
        keep[np.asarray(ds.trainSeq.get(x, []), np.int64)] = False
        keep[ds.testRatings[x]] = False
        out[x] = every[keep[1:]].tolist()
    return out


@pytest.fixture(scope="module")
def toy():
    return _run_cli().get_dataset("synthetic:30:50:600", "", "all")


def test_lazy_negatives_equal_the_eager_lists(toy):
    want = _eager_negatives(toy)
    negs = toy.testNegatives
    assert len(negs) == toy.num_users == len(want) == 31
    assert not isinstance(negs, list)  # nothing per user is held
    for x in range(toy.num_users):
        assert negs[x] == want[x] and isinstance(negs[x], list)
    assert negs[-1] == want[-1]
    with pytest.raises(IndexError):
        negs[toy.num_users]


class FakeRanker:
    """Scores from a fixed table quantised to a few levels, so that ties with the
    test item's score are common; rank() and positions_all() in numpy."""

    def __init__(self, ds, seed=3):
        rng = np.random.default_rng(seed)
        self.S = rng.integers(0, 6, size=(ds.num_users, ds.num_items)).astype(np.float32) / 4
        self.ds = ds

    def rank(self, users, items):
        return self.S[np.asarray(users), np.asarray(items)].reshape(-1, 1)

    def positions_all(self, users, test_items, train):
        out = []
        for u, t in zip(np.asarray(users).tolist(), np.asarray(test_items).tolist()):
            keep = np.ones(self.ds.num_items, bool)
            keep[[0, t]] = False
            keep[[i for (a, i) in train.keys() if a == u]] = False
            out.append(int((self.S[u][keep] >= self.S[u, t]).sum()))
        return np.asarray(out, np.int32)


def test_evaluate_model_all_agrees_with_evaluate_model(toy):
    ev = importlib.import_module(PKG + ".evaluation")
    m = FakeRanker(toy)
    tied = sum(1 for u in range(1, toy.num_users)
               if (m.S[u, toy.testNegatives[u]] == m.S[u, toy.testRatings[u]]).any())
    assert tied >= 2  # the >= of the rank is exercised
    for K in (100, 5):
        want = ev.evaluate_model(m, toy.testRatings, toy.testNegatives, K)
        got = ev.evaluate_model_all(m, toy.testRatings, toy.trainMatrix, K)
        assert got[0] == want[0] and got[1] == want[1]
        assert len(got[0]) == toy.num_users - 1
    assert 0 < sum(ev.evaluate_model_all(m, toy.testRatings, toy.trainMatrix, 5)[0]) < toy.num_users - 1
    assert ev.evaluate_model_all(m, [None], toy.trainMatrix, 5) == ([], [])
