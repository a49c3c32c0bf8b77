"""List-level robustness without a GPU: the numpy yardstick by hand and by its
properties, the header, the build and the binding, the host-only workspace query,
the checks that fire before any launch or native call, item_popularity, and the
CLI flag and file."""
import ctypes
import importlib
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lists_ref
from conftest import PKG, REPO

NAMES = ("acf_list_compare", "acf_list_exposure", "acf_exposure_metrics_workspace", "acf_exposure_metrics")


@pytest.fixture(scope="module")
def native():
    return importlib.import_module(PKG + "._native")


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".evaluate")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module(PKG + ".cli")


# ---- the yardstick ------------------------------------------------------------------
def test_yardstick_compare_by_hand():
    rows, scored = lists_ref.compare_row([1, 2, 3], [1, 3, 2], (1, 2, 3), 0.5)
    assert scored
    assert [r[0] for r in rows] == [1.0, 1.0, 3.0]          # X = (1, 1, 3)
    assert [r[1] for r in rows] == [1.0, 1 / 3, 1.0]
    assert rows[2][2] == 0.875                               # 1 * 1/8 + 1 * (1/2 + 1/8 + 1/8)
    # -1 is "none" wherever it stands; the longer list sets the depth
    rows, scored = lists_ref.compare_row([4, -1, -1], [7, 4, 9], (3,), 0.5)
    assert scored and rows[0][0] == 1.0 and rows[0][1] == 1 / 3   # 1 / (1 + 3 - 1)
    rows, scored = lists_ref.compare_row([-1, -1], [-1, -1], (1, 2), 0.9)
    assert not scored and rows == [(0.0, 0.0, 0.0)] * 2


def test_yardstick_exposure_by_hand():
    total, cov, gini, ent, arp, aplt = lists_ref.exposure_metrics_row([0, 0, 4], pop=[5, 1, 3], tail=[1, 1, 0])
    assert (total, cov, gini, ent, arp, aplt) == (4.0, 1 / 3, 2 / 3, 0.0, 3.0, 0.0)
    for N in (1, 2, 7, 64):
        row = lists_ref.exposure_metrics_row([3] * N, tail=[1] * N)
        assert row[0] == 3.0 * N and row[1] == 1.0 and row[2] == 0.0 and row[5] == 1.0
        assert abs(row[3] - math.log2(N)) <= 1e-12
    assert lists_ref.exposure_metrics_row([0, 0, 0]) == (0.0,) * 6
    counts = lists_ref.exposure_counts([[2, 0, 5, -1], [2, 2, 9, 1]], 6, (1, 3, 4))
    assert counts.tolist() == [[0, 0, 2, 0, 0, 0], [1, 0, 3, 0, 0, 1], [1, 1, 3, 0, 0, 1]]


@pytest.mark.parametrize("p", [0.5, 0.9, 0.98])
def test_yardstick_properties(p):
    rng = np.random.default_rng(7)
    k, cuts = 20, (1, 10, 20)
    A = np.stack([rng.permutation(40)[:k] for _ in range(6)])
    same, _, ns = lists_ref.compare(A, A, cuts, p)
    assert (same[:, :, 1] == 1.0).all() and np.abs(same[:, :, 2] - 1.0).max() <= 1e-12
    assert (same[:, :, 0] == np.array(cuts)).all() and ns.tolist() == [6, 6, 6]
    disjoint, mean, _ = lists_ref.compare(A, A + 100, cuts, p)
    assert (disjoint == 0).all() and (mean == 0).all()
    B = np.stack([rng.permutation(40)[:k] for _ in range(6)])
    B[0, 15:] = -1
    ab, ba = lists_ref.compare(A, B, cuts, p), lists_ref.compare(B, A, cuts, p)
    assert all(np.array_equal(x, y) for x, y in zip(ab, ba))
    assert (0 < ab[0][:, 2, 2]).all() and (ab[0][:, 2, 2] < 1).all()


# ---- header, build, binding --------------------------------------------------------------
def test_header_build_and_binding(native):
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in native.SIGNATURES
    assert set(NAMES) <= native.exported_symbols()
    build_native = importlib.import_module(PKG + ".build_native")
    assert any(h.endswith("csrc/acf_lists.h") for h in build_native.LIBS["apr"]["headers"])
    rank = open(os.path.join(REPO, PKG, "csrc", "acf_rank.hip")).read()
    assert rank.index('#include "acf_eval_multi.h"') < rank.index('#include "acf_lists.h"')
    assert native.load().acf_apr_abi_version() == native.ABI_VERSION == 2


# ---- host-only native calls ---------------------------------------------------------------
def _ws(native, num_items, n_cut):
    size = ctypes.c_size_t(0)
    rc = native.load().acf_exposure_metrics_workspace(num_items, n_cut, ctypes.byref(size))
    return rc, size.value


def test_workspace_query_is_host_only(native):
    # (no device in this process: the query must not need one)
    rc, small = _ws(native, 1, 1)
    assert rc == native.ACF_OK and small >= 4 + 5 * 8 + 8
    rc, one = _ws(native, 9916, 1)
    rc3, three = _ws(native, 9916, 3)
    assert rc == rc3 == native.ACF_OK and 9916 * 4 <= one < three and three >= 3 * 9916 * 4
    assert _ws(native, 1 << 24, 8)[0] == native.ACF_OK
    for bad in ((0, 1), (-5, 1), (10, 0), (10, 9)):
        assert _ws(native, *bad)[0] == native.ACF_E_INVALID, bad
    assert native.load().acf_exposure_metrics_workspace(10, 1, None) == native.ACF_E_INVALID
    ops = importlib.import_module(PKG + ".ops")
    assert ops.exposure_metrics_workspace(9916, 3) == three
    for bad in ((0, 1), (10, 0), (10, 9), (10.0, 1)):
        with pytest.raises(ValueError):
            ops.exposure_metrics_workspace(*bad)


def test_bad_arguments_are_invalid_before_any_launch(native):
    lib = native.load()
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)  # a non-NULL pointer that is never dereferenced
    cuts = (ctypes.c_int32 * 9)(*range(1, 10))
    c2 = lambda a, b: (ctypes.c_int32 * 2)(a, b)  # noqa: E731

    def compare(**kw):
        a = {**dict(A=p, B=p, n=4, k=16, cuts=cuts, nc=2, p=0.9, per_user=p, mean=p, n_scored=p), **kw}
        return lib.acf_list_compare(a["A"], a["B"], a["n"], a["k"], a["cuts"], a["nc"], a["p"], a["per_user"],
                                    a["mean"], a["n_scored"], None)

    for bad in (dict(A=None), dict(B=None), dict(per_user=None), dict(mean=None), dict(n_scored=None), dict(cuts=None),
                dict(n=-1), dict(k=0), dict(k=129), dict(cuts=c2(4, 0)), dict(cuts=c2(4, 17)), dict(nc=9), dict(nc=0),
                dict(p=0.0), dict(p=1.0), dict(p=-0.5), dict(p=float("nan"))):
        assert compare(**bad) == native.ACF_E_INVALID, bad
    assert b"" != lib.acf_apr_last_error()

    def exposure(**kw):
        a = {**dict(lists=p, n=4, k=16, N=100, cuts=cuts, nc=2, counts=p), **kw}
        return lib.acf_list_exposure(a["lists"], a["n"], a["k"], a["N"], a["cuts"], a["nc"], a["counts"], None)

    for bad in (dict(lists=None), dict(counts=None), dict(cuts=None), dict(n=-1), dict(k=0), dict(k=129), dict(N=0),
                dict(cuts=c2(4, 0)), dict(cuts=c2(4, 17)), dict(nc=9), dict(n=1 << 25, k=128)):
        assert exposure(**bad) == native.ACF_E_INVALID, bad

    def metrics(**kw):
        a = {**dict(counts=p, N=100, nc=2, pop=None, tail=None, out=p, ws=p, wsb=1 << 20), **kw}
        return lib.acf_exposure_metrics(a["counts"], a["N"], a["nc"], a["pop"], a["tail"], a["out"], a["ws"],
                                        a["wsb"], None)

    for bad in (dict(counts=None), dict(out=None), dict(ws=None), dict(N=0), dict(nc=0), dict(nc=9), dict(wsb=64)):
        assert metrics(**bad) == native.ACF_E_INVALID, bad


def test_ops_checks_fire_before_any_native_call(monkeypatch):
    ops = importlib.import_module(PKG + ".ops")
    nat = importlib.import_module(PKG + "._native")

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(ops, "call", boom)
    monkeypatch.setattr(nat, "call", boom)
    A = torch.zeros((4, 16), dtype=torch.int32)

    def fails(fn, match, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            fn(**kw)

    ok = dict(A=A, B=A.clone(), cutoffs=(1, 16), p=0.9)
    cmp = lambda **kw: fails(ops.list_compare, **kw)  # noqa: E731
    cmp(match="int32", exc=TypeError, **{**ok, "A": A.long()})
    cmp(match="int32", exc=TypeError, **{**ok, "B": A.float()})
    cmp(match="int32", exc=TypeError, **{**ok, "A": A.numpy()})
    cmp(match="2-D", **{**ok, "A": A.reshape(-1)})
    cmp(match="one shape", **{**ok, "B": A[:3].clone()})
    cmp(match="contiguous", **{**ok, "A": torch.zeros((16, 4), dtype=torch.int32).T})
    cmp(match="k must", **{**ok, "A": torch.zeros((2, 129), dtype=torch.int32), "B": torch.zeros((2, 129), dtype=torch.int32)})
    cmp(match="cutoff", **{**ok, "cutoffs": (0,)})
    cmp(match="cutoff", **{**ok, "cutoffs": (17,)})
    cmp(match="cutoff", **{**ok, "cutoffs": (2.0,)})
    cmp(match="cutoffs", **{**ok, "cutoffs": ()})
    cmp(match="cutoffs", **{**ok, "cutoffs": tuple(range(1, 10))})
    for p in (0.0, 1.0, -1.0, 1.5, "0.9", float("nan")):
        cmp(match="p must", **{**ok, "p": p})
    cmp(match="HIP device", **ok)  # CPU lists: there is no CPU path

    okx = dict(lists=A, num_items=50, cutoffs=(1, 16))
    exp = lambda **kw: fails(ops.list_exposure, **kw)  # noqa: E731
    exp(match="int32", exc=TypeError, **{**okx, "lists": A.long()})
    exp(match="2-D", **{**okx, "lists": A.reshape(2, 2, 16)})
    exp(match="cutoff", **{**okx, "cutoffs": (17,)})
    exp(match="num_items", **{**okx, "num_items": 0})
    exp(match="num_items", **{**okx, "num_items": 50.0})
    exp(match="num_items", **{**okx, "num_items": 1 << 31})
    exp(match="HIP device", **okx)

    counts = torch.zeros((2, 50), dtype=torch.int32)
    okm = dict(counts=counts, pop=torch.zeros(50, dtype=torch.int32), tail=torch.zeros(50, dtype=torch.uint8))
    met = lambda **kw: fails(ops.exposure_metrics, **kw)  # noqa: E731
    met(match="int32", exc=TypeError, **{**okm, "counts": counts.long()})
    met(match="2-D", **{**okm, "counts": counts.reshape(-1)})
    met(match="counts", **{**okm, "counts": torch.zeros((9, 50), dtype=torch.int32)})
    met(match="pop", exc=TypeError, **{**okm, "pop": torch.zeros(50)})
    met(match="tail", exc=TypeError, **{**okm, "tail": torch.zeros(50, dtype=torch.int32)})
    met(match="pop", **{**okm, "pop": torch.zeros(49, dtype=torch.int32)})
    met(match="tail", **{**okm, "tail": torch.zeros(51, dtype=torch.uint8)})
    met(match="HIP device", **okm)


# ---- item_popularity --------------------------------------------------------------------------
def _dataset():
    # six items; train lists: user 0 -> {1, 3, 5}, user 1 -> {1, 3}, user 2 -> {1, 4}, user 3 -> {0}
    off, items = np.array([0, 3, 5, 7, 8], np.int64), np.array([1, 3, 5, 1, 3, 1, 4, 0], np.int32)
    return SimpleNamespace(num_users=4, num_items=6, sorted_lists=lambda: (off, items))


def test_item_popularity(ev):
    pop, tail = ev.item_popularity(_dataset())  # head: ceil(0.2 * 6) = 2 items
    assert pop.dtype == np.int32 and pop.tolist() == [1, 3, 0, 2, 1, 1]
    assert tail.dtype == bool and tail.tolist() == [True, False, True, False, True, True]
    # three items: 1, 3, then the tie of 0, 4 and 5 goes to the lower id
    assert ev.item_popularity(_dataset(), head_share=0.5)[1].tolist() == [False, False, True, False, True, True]
    assert ev.item_popularity(_dataset(), head_share=4 / 6)[1].tolist() == [False, False, True, False, False, True]
    assert ev.item_popularity(_dataset(), head_share=0.0)[1].all()
    assert not ev.item_popularity(_dataset(), head_share=1.0)[1].any()
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            ev.item_popularity(_dataset(), head_share=bad)


def test_cutoffs_above_k_are_an_error(ev):
    with pytest.raises(ValueError, match="cutoff"):
        ev.exposure((None, None), _dataset(), k=10, cutoffs=(5, 11))
    with pytest.raises(ValueError, match="cutoff"):
        ev.list_robustness(None, _dataset(), None, [0.5], k=10, cutoffs=(1, 11))


def test_model_layers_expose_the_list_methods(acf):
    model = importlib.import_module(PKG + ".model")
    rec = importlib.import_module(PKG + ".recommender")
    for cls in (model.MF, rec.APR):
        assert callable(cls.exposure) and callable(cls.list_robustness)


# ---- the CLI ----------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_cli_flag_and_file(cli, flavor, tmp_path):
    assert cli.parse_args([], flavor).robust_lists == []
    a = cli.parse_args(["--robust_eps", "0.5", "--robust_lists", "1, 10,100"], flavor)
    assert a.robust_lists == [1, 10, 100] and a.robust_eps == [0.5]
    for bad in ("0", "129", "x", "", "1,2,3,4,5,6,7,8,9", "2.5"):
        with pytest.raises(SystemExit):
            cli.parse_args(["--robust_lists", bad], flavor)
    rows = [("clean", 0.0, 1, 1.0, 1.0, 1.0, 0.1, 2 / 3, math.log2(3), 1 / 7, 0.3),
            ("grad", 0.5, 10, 1 / 3, 0.1 + 0.2, 9.999999999999999, 1e-300, 0.7, 5e-324, 123456.789, 0.0)]
    cli.write_lists(str(tmp_path / "o"), "run.lists", rows)
    got = cli.read_lists(str(tmp_path / "o" / "run.lists"))
    assert got == rows and isinstance(got[0][2], int)
    assert (tmp_path / "o" / "run.lists").read_text().splitlines()[0].split("\t")[:3] == ["clean", "0.0", "1"]
    (tmp_path / "bad.lists").write_text("grad\t0.5\t10\t1.0\n")
    with pytest.raises(ValueError):
        cli.read_lists(str(tmp_path / "bad.lists"))
    with pytest.raises(ValueError):
        cli.write_lists(str(tmp_path / "o"), "short.lists", [("grad", 0.5, 10, 1.0)])
