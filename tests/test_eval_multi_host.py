"""Multi-item evaluation without a GPU: the header and the binding, the host-only
workspace query, the numpy metrics (the yardstick of the device metrics), the plan
builder, the rating-file reader, the CLI flag and file, and the checks that fire
before any native call."""
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

NAMES = ("acf_eval_positions_multi_workspace", "acf_eval_positions_multi", "acf_eval_rank_metrics")


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".evaluate")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module(PKG + ".cli")


@pytest.fixture(scope="module")
def native():
    return importlib.import_module(PKG + "._native")


def test_header_binding_and_exports(native):
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in native.SIGNATURES
    assert set(NAMES) <= native.exported_symbols()
    build_native = importlib.import_module(PKG + ".build_native")
    assert any(h.endswith("csrc/acf_eval_multi.h") for h in build_native.LIBS["apr"]["headers"])
    assert {"eval_positions_multi", "rank_metrics"} <= set(importlib.import_module(PKG + ".torch_ops").OPS)


def _ws(native, n_users, n_tests, num_cand):
    size = ctypes.c_size_t(0)
    rc = native.load().acf_eval_positions_multi_workspace(n_users, n_tests, num_cand, ctypes.byref(size))
    return rc, size.value


def test_workspace_query_is_host_only(native):
    # (no device in this process: the query must not need one)
    rc, one = _ws(native, 6040, 60400, 3706)
    assert rc == native.ACF_OK
    assert one < 6040 * 3706 * 4 // 8  # far below the U x I score array
    rc, few = _ws(native, 3, 15, 70000)
    assert rc == native.ACF_OK and few >= 16 + 2 * 15 * 4  # several strips' counts
    rc, single = _ws(native, 100000, 500000, 1000)
    assert rc == native.ACF_OK and single < 1 << 20  # enough tiles: one strip, no partial counts
    assert _ws(native, 0, 0, 1)[0] == native.ACF_OK
    for bad in ((-1, 5, 100), (3, -5, 100), (3, 5, 0), (3, 5, -7), (3, 1 << 31, 100)):
        assert _ws(native, *bad)[0] == native.ACF_E_INVALID, bad
    assert native.load().acf_eval_positions_multi_workspace(3, 5, 100, None) == native.ACF_E_INVALID
    ops = importlib.import_module(PKG + ".ops")
    assert ops.eval_positions_multi_workspace(3, 15, 70000) == few


def test_workspace_grid_matches_the_recorded_bytes(native):
    """The strip cut is ABI: every byte count equals the one recorded before the
    sweeps shared one strip function (tests/golden/make_sweep_strips.py)."""
    with open(os.path.join(REPO, "tests", "golden", "sweep_strips.json")) as f:
        want = json.load(f)["multi"]
    assert len(want) == 8 * 7 * 2
    got = {key: _ws(native, *map(int, key.split(","))) for key in want}
    assert got == {key: (native.ACF_OK, size) for key, size in want.items()}


def test_bad_arguments_are_invalid_before_any_launch(native):
    lib = native.load()
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)  # a non-NULL pointer that is never dereferenced
    cuts = (ctypes.c_int32 * 9)(*range(1, 10))
    metrics = lambda n, c, nc, out=p: lib.acf_eval_rank_metrics(p, p, n, p, c, nc, p, p, p, out, p, None)  # noqa: E731
    assert metrics(-1, cuts, 2) == native.ACF_E_INVALID
    assert metrics(4, cuts, 9) == native.ACF_E_INVALID
    assert metrics(4, (ctypes.c_int32 * 2)(10, 0), 2) == native.ACF_E_INVALID
    assert metrics(4, (ctypes.c_int32 * 2)(10, 1025), 2) == native.ACF_E_INVALID
    assert metrics(4, cuts, 2, None) == native.ACF_E_INVALID
    pos = lambda **k: lib.acf_eval_positions_multi(*[{**dict(  # noqa: E731
        P=p, Q=p, U1=10, I1=100, d=8, users=p, toff=p, titems=p, n=2, T=5, cand=100, eoff=None, ex=None, out=p,
        ws=p, wsb=1 << 20, check=0, stream=None), **k}[a] for a in (
        "P", "Q", "U1", "I1", "d", "users", "toff", "titems", "n", "T", "cand", "eoff", "ex", "out", "ws", "wsb",
        "check", "stream")])
    for bad in (dict(n=-1), dict(T=-1), dict(cand=0), dict(cand=101), dict(wsb=8), dict(out=None), dict(ws=None),
                dict(d=6), dict(eoff=p), dict(users=None)):
        assert pos(**bad) == native.ACF_E_INVALID, bad


def test_metrics_reproduce_the_single_item_metrics(ev):
    rng = np.random.default_rng(3)
    n, K = 200, 100
    pos = rng.integers(0, 300, n)
    pos[:5] = [0, 1, 99, 100, 299]
    n_neg = rng.integers(300, 900, n)
    ks = list(range(1, K + 1))
    single = ev.metrics_from_positions(pos, n_neg, K).mean(axis=0)  # [3, K]: hr, ndcg, auc
    # 8 cutoffs is the device's limit, not the yardstick's
    got = ev.metrics_from_positions_multi(pos, np.arange(n + 1), n_neg, ks)
    np.testing.assert_allclose(got["mean_cut"][:, 0], single[0], rtol=0, atol=1e-12)  # hit = hr
    np.testing.assert_allclose(got["mean_cut"][:, 1], single[0], rtol=0, atol=1e-12)  # recall = hr when m = 1
    np.testing.assert_allclose(got["mean_cut"][:, 3], single[1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["mean_free"][1], single[2][0], rtol=0, atol=1e-12)
    assert got["n_scored"] == n


def test_metrics_by_hand(ev):
    l2 = np.log2
    # user 0: positions (2, 0) -> r = (0, 2), m = 2; user 1: nothing; user 2: the tied pair (1, 1)
    got = ev.metrics_from_positions_multi([2, 0, 1, 1], [0, 2, 2, 4], [10, 5, 4], [1, 2, 3])
    u0 = got["per_user"][0]
    idcg2 = 1 / l2(2) + 1 / l2(3)
    np.testing.assert_allclose(u0[0], [1, 0.5, 1.0, 1.0 / (1 / l2(2)), 1.0], rtol=1e-15)         # K = 1
    np.testing.assert_allclose(u0[1], [1, 0.5, 0.5, 1.0 / idcg2, 1.0 / 2], rtol=1e-15)            # K = 2
    np.testing.assert_allclose(u0[2], [1, 1.0, 2 / 3, (1 + 1 / l2(4)) / idcg2, (1 + 2 / 3) / 2], rtol=1e-15)
    np.testing.assert_allclose(got["per_user_free"][0], [1.0, (1 + (1 - 1 / 10)) / 2], rtol=1e-15)
    assert (got["per_user"][1] == 0).all() and (got["per_user_free"][1] == 0).all()
    u2 = got["per_user"][2]
    assert (u2[0] == 0).all()                                                                     # K = 1: r = 1 misses
    np.testing.assert_allclose(u2[1], [1, 1.0, 1.0, (2 / l2(3)) / idcg2, (1 / 2 + 2 / 2) / 2], rtol=1e-15)
    np.testing.assert_allclose(got["per_user_free"][2], [0.5, ((1 - 1 / 4) + 1) / 2], rtol=1e-15)
    # the empty user is left out of the means
    assert got["n_scored"] == 2
    np.testing.assert_allclose(got["mean_cut"], (got["per_user"][0] + got["per_user"][2]) / 2, rtol=1e-15)
    np.testing.assert_allclose(got["mean_free"], (got["per_user_free"][0] + got["per_user_free"][2]) / 2, rtol=1e-15)
    none = ev.metrics_from_positions_multi([], [0, 0], [3], [5])
    assert none["n_scored"] == 0 and (none["mean_cut"] == 0).all() and (none["mean_free"] == 0).all()


def _dataset():
    # trainList: user 0 -> {1, 3, 5, 7}, user 1 -> {}, user 2 -> {0, 9}
    off, items = np.array([0, 4, 4, 6], np.int64), np.array([1, 3, 5, 7, 0, 9], np.int32)
    return SimpleNamespace(num_users=3, num_items=10, sorted_lists=lambda: (off, items))


def test_init_eval_multi(ev):
    plan = ev.init_eval_multi(_dataset(), {2: [9, 4, 9, 4, 2], 0: [5, 8, 5]})
    assert plan.users.tolist() == [0, 2] and plan.num_candidates == 10
    assert plan.test_off.tolist() == [0, 2, 5] and plan.test_items.tolist() == [5, 8, 9, 4, 2]  # first occurrences
    assert plan.test_off.dtype == np.int64 and plan.test_items.dtype == np.int32
    assert plan.excl_off.tolist() == [0, 3, 4] and plan.excl.tolist() == [1, 3, 7, 0]  # train minus test
    assert plan.n_neg.tolist() == [10 - 3 - 2, 10 - 1 - 3] and plan.n_neg.dtype == np.int32
    plan = ev.init_eval_multi(_dataset(), [[2], [], [1, 1]])
    assert plan.users.tolist() == [0, 1, 2] and plan.test_off.tolist() == [0, 1, 1, 2]
    assert plan.n_neg.tolist() == [5, 10, 7]
    plan = ev.init_eval_multi(_dataset(), {0: [2]}, users=[1, 0, 0])
    assert plan.test_off.tolist() == [0, 0, 1, 2] and plan.excl_off.tolist() == [0, 0, 4, 8]
    for bad in ({0: [10]}, {0: [-1]}, {3: [1]}, {0: [1.5]}, {1: list(range(10))}):
        with pytest.raises(ValueError):
            ev.init_eval_multi(_dataset(), bad)
    with pytest.raises(ValueError):
        ev.init_eval_multi(_dataset(), [[1]], users=[0, 1])


def test_load_test_lists(tmp_path):
    data = importlib.import_module(PKG + ".data")
    f = tmp_path / "held.rating"
    f.write_text("7\t3\t5\t978300760\n2\t9\n7\t1\t4\t0\n\n7\t3\n4.0\t6.0\t1.0\n")
    assert data.load_test_lists(str(f)) == {7: [3, 1, 3], 2: [9], 4: [6]}
    for bad in ("7\n", "a\t3\n", "1.5\t3\n", "-1\t3\n"):
        f.write_text(bad)
        with pytest.raises(ValueError):
            data.load_test_lists(str(f))


@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_cli_flag_and_file(cli, ev, flavor, tmp_path):
    a = cli.parse_args([], flavor)
    assert a.test_multi is None and a.cutoffs == [10, 50, 100]
    a = cli.parse_args(["--test_multi", "held.tsv", "--cutoffs", "5, 20,1024"], flavor)
    assert a.test_multi == "held.tsv" and a.cutoffs == [5, 20, 1024]
    for bad in ("0", "1025", "x", "", "1,2,3,4,5,6,7,8,9", "2.5"):
        with pytest.raises(SystemExit):
            cli.parse_args(["--cutoffs", bad], flavor)
    cuts = (5, 20)
    names = ev.metric_names(cuts)
    assert names == ["hit@5", "recall@5", "precision@5", "ndcg@5", "map@5", "hit@20", "recall@20", "precision@20",
                     "ndcg@20", "map@20", "mrr", "auc", "n_users"]
    vals = {k: 1.0 / (3 + i) for i, k in enumerate(names)}
    vals["n_users"] = 41
    cli.write_multi(str(tmp_path / "o"), "run.multi", dict(reversed(list(vals.items()))), cuts)
    lines = (tmp_path / "o" / "run.multi").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in lines] == names  # a fixed order, whatever the dict's
    got = cli.read_multi(str(tmp_path / "o" / "run.multi"))
    assert got == vals and list(got) == names and isinstance(got["n_users"], int)
    (tmp_path / "bad.multi").write_text("mrr\t0.5\textra\n")
    with pytest.raises(ValueError):
        cli.read_multi(str(tmp_path / "bad.multi"))


def test_checks_fire_before_any_native_call(monkeypatch):
    ops = importlib.import_module(PKG + ".ops")
    nat = importlib.import_module(PKG + "._native")

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(ops, "call", boom)
    monkeypatch.setattr(nat, "call", boom)
    P, Q = torch.zeros(6, 8), torch.zeros(20, 8)
    ok = dict(P=P, Q=Q, users=np.array([0, 3], np.int32), test_off=np.array([0, 2, 5]),
              test_items=np.array([1, 2, 3, 4, 5], np.int32), num_candidates=20)

    def fails(match, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            ops.eval_positions_multi(**{**ok, **kw})

    fails(r"test_off\[0\]", test_off=np.array([1, 2, 5]))
    fails("non-decreasing", test_off=np.array([0, 6, 5]))
    fails(r"test_off\[-1\]", test_off=np.array([0, 2, 4]))
    fails("test_off", test_off=np.array([0, 5]))
    fails("test_off", test_off=np.array([[0, 2, 5]]))
    fails("test_off", test_off=np.array([0.0, 2.0, 5.0]))
    fails("test_items", test_items=np.array([1.0, 2.0, 3.0, 4.0, 5.0]))
    fails("test_items", test_items=np.zeros((5, 1), np.int32))
    fails("users", users=np.array([0.5, 3.0]))
    fails("go together", excl_off=np.array([0, 0, 0]))
    fails("excl_off", excl_off=np.array([0, 1]), excl_items=np.array([4], np.int32))
    fails(r"excl_off\[-1\]", excl_off=np.array([0, 1, 3]), excl_items=np.array([4, 5], np.int32))
    fails("excl_items", excl_off=np.array([0, 1, 2]), excl_items=np.array([4.0, 5.0]))
    fails("num_candidates", num_candidates=0)
    fails("num_candidates", num_candidates=21)
    fails("num_candidates", num_candidates=20.0)
    fails("float32", exc=TypeError, Q=Q.double())
    fails("HIP device")  # CPU tables: there is no CPU path

    pos, nn = torch.zeros(5, dtype=torch.int32), torch.ones(2, dtype=torch.int32)

    def mfails(match, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            ops.rank_metrics(**{**dict(positions=pos, test_off=np.array([0, 2, 5]), n_neg=nn, cutoffs=(10,)), **kw})

    mfails("cutoff", cutoffs=(0,))
    mfails("cutoff", cutoffs=(1025,))
    mfails("cutoff", cutoffs=(10.0,))
    mfails("cutoffs", cutoffs=tuple(range(1, 10)))
    mfails("cutoffs", cutoffs=5)
    mfails("int32", exc=TypeError, positions=pos.long())
    mfails("HIP device")


def test_model_layers_expose_evaluate_multi(acf):
    model = importlib.import_module(PKG + ".model")
    rec = importlib.import_module(PKG + ".recommender")
    for cls in (model.MF, rec.APR):
        assert callable(cls.evaluate_multi)
