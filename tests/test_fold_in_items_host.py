"""Item fold-in without a GPU: the header and binding, the negative draw, the
rating-file parser on the item column, the argparse rules, the checks that fire
before any native call, the model layers, and the CPU check of the GPU fixtures'
seeds (the C oracle against the other restatement)."""
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import PKG, REPO


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".evaluate")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module(PKG + ".cli")


def test_header_and_binding_declare_fold_in_items():
    native = importlib.import_module(PKG + "._native")
    ops = importlib.import_module(PKG + ".ops")
    build_native = importlib.import_module(PKG + ".build_native")
    assert "acf_fold_in_items" in native.SIGNATURES
    assert len(native.SIGNATURES["acf_fold_in_items"][1]) == 20
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    m = re.search(r"int acf_fold_in_items\(([^;]*)\);", text)
    assert m and len(m.group(1).split(",")) == 20
    assert "#define ACF_FOLD_MAX_BATCH 512" in text and ops.FOLD_MAX_BATCH == 512
    # the library hash covers the new header, and the header says why there is no i == j case
    assert any(h.endswith("csrc/acf_fold_items.h") for h in build_native.LIBS["apr"]["headers"])
    head = open(os.path.join(REPO, PKG, "csrc", "acf_fold_items.h")).read()
    assert "can never equal the new item" in head


def test_fold_item_negatives_rule_and_seed(ev):
    _, off, users = ev.fold_lists([[0, 1, 2], [3], [], [1, 3]])
    a = ev.fold_item_negatives(off, users, 10, 50, seed=3)
    assert a.shape == (50, 6) and a.dtype == np.int32
    assert ((a >= 0) & (a < 10)).all()
    assert set(a.reshape(-1).tolist()) == set(range(10))  # plain uniform without a train CSR
    np.testing.assert_array_equal(a, ev.fold_item_negatives(off, users, 10, 50, seed=3))
    assert (a != ev.fold_item_negatives(off, users, 10, 50, seed=4)).any()
    assert ev.fold_item_negatives(off, users, 10, 0).shape == (0, 6)
    # a train CSR of the four existing users: user 0 trained on items 0..7, user 1 on 9, user 2 on none,
    # user 3 on 2, 4, 6, 8 (and on an item outside the table, which is ignored)
    eo = np.array([0, 8, 9, 9, 14])
    ex = np.array([0, 1, 2, 3, 4, 5, 6, 7, 9, 2, 4, 6, 8, 77])
    b = ev.fold_item_negatives(off, users, 10, 400, seed=3, excl_off=eo, excl=ex)
    assert b.shape == (400, 6) and ((b >= 0) & (b < 10)).all()
    train = {0: {0, 1, 2, 3, 4, 5, 6, 7}, 1: {9}, 2: set(), 3: {2, 4, 6, 8}}
    for k, u in enumerate(users.tolist()):
        drawn = set(b[:, k].tolist())
        assert not drawn & train[u]
        assert drawn == set(range(10)) - train[u]  # uniform over what is left: everything admissible turns up
    counts = np.bincount(b[:, users == 3].reshape(-1), minlength=10)[[0, 1, 3, 5, 7, 9]]
    assert counts.min() > 0.6 * counts.mean() and counts.max() < 1.4 * counts.mean()
    np.testing.assert_array_equal(b, ev.fold_item_negatives(off, users, 10, 400, seed=3, excl_off=eo, excl=ex))
    assert (b != ev.fold_item_negatives(off, users, 10, 400, seed=5, excl_off=eo, excl=ex)).any()
    with pytest.raises(ValueError, match="every item"):
        ev.fold_item_negatives(np.array([0, 1]), np.array([0]), 3, 1, excl_off=np.array([0, 3]),
                               excl=np.array([0, 1, 2]))
    with pytest.raises(ValueError, match="outside"):
        ev.fold_item_negatives(np.array([0, 1]), np.array([4]), 10, 1, excl_off=eo, excl=ex)
    with pytest.raises(ValueError, match="outside"):
        ev.fold_item_negatives(np.array([0, 1]), np.array([-1]), 10, 1)
    with pytest.raises(ValueError, match="item_off"):
        ev.fold_item_negatives(np.array([0, 2]), np.array([1]), 10, 1)
    with pytest.raises(ValueError, match="go together"):
        ev.fold_item_negatives(np.array([0, 1]), np.array([1]), 10, 1, excl_off=eo)
    with pytest.raises(ValueError, match="positive"):
        ev.fold_item_negatives(np.array([0, 1]), np.array([1]), 0, 1)


def test_rating_file_parser_on_the_item_column(cli, tmp_path):
    f = tmp_path / "new.rating"
    f.write_text("7\t3\t5\t978300760\n7\t1\t4\t978300761\n\n2\t3\n7\t3\t1\t0\n4.0\t6.0\t1.0\n")
    assert cli.read_fold_items_file(str(f)) == {3: [7, 7, 2], 1: [7], 6: [4]}
    for bad in ("7\n", "a\t3\n", "3\t1.5\n", "3\t-1\n"):
        f.write_text(bad)
        with pytest.raises(ValueError):
            cli.read_fold_items_file(str(f))


@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_argparse_rules(cli, flavor, capsys):
    assert cli.parse_args([], flavor).fold_in_items is None
    a = cli.parse_args(["--fold_in_items", "f.tsv", "--topk", "7"], flavor)
    assert a.fold_in_items == "f.tsv" and a.topk == 7 and a.fold_in is None
    with pytest.raises(SystemExit):
        cli.parse_args(["--fold_in_items", "f.tsv"], flavor)
    assert "--topk" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_args(["--fold_in_items", "f.tsv", "--topk", "0"], flavor)
    a = cli.parse_args(["--fold_in_items", "f.tsv", "--fold_in", "g.tsv", "--topk", "3"], flavor)
    assert a.fold_in_items == "f.tsv" and a.fold_in == "g.tsv"


def test_checks_fire_before_any_native_call(monkeypatch, ev):
    ops = importlib.import_module(PKG + ".ops")
    native = importlib.import_module(PKG + "._native")

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(ops, "call", boom)
    monkeypatch.setattr(native, "call", boom)
    P, Q = torch.zeros(30, 8), torch.zeros(20, 8)
    off, users = np.array([0, 2, 5]), np.array([1, 2, 3, 4, 5], np.int32)
    neg = np.zeros((2, 5), np.int32)
    hp = ops.StepHParams(adver=1)
    ok = dict(P=P, Q=Q, item_off=off, user_pos=users, item_neg=neg, hp=hp, epochs=2, batch=4)

    def fails(match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.fold_in_items(**{**ok, **kw})

    fails(r"item_off\[0\]", item_off=np.array([1, 2, 5]))
    fails("non-decreasing", item_off=np.array([0, 3, 2, 5]))
    fails(r"item_off\[-1\] must be len\(user_pos\)", item_off=np.array([0, 2, 4]))
    fails("item_off", item_off=np.array([[0, 5]]))
    fails("item_off", item_off=np.array([0.0, 5.0]))
    fails("item_neg", item_neg=np.zeros((2, 4), np.int32))
    fails("item_neg", item_neg=np.zeros((3, 5), np.int32))
    fails("item_neg", item_neg=np.zeros(10, np.int32))
    fails("batch", batch=513)
    fails("batch", batch=0)
    fails("batch", batch=64.0)
    fails("epochs", epochs=-1, item_neg=np.zeros((0, 5), np.int32))
    fails("adv", hp=ops.StepHParams(adver=1, adv="random"))
    fails("zero_delta", hp=ops.StepHParams(adver=1, zero_delta=1))
    fails("StepHParams", hp=None)
    fails("HIP device")                                  # CPU tables: there is no CPU path
    fails("float32", P=P.double())
    # the evaluate layer refuses a user that is no row of the user table before anything else
    with pytest.raises(ValueError, match="outside"):
        ev.fold_in_items((P, Q), [[1, 30]], epochs=1)


def test_model_layers_expose_item_fold_in(acf, ev):
    model = importlib.import_module(PKG + ".model")
    rec = importlib.import_module(PKG + ".recommender")
    for cls in (model.MF, rec.APR):
        assert callable(cls.fold_in_items) and callable(cls.audience_new)
    for name in ("fold_in_items", "audience_new", "extend_items", "fold_item_negatives"):
        assert callable(getattr(ev, name))
    torch_ops = importlib.import_module(PKG + ".torch_ops")
    assert "fold_in_items" in torch_ops.OPS
    # the plugin takes a matrix with one COLUMN per new item, or lists
    import scipy.sparse as sp
    m = sp.dok_matrix((6, 3), dtype=np.float32)
    for u, c in ((0, 0), (4, 0), (2, 2), (5, 2), (1, 2)):
        m[u, c] = 1.0
    lists = rec.APR._new_item_lists(m)
    assert [sorted(np.asarray(x).tolist()) for x in lists] == [[0, 4], [], [1, 2, 5]]
    assert rec.APR._new_item_lists([[1], [2]]) == [[1], [2]]


def test_extend_items_appends_the_folded_rows(ev):
    P, Q = torch.arange(40.0).reshape(5, 8), torch.arange(56.0).reshape(7, 8)
    model = types.SimpleNamespace(embedding_P=P, embedding_Q=Q, num_users=4, num_items=6)  # one padding row each
    rows = -torch.ones(2, 8)
    ext = ev.extend_items(model, ev.FoldInItems([0, 1], np.array([0, 0, 0]), np.zeros(0, np.int32), rows, None, None))
    assert ext.num_users == 4 and ext.num_items == 8 and ext.embedding_P is P
    assert torch.equal(ext.embedding_Q, torch.cat([Q[:6], rows]))  # the padding row is dropped, ids 6 and 7 are new
    assert model.embedding_Q is Q and model.num_items == 6          # the model is not modified
    ext = ev.extend_items((P, Q), rows)
    assert ext.num_items == 9 and torch.equal(ext.embedding_Q[7:], rows)


def test_similar_items_without_rows_is_unchanged(ev, monkeypatch):
    """rows=None passes exactly what the call passed before there was a rows argument"""
    seen = {}

    def fake(T, queries, k, metric="cosine", **kw):
        seen.update(kw, T=T, queries=queries, k=k, metric=metric)
        z = torch.zeros(len(queries), k)
        return z.int(), z
    monkeypatch.setattr(ev.ops, "neighbors_topk", fake)
    Q = torch.zeros(7, 8)
    model = types.SimpleNamespace(embedding_P=torch.zeros(5, 8), embedding_Q=Q, num_users=4, num_items=6)
    ev.similar_items(model, [3, 1], k=2, metric="dot")
    assert seen["T"] is Q and seen["queries"].tolist() == [3, 1] and seen["k"] == 2 and seen["metric"] == "dot"
    assert seen["X"] is None and seen["exclude_self"] is True and seen["num_candidates"] == 6
    rows = torch.ones(2, 8)
    ev.similar_items(model, [0, 1], k=2, rows=rows)
    assert seen["X"] is rows and seen["exclude_self"] is False and seen["num_candidates"] == 6
    ev.similar_items(model, [0], k=2, rows=ev.FoldInItems([0, 1], None, None, rows, None, None))
    assert seen["X"] is rows and seen["exclude_self"] is False


def test_fixture_seeds_leave_headroom_on_the_cpu(oracle):
    """Every multi-step fixture of tests/test_gpu_fold_in_items.py: the C oracle
    driven per item and slice agrees with apr_oracle.tf_graph_step driven the same
    way (another summation order) to a TENTH of the fp32_parity bar with no
    outlier; single-step items to rtol 1e-5 / atol 1e-6 outright."""
    import apr_oracle
    G = importlib.import_module("test_gpu_fold_in_items")
    ops = importlib.import_module(PKG + ".ops")

    def tf_step(Pc, Qx, aP, aQ, u, i, j, hp):
        return apr_oracle.tf_graph_step(Pc, Qx, aP, aQ, u, i, j, hp)[0]

    def both(name, P, Q, off, flat, neg, batch, init=None, acc=None, items=None, **hpkw):
        _, ohp = G.hparams(ops, apr_oracle, **hpkw)
        a = G.oracle_fold_items(G.c_step(oracle), P, Q, off, flat, neg, ohp, batch, init, acc, items)
        b = G.oracle_fold_items(tf_step, P, Q, off, flat, neg, ohp, batch, init, acc, items)
        E = neg.shape[0]
        a, b = [a[0], a[1], a[2].T], [b[0], b[1], b[2].T]  # one row per item
        if items is not None:
            a, b = [x[items] for x in a], [x[items] for x in b]
            off = np.r_[0, np.cumsum(np.diff(off)[items])]
        steps = E * -(-np.diff(off) // batch)
        one, many = np.flatnonzero(steps <= 1), np.flatnonzero(steps > 1)
        for x, y, what in zip(a, b, ("Q_new", "acc_new", "loss")):
            np.testing.assert_allclose(x[one], y[one], rtol=1e-5, atol=1e-6, err_msg=f"{name} {what}")
            if len(many):
                want = y[many].astype(np.float64)
                err = np.abs(x[many].astype(np.float64) - want)
                assert err.max() <= 1e-6 * max(1.0, np.abs(want).max()), f"{name} {what}: {err.max():.3e}"
                assert not (err > 1e-6 + 1e-5 * np.abs(want)).any(), f"{name} {what}: outliers"

    for d, reg in [(8, 0.0), (48, 0.0), (64, 0.0), (64, 0.01), (128, 0.0), (512, 0.0)]:
        P, Q, off, flat, neg = G.step_case(d)
        both(f"step d={d} reg={reg}", P, Q, off, flat, neg, 64, reg=reg)
    P, Q, off, flat, neg, init, acc = G.epochs_case()
    both("epochs", P, Q, off, flat, neg, 64, init, acc)
    for d in G.PADDED_SEEDS:
        P, Q, off, flat, neg, init, acc = G.padded_case(d)
        both(f"padded d={d}", P, Q, off, flat, neg, 64, init, acc)
    P, Q, off, flat, neg, init = G.grid_case()
    both("grid", P, Q, off, flat, neg, 512, init, items=G.grid_picks())
    ev = importlib.import_module(PKG + ".evaluate")
    P, Q, lists = G.planted_case()
    _, off, flat = ev.fold_lists(lists)
    both("planted", P, Q, off, flat, ev.fold_item_negatives(off, flat, Q.shape[0], 10, 4), 512)
