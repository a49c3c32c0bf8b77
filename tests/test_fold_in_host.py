"""Fold-in without a GPU: the CSR builder, the negative draw, the rating-file
parser, the checks that fire before any native call, the argparse rules, and the
CPU check of the GPU fixtures' seeds (the oracle against the other restatement)."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".evaluate")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module(PKG + ".cli")


def test_header_and_binding_declare_fold_in():
    native = importlib.import_module(PKG + "._native")
    ops = importlib.import_module(PKG + ".ops")
    assert "acf_fold_in_users" in native.SIGNATURES
    import os
    from conftest import REPO
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    assert "#define ACF_FOLD_MAX_BATCH 512" in text and ops.FOLD_MAX_BATCH == 512


def test_fold_lists_sorts_and_deduplicates(ev):
    keys, off, items = ev.fold_lists([[5, 1, 5, 3], [], np.array([9, 2]), (7,)])
    assert keys == [0, 1, 2, 3]
    assert off.dtype == np.int64 and items.dtype == np.int32
    assert off.tolist() == [0, 3, 3, 5, 6] and items.tolist() == [1, 3, 5, 2, 9, 7]
    keys, off, items = ev.fold_lists({30: [4, 4], 7: [8, 2], 100000: []})
    assert keys == [7, 30, 100000]
    assert off.tolist() == [0, 2, 3, 3] and items.tolist() == [2, 8, 4]
    keys, off, items = ev.fold_lists([])
    assert keys == [] and off.tolist() == [0] and items.size == 0
    with pytest.raises(ValueError):
        ev.fold_lists([[1, -2]])
    with pytest.raises(ValueError):
        ev.fold_lists([[1.5, 2.0]])
    with pytest.raises(ValueError):
        ev.fold_lists([[[1, 2], [3, 4]]])


def test_fold_negatives_rule_and_seed(ev):
    _, off, items = ev.fold_lists([[0, 1, 2, 3, 4, 5, 6, 7], [9], [], [2, 4, 6, 8]])
    a = ev.fold_negatives(off, items, 10, 50, seed=3)
    assert a.shape == (50, 13) and a.dtype == np.int32
    assert ((a >= 0) & (a < 10)).all()
    for r in range(4):
        own = set(items[off[r]:off[r + 1]].tolist())
        assert not own & set(a[:, off[r]:off[r + 1]].reshape(-1).tolist())
    assert set(a[:, :8].reshape(-1).tolist()) == {8, 9}  # uniform over what is left
    np.testing.assert_array_equal(a, ev.fold_negatives(off, items, 10, 50, seed=3))
    assert (a != ev.fold_negatives(off, items, 10, 50, seed=4)).any()
    assert ev.fold_negatives(off, items, 10, 0).shape == (0, 13)
    with pytest.raises(ValueError, match="every item"):
        ev.fold_negatives(np.array([0, 3]), np.array([0, 1, 2]), 3, 1)
    with pytest.raises(ValueError, match="outside"):
        ev.fold_negatives(np.array([0, 1]), np.array([12]), 10, 1)


def test_rating_file_parser(cli, tmp_path):
    f = tmp_path / "new.rating"
    f.write_text("7\t3\t5\t978300760\n7\t1\t4\t978300761\n\n2\t9\n7\t3\t1\t0\n4.0\t6.0\t1.0\n")
    assert cli.read_fold_file(str(f)) == {7: [3, 1, 3], 2: [9], 4: [6]}
    for bad in ("7\n", "a\t3\n", "1.5\t3\n", "-1\t3\n"):
        f.write_text(bad)
        with pytest.raises(ValueError):
            cli.read_fold_file(str(f))
    cli.write_fold_users(str(tmp_path), "x.foldin.users", [2, 4, 7])
    assert (tmp_path / "x.foldin.users").read_text() == "2\n4\n7\n"


@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_argparse_rules(cli, flavor, capsys):
    assert cli.parse_args([], flavor).fold_in is None
    a = cli.parse_args(["--fold_in", "f.tsv", "--topk", "7"], flavor)
    assert a.fold_in == "f.tsv" and a.topk == 7
    with pytest.raises(SystemExit):
        cli.parse_args(["--fold_in", "f.tsv"], flavor)
    assert "--topk" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_args(["--fold_in", "f.tsv", "--topk", "0"], flavor)


def test_checks_fire_before_any_native_call(monkeypatch):
    ops = importlib.import_module(PKG + ".ops")
    native = importlib.import_module(PKG + "._native")

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(ops, "call", boom)
    monkeypatch.setattr(native, "call", boom)
    Q = torch.zeros(20, 8)
    off, items = np.array([0, 2, 5]), np.array([1, 2, 3, 4, 5], np.int32)
    neg = np.zeros((2, 5), np.int32)
    hp = ops.StepHParams(adver=1)
    ok = dict(Q=Q, user_off=off, item_pos=items, item_neg=neg, hp=hp, epochs=2, batch=4)

    def fails(match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.fold_in_users(**{**ok, **kw})

    fails(r"user_off\[0\]", user_off=np.array([1, 2, 5]))
    fails("non-decreasing", user_off=np.array([0, 3, 2, 5]))
    fails(r"user_off\[-1\]", user_off=np.array([0, 2, 4]))
    fails("user_off", user_off=np.array([[0, 5]]))
    fails("user_off", user_off=np.array([0.0, 5.0]))
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
    fails("HIP device")                                  # a CPU table: there is no CPU path
    fails("float32", Q=Q.double())


def test_model_layers_expose_fold_in(acf):
    model = importlib.import_module(PKG + ".model")
    rec = importlib.import_module(PKG + ".recommender")
    ev = importlib.import_module(PKG + ".evaluate")
    for cls in (model.MF, rec.APR):
        assert callable(cls.fold_in) and callable(cls.recommend_new)
    assert callable(ev.fold_in) and callable(ev.recommend_new)
    torch_ops = importlib.import_module(PKG + ".torch_ops")
    assert "fold_in_users" in torch_ops.OPS


def test_fixture_seeds_leave_headroom_on_the_cpu(oracle):
    """Every multi-step fixture of tests/test_gpu_fold_in.py: the C oracle driven
    per user and slice agrees with apr_oracle.tf_graph_step driven the same way
    (another summation order) to a TENTH of the fp32_parity bar with no outlier;
    single-step users to rtol 1e-5 / atol 1e-6 outright."""
    import apr_oracle
    G = importlib.import_module("test_gpu_fold_in")
    ops = importlib.import_module(PKG + ".ops")

    def tf_step(P1, Qc, a1, aQ, u, i, j, hp):
        return apr_oracle.tf_graph_step(P1, Qc, a1, aQ, u, i, j, hp)[0]

    def both(name, Q, off, flat, neg, batch, init=None, acc=None, users=None, **hpkw):
        _, ohp = G.hparams(ops, apr_oracle, **hpkw)
        a = G.oracle_fold(G.c_step(oracle), Q, off, flat, neg, ohp, batch, init, acc, users)
        b = G.oracle_fold(tf_step, Q, off, flat, neg, ohp, batch, init, acc, users)
        E = neg.shape[0]
        a, b = [a[0], a[1], a[2].T], [b[0], b[1], b[2].T]  # one row per user
        if users is not None:
            a, b = [x[users] for x in a], [x[users] for x in b]
            off = np.r_[0, np.cumsum(np.diff(off)[users])]
        steps = E * -(-np.diff(off) // batch)
        one, many = np.flatnonzero(steps <= 1), np.flatnonzero(steps > 1)
        for x, y, what in zip(a, b, ("P_new", "acc_new", "loss")):
            np.testing.assert_allclose(x[one], y[one], rtol=1e-5, atol=1e-6, err_msg=f"{name} {what}")
            if len(many):
                want = y[many].astype(np.float64)
                err = np.abs(x[many].astype(np.float64) - want)
                assert err.max() <= 1e-6 * max(1.0, np.abs(want).max()), f"{name} {what}: {err.max():.3e}"
                assert not (err > 1e-6 + 1e-5 * np.abs(want)).any(), f"{name} {what}: outliers"

    for d, reg in [(8, 0.0), (48, 0.0), (64, 0.0), (64, 0.01), (128, 0.0), (512, 0.0)]:
        Q, off, flat, neg = G.step_case(d)
        both(f"step d={d} reg={reg}", Q, off, flat, neg, 64, reg=reg)
    for d, seed in G.EPOCH_SEEDS.items():
        Q, off, flat, neg, init, acc = G.epochs_case(seed, d)
        both(f"epochs d={d}", Q, off, flat, neg, 64, init, acc)
    for d in G.PADDED_SEEDS:
        Q, off, flat, neg, init, acc = G.padded_case(d)
        both(f"padded d={d}", Q, off, flat, neg, 64, init, acc)
    Q, off, flat, neg, init = G.grid_case()
    both("grid", Q, off, flat, neg, 512, init, users=G.grid_picks())
    ev = importlib.import_module(PKG + ".evaluate")
    Q, lists = G.planted_case()
    _, off, flat = ev.fold_lists(lists)
    both("planted", Q, off, flat, ev.fold_negatives(off, flat, Q.shape[0], 10, 4), 512)
