"""Nearest-neighbour lists without a GPU: the numpy yardstick (nbr_ref.py) against
an fp64 computation, the host-only workspace query, argument validation of
ops.neighbors_topk, the CLI's --similar flags and NeuMF's refusal."""
import ctypes
import importlib
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nbr_ref
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


# ---- the reference itself ----------------------------------------------------------
def _fp64_scores(T, X, q, metric):
    A, B = X[q].astype(np.float64), T.astype(np.float64)
    if metric == "dot":
        return A @ B.T
    if metric == "cosine":
        return (A @ B.T) / (np.linalg.norm(A, axis=1)[:, None] * np.linalg.norm(B, axis=1)[None, :])
    return -((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)


@pytest.mark.parametrize("metric", nbr_ref.METRICS)
@pytest.mark.parametrize("d", [4, 64])
def test_reference_agrees_with_fp64(metric, d):
    """Well-separated random data: the fp32 chain is within d rounding steps of
    the fp64 value, and wherever two fp64 scores differ by more than that band the
    fp32 order is the fp64 order, so the lists agree where the data decides."""
    rng = np.random.default_rng(10 + d)
    T = rng.standard_normal((200, d)).astype(np.float32)
    X = rng.standard_normal((30, d)).astype(np.float32)
    q = rng.permutation(30)[:12]
    got = nbr_ref.nbr_scores(T, X, q, metric)
    want = _fp64_scores(T, X, q, metric)
    assert got.dtype == np.float32 and got.shape == want.shape
    # |error| <= (d + 3) eps * sum |terms| <= (d + 3) eps * the Cauchy-Schwarz bound of the metric
    na = np.linalg.norm(X[q].astype(np.float64), axis=1)[:, None]
    nb = np.linalg.norm(T.astype(np.float64), axis=1)[None, :]
    scale = {"dot": na * nb, "cosine": np.ones_like(want), "euclid": (na + nb) ** 2}[metric]
    band = (d + 3) * 2.0 ** -23 * scale
    assert (np.abs(got - want) <= band).all()
    K = 10
    items, scores = nbr_ref.nbr_reference(T, X, q, metric, K, exclude_self=False)
    order = np.argsort(-want, axis=1, kind="stable")[:, :K + 1]
    forced = 0
    for j in range(len(q)):
        top = want[j, order[j]]
        if (top[:-1] - top[1:] > 2 * band[j].max()).all():  # separated by more than the band: the order is forced
            np.testing.assert_array_equal(items[j], order[j, :K])
            forced += 1
    assert forced >= len(q) // 2  # the data is what it claims
    np.testing.assert_array_equal(scores, np.take_along_axis(got, items.astype(np.int64), 1))


def test_reference_rules():
    """Self-exclusion, set semantics of the lists, ties to the lower id, the tail,
    the zero rows and the negative underflow of the cosine."""
    T = np.zeros((6, 4), np.float32)
    T[0] = [1, 0, 0, 0]
    T[1] = [2, 0, 0, 0]      # the same direction as row 0
    T[2] = [0, 1, 0, 0]
    T[4] = [1, 0, 0, 0]      # a copy of row 0; rows 3 and 5 are zero
    it, sc = nbr_ref.nbr_reference(T, None, [0], "cosine", 8)
    np.testing.assert_array_equal(it[0], [1, 4, 2, 3, 5, -1, -1, -1])
    np.testing.assert_array_equal(sc[0, :5], [1, 1, 0, 0, 0])
    assert np.isneginf(sc[0, 5:]).all() and not np.signbit(sc[0, :5]).any()
    it, _ = nbr_ref.nbr_reference(T, None, [0], "cosine", 3, exclude_self=False, lists=[[1, 1, -1, 99, 4]])
    np.testing.assert_array_equal(it[0], [0, 2, 3])
    it, sc = nbr_ref.nbr_reference(T, None, [0, 3], "euclid", 2)
    np.testing.assert_array_equal(it, [[4, 1], [5, 0]])  # row 5 is zero like row 3
    assert sc[0, 0] == 0 and not np.signbit(sc[0, 0]) and sc[0, 1] == -1
    # a query outside the table is row 0 (and id 0 for the self-exclusion)
    a = nbr_ref.nbr_reference(T, None, [17], "dot", 3)
    b = nbr_ref.nbr_reference(T, None, [0], "dot", 3)
    np.testing.assert_array_equal(a[0], b[0])
    with pytest.raises(IndexError):
        nbr_ref.nbr_reference(T, None, [17], "dot", 3, check=True)
    # s = -1e-44 (a denormal), den = 1e32: the quotient underflows to -0.0 and is stored as +0.0
    A = np.array([[1e-22, 1e16, 0, 0]], np.float32)
    B = np.array([[-1e-22, 0, 1e16, 0]], np.float32)
    s = nbr_ref.seq_dot(A, B)
    assert s[0, 0] < 0
    with np.errstate(all="ignore"):
        raw = s / (nbr_ref.row_norms(A)[:, None] * nbr_ref.row_norms(B)[None, :])
    assert raw[0, 0] == 0 and np.signbit(raw[0, 0])
    got = nbr_ref.nbr_scores(B, A, [0], "cosine")
    assert got[0, 0] == 0 and not np.signbit(got[0, 0])


# ---- the C-ABI's host side -----------------------------------------------------------
def test_header_declares_both_functions():
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    fns = set(re.findall(r"^\s*int\s+(acf_\w+)\s*\(", text, re.M))
    assert {"acf_neighbors_topk", "acf_neighbors_topk_workspace"} <= fns
    assert "-0.0" in text[text.index("nearest-neighbour lists"):text.index("acf_neighbors_topk_workspace(")]


def test_workspace_query(native, ops):
    """Host-only; grows with k; holds the top-K partial lists and, on top of
    them, the num_candidates floats of candidate norms the cosine metric uses; far
    below a score matrix or a normalised copy of the table."""
    w = ops.neighbors_topk_workspace
    assert w(64, 5_000_000, 10) < w(64, 5_000_000, 100) < w(64, 5_000_000, 128)
    assert w(17, 300, 1) < w(17, 300, 10)
    for n, c, k in ((17, 300, 10), (3, 40_000, 100), (1024, 5_000_000, 100), (3706, 3706, 100)):
        lists = ops.recommend_topk_workspace(n, c, k, "valu")
        assert lists + 4 * c <= w(n, c, k) <= lists + 4 * c + 64
    assert w(1024, 5_000_000, 100) < 128 << 20  # the normalised copy alone would be 1.28 GB at d = 64
    assert w(10, 0, 5) > 0
    for k in (0, 129, -1):
        with pytest.raises(ValueError, match="k must be"):
            w(10, 10, k)
        with pytest.raises(native.NativeError, match="k must be"):
            native.call("acf_neighbors_topk_workspace", 10, 10, k, ctypes.byref(ctypes.c_size_t()))
    with pytest.raises(native.NativeError):
        native.call("acf_neighbors_topk_workspace", 10, 10, 10, None)


def test_neighbors_topk_validates_before_any_launch(ops):
    T = torch.zeros(6, 8)
    q = torch.zeros(4, dtype=torch.int32)
    for k in (0, 129, -2, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            ops.neighbors_topk(T, q, k)
    with pytest.raises(ValueError, match="metric must be"):
        ops.neighbors_topk(T, q, 3, metric="manhattan")
    with pytest.raises(ValueError, match="HIP device"):
        ops.neighbors_topk(T, q, 3)
    with pytest.raises(TypeError):
        ops.neighbors_topk(T.double(), q, 3)
    assert ops.NEIGHBOR_METRICS == {"dot": 0, "cosine": 1, "euclid": 2}


# ---- layers ------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_parse_args_accepts_similar(flavor, tmp_path, capsys):
    cli = importlib.import_module(PKG + ".cli")
    a = cli.parse_args([], flavor)
    assert a.similar is None and a.similar_metric == "cosine"
    a = cli.parse_args(["--similar", "ids.txt", "--topk", "7", "--similar_metric", "euclid"], flavor)
    assert a.similar == "ids.txt" and a.topk == 7 and a.similar_metric == "euclid"
    assert cli.parse_args(["--similar", "x", "--topk", "1", "--similar_metric", "dot"], flavor).similar_metric == "dot"
    with pytest.raises(SystemExit):
        cli.parse_args(["--similar", "ids.txt"], flavor)  # needs --topk
    with pytest.raises(SystemExit):
        cli.parse_args(["--similar", "ids.txt", "--topk", "5", "--similar_metric", "l1"], flavor)
    capsys.readouterr()
    f = tmp_path / "ids.txt"
    f.write_text("4\n\n0\n17\n4\n")
    assert cli.read_id_file(f) == [4, 0, 17, 4]
    f.write_text("4\nx\n")
    with pytest.raises(ValueError, match="line 1"):
        cli.read_id_file(f)
    f.write_text("-3\n")
    with pytest.raises(ValueError, match=">= 0"):
        cli.read_id_file(f)


def test_neumf_has_no_single_similarity():
    neumf = importlib.import_module(PKG + ".neumf")
    m = object.__new__(neumf.NeuMF)  # the constructor needs a device; the refusal does not
    with pytest.raises(NotImplementedError, match="two item tables"):
        m.similar_items([1, 2], k=5)
    with pytest.raises(NotImplementedError, match="two user tables"):
        m.similar_users([1])
    with pytest.raises(NotImplementedError):
        object.__new__(neumf.AdversarialNeuMF).similar_items([1])


def test_model_layers_expose_the_neighbours(acf):
    rec = importlib.import_module(PKG + ".recommender")
    for cls in (acf.MF, acf.APR, rec.Recommender):
        assert callable(getattr(cls, "similar_items")) and callable(getattr(cls, "similar_users"))
    ev = importlib.import_module(PKG + ".evaluate")
    m = SimpleNamespace(embedding_P=torch.zeros(5, 8), embedding_Q=torch.zeros(9, 8), num_users=4, num_items=8)
    assert ev._neighbor_tables(m)[2:] == (4, 8)            # the padding rows stay out
    assert ev._neighbor_tables((m.embedding_P, m.embedding_Q))[2:] == (5, 9)
    with pytest.raises(ValueError, match="HIP device"):     # reaches the op; no CPU path
        ev.similar_items(m, [0, 1], k=3)
    with pytest.raises(ValueError, match="HIP device"):
        ev.similar_users(m, [0], k=3, metric="euclid")
