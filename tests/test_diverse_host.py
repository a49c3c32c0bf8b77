"""Diversified top-K without a GPU: the numpy yardstick (tests/diverse_ref.py)
against a brute-force MMR and an all-pairs ILS written one scalar at a time, its
properties, the header and the binding, the checks that fire before any native
call, the relevance normalisation's edge cases, and the CLI flag and file."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import diverse_ref as ref
from conftest import PKG, REPO

NAMES = ("acf_list_similarity", "acf_rerank_mmr")
f32 = np.float32


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".evaluate")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module(PKG + ".cli")


# ---- brute force: one scalar operation at a time ------------------------------------------------
def _dot(a, b):
    s = f32(0.0)
    for x, y in zip(a, b):
        s = f32(s + f32(x * y))
    return s


def _sim(a, b, metric):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if metric == "euclid":
        s = f32(0.0)
        for x, y in zip(a, b):
            diff = f32(x - y)
            s = f32(s + f32(diff * diff))
        return f32(f32(0.0) - s)
    s = _dot(a, b)
    if metric == "dot":
        return s
    den = f32(np.sqrt(_dot(a, a)) * np.sqrt(_dot(b, b)))
    return f32(f32(s / den) + f32(0.0)) if den > 0 else f32(0.0)


def _row_of(T, i):
    return T[i if 0 <= i < len(T) else 0]


def _brute_mmr(T, cand, rel, k_out, lam, metric):
    lam = f32(lam)
    oml = f32(f32(1.0) - lam)
    out = []
    for ids, rs in zip(cand, rel):
        open_ = [i >= 0 and np.isfinite(r) for i, r in zip(ids, rs)]
        pen, picks = [None] * len(ids), []
        for j in range(k_out):
            best, best_o = -1, None
            for c in range(len(ids)):  # upward, ">" alone
                if not open_[c]:
                    continue
                o = f32(lam * rs[c]) if j == 0 else f32(f32(lam * rs[c]) - f32(oml * pen[c]))
                if best < 0 or o > best_o:
                    best, best_o = c, o
            if best < 0:
                picks.append((-1, f32(-np.inf), f32(-np.inf)))
                continue
            picks.append((int(ids[best]), rs[best], best_o))
            open_[best] = False
            for c in range(len(ids)):
                if open_[c]:
                    s = _sim(_row_of(T, ids[c]), _row_of(T, ids[best]), metric)
                    pen[c] = s if pen[c] is None else max(pen[c], s)
        out.append(picks)
    return out


def _brute_ils(T, row, K, metric):
    ids = [i for i in row[:K] if i >= 0]
    if len(ids) < 2:
        return 0.0
    S = np.float64(0.0)
    for b in range(len(ids)):
        c = np.float64(0.0)
        for a in range(b):
            c = c + np.float64(_sim(_row_of(T, ids[a]), _row_of(T, ids[b]), metric))
        S = S + c
    return S / np.float64(len(ids) * (len(ids) - 1) // 2)


def _tiny(seed, n=6, m=7, d=8, rows=9):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((rows, d)).astype(f32)
    T[4], T[6] = T[1], 0.0
    cand = rng.integers(-1, rows, (n, m)).astype(np.int32)
    rel = (rng.integers(-4, 5, (n, m)) * 0.5).astype(f32)
    rel[1, 2], rel[1, 3], rel[2, 0] = np.nan, np.inf, -np.inf
    cand[3], cand[4, 1:] = -1, -1
    cand[5, 0] = rows + 3  # out of range: row 0
    return T, cand, rel


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_yardstick_mmr_is_the_brute_force(metric, lam):
    T, cand, rel = _tiny(3)
    for k_out in (1, 4, 7):
        items, r, obj = ref.rerank_mmr(T, cand, rel, k_out, lam, metric)
        want = _brute_mmr(T, cand, rel, k_out, lam, metric)
        for row in range(len(cand)):
            for j in range(k_out):
                wi, wr, wo = want[row][j]
                assert items[row, j] == wi, (row, j)
                assert r[row, j].tobytes() == f32(wr).tobytes() and obj[row, j] == wo, (row, j)
    assert (items[3] == -1).all() and np.isneginf(obj[3]).all() and np.isneginf(r[3]).all()
    assert (items[4, 1:] == -1).all() and items[4, 0] == cand[4, 0]


@pytest.mark.parametrize("metric", ref.METRICS)
def test_yardstick_ils_is_the_all_pairs_mean(metric):
    T, lists, _ = _tiny(5)
    cuts = (1, 2, 5, 7)
    ils, means = ref.list_similarity(T, lists, cuts, metric)
    for r in range(len(lists)):
        for q, K in enumerate(cuts):
            assert ils[r, q] == _brute_ils(T, lists[r], K, metric), (r, K)
    for q, K in enumerate(cuts):
        scored = [(lists[r, :K] >= 0).sum() >= 2 for r in range(len(lists))]
        want = sum(ils[r, q] for r in range(len(lists)) if scored[r]) / max(1, sum(scored))
        assert abs(means[q] - want) <= 1e-15 * max(1.0, abs(want)) and (any(scored) or means[q] == 0.0)
    assert not ils[3].any() and not ils[4].any()  # no entry, one entry
    assert ref.tree_mean([1.0, 5.0, 9.0], [True, False, True]) == 5.0 and ref.tree_mean([2.0], [False]) == 0.0


def test_yardstick_properties():
    T, cand, rel = _tiny(8, m=9)
    cand, rel = np.abs(cand), np.where(np.isfinite(rel), rel, f32(0.0))
    # lam = 1 on a pool sorted by relevance: its first k_out entries
    order = np.argsort(-rel, axis=1, kind="stable")
    cs, rs = np.take_along_axis(cand, order, 1), np.take_along_axis(rel, order, 1)
    for metric in ref.METRICS:
        items, r, obj = ref.rerank_mmr(T, cs, rs, 5, 1.0, metric)
        assert np.array_equal(items, cs[:, :5]) and np.array_equal(r, rs[:, :5]) and np.array_equal(obj, rs[:, :5])
    # every pool position is picked once; duplicated table rows tie to the lower position
    items, _, _ = ref.rerank_mmr(T, cand, rel, 9, 0.4, "cosine")
    assert np.array_equal(np.sort(items, axis=1), np.sort(cand, axis=1))
    items, _, obj = ref.rerank_mmr(T, np.array([[4, 1, 4, 1]], np.int32), np.full((1, 4), 0.5, f32), 4, 0.5, "dot")
    assert items.tolist() == [[4, 1, 4, 1]] and obj[0, 1] == obj[0, 2] == obj[0, 3]
    # a zero row scores +0.0 under cosine; identical rows 0.0 under euclid; the sims are symmetric
    s = ref.pair_sims(T, np.array([[6, 1, 4, 2]]), "cosine")[0]
    assert not s[0].any() and not np.signbit(s[0]).any() and np.array_equal(s, s.T)
    assert ref.pair_sims(T, np.array([[1, 4]]), "euclid")[0, 0, 1] == 0.0
    # ILS of a list of copies of one item is the self-similarity, whatever the cutoff
    ils, _ = ref.list_similarity(T, np.array([[1, 4, 1, 4]]), (2, 3, 4), "euclid")
    assert not ils.any()


# ---- the header, the build, the binding ---------------------------------------------------------
def test_header_binding_and_build_list():
    native = importlib.import_module(PKG + "._native")
    build = importlib.import_module(PKG + ".build_native")
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, re.M) and name in native.SIGNATURES
    assert native.ABI_VERSION == 2 and "#define ACF_APR_ABI_VERSION 2" in text
    assert any(h.endswith("csrc/acf_diverse.h") for h in build.LIBS["apr"]["headers"])
    rank = open(os.path.join(REPO, PKG, "csrc", "acf_rank.hip")).read()
    assert '#include "acf_diverse.h"' in rank


# ---- the checks that fire before any native call ------------------------------------------------
def test_argument_errors_raise_before_any_native_call(monkeypatch):
    ops = importlib.import_module(PKG + ".ops")

    def never(*a, **kw):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(ops, "call", never)
    T = torch.zeros(5, 8)
    cand = torch.zeros(3, 4, dtype=torch.int32)
    rel = torch.zeros(3, 4)
    type_errors = [lambda: ops.rerank_mmr(T.double(), cand, rel, 2, 0.5), lambda: ops.rerank_mmr(None, cand, rel, 2, 0.5),
                   lambda: ops.rerank_mmr(T, cand.long(), rel, 2, 0.5), lambda: ops.rerank_mmr(T, cand, rel.half(), 2, 0.5),
                   lambda: ops.rerank_mmr(T, cand, rel.numpy(), 2, 0.5),
                   lambda: ops.list_similarity(T[0], cand, (1,)), lambda: ops.list_similarity(T, cand.float(), (1,))]
    value_errors = [lambda: ops.rerank_mmr(T, cand, rel, 0, 0.5), lambda: ops.rerank_mmr(T, cand, rel, 5, 0.5),
                    lambda: ops.rerank_mmr(T, cand, rel, True, 0.5), lambda: ops.rerank_mmr(T, cand, rel, 2.0, 0.5),
                    lambda: ops.rerank_mmr(T, cand, rel, 2, -0.1), lambda: ops.rerank_mmr(T, cand, rel, 2, 1.01),
                    lambda: ops.rerank_mmr(T, cand, rel, 2, float("nan")), lambda: ops.rerank_mmr(T, cand, rel, 2, "0.5"),
                    lambda: ops.rerank_mmr(T, cand, rel, 2, 0.5, metric="l1"),
                    lambda: ops.rerank_mmr(T, cand, rel[:2], 2, 0.5), lambda: ops.rerank_mmr(T, cand, rel.t(), 2, 0.5),
                    lambda: ops.rerank_mmr(T, cand[0], rel[0], 2, 0.5),
                    lambda: ops.rerank_mmr(T, torch.zeros(3, 129, dtype=torch.int32), torch.zeros(3, 129), 2, 0.5),
                    lambda: ops.rerank_mmr(torch.zeros(5, 6), cand, rel, 2, 0.5),
                    lambda: ops.rerank_mmr(torch.zeros(0, 8), cand, rel, 2, 0.5),
                    lambda: ops.rerank_mmr(torch.zeros(8, 5).t(), cand, rel, 2, 0.5),
                    lambda: ops.list_similarity(T, cand, ()), lambda: ops.list_similarity(T, cand, (5,)),
                    lambda: ops.list_similarity(T, cand, (0,)), lambda: ops.list_similarity(T, cand, range(1, 10)),
                    lambda: ops.list_similarity(T, cand, (1,), metric="jaccard"),
                    lambda: ops.list_similarity(T, cand.t(), (1,)),
                    # everything else in order: tensors on the CPU are what fails last
                    lambda: ops.rerank_mmr(T, cand, rel, 2, 0.5), lambda: ops.list_similarity(T, cand, (1, 4))]
    for bad in type_errors:
        with pytest.raises(TypeError):
            bad()
    for bad in value_errors:
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="HIP device"):
        ops.rerank_mmr(T, cand, rel, 2, 0.5)


def test_evaluate_argument_errors(ev):
    tables = (torch.zeros(4, 8), torch.zeros(9, 8))
    with pytest.raises(ValueError, match="pool"):
        ev.recommend_diverse(tables, users=[0], k=11, pool=10)
    with pytest.raises(ValueError, match="pool"):
        ev.recommend_diverse(tables, users=[0], k=5, pool=129)
    with pytest.raises(ValueError, match="rel_norm"):
        ev.recommend_diverse(tables, users=[0], k=5, pool=8, rel_norm="softmax")
    with pytest.raises(ValueError, match="dataset"):
        ev.recommend_diverse(tables, k=5, pool=8)
    with pytest.raises(ValueError, match="cutoff"):
        ev.diversity_tradeoff(tables, None, k=5, pool=8, cutoffs=(6,))


# ---- relevance normalisation -------------------------------------------------------------------
def test_rel_norm_edge_cases(ev):
    items = torch.tensor([[3, 1, 2, 0], [5, 5, 5, 5], [-1, 7, -1, -1], [-1, -1, -1, -1], [4, -1, 6, -1]], dtype=torch.int32)
    ninf = float("-inf")
    scores = torch.tensor([[2.0, 1.0, 0.5, -2.0], [0.25, 0.25, 0.25, 0.25], [ninf, 3.0, ninf, ninf],
                           [ninf, ninf, ninf, ninf], [1.0, ninf, -1.0, ninf]])
    rel = ev.normalise_relevance(items, scores, "minmax")
    assert rel.dtype == torch.float32 and rel.is_contiguous()
    assert rel[0].tolist() == [1.0, 0.75, 0.625, 0.0]
    assert rel[1].tolist() == [0.0] * 4          # a constant row
    assert rel[2].tolist() == [0.0] * 4          # one valid entry
    assert rel[3].tolist() == [0.0] * 4          # none
    assert rel[4].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert torch.isfinite(rel).all()
    assert ev.normalise_relevance(items, scores, "none") is scores
    with pytest.raises(ValueError):
        ev.normalise_relevance(items, scores, "zscore")
    # min-max keeps the order, so lam = 1 keeps the pool's
    got = ref.rerank_mmr(np.eye(8, dtype=f32), items[:1].numpy(), rel[:1].numpy(), 4, 1.0, "cosine")[0]
    assert got.tolist() == [[3, 1, 2, 0]]


def test_pool_scores_finds_the_original_scores(ev):
    pool = torch.tensor([[9, 4, 7, -1], [2, 3, -1, -1]], dtype=torch.int32)
    scores = torch.tensor([[3.0, 2.0, 1.0, float("-inf")], [0.5, 0.25, float("-inf"), float("-inf")]])
    picked = torch.tensor([[7, 9, 4], [3, 2, -1]], dtype=torch.int32)
    assert ev._pool_scores(pool, scores, picked).tolist() == [[1.0, 3.0, 2.0], [0.25, 0.5, float("-inf")]]


# ---- the CLI -----------------------------------------------------------------------------------
def test_cli_flags_and_file_round_trip(cli, tmp_path):
    args = cli.parse_args(["--diverse_lambda", "1,0.7,0.5", "--topk", "10"])
    assert args.diverse_lambda == [1.0, 0.7, 0.5] and args.diverse_pool == 128 and args.diverse_metric == "cosine"
    assert cli.parse_args([]).diverse_lambda == []
    for bad in (["--diverse_lambda", "0.5"], ["--diverse_lambda", "1.5", "--topk", "5"],
                ["--diverse_lambda", "-1", "--topk", "5"], ["--diverse_lambda", "x", "--topk", "5"],
                ["--diverse_lambda", "0.5", "--topk", "20", "--diverse_pool", "10"],
                ["--diverse_lambda", "0.5", "--topk", "5", "--diverse_pool", "200"],
                ["--diverse_lambda", "0.5", "--topk", "5", "--diverse_metric", "l1"],
                ["--diverse_lambda", "0.5", "--topk", "5", "--model", "apr", "--grid_eps", "0.1,0.5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    rows = [(1.0, 10, 0.1, 1 / 3, 0.9123456789012345, 5000.0, 0.25, 0.8, 7.5, 12.25, 0.0),
            (0.5, 10, 0.05, 2e-17, -0.1, 5000.0, 0.5, 0.7, 8.0, 9.0, 0.125)]
    cli.write_diverse(str(tmp_path), "run.diverse", rows)
    assert cli.read_diverse(str(tmp_path / "run.diverse")) == rows
    with pytest.raises(ValueError):
        cli.write_diverse(str(tmp_path), "bad.diverse", [(1.0, 10, 0.1)])
    (tmp_path / "short.diverse").write_text("1.0\t10\t0.5\n")
    with pytest.raises(ValueError):
        cli.read_diverse(str(tmp_path / "short.diverse"))
