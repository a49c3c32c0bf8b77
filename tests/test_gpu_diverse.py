"""Diversified top-K on the GPU: ops.list_similarity and ops.rerank_mmr against the
numpy yardstick (tests/diverse_ref.py), bit for bit -- every operation of the
contract is defined (fp32 chains rounded per operation, fp64 sums in a fixed
order), so ids, rel, obj, ils and means are compared with == on the bytes, no
tolerance -- then evaluate.recommend_diverse / diversity / diversity_tradeoff and
the CLI's .diverse file end to end.

The shapes cover one and two slots per lane (m, k <= 64 and above), rows that are
staged in LDS and rows read from global memory (m (d + 4) 4 bytes above 60 KB:
(63, 260), (128, 260), (128, 1024)), d that is no multiple of the float4 stride's
bank period, and more than one workgroup."""
import glob
import importlib
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diverse_ref as ref

pytestmark = pytest.mark.gpu
PKG = "adversarial-collaborative-filtering_amd"
ROWS = 48  # table rows: fewer than a long pool has positions, so ids repeat

# (n, m, d): every n of {1, 5, 257}, m of {1, 2, 63, 64, 65, 128}, d of {4, 8, 60, 64, 260, 1024}
SHAPES = [(1, 1, 4), (5, 2, 8), (257, 63, 60), (5, 64, 64), (257, 65, 8), (5, 128, 64), (257, 128, 4),
          (1, 128, 260), (5, 63, 260), (5, 2, 260), (5, 128, 1024), (1, 14, 1024)]
LAMS = (0.0, 0.3, 1.0)


def _T(x, dev):
    return torch.tensor(np.ascontiguousarray(x), device=dev)


def _bits(x):
    x = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), what


def _table(d, seed):
    """[ROWS, d]: random rows, row 7 a copy of row 3 and row 11 of row 2 (ties that fall to the pool position),
    row 5 all zeros (cosine +0.0), row 9 = -row 3."""
    rng = np.random.default_rng(seed)
    T = (rng.standard_normal((ROWS, d)) * 0.5).astype(np.float32)
    T[7], T[11], T[5], T[9] = T[3], T[2], 0.0, -T[3]
    return T


def _pools(n, m, seed):
    """cand [n, m], rel [n, m]: random ids (repeats), relevances on a coarse grid (ties), then the special
    rows: holes in the middle and at the tail, non-finite relevances, no valid entry, one valid entry."""
    rng = np.random.default_rng(seed)
    cand = rng.integers(0, ROWS, (n, m)).astype(np.int32)
    rel = (rng.integers(-8, 9, (n, m)) * 0.25).astype(np.float32)
    fine = rng.random(n) < 0.5
    rel[fine] = rng.standard_normal((int(fine.sum()), m)).astype(np.float32)
    for r in range(n):
        kind = r % 7
        if kind == 1:  # holes in the middle
            cand[r, rng.random(m) < 0.3] = -1
        elif kind == 2:  # a -1 tail
            cand[r, m // 2:] = -1
        elif kind == 3:  # non-finite relevances
            bad = rng.random(m) < 0.3
            rel[r, bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
        elif kind == 4 and r % 14 == 4:  # no valid entry: no id, or no finite relevance
            cand[r] = -1
        elif kind == 4:
            rel[r] = np.nan
        elif kind == 5:  # one valid entry
            cand[r] = -1
            cand[r, m // 3] = 3
        elif kind == 6:  # the duplicated rows, the zero row and the opposite row, equal relevance
            cand[r] = np.array([3, 7, 2, 11, 5, 9], np.int32)[np.arange(m) % 6]
            rel[r] = 0.5
    return cand, rel


_SIMS = {}


def _sims(T, ids, key):
    """pair_sims once per (shape, metric, seed): the reference shared by the tests of a shape, left unchanged."""
    if key not in _SIMS:
        _SIMS[key] = ref.pair_sims(T, ids, key[-1])
        _SIMS[key].setflags(write=False)
    return _SIMS[key]


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-m%d-d%d" % s)
def test_mmr_matches_the_yardstick(ops, dev, shape, metric):
    n, m, d = shape
    T = _table(d, 10 + d)
    cand, rel = _pools(n, m, n + m)
    sims = _sims(T, cand, ("mmr", shape, metric))
    Td, cd, rd = _T(T, dev), _T(cand, dev), _T(rel, dev)
    for lam in LAMS:
        for k_out in sorted({1, m}):
            got = ops.rerank_mmr(Td, cd, rd, k_out, lam, metric)
            again = ops.rerank_mmr(Td, cd, rd, k_out, lam, metric)
            want = ref.rerank_mmr(T, cand, rel, k_out, lam, metric, sims=sims)
            for g, a, w, name in zip(got, again, want, ("items", "rel", "obj")):
                assert tuple(g.shape) == (n, k_out)
                _same(g, w, (name, lam, k_out))
                assert torch.equal(g.view(torch.int32), a.view(torch.int32)), ("two runs", name, lam, k_out)
    # the tail: a row's picks are as many as its valid entries
    nvalid = ((cand >= 0) & np.isfinite(rel)).sum(axis=1)
    items = got[0].cpu().numpy()
    assert np.array_equal((items >= 0).sum(axis=1), np.minimum(nvalid, k_out))


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-k%d-d%d" % s)
def test_ils_matches_the_yardstick(ops, dev, shape, metric):
    n, k, d = shape
    T = _table(d, 10 + d)
    lists, _ = _pools(n, k, n + k)
    cuts = tuple(sorted({c for c in (1, 2, 3, k // 2, 63, 64, 65, k - 1, k) if 1 <= c <= k}))[-8:]
    sims = _sims(T, lists, ("ils", shape, metric))
    Td, ld = _T(T, dev), _T(lists, dev)
    got = ops.list_similarity(Td, ld, cuts, metric)
    again = ops.list_similarity(Td, ld, cuts, metric)
    want = ref.list_similarity(T, lists, cuts, metric, sims=sims)
    assert tuple(got[0].shape) == (n, len(cuts)) and tuple(got[1].shape) == (len(cuts),)
    _same(got[0], want[0], "ils")
    _same(got[1], want[1], "means")
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    # rows with fewer than two valid entries: 0.0, and not in the mean
    ils = got[0].cpu().numpy()
    for q, K in enumerate(cuts):
        few = (lists[:, :K] >= 0).sum(axis=1) < 2
        assert not ils[few, q].any()
        if few.all():
            assert float(got[1][q]) == 0.0
    # a subset of the cutoffs, in another order: the same columns
    if len(cuts) > 2:
        sub = (cuts[-1], cuts[0])
        part = ops.list_similarity(Td, ld, sub, metric)[0]
        assert torch.equal(part[:, 0], got[0][:, -1]) and torch.equal(part[:, 1], got[0][:, 0])


@pytest.mark.parametrize("metric", ref.METRICS)
def test_a_row_does_not_depend_on_its_batch(ops, dev, metric):
    n, m, d = 257, 128, 8
    T = _table(d, 3)
    cand, rel = _pools(n, m, 77)
    Td = _T(T, dev)
    full = ops.rerank_mmr(Td, _T(cand, dev), _T(rel, dev), m, 0.3, metric)
    full_ils = ops.list_similarity(Td, _T(cand, dev), (2, 64, 128), metric)[0]
    for rows in (slice(0, 1), slice(250, 257), slice(100, 105)):
        part = ops.rerank_mmr(Td, _T(cand[rows], dev), _T(rel[rows], dev), m, 0.3, metric)
        for f, p in zip(full, part):
            assert torch.equal(f[rows].view(torch.int32), p.view(torch.int32))
        assert torch.equal(full_ils[rows], ops.list_similarity(Td, _T(cand[rows], dev), (2, 64, 128), metric)[0])


@pytest.mark.parametrize("m,d", [(5, 8), (128, 64), (65, 260)])
def test_an_id_out_of_range(ops, dev, m, d):
    """ACF_E_RANGE with check; without it the id is read as row 0 and comes back as it was given."""
    native = importlib.import_module(PKG + "._native")
    T = _table(d, 5)
    cand, rel = _pools(5, m, 9)
    rel = np.where(np.isfinite(rel), rel, np.float32(0.25))
    cand[2, m - 1], cand[4, 0] = ROWS, 2 ** 31 - 1
    Td, cd, rd = _T(T, dev), _T(cand, dev), _T(rel, dev)
    for call in (lambda c: ops.rerank_mmr(Td, cd, rd, m, 0.3, "cosine", check=c),
                 lambda c: ops.list_similarity(Td, cd, (1, m), "cosine", check=c)):
        with pytest.raises(native.NativeIndexError) as e:
            call(True)
        assert e.value.code == native.ACF_E_RANGE
        call(False)
    got = ops.rerank_mmr(Td, cd, rd, m, 0.3, "cosine", check=False)
    want = ref.rerank_mmr(T, cand, rel, m, 0.3, "cosine")
    for g, w in zip(got, want):
        _same(g, w, "row 0 for the id out of range")
    assert ROWS in got[0][2].cpu().tolist() and 2 ** 31 - 1 in got[0][4].cpu().tolist()
    ils = ops.list_similarity(Td, cd, (1, m), "cosine", check=False)
    want = ref.list_similarity(T, cand, (1, m), "cosine")
    _same(ils[0], want[0], "ils")
    _same(ils[1], want[1], "means")
    # an id past the largest cutoff is still an id out of range
    if m > 2:
        cand[4, 0] = 1  # row 2's, at position m - 1, is left
        with pytest.raises(native.NativeIndexError):
            ops.list_similarity(Td, _T(cand, dev), (1, 2), "cosine")


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("d", [4, 64, 260])
def test_the_similarity_is_the_neighbour_lists(ops, dev, metric, d):
    """ILS at K = 2 of [a, b] is (double) of neighbors_topk's score of b as a neighbour of a; obj at step 1
    with lam = 0 is -(1.0f * that score)."""
    T = _table(d, 21)
    Td = _T(T, dev)
    a = np.arange(ROWS, dtype=np.int32)
    b = ((a * 7 + 3) % ROWS).astype(np.int32)
    b = np.where(b == a, (a + 1) % ROWS, b).astype(np.int32)
    items, scores = ops.neighbors_topk(Td, _T(a, dev), ROWS - 1, metric=metric)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    s = np.array([scores[r, list(items[r]).index(b[r])] for r in range(ROWS)], np.float32)
    pairs = _T(np.stack([a, b], axis=1), dev)
    ils, _ = ops.list_similarity(Td, pairs, (2,), metric)
    _same(ils[:, 0], s.astype(np.float64), "ils@2")
    rel = _T(np.tile(np.array([1.0, 0.0], np.float32), (ROWS, 1)), dev)
    got_items, _, obj = ops.rerank_mmr(Td, pairs, rel, 2, 0.0, metric)
    assert np.array_equal(got_items.cpu().numpy(), np.stack([a, b], axis=1))  # lam = 0: a tie, the lower position
    assert np.array_equal(obj[:, 1].cpu().numpy(), -(np.float32(1.0) * s))
    assert not obj[:, 0].cpu().numpy().any()


def test_lam_one_keeps_the_order_of_relevance(ops, dev):
    rng = np.random.default_rng(4)
    T = _table(64, 8)
    rel = -np.sort(-rng.standard_normal((9, 100)).astype(np.float32), axis=1)
    cand = rng.integers(0, ROWS, (9, 100)).astype(np.int32)
    items, r, obj = ops.rerank_mmr(_T(T, dev), _T(cand, dev), _T(rel, dev), 30, 1.0, "cosine")
    assert np.array_equal(items.cpu().numpy(), cand[:, :30])
    _same(r, rel[:, :30], "rel")
    _same(obj[:, 0], rel[:, 0], "obj at step 0")


def test_argument_errors_reach_no_kernel(ops, dev):
    native = importlib.import_module(PKG + "._native")
    T = _T(_table(8, 1), dev)
    cand = _T(np.zeros((3, 4), np.int32), dev)
    rel = _T(np.zeros((3, 4), np.float32), dev)
    for bad in (lambda: ops.rerank_mmr(T, cand, rel, 5, 0.5), lambda: ops.rerank_mmr(T, cand, rel, 0, 0.5),
                lambda: ops.rerank_mmr(T, cand, rel, 2, 1.5), lambda: ops.rerank_mmr(T, cand, rel, 2, float("nan")),
                lambda: ops.rerank_mmr(T, cand, rel, 2, 0.5, metric="manhattan"),
                lambda: ops.rerank_mmr(T, cand, rel[:, :3].contiguous(), 2, 0.5),
                lambda: ops.rerank_mmr(T, cand.cpu(), rel, 2, 0.5),
                lambda: ops.list_similarity(T, cand, (5,)), lambda: ops.list_similarity(T, cand, ()),
                lambda: ops.list_similarity(T, cand, (1, 2), metric="l1"),
                lambda: ops.list_similarity(T.cpu(), cand, (1, 2))):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ops.rerank_mmr(T.double(), cand, rel, 2, 0.5), lambda: ops.rerank_mmr(T, cand.long(), rel, 2, 0.5),
                lambda: ops.rerank_mmr(T, cand, rel.double(), 2, 0.5), lambda: ops.list_similarity(T, cand.long(), (1,))):
        with pytest.raises(TypeError):
            bad()
    # the C side refuses the same before any launch
    lib = native.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    out_i, out_f = torch.empty_like(cand), torch.empty_like(rel)
    ils, means = torch.empty(3, 1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    import ctypes
    cut = (ctypes.c_int32 * 1)(5)

    def mmr(m=4, k=2, lam=0.5, metric=1, d=8):
        return lib.acf_rerank_mmr(T.data_ptr(), ROWS, d, cand.data_ptr(), rel.data_ptr(), 3, m, k, lam, metric,
                                  out_i.data_ptr(), out_f.data_ptr(), out_f.data_ptr(), 1, st)
    for kw in (dict(m=0), dict(m=129), dict(k=0), dict(k=5), dict(lam=-0.1), dict(lam=1.5), dict(metric=3), dict(d=6)):
        assert mmr(**kw) == native.ACF_E_INVALID, kw
    for k, ncut, metric in ((0, 1, 1), (129, 1, 1), (4, 0, 1), (4, 9, 1), (4, 1, -1), (4, 1, 1)):  # the last: cutoff 5 > k
        assert lib.acf_list_similarity(T.data_ptr(), ROWS, 8, cand.data_ptr(), 3, k, cut, ncut, metric,
                                       ils.data_ptr(), means.data_ptr(), 1, st) == native.ACF_E_INVALID
    # n = 0: nothing to do
    none_i, none_f = cand[:0].contiguous(), rel[:0].contiguous()
    assert all(t.shape == (0, 2) for t in ops.rerank_mmr(T, none_i, none_f, 2, 0.5))
    ils0, means0 = ops.list_similarity(T, none_i, (1, 2))
    assert ils0.shape == (0, 2) and not means0.any()


# ---- end to end: a small MF whose items come in clusters of near-duplicates ----------------------
U, I, D, K, POOL = 150, 240, 8, 10, 64


@pytest.fixture(scope="module")
def world(acf, dev):
    data = importlib.import_module(PKG + ".data")
    ds = data.synthetic_dataset(U, I, 3000, seed=7)
    args = SimpleNamespace(embed_size=D, lr=0.05, reg=0.0, dns=1, adv="grad", eps=0.5, adver=0, reg_adv=1.0, epochs=0,
                           seed=3)
    m = acf.MF(U, I, args).build_graph(device=dev)
    rng = np.random.default_rng(12)
    centres = rng.standard_normal((6, D)).astype(np.float32)
    Q = centres[rng.integers(0, 6, I + 1)] + 0.02 * rng.standard_normal((I + 1, D)).astype(np.float32)
    m.load_embeddings((rng.standard_normal((U + 1, D)) * 0.5).astype(np.float32), Q.astype(np.float32))
    return m, ds


def test_tradeoff_rows(ops, dev, world):
    ev = importlib.import_module(PKG + ".evaluate")
    m, ds = world
    rows = m.diversity_tradeoff(ds, lams=(1.0, 0.5), k=K, pool=POOL, cutoffs=(5, K))
    assert [(r[0], r[1]) for r in rows] == [(1.0, 5), (1.0, K), (0.5, 5), (0.5, K)] and all(len(r) == 11 for r in rows)
    plain, _ = ev.recommend(m, ds, k=K)
    tests = np.array([ds.testRatings[u][1] for u in range(U)])
    for row, c in zip(rows[:2], (5, K)):
        hit = (plain[:, :c] == tests[:, None])
        assert row[2] == hit.any(axis=1).mean()
        p = np.where(hit.any(axis=1), hit.argmax(axis=1), c)
        want = np.where(hit.any(axis=1), math.log(2) / np.log(p + 2.0), 0.0).mean()
        assert abs(row[3] - want) <= 1e-12
    # lam = 1 is the plain top-K: the same lists, the same ILS and exposure as the model's own
    items, scores = m.recommend_diverse(ds, k=K, pool=POOL, lam=1.0)
    plain_items, plain_scores = ev.recommend(m, ds, k=K)
    assert np.array_equal(items, plain_items) and np.array_equal(scores, plain_scores)
    assert [r[4] for r in rows[:2]] == [r[1] for r in m.diversity(ds, k=K, cutoffs=(5, K))]
    assert [r[5:] for r in rows[:2]] == [r[1:] for r in m.exposure(ds, k=K, cutoffs=(5, K))]
    # diversifying: the lists are less alike, strictly
    assert rows[3][4] < rows[1][4] and rows[2][4] < rows[0][4]
    items, scores = m.recommend_diverse(ds, users=[3, 3, 149], k=K, pool=POOL, lam=0.5)
    assert items.shape == (3, K) and np.array_equal(items[0], items[1]) and (items >= 0).all()
    Pn, Qn = m.embedding_P.cpu().numpy(), m.embedding_Q.cpu().numpy()
    for r, u in enumerate((3, 3, 149)):
        assert len(set(items[r])) == K
        np.testing.assert_allclose(scores[r], Qn[items[r]] @ Pn[u], rtol=1e-5, atol=1e-6)
    raw, _ = m.recommend_diverse(ds, users=[3], k=K, pool=POOL, lam=0.5, rel_norm="none", metric="dot")
    assert raw.shape == (1, K)


def test_neumf_has_no_item_similarity(acf):
    neumf = importlib.import_module(PKG + ".neumf")
    for name in ("recommend_diverse", "diversity", "diversity_tradeoff"):
        with pytest.raises(NotImplementedError):
            getattr(neumf.NeuMF, name)(None, None)


def test_cli_writes_diverse_file(acf, tmp_path, monkeypatch):
    cli = importlib.import_module(PKG + ".cli")
    monkeypatch.chdir(tmp_path)
    rc = cli.main(["--path", str(tmp_path) + "/", "--opath", "t/", "--dataset", "synthetic:300:200:8000", "--model", "bpr",
                   "--epochs", "1", "--verbose", "1", "--embed_size", "8", "--eval_mode", "all", "--topk", "5",
                   "--diverse_lambda", "1,0.5", "--diverse_pool", "20", "--diverse_metric", "euclid"])
    assert rc == 0
    files = glob.glob(str(tmp_path / "out" / "t" / "*.diverse"))
    assert len(files) == 1
    rows = cli.read_diverse(files[0])
    assert [(r[0], r[1]) for r in rows] == [(1.0, 5), (0.5, 5)]
    assert all(math.isfinite(x) for r in rows for x in r[2:])
