"""Nearest-neighbour lists on the GPU (ops.neighbors_topk, acf_neighbors_topk): ids
equal and score BITS equal to the numpy yardstick of nbr_ref.py for the dot,
cosine and Euclidean metrics.  No tolerances anywhere.  The shapes are the
smallest at which each piece can go wrong: a partial last step (300 rows against
256 candidates a step), a partial last row tile (17 queries against 8 a
workgroup), more than one strip (so the merge kernel runs), K = 1 / 10 / 128."""
import functools
import glob
import importlib
import os

import numpy as np
import pytest
import torch

import nbr_ref
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
METRICS = nbr_ref.METRICS


def run(ops, dev, T, queries, k, metric, X=None, num_cand=None, exclude_self=True, lists=None, check=True):
    off = flat = None
    if lists is not None:
        off, flat = nbr_ref.csr(lists)
    tT = torch.tensor(T, device=dev)
    tX = None if X is None else torch.tensor(X, device=dev)
    it, sc = ops.neighbors_topk(tT, torch.tensor(np.asarray(queries, np.int32), device=dev), k, metric, X=tX,
                                num_candidates=num_cand, exclude_self=exclude_self, excl_off=off, excl_items=flat,
                                check=check)
    assert it.dtype == torch.int32 and sc.dtype == torch.float32 and tuple(it.shape) == (len(queries), k)
    return it, sc


def assert_same(got, want):
    """torch (items, scores) against the reference's numpy pair: ids and score bits."""
    wi, ws = torch.from_numpy(np.array(want[0])), torch.from_numpy(np.array(want[1]))  # copies: the cache is read-only
    assert torch.equal(got[0].cpu(), wi)
    assert torch.equal(got[1].cpu().view(torch.int32), ws.view(torch.int32))


def strips(ops, n, c, k):
    """S of the call's strip cut, from the workspace query: 16-byte head, n * S * k keys, c norms."""
    lists = ops.neighbors_topk_workspace(n, c, k) - 16 - 4 * c
    assert lists % (n * k * 8) == 0
    return lists // (n * k * 8)


# ---- 1. metrics x dims ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case(d, metric):
    """300 x d, 17 queries (permuted, one repeated); rows 280.. are exact or
    (1 +- 1e-7) near-copies of rows 0..19, so ties and near ties reach the lists.
    The reference at K = 128, computed once: a shorter list is its prefix."""
    rng = np.random.default_rng(200 + d)
    T = rng.standard_normal((300, d)).astype(np.float32)
    for j in range(20):
        T[280 + j] = T[j] * np.float32(1 + (j % 5 - 2) * 1e-7) if j % 3 else T[j]
    q = np.concatenate([rng.permutation(300)[:14], [0, 3, 3]]).astype(np.int32)
    want = nbr_ref.nbr_reference(T, None, q, metric, 128)
    for a in want:
        a.setflags(write=False)
    return T, q, want


@pytest.mark.parametrize("K", [1, 10, 128])
@pytest.mark.parametrize("d", [4, 64, 128])
@pytest.mark.parametrize("metric", METRICS)
def test_metrics_and_dims(ops, dev, metric, d, K):
    T, q, want = small_case(d, metric)
    assert_same(run(ops, dev, T, q, K, metric), (want[0][:, :K], want[1][:, :K]))
    assert not (want[0] == q[:, None]).any()  # no query is its own neighbour


# ---- 2. self-exclusion and exclusion lists ----------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_self_and_lists(ops, dev, metric):
    rng = np.random.default_rng(21)
    T = rng.standard_normal((300, 16)).astype(np.float32)
    q = np.array([5, 299, 5, 0, 256, 5, 255, 17, 100], np.int32)
    K = 20
    for self_ in (True, False):
        got = run(ops, dev, T, q, K, metric, exclude_self=self_)
        assert_same(got, nbr_ref.nbr_reference(T, None, q, metric, K, exclude_self=self_))
        it = got[0].cpu().numpy()
        has_self = (it == q[:, None]).any(axis=1)
        assert not has_self.any() if self_ else (has_self.all() or metric == "dot")  # cosine 1 / distance 0 lead
        for g in got:  # the query repeated three times: three identical lists
            g = g.cpu().view(torch.int32)
            assert torch.equal(g[0], g[2]) and torch.equal(g[0], g[5])
    # lists that take some of each query's true best away: unsorted, repeated, -1 and out-of-range entries
    best = nbr_ref.nbr_reference(T, None, q, metric, 12)[0]
    clean = [np.unique(np.concatenate([b[::2], rng.integers(0, 300, 10)])).astype(np.int32) for b in best]
    messy = [rng.permutation(np.concatenate([x, x[:4], x[:1], [-1, -1, 300, 301, 2**31 - 1, -2**31]])).astype(np.int32)
             for x in clean]
    for self_ in (True, False):
        want = nbr_ref.nbr_reference(T, None, q, metric, K, exclude_self=self_, lists=clean)
        assert_same(run(ops, dev, T, q, K, metric, exclude_self=self_, lists=clean), want)
        assert_same(run(ops, dev, T, q, K, metric, exclude_self=self_, lists=messy), want)
    # another query table: "self" is just the candidate with the query's id
    X = rng.standard_normal((40, 16)).astype(np.float32)
    qx = np.array([39, 0, 7, 7], np.int32)
    for self_ in (True, False):
        assert_same(run(ops, dev, T, qx, K, metric, X=X, exclude_self=self_),
                    nbr_ref.nbr_reference(T, X, qx, metric, K, exclude_self=self_))


# ---- 3. ties ---------------------------------------------------------------------------
def test_ties_go_to_the_lower_id(ops, dev):
    """Rows 100..355 are one vector v and row 7 is 2 v: under cosine all of them tie
    with equal bits (2 v scales s, nb and den by exact powers of two), more than K =
    128 of them, so the list is the lowest ids; under Euclid the copies are at +0.0."""
    rng = np.random.default_rng(3)
    T = rng.standard_normal((600, 8)).astype(np.float32)
    v = rng.standard_normal(8).astype(np.float32)
    T[100:356] = v
    T[7] = v * np.float32(2)
    K = 128
    it, sc = run(ops, dev, T, [100], K, "cosine")
    assert_same((it, sc), nbr_ref.nbr_reference(T, None, [100], "cosine", K))
    np.testing.assert_array_equal(it.cpu().numpy()[0], np.r_[7, 101:228])
    bits = sc.cpu().view(torch.int32).numpy()[0]
    assert (bits == bits[0]).all()
    it, sc = run(ops, dev, T, [100], K, "euclid")
    assert_same((it, sc), nbr_ref.nbr_reference(T, None, [100], "euclid", K))
    np.testing.assert_array_equal(it.cpu().numpy()[0], np.arange(101, 229))
    assert (sc.cpu().view(torch.int32).numpy() == 0).all()  # +0.0: not one sign bit
    it, sc = run(ops, dev, T, [100], 10, "euclid", exclude_self=False)
    np.testing.assert_array_equal(it.cpu().numpy()[0], np.arange(100, 110))
    assert (sc.cpu().view(torch.int32).numpy() == 0).all()


# ---- 4. zero and tiny rows ----------------------------------------------------------------
def test_zero_and_tiny_rows(ops, dev):
    """Cosine.  Row 3 is zero (as a candidate and as a query); rows 20 / 21 are v
    scaled by 1e-22 and by -1e16 (their cosine is about -1: both norms scale
    along); rows 22 / 23 hold 1e-22 against -1e-22 next to 1e16 components that do
    not meet, so s = -1e-44 over den = 1e32 underflows on the negative side and is
    stored as +0.0.  All of these +0.0 scores sort by id."""
    rng = np.random.default_rng(4)
    d = 8
    T = rng.standard_normal((40, d)).astype(np.float32)
    v = rng.standard_normal(d).astype(np.float32)
    T[3] = 0
    T[20] = v * np.float32(1e-22)
    T[21] = v * np.float32(-1e16)
    T[22] = 0
    T[22, :2] = [1e-22, 1e16]
    T[23] = 0
    T[23, [0, 2]] = [-1e-22, 1e16]
    q = np.array([3, 22, 20, 0, 23], np.int32)
    K = 39
    want = nbr_ref.nbr_reference(T, None, q, "cosine", K)
    s = nbr_ref.seq_dot(T[22:23], T[23:24])[0, 0]
    with np.errstate(all="ignore"):
        raw = s / (nbr_ref.row_norms(T[22:23]) * nbr_ref.row_norms(T[23:24]))[0]
    assert s < 0 and raw == 0 and np.signbit(raw)  # the case is what it claims
    got = run(ops, dev, T, q, K, "cosine")
    assert_same(got, want)
    it, sc = got[0].cpu().numpy(), got[1].cpu().numpy()
    bits = sc.view(np.uint32)
    np.testing.assert_array_equal(it[0], np.delete(np.arange(40), 3))  # a zero query: all +0.0, by id
    assert (bits[0] == 0).all()
    assert bits[1][it[1] == 23] == 0 and bits[4][it[4] == 22] == 0       # the underflowed pair: +0.0
    assert bits[3][it[3] == 3] == 0                                      # a zero candidate: +0.0
    assert not (bits == 0x80000000).any()
    for r in range(len(q)):  # the +0.0 scores of a row are consecutive and ascending in id
        z = it[r][bits[r] == 0]
        assert (np.diff(z) > 0).all()
    assert sc[2][it[2] == 21] < -0.9  # about -1: the 1e-22 row's squares are a few dozen denormal steps
    # dot and Euclid stay exact on the same rows
    for metric in ("dot", "euclid"):
        assert_same(run(ops, dev, T, q, K, metric), nbr_ref.nbr_reference(T, None, q, metric, K))


# ---- 5. short lists ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_short_lists(ops, dev, metric):
    T, q, _ = small_case(64, metric)
    it, sc = run(ops, dev, T, q, 10, metric, num_cand=5)
    assert_same((it, sc), nbr_ref.nbr_reference(T, None, q, metric, 10, num_cand=5))
    it, sc = it.cpu().numpy(), sc.cpu().numpy()
    n = np.where(q < 5, 4, 5)  # a query below 5 loses itself
    for r in range(len(q)):
        assert (it[r, :n[r]] >= 0).all() and (it[r, n[r]:] == -1).all() and np.isneginf(sc[r, n[r]:]).all()
    it, sc = run(ops, dev, T, q, 128, metric, num_cand=200)
    assert_same((it, sc), nbr_ref.nbr_reference(T, None, q, metric, 128, num_cand=200))
    assert int(it.max()) < 200 and int(it.min()) >= 0
    it, sc = run(ops, dev, T, q, 3, metric, num_cand=0)
    assert (it.cpu().numpy() == -1).all() and np.isneginf(sc.cpu().numpy()).all()
    it, sc = run(ops, dev, T, np.zeros(0, np.int32), 3, metric)
    assert tuple(it.shape) == (0, 3) and tuple(sc.shape) == (0, 3)


# ---- 6. several strips: the merge kernel ---------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_several_strips(ops, dev, metric):
    n, rows, d, K = 3, 40_000, 16, 100
    assert strips(ops, n, rows, K) > 1
    rng = np.random.default_rng(6)
    T = rng.integers(-2, 3, (rows, d)).astype(np.float32)  # integer rows: ties across the strips
    q = np.array([39_999, 0, 20_000], np.int32)
    a = run(ops, dev, T, q, K, metric)
    b = run(ops, dev, T, q, K, metric)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert_same(a, nbr_ref.nbr_reference(T, None, q, metric, K))


# ---- 7. cross-checks against the top-K kernel ---------------------------------------------------------
def test_dot_is_recommend_topk(ops, dev):
    rng = np.random.default_rng(7)
    T = torch.tensor(rng.standard_normal((700, 64)).astype(np.float32), device=dev)
    P = torch.tensor(rng.standard_normal((90, 64)).astype(np.float32), device=dev)
    q = torch.tensor(rng.permutation(700)[:33].astype(np.int32), device=dev)
    u = torch.tensor(rng.permutation(90)[:33].astype(np.int32), device=dev)
    for K in (1, 100):
        a = ops.neighbors_topk(T, q, K, "dot", exclude_self=False)
        b = ops.recommend_topk(T, T, q, K)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        a = ops.neighbors_topk(T, u, K, "dot", X=P, num_candidates=677, exclude_self=False)
        b = ops.recommend_topk(P, T, u, K, 677)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- 8. errors -------------------------------------------------------------------------------------
def test_errors(ops, dev):
    native = importlib.import_module(PKG + "._native")
    rng = np.random.default_rng(8)
    Tn = rng.standard_normal((50, 8)).astype(np.float32)
    T = torch.tensor(Tn, device=dev)
    q = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=dev)
    it = torch.full((4, 3), 7, dtype=torch.int32, device=dev)
    sc = torch.full((4, 3), 7.0, dtype=torch.float32, device=dev)
    need = ops.neighbors_topk_workspace(4, 50, 3)
    work = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)

    def call(metric, nbytes, k=3):
        native.call("acf_neighbors_topk", T.data_ptr(), 50, 8, T.data_ptr(), 50, q.data_ptr(), 4, 50, metric, 1,
                    None, None, k, it.data_ptr(), sc.data_ptr(), work.data_ptr(), nbytes, 1, None)

    for args, msg in (((1, need - 8), "workspace too small"), ((0, 8), "workspace too small"), ((3, need), "metric"),
                      ((-1, need), "metric"), ((1, need, 0), "k must be"), ((1, need, 129), "k must be")):
        with pytest.raises(native.NativeError, match=msg) as e:
            call(*args)
        assert e.value.code == native.ACF_E_INVALID
    torch.cuda.synchronize()
    assert (it == 7).all() and (sc == 7.0).all()  # refused before any launch
    call(1, need)
    torch.cuda.synchronize()
    assert_same((it, sc), nbr_ref.nbr_reference(Tn, None, [1, 2, 3, 4], "cosine", 3))
    # a query outside the table
    for bad in ([0, 50], [-1]):
        for metric in METRICS:
            with pytest.raises(native.NativeIndexError):
                ops.neighbors_topk(T, torch.tensor(bad, dtype=torch.int32, device=dev), 3, metric)
            got = ops.neighbors_topk(T, torch.tensor(bad, dtype=torch.int32, device=dev), 3, metric, check=False)
            assert_same(got, nbr_ref.nbr_reference(Tn, None, bad, metric, 3))  # read as row 0
    with pytest.raises(ValueError):
        ops.neighbors_topk(T, q, 3, num_candidates=51)
    with pytest.raises(ValueError):
        ops.neighbors_topk(T, q, 3, X=torch.zeros(4, 16, device=dev))
    with pytest.raises(ValueError):
        ops.neighbors_topk(T, q, 3, excl_off=np.zeros(2, np.int64), excl_items=np.zeros(0, np.int32))


# ---- 9. model layer and CLI -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def video(acf, tmp_path_factory):
    z = np.load(os.path.join(GOLDEN, "video_data.npz"))
    d = tmp_path_factory.mktemp("data")
    with open(d / "Video.train.rating", "w") as f:
        for a, b, r in zip(z["train_u"], z["train_i"], z["train_r"]):
            f.write(f"{a}\t{b}\t{r}\t1\n")
    with open(d / "Video.test.rating", "w") as f:
        for a, b in zip(z["test_u"], z["test_i"]):
            f.write(f"{a}\t{b}\t1\t1\n")
    return acf.OriginalDataset(str(d / "Video"))


def test_model_layer_on_video(acf, ops, video, dev):
    from argparse import Namespace
    ev = importlib.import_module(PKG + ".evaluate")
    ds = video
    args = Namespace(embed_size=32, lr=0.05, reg=0.0, dns=1, adv="grad", eps=0.5, adver=0, reg_adv=1.0,
                     epochs=1, seed=11)
    m = acf.MF(ds.num_users, ds.num_items, args).build_graph(device=dev)
    I, U = ds.num_items, ds.num_users
    assert m.embedding_Q.shape[0] == I + 1 and m.embedding_P.shape[0] == U + 1
    with torch.no_grad():  # the padding rows would be everybody's nearest neighbour if they were candidates
        m.embedding_Q[I] = 0
        m.embedding_P[U] = 0
    rng = np.random.default_rng(9)
    items = np.concatenate([rng.permutation(I)[:50], [I - 1, 0]])
    K = 20
    for metric in METRICS:
        ids, scores = m.similar_items(items, K, metric=metric)
        assert ids.shape == (52, K) and ids.dtype == np.int32 and scores.dtype == np.float32
        assert (ids >= 0).all() and (ids < I).all() and not (ids == items[:, None]).any()
        assert (np.diff(scores, axis=1) <= 0).all()
        it, sc = ops.neighbors_topk(m.embedding_Q[:I].contiguous(), items.astype(np.int32), K, metric)
        np.testing.assert_array_equal(ids, it.cpu().numpy())
        np.testing.assert_array_equal(scores.view(np.uint32), sc.cpu().numpy().view(np.uint32))
    # under Euclid the zero padding row would be near these small rows: it is no candidate
    ids, _ = ev.similar_items(m, items, K, "euclid", num_candidates=I + 1)
    assert (ids == I).any()
    ids, _ = ev.similar_items(m, items, K, "euclid")
    assert not (ids == I).any()
    # users: the same through every layer
    users = rng.permutation(U)[:30]
    ids, scores = m.similar_users(users, K)
    it, sc = ops.neighbors_topk(m.embedding_P[:U].contiguous(), users.astype(np.int32), K, "cosine")
    np.testing.assert_array_equal(ids, it.cpu().numpy())
    np.testing.assert_array_equal(scores.view(np.uint32), sc.cpu().numpy().view(np.uint32))
    assert not (ids == users[:, None]).any()
    r = acf.APR(U, I, 32, seed=11, device=dev)
    r.build_graph()
    r.model.load_embeddings(m.embedding_P.cpu(), m.embedding_Q.cpu())
    np.testing.assert_array_equal(r.similar_users(users, K)[0], ids)
    np.testing.assert_array_equal(r.similar_items(items, K, metric="dot")[0], m.similar_items(items, K, "dot")[0])
    # rows: other rows against the user table, nothing self-excluded
    rows = m.embedding_P[users[:6]].contiguous()
    ids, scores = m.similar_users(np.arange(6), 5, rows=rows)
    np.testing.assert_array_equal(ids[:, 0], users[:6])  # copies of users: each finds its original first
    f = m.fold_in([ds.trainList[u][:20] for u in range(4)], epochs=2)
    ids, scores = m.similar_users(np.arange(len(f)), 7, rows=f)
    it, sc = ops.neighbors_topk(m.embedding_P, np.arange(len(f), dtype=np.int32), 7, "cosine", X=f.P,
                                num_candidates=U, exclude_self=False)
    np.testing.assert_array_equal(ids, it.cpu().numpy())
    np.testing.assert_array_equal(scores.view(np.uint32), sc.cpu().numpy().view(np.uint32))
    assert (ids >= 0).all() and (ids < U).all()


def test_cli_writes_similar_file(acf, tmp_path, monkeypatch):
    cli = importlib.import_module(PKG + ".cli")
    ev = importlib.import_module(PKG + ".evaluate")
    seen = {}
    real = ev.similar_items

    def spy(model, items, k=10, metric="cosine", num_candidates=None):
        out = real(model, items, k=k, metric=metric, num_candidates=num_candidates)
        seen.update(model=model, items=list(items), k=k, metric=metric, ids=out[0])
        return out

    monkeypatch.setattr(ev, "similar_items", spy)
    monkeypatch.chdir(tmp_path)
    query = [7, 0, 199, 7, 42]
    (tmp_path / "ids.txt").write_text("".join("%d\n" % i for i in query))
    rc = cli.main(["--path", str(tmp_path) + "/", "--opath", "t/", "--dataset", "synthetic:300:200:8000", "--model",
                   "bpr", "--epochs", "1", "--verbose", "1", "--embed_size", "16", "--eval_mode", "all", "--topk",
                   "5", "--similar", str(tmp_path / "ids.txt"), "--similar_metric", "euclid"])
    assert rc == 0
    files = glob.glob(str(tmp_path / "out" / "t" / "*.similar"))
    assert len(files) == 1
    ids = cli.read_topk(files[0])
    assert seen["items"] == query and seen["k"] == 5 and seen["metric"] == "euclid"
    np.testing.assert_array_equal(ids, seen["ids"])  # the file parses back to the ids
    m = seen["model"]
    it, _ = importlib.import_module(PKG + ".ops").neighbors_topk(
        m.embedding_Q[:m.num_items].contiguous(), np.asarray(query, np.int32), 5, "euclid")
    np.testing.assert_array_equal(ids, it.cpu().numpy())
    assert ids.shape == (5, 5) and (ids >= 0).all() and (ids < 200).all()
    assert not (ids == np.asarray(query)[:, None]).any()
    np.testing.assert_array_equal(ids[0], ids[3])
