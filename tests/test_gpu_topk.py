"""Top-K recommendation lists on the GPU (ops.recommend_topk, acf_recommend_topk):
items equal and scores BIT-equal to a numpy restatement, for the MFMA sweep, the
VALU sweep and auto alike.  No tolerances anywhere.

Reference (this file, numpy): the score is the sequential product-round then
add-round chain in f32 (seq_dot's bits), the order np.lexsort((ids, -score)) per
user after masking the exclusion SET."""
import functools
import glob
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
KERNELS = ("auto", "mfma", "valu")


def ref_scores(P, Q, users):
    """[n, I] f32: s = s + P[u][:, k] * Q[:, k] for k in order (each op rounds to f32)."""
    Pu = P[users]
    s = np.zeros((len(users), Q.shape[0]), np.float32)
    for k in range(P.shape[1]):
        s = s + Pu[:, k, None] * Q[None, :, k]
    return s


def ref_topk(scores, num_cand, lists, K):
    n = scores.shape[0]
    items = np.full((n, K), -1, np.int32)
    out = np.full((n, K), -np.inf, np.float32)
    for j in range(n):
        keep = np.ones(num_cand, bool)
        ex = np.asarray(lists[j], np.int64)
        keep[ex[(ex >= 0) & (ex < num_cand)]] = False
        ids = np.nonzero(keep)[0]
        s = scores[j, ids]
        sel = ids[np.lexsort((ids, -s))][:K]
        items[j, :len(sel)] = sel
        out[j, :len(sel)] = scores[j, sel]
    return items, out


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return off, flat.astype(np.int32)


def run(ops, dev, P, Q, users, K, num_cand, lists, kernel):
    off, flat = csr(lists)
    it, sc = ops.recommend_topk(torch.tensor(P, device=dev), torch.tensor(Q, device=dev),
                                torch.tensor(users, device=dev), K, num_cand, off, flat, kernel=kernel)
    assert it.dtype == torch.int32 and sc.dtype == torch.float32 and tuple(it.shape) == (len(users), K)
    return it.cpu().numpy(), sc.cpu().numpy()


def assert_same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))  # bit-equal


# ---- ragged tiles with near ties ------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_case(d):
    """U1 = 150, I1 = 700, 133 users (permuted, 3 repeated), 677 candidates: ragged
    against the 64 x 128 tiling.  Rows 600.. of Q are exact or (1 +- 1e-7..2e-7)
    near-copies of rows 0..99, so ties and error-band cases reach most top-K lists."""
    rng = np.random.default_rng(100 + d)
    U1, I1, num_cand = 150, 700, 677
    P = rng.standard_normal((U1, d)).astype(np.float32)
    Q = rng.standard_normal((I1, d)).astype(np.float32)
    for k in range(100):
        Q[600 + k] = Q[k] * np.float32(1 + (k % 5 - 2) * 1e-7) if k % 3 else Q[k]
    users = rng.permutation(U1)[:130].astype(np.int32)
    users = np.concatenate([users, users[[5, 5, 77]]])
    lists = [rng.integers(0, num_cand, 20).astype(np.int32) for _ in users]
    scores = ref_scores(P, Q, users)
    scores.setflags(write=False)
    return P, Q, users, num_cand, lists, scores


@pytest.mark.parametrize("K", [1, 10, 100, 128])
@pytest.mark.parametrize("d", [16, 64, 100, 256])
def test_ragged_tiles_with_near_ties(ops, dev, d, K):
    P, Q, users, num_cand, lists, scores = ragged_case(d)
    want = ref_topk(scores, num_cand, lists, K)
    got = {kern: run(ops, dev, P, Q, users, K, num_cand, lists, kern) for kern in KERNELS}
    for kern in KERNELS:
        assert_same(got[kern], want)
    assert_same(got["mfma"], got["valu"])
    assert_same(got["auto"], got["mfma"])
    if K == 100 and d == 64:  # the case is what it claims: exact ties inside the lists
        s = want[1]
        assert (s[:, 1:] == s[:, :-1]).any()


# ---- all ties: the admission buffer's worst case ---------------------------------
def test_all_ties(ops, dev):
    rng = np.random.default_rng(3)
    n, I1, d, K = 40, 1000, 16, 10
    P = rng.standard_normal((n, d)).astype(np.float32)
    Q = np.repeat(rng.standard_normal((1, d)).astype(np.float32), I1, axis=0)
    users = np.arange(n, dtype=np.int32)
    lists = [rng.integers(0, 30, 8).astype(np.int32) for _ in users]  # among the lowest ids
    want_items = np.stack([np.setdiff1d(np.arange(I1), x)[:K] for x in lists]).astype(np.int32)
    want = ref_topk(ref_scores(P, Q, users), I1, lists, K)
    np.testing.assert_array_equal(want[0], want_items)
    for kern in KERNELS:
        assert_same(run(ops, dev, P, Q, users, K, I1, lists, kern), want)


# ---- integer-valued tables: many exact ties ----------------------------------------
def test_integer_tables(ops, dev):
    rng = np.random.default_rng(4)
    n, I1, d, K = 50, 200, 16, 100
    P = rng.integers(-3, 4, (n, d)).astype(np.float32)
    Q = rng.integers(-3, 4, (I1, d)).astype(np.float32)
    users = rng.permutation(n).astype(np.int32)
    lists = [rng.integers(0, I1, 10).astype(np.int32) for _ in users]
    want = ref_topk(ref_scores(P, Q, users), I1, lists, K)
    assert (want[1][:, 1:] == want[1][:, :-1]).sum() > n  # ties are everywhere
    for kern in KERNELS:
        assert_same(run(ops, dev, P, Q, users, K, I1, lists, kern), want)


# ---- fewer than K candidates ----------------------------------------------------------
@pytest.mark.parametrize("kern", KERNELS)
def test_too_few_candidates(ops, dev, kern):
    rng = np.random.default_rng(5)
    n, I1, d, K = 70, 90, 32, 10
    P = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((I1, d)).astype(np.float32)
    users = np.arange(n, dtype=np.int32)
    lists = [rng.permutation(50)[:45].astype(np.int32) for _ in users]
    scores = ref_scores(P, Q, users)
    want = ref_topk(scores, 50, lists, K)
    assert (want[0][:, :5] >= 0).all() and (want[0][:, 5:] == -1).all() and np.isneginf(want[1][:, 5:]).all()
    assert_same(run(ops, dev, P, Q, users, K, 50, lists, kern), want)
    it, sc = run(ops, dev, P, Q, users, K, 0, [[] for _ in users], kern)
    assert (it == -1).all() and np.isneginf(sc).all()
    it, sc = run(ops, dev, P, Q, users, K, 0, lists, kern)  # lists of items that are no candidates
    assert (it == -1).all() and np.isneginf(sc).all()


# ---- exclusion list shapes --------------------------------------------------------------
def test_exclusion_lists_are_sets(ops, dev):
    """Unsorted, repeated, -1 and >= num_candidates entries: same result as the cleaned lists;
    no exclusion arguments: nothing excluded."""
    rng = np.random.default_rng(6)
    U1, I1, d, K, num_cand = 90, 400, 64, 20, 333
    P = rng.standard_normal((U1, d)).astype(np.float32)
    Q = rng.standard_normal((I1, d)).astype(np.float32)
    users = rng.permutation(U1)[:77].astype(np.int32)
    scores = ref_scores(P, Q, users)
    # exclude some of each user's true best, so that a missed exclusion changes the answer
    best = np.argsort(-scores[:, :num_cand], axis=1, kind="stable")[:, :12]
    clean = [np.unique(np.concatenate([b[::2], rng.integers(0, num_cand, 10)])).astype(np.int32) for b in best]
    messy = [rng.permutation(np.concatenate([x, x[:4], x[:1], [-1, -1, num_cand, I1 - 1, I1 + 5, 2**31 - 1,
                                                                -2**31]])).astype(np.int32)
             for x in clean]
    want = ref_topk(scores, num_cand, clean, K)
    for kern in KERNELS:
        assert_same(run(ops, dev, P, Q, users, K, num_cand, clean, kern), want)
        assert_same(run(ops, dev, P, Q, users, K, num_cand, messy, kern), want)
    none = ref_topk(scores, I1, [[] for _ in users], K)
    for kern in KERNELS:
        it, sc = ops.recommend_topk(torch.tensor(P, device=dev), torch.tensor(Q, device=dev),
                                    torch.tensor(users, device=dev), K, kernel=kern)
        assert_same((it.cpu().numpy(), sc.cpu().numpy()), none)


# ---- several strips per user (the merge), long lists ------------------------------------------
def test_many_strips_merge(ops, dev):
    """Few users and many candidates: the grid is filled with strips of the candidate
    range, and the merge kernel selects from many partial lists (ties across strips)."""
    rng = np.random.default_rng(7)
    n, I1, d, K = 5, 20011, 8, 128
    P = rng.integers(-2, 3, (n, d)).astype(np.float32)
    Q = rng.integers(-2, 3, (I1, d)).astype(np.float32)
    users = np.array([4, 0, 3, 3, 1], np.int32)
    lists = [rng.integers(0, I1, 3000).astype(np.int32) for _ in users]
    want = ref_topk(ref_scores(P, Q, users), I1, lists, K)
    for kern in KERNELS:
        assert_same(run(ops, dev, P, Q, users, K, I1, lists, kern), want)


# ---- cross-check against the ranking op ----------------------------------------------------------
def test_agrees_with_eval_positions(ops, dev):
    """Excluding the train lists only: a test item ranked p < K by eval_positions_all
    (which excludes train + test) with a unique score sits at items[k, p]."""
    rng = np.random.default_rng(8)
    U1, I1, d, K = 200, 500, 64, 50
    P = rng.standard_normal((U1, d)).astype(np.float32)
    Q = rng.standard_normal((I1, d)).astype(np.float32)
    users = rng.permutation(U1)[:160].astype(np.int32)
    scores = ref_scores(P, Q, users)
    tests = np.argsort(-scores, axis=1)[np.arange(len(users)), rng.integers(0, 2 * K, len(users))].astype(np.int32)
    train = [np.setdiff1d(rng.integers(0, I1, 25), [t]).astype(np.int32) for t in tests]
    off, flat = csr(train)
    both = [np.union1d(x, [t]).astype(np.int32) for x, t in zip(train, tests)]
    off2, flat2 = csr(both)
    tP, tQ, tu = torch.tensor(P, device=dev), torch.tensor(Q, device=dev), torch.tensor(users, device=dev)
    pos = ops.eval_positions_all(tP, tQ, tu, torch.tensor(tests, device=dev), I1, off2, flat2).cpu().numpy()
    items = ops.recommend_topk(tP, tQ, tu, K, I1, off, flat)[0].cpu().numpy()
    checked = 0
    for k in range(len(users)):
        unique = (scores[k] == scores[k, tests[k]]).sum() == 1
        if pos[k] < K and unique:
            assert items[k, pos[k]] == tests[k]
            checked += 1
    assert checked > 20


def test_deterministic(ops, dev):
    P, Q, users, num_cand, lists, _ = ragged_case(64)
    for kern in ("mfma", "valu"):
        a = run(ops, dev, P, Q, users, 100, num_cand, lists, kern)
        b = run(ops, dev, P, Q, users, 100, num_cand, lists, kern)
        assert_same(a, b)


def test_torch_op(ops, dev):
    acf_ops = importlib.import_module(PKG + ".torch_ops").load()
    P, Q, users, num_cand, lists, _ = ragged_case(64)
    off, flat = csr(lists)
    tP, tQ, tu = torch.tensor(P, device=dev), torch.tensor(Q, device=dev), torch.tensor(users, device=dev)
    it, sc = acf_ops.recommend_topk(tP, tQ, tu, 10, num_cand, torch.tensor(off, device=dev),
                                    torch.tensor(flat, device=dev))
    want = ops.recommend_topk(tP, tQ, tu, 10, num_cand, off, flat)
    assert torch.equal(it, want[0]) and torch.equal(sc.view(torch.int32), want[1].view(torch.int32))
    with pytest.raises(Exception, match="k must be"):
        acf_ops.recommend_topk(tP, tQ, tu, 129, num_cand, torch.tensor(off, device=dev),
                               torch.tensor(flat, device=dev))
    with pytest.raises(Exception):
        acf_ops.recommend_topk(tP.cpu(), tQ.cpu(), tu.cpu(), 10, num_cand, torch.tensor(off), torch.tensor(flat))


def test_index_and_argument_checks(ops, dev):
    native = importlib.import_module(PKG + "._native")
    P = torch.zeros(10, 8, device=dev)
    Q = torch.zeros(20, 8, device=dev)
    with pytest.raises(native.NativeIndexError):
        ops.recommend_topk(P, Q, torch.tensor([0, 10], dtype=torch.int32, device=dev), 3)
    with pytest.raises(native.NativeIndexError):
        ops.recommend_topk(P, Q, torch.tensor([-1], dtype=torch.int32, device=dev), 3)
    with pytest.raises(ValueError):
        ops.recommend_topk(P, Q, [0], 3, num_candidates=21)
    with pytest.raises(ValueError):
        ops.recommend_topk(P, Q, [0, 1], 3, 20, np.zeros(2, np.int64), np.zeros(0, np.int32))  # excl_off too short
    it, sc = ops.recommend_topk(P, Q, np.zeros(0, np.int32), 3)
    assert tuple(it.shape) == (0, 3) and tuple(sc.shape) == (0, 3)
    # the C entry point refuses a workspace below the queried size
    u = torch.zeros(4, dtype=torch.int32, device=dev)
    off = torch.zeros(5, dtype=torch.int64, device=dev)
    ex = torch.zeros(1, dtype=torch.int32, device=dev)
    it = torch.empty((4, 3), dtype=torch.int32, device=dev)
    sc = torch.empty((4, 3), dtype=torch.float32, device=dev)
    need = ops.recommend_topk_workspace(4, 20, 3)
    work = torch.empty(need // 8, dtype=torch.int64, device=dev)
    with pytest.raises(native.NativeError, match="workspace too small"):
        native.call("acf_recommend_topk", P.data_ptr(), Q.data_ptr(), 10, 20, 8, u.data_ptr(), 4, 20,
                    off.data_ptr(), ex.data_ptr(), 3, it.data_ptr(), sc.data_ptr(), work.data_ptr(), need - 8, 0,
                    None)


# ---- model layer and CLI ---------------------------------------------------------------------------
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
    users = np.random.default_rng(9).permutation(ds.num_users)[:500]
    K = 20
    items, scores = m.recommend(users, K, dataset=ds)
    assert items.shape == (500, K) and items.dtype == np.int32 and scores.dtype == np.float32
    assert (items >= 0).all() and (items < ds.num_items).all()
    for u, row in zip(users.tolist(), items):
        assert not set(row.tolist()) & set(ds.trainList[u]), u
        assert len(set(row.tolist())) == K
    assert (np.diff(scores, axis=1) <= 0).all()
    off, flat = ev.train_exclusions(ds, users)
    it, sc = ops.recommend_topk(m.embedding_P, m.embedding_Q, users.astype(np.int32), K, ds.num_items, off, flat)
    np.testing.assert_array_equal(items, it.cpu().numpy())
    np.testing.assert_array_equal(scores.view(np.uint32), sc.cpu().numpy().view(np.uint32))
    # without a dataset every item row is a candidate
    allrows, _ = m.recommend(users[:10], K)
    assert allrows.shape == (10, K)
    # the Recommender wrapper: the same tables, the exclusions from a train matrix
    r = acf.APR(ds.num_users, ds.num_items, 32, seed=11, device=dev)
    r.build_graph()
    r.model.load_embeddings(m.embedding_P.cpu(), m.embedding_Q.cpu())
    got, got_scores = r.recommend(users, K, train=ds.trainMatrix)
    coo = ds.trainMatrix.tocoo()
    by_user = {}
    for u, i in zip(coo.row.tolist(), coo.col.tolist()):
        by_user.setdefault(u, []).append(i)
    lists = [by_user.get(u, []) for u in users.tolist()]
    for row, ex in zip(got, lists):
        assert not set(row.tolist()) & set(ex)
    off, flat = csr(lists)
    it, sc = ops.recommend_topk(m.embedding_P, m.embedding_Q, users.astype(np.int32), K, ds.num_items, off, flat)
    np.testing.assert_array_equal(got, it.cpu().numpy())
    np.testing.assert_array_equal(got_scores.view(np.uint32), sc.cpu().numpy().view(np.uint32))


def test_cli_writes_topk_file(acf, tmp_path, monkeypatch):
    cli = importlib.import_module(PKG + ".cli")
    data = importlib.import_module(PKG + ".data")
    monkeypatch.chdir(tmp_path)
    name = "synthetic:300:200:8000"
    rc = cli.main(["--path", str(tmp_path) + "/", "--opath", "t/", "--dataset", name, "--model", "bpr",
                   "--epochs", "1", "--verbose", "1", "--embed_size", "16", "--eval_mode", "all", "--topk", "5"])
    assert rc == 0
    files = glob.glob(str(tmp_path / "out" / "t" / "*.topk"))
    assert len(files) == 1
    items = cli.read_topk(files[0])
    ds = data.get_dataset(name, seed=2019)  # the CLI's dataset (seeded)
    assert items.shape == (ds.num_users, 5)
    assert (items >= 0).all() and (items < ds.num_items).all()
    for u in range(ds.num_users):
        assert not set(items[u].tolist()) & set(ds.trainList[u])
