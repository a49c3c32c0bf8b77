"""The GPU epoch sampler (k_perm_keys, the 64-bit radix sort, k_negatives;
ops.sample_epoch, DeviceSampler) against its numpy restatement
(tests/sampler_ref.py): all three outputs equal, element for element, no
tolerance.  What the restatement's streams look like statistically is checked on
the CPU in tests/test_sampler_host.py."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import sampler_ref as ref
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu


def _gpu_epoch(ops, dev, pu, pi, B, num_items, off, items, seed, max_tries=1 << 20, check=True, alias=None):
    tab = None if alias is None else (torch.tensor(alias[0], device=dev), torch.tensor(alias[1], device=dev))
    out = ops.sample_epoch(torch.tensor(np.asarray(pu, np.int32), device=dev),
                           torch.tensor(np.asarray(pi, np.int32), device=dev), B, num_items,
                           torch.tensor(np.asarray(off, np.int64), device=dev),
                           torch.tensor(np.asarray(items, np.int32), device=dev), seed, max_tries=max_tries,
                           check=check, alias=tab)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want):
    for name, g, w in zip(("user", "item_pos", "item_neg"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)


# ---------------------------------------------------------------------------
# sizes: empty epoch, exact multiple, a tail that is shuffled in but dropped
# ---------------------------------------------------------------------------
SIZES = [(B, n) for B in (1, 64, 100) for n in (B - 1, B, B + 1, 3 * B + 7)] + [(512, 70_001)]


def _small_lists(rng, num_users, num_items, most):
    rows = [np.sort(rng.choice(num_items, size=int(rng.integers(0, most + 1)), replace=False)) for _ in range(num_users)]
    off = np.zeros(num_users + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, np.concatenate(rows).astype(np.int32)


@pytest.mark.parametrize("B,n_pos", SIZES)
def test_epoch_equals_restatement_at_every_size(ops, dev, B, n_pos):
    """n_pos = 70,001 takes the radix sort over more than one block."""
    rng = np.random.default_rng(n_pos * 131 + B)
    off, items = _small_lists(rng, 7, 40, 12)
    pu = rng.integers(0, 7, n_pos).astype(np.int32)
    pi = rng.integers(0, 40, n_pos).astype(np.int32)
    seed = ref.device_seed(B, n_pos)
    want = ref.sample_epoch(pu, pi, B, 40, off, items, seed)
    assert want[3] == 0 and len(want[0]) == (n_pos // B) * B
    _same(_gpu_epoch(ops, dev, pu, pi, B, 40, off, items, seed), want[:3])


# ---------------------------------------------------------------------------
# list edges x proposal tables
# ---------------------------------------------------------------------------
EDGE_N_POS, EDGE_B = 523, 100  # n_out = 500: two blocks, the second partial


def _weights(num_items, table):
    if table == "uniform":
        return None
    if table == "equal":
        return np.ones(num_items, np.float32)
    w = (np.random.default_rng(0).gamma(0.7, size=num_items) + 0.01).astype(np.float32)  # test_gpu_sampler's
    if table == "zeros":
        w[np.arange(num_items) % 3 == 1] = 0
    return w


def _hole(num_items):
    """The one item the all-but-one user may draw: the heaviest of the gamma
    weights that the zero-weight table keeps, so every table reaches it within
    max_tries (uniform: 1/num_items per draw, 2^20 tries = 16 num_items at 65,537)."""
    return int(np.argmax(_weights(num_items, "zeros")))


def edge_lists(num_items):
    """(kind -> user id, list_off, list_items): the users of the issue, lists sorted,
    packed so that each list's ends touch a neighbour's."""
    everything = np.arange(num_items, dtype=np.int32)
    rows = {"empty": everything[:0]}
    if num_items >= 2:
        rows["first"] = everything[:1]
        rows["last"] = everything[-1:]
    if num_items >= 40:
        rows["all_but_one"] = np.delete(everything, _hole(num_items))
        n_long = 1500 if num_items > 2000 else num_items // 2
        rows["long"] = np.sort(np.random.default_rng(num_items).choice(num_items, n_long, replace=False)).astype(np.int32)
    order = [k for k in ("long", "first", "empty", "all_but_one", "last") if k in rows]
    ids = {k: n for n, k in enumerate(order)}
    lens = [len(rows[k]) for k in order] + [0]  # a trailing user with an empty list
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return ids, off, np.concatenate([rows[k] for k in order]).astype(np.int32)


def edge_case(num_items, kind, seed):
    """Pairs whose epoch has `kind` at x = 0 and at x = n_out - 1 (and the
    all-but-one user, whose draws are long, at x = 1 and n_out - 2 only)."""
    ids, off, items = edge_lists(num_items)
    rng = np.random.default_rng(num_items + 7 * len(kind))
    cheap = [v for k, v in ids.items() if k != "all_but_one"]
    pu = rng.choice(cheap, EDGE_N_POS).astype(np.int32)
    pi = rng.integers(0, num_items, EDGE_N_POS).astype(np.int32)
    perm = ref.epoch_perm(EDGE_N_POS, seed)
    n_out = (EDGE_N_POS // EDGE_B) * EDGE_B
    if "all_but_one" in ids:
        pu[perm[[1, n_out - 2]]] = ids["all_but_one"]
    pu[perm[[0, n_out - 1]]] = ids[kind]
    return pu, pi, off, items, ids


# a one-item table with a zero weight would be all zero, which alias_table refuses
EDGE_CASES = [(n, t) for n in (1, 2, 40, 65_537) for t in ("uniform", "gamma", "zeros", "equal")
              if (n, t) != (1, "zeros")]


@pytest.mark.parametrize("num_items,table", EDGE_CASES)
def test_list_edges_equal_restatement(ops, dev, num_items, table):
    """num_items = 2 under the table with a zero weight leaves the owner of item
    0 nothing to draw (item 1 weighs 0): that case compares the -1s instead."""
    w = _weights(num_items, table)
    alias = None if w is None else ops.alias_table(w)
    max_tries = 1 << 20 if num_items > 40 else 4096
    seed = ref.device_seed(5, num_items % 11)
    ids = edge_lists(num_items)[0]
    for kind in ids:
        pu, pi, off, items, _ = edge_case(num_items, kind, seed)
        want = ref.sample_epoch(pu, pi, EDGE_B, num_items, off, items, seed, max_tries, alias)
        assert want[0][0] == ids[kind] and want[0][-1] == ids[kind]
        stuck = table == "zeros" and num_items == 2
        assert want[3] == (2 if stuck else 0), kind
        if not stuck:
            assert want[2].min() >= 0
        if table == "equal":  # every column keeps itself: the uniform path, draw for draw
            np.testing.assert_array_equal(want[2], ref.sample_epoch(pu, pi, EDGE_B, num_items, off, items, seed,
                                                                    max_tries)[2])
        got = _gpu_epoch(ops, dev, pu, pi, EDGE_B, num_items, off, items, seed, max_tries, check=not stuck,
                         alias=alias)
        _same(got, want[:3])


def test_alias_compare_at_its_edge(ops, dev):
    """`r >= prob[j]` where r == prob[j] exactly, which chance reaches once in 2^24
    draws: the seed is solved for (sampler_ref.seed_for_word) so that the first
    attempt at x = 0, or at x = n_out - 1, hashes to a chosen word.  A
    zero-weight column (prob 0) at r = 0 must yield its alias, never itself; a
    column with prob 0.5 yields its alias at 0x800000 * 2^-24 and itself one
    step below; a column with prob 1 keeps itself at the largest r."""
    w = np.array([1, 3, 0, 4], np.float32)
    prob, alias = ops.alias_table(w)
    np.testing.assert_array_equal(prob, np.array([0.5, 1.0, 0.0, 0.5], np.float32))
    np.testing.assert_array_equal(alias, [3, 1, 3, 1])
    n_pos, B = 300, 100
    pu, pi = np.zeros(n_pos, np.int32), np.arange(n_pos, dtype=np.int32) % 4
    off, items = np.zeros(2, np.int64), np.zeros(0, np.int32)
    middle = 0x2545F491 << 24  # bits 24..55: neither the column nor r reads them
    for word, yields in (((2 << 62) | middle, 3), ((2 << 62) | middle | 1, 3), (middle | 0x800000, 3),
                         (middle | 0x7FFFFF, 0), (middle | 0x800001, 3), ((1 << 62) | middle | 0xFFFFFF, 1),
                         ((3 << 62) | middle | 0x800000, 1), ((3 << 62) | middle | 0x7FFFFF, 3)):
        for x in (0, n_pos - 1):
            seed = ref.seed_for_word(word, x)
            want = ref.sample_epoch(pu, pi, B, 4, off, items, seed, alias=(prob, alias))
            assert want[3] == 0 and want[2][x] == yields, (hex(word), x)
            assert not (want[2] == 2).any()  # the zero-weight item is never drawn
            _same(_gpu_epoch(ops, dev, pu, pi, B, 4, off, items, seed, alias=(prob, alias)), want[:3])


# ---------------------------------------------------------------------------
# error paths: codes, not faults
# ---------------------------------------------------------------------------
def test_bad_users_and_give_up_are_error_codes(ops, dev):
    native = import_module(PKG + "._native")
    rng = np.random.default_rng(3)
    # user 0 owns every item of 64 but 17; user 1 owns nothing
    off = np.array([0, 63, 63], np.int64)
    items = np.array([k for k in range(64) if k != 17], np.int32)
    n_pos, B, seed = 300, 64, ref.device_seed(3, 0)
    clean_u = np.ones(n_pos, np.int32)
    pi = rng.integers(0, 64, n_pos).astype(np.int32)
    perm = ref.epoch_perm(n_pos, seed)

    def run(pu, max_tries, check):
        return _gpu_epoch(ops, dev, pu, pi, B, 64, off, items, seed, max_tries, check)

    clean = ref.sample_epoch(clean_u, pi, B, 64, off, items, seed, 1024)
    assert clean[3] == 0
    _same(run(clean_u, 1024, True), clean[:3])

    # a user id equal to num_lists, and -1, at the ends of the epoch and inside
    bad_u = clean_u.copy()
    bad_u[perm[[0, 100]]] = 2
    bad_u[perm[[255, 7]]] = -1
    want = ref.sample_epoch(bad_u, pi, B, 64, off, items, seed, 1024)
    assert want[3] == 1
    np.testing.assert_array_equal(np.flatnonzero(want[2] == -1), [0, 7, 100, 255])
    with pytest.raises(native.NativeIndexError, match="user outside trainList"):
        run(bad_u, 1024, True)
    _same(run(bad_u, 1024, False), want[:3])
    _same(run(clean_u, 1024, True), clean[:3])

    # the all-but-one user at 64 tries
    tight_u = clean_u.copy()
    tight_u[perm[:256:2]] = 0
    want = ref.sample_epoch(tight_u, pi, B, 64, off, items, seed, 64)
    assert want[3] == 2 and 0 < (want[2] == -1).sum() < 128
    with pytest.raises(native.NativeIndexError, match="no admissible negative"):
        run(tight_u, 64, True)
    _same(run(tight_u, 64, False), want[:3])
    loose = ref.sample_epoch(tight_u, pi, B, 64, off, items, seed, 1024)
    assert loose[3] == 0
    _same(run(tight_u, 1024, True), loose[:3])

    # both at once: one message names both
    both_u = tight_u.copy()
    both_u[perm[1]] = 2
    want = ref.sample_epoch(both_u, pi, B, 64, off, items, seed, 64)
    assert want[3] == 3
    with pytest.raises(native.NativeIndexError, match="user outside trainList no admissible negative"):
        run(both_u, 64, True)
    _same(run(both_u, 64, False), want[:3])
    _same(run(clean_u, 1024, True), clean[:3])


# ---------------------------------------------------------------------------
# DeviceSampler
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ds(acf):
    return acf.synthetic_dataset(400, 250, 12000, seed=5)


def _epoch_np(ep):
    return tuple(t.cpu().numpy() for t in (ep.user, ep.item_pos, ep.item_neg))


def _want_epoch(ds, B, seed, epoch, alias=None):
    off, items = ds.sorted_lists()
    want = ref.sample_epoch(ds.pair_user, ds.pair_item, B, ds.num_items, off, items, ref.device_seed(seed, epoch),
                            alias=alias)
    assert want[3] == 0
    return want[:3]


@pytest.mark.parametrize("seed,epoch", [(0, 0), (3, 0), (3, 1), (2 ** 31, 5)])
def test_device_sampler_epoch_equals_restatement(acf, dev, small_ds, seed, epoch):
    ep = acf.DeviceSampler(small_ds, 100, dev, seed=seed).epoch(epoch)
    assert ep.n_batches == len(small_ds.pair_user) // 100
    _same(_epoch_np(ep), _want_epoch(small_ds, 100, seed, epoch))


def test_device_sampler_with_weights_equals_restatement(acf, ops, dev, small_ds):
    w = np.bincount(small_ds.pair_item, minlength=small_ds.num_items).astype(np.float32) ** 0.75
    ep = acf.DeviceSampler(small_ds, 128, dev, seed=2, weights=w).epoch(4)
    _same(_epoch_np(ep), _want_epoch(small_ds, 128, 2, 4, alias=ops.alias_table(w)))


def test_device_dataset_path_gives_the_host_path_s_epoch(acf, dev, small_ds):
    data = import_module(PKG + ".data")
    off, items = small_ds.sorted_lists()
    dd = data.DeviceDataset(small_ds.num_users, small_ds.num_items,
                            torch.tensor(small_ds.pair_user, dtype=torch.int32, device=dev),
                            torch.tensor(small_ds.pair_item, dtype=torch.int32, device=dev),
                            torch.tensor(off, dtype=torch.int64, device=dev),
                            torch.tensor(items, dtype=torch.int32, device=dev))
    a = acf.DeviceSampler(dd, 100, dev, seed=3).epoch(2)
    b = acf.DeviceSampler(small_ds, 100, dev, seed=3).epoch(2)
    _same(_epoch_np(a), _epoch_np(b))
    _same(_epoch_np(a), _want_epoch(small_ds, 100, 3, 2))


@pytest.fixture(scope="module")
def video(acf, tmp_path_factory):
    z = np.load(os.path.join(GOLDEN, "video_data.npz"))
    d = tmp_path_factory.mktemp("data")
    with open(d / "Video.train.rating", "w") as f:
        f.writelines(f"{a}\t{b}\t{r}\t1\n" for a, b, r in zip(z["train_u"], z["train_i"], z["train_r"]))
    with open(d / "Video.test.rating", "w") as f:
        f.writelines(f"{a}\t{b}\t1\t1\n" for a, b in zip(z["test_u"], z["test_i"]))
    return acf.OriginalDataset(str(d / "Video"))


def test_video_epoch_equals_restatement(acf, dev, video):
    """The reference's own data, trainList misalignment included: the epoch is
    the restatement's over sorted_lists()."""
    ep = acf.DeviceSampler(video, 512, dev, seed=3).epoch(0)
    _same(_epoch_np(ep), _want_epoch(video, 512, 3, 0))
