"""CPU checks of the sampler's restatement (tests/sampler_ref.py), of the alias
table (ops.alias_table, a host function) and of the host sampler (sampler.py).

tests/test_gpu_sampler_exact.py holds the GPU sampler to the restatement bit for
bit, so the statistical claims about the sampler are made here, on the
restatement, where millions of draws are cheap: the shuffle is uniform over
deciles, negatives are uniform over the admissible items, the alias path follows
the weights, and the shuffle and the negatives (which share one seed) are
independent.  Every chi-square uses test_alias_negatives_follow_the_weights' bar,
p > 1e-4."""
import numpy as np
import pytest
from scipy import stats

import sampler_ref as ref

P_BAR = 1e-4


# ---------------------------------------------------------------------------
# mix64
# ---------------------------------------------------------------------------
def _mix64_int(z):
    m = ref.MASK64
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_mix64_wraps_like_python_ints():
    rng = np.random.default_rng(0)
    words = [0, ref.MASK64, 1, 1 << 63, (1 << 63) - 1] + [int(w) for w in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]
    got = ref.mix64(np.array(words, dtype=np.uint64))
    assert got.dtype == np.uint64
    assert [int(g) for g in got] == [_mix64_int(w) for w in words]
    assert int(ref.mix64(np.uint64(words[7]))) == _mix64_int(words[7])  # a scalar, too


def test_unmix64_and_seed_for_word_invert_the_hash():
    rng = np.random.default_rng(1)
    for w in [0, ref.MASK64] + [int(w) for w in rng.integers(0, 1 << 64, 200, dtype=np.uint64)]:
        assert _mix64_int(ref.unmix64(w)) == w and ref.unmix64(_mix64_int(w)) == w
    for h, x, a in ((0, 0, 0), (ref.MASK64, 499, 0), (0x8000000000800000, 7, 3), (12345, 70000, 1023)):
        seed = ref.seed_for_word(h, x, a)
        assert int(ref.attempt_words(x, seed, a)) == h


def test_alias_compare_edge_on_the_restatement():
    """r >= prob[j] at r == prob[j] yields the alias; one step of 2^-24 below, the column."""
    alias = (np.array([0.5, 1.0, 0.0, 0.5], np.float32), np.array([3, 1, 3, 1], np.int32))
    col0, col2 = 0 << 62, 2 << 62
    words = np.array([col2, col2 | 1, col0 | 0x800000, col0 | 0x7FFFFF, col0 | 0x800001, (1 << 62) | 0xFFFFFF],
                     dtype=np.uint64)
    np.testing.assert_array_equal(ref.propose(words, 4, alias), [3, 3, 3, 0, 3, 1])


def test_device_seed_is_the_64_bit_wrap():
    assert ref.device_seed(0, 0) == 1
    assert ref.device_seed(3, 1) == 3 * 0x9E3779B1 + 0x85EBCA77 + 1
    assert ref.device_seed(2 ** 62, 5) == (2 ** 62 * 0x9E3779B1 + 5 * 0x85EBCA77 + 1) % 2 ** 64


# ---------------------------------------------------------------------------
# shuffle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 6000])
def test_epoch_perm_is_a_permutation(n):
    for seed in (0, ref.device_seed(3, 0), ref.MASK64):
        p = ref.epoch_perm(n, seed)
        assert p.shape == (n,)
        np.testing.assert_array_equal(np.sort(p), np.arange(n))


def test_epochs_and_seeds_give_different_permutations():
    perms = [ref.epoch_perm(6000, ref.device_seed(s, e)) for s in (0, 3) for e in (0, 1, 2)]
    for a in range(len(perms)):
        for b in range(a + 1, len(perms)):
            # two uniform permutations of 6000 share 1 fixed point on average
            assert (perms[a] == perms[b]).sum() < 20


def test_shuffle_moves_every_decile_everywhere():
    """(source decile, destination decile) of the shuffle of 6000 positives,
    DeviceSampler seed 3, epochs 0..7: 100 cells of expectation 60.  A
    permutation fixes both margins, so the statistic has 9 * 9 degrees of
    freedom (measured p: 0.043 at epoch 0, 0.25 to 0.55 at the others; with the
    99 of a free table, 0.34 to 0.94)."""
    n = 6000
    for e in range(8):
        p = ref.epoch_perm(n, ref.device_seed(3, e))
        table = np.zeros((10, 10))
        np.add.at(table, (p * 10 // n, np.arange(n) * 10 // n), 1)
        stat = ((table - 60.0) ** 2 / 60.0).sum()
        pv = stats.chi2.sf(stat, 81)
        print(f"shuffle epoch {e}: chi2 {stat:.1f}, p {pv:.3f}")
        assert pv > P_BAR, (e, stat, pv)
    # neither end of the range is pinned
    ends = {int(ref.epoch_perm(n, ref.device_seed(3, e))[-1]) for e in range(8)}
    starts = {int(ref.epoch_perm(n, ref.device_seed(3, e))[0]) for e in range(8)}
    assert len(ends) == 8 and len(starts) == 8


# ---------------------------------------------------------------------------
# negatives, uniform proposals
# ---------------------------------------------------------------------------
I_SMALL, USERS, PER = 40, 200, 500


def _owners_epoch(e):
    """200 users x 500 positives; users 100..199 own items 0..4, the others nothing."""
    pu = np.repeat(np.arange(USERS), PER).astype(np.int32)
    pi = np.zeros(USERS * PER, np.int32)
    off = np.zeros(USERS + 1, np.int64)
    off[101:] = 5 * np.arange(1, 101)
    items = np.tile(np.arange(5, dtype=np.int32), 100)
    seed = ref.device_seed(3, e)
    u, _, j, err = ref.sample_epoch(pu, pi, 1000, I_SMALL, off, items, seed)
    assert err == 0 and len(u) == USERS * PER
    return u, j, ref.epoch_perm(len(pu), seed)


@pytest.mark.parametrize("e", range(4))
def test_uniform_negatives_are_uniform_over_the_admissible_items(e):
    """Measured p over the eight (epoch, group) cells: >= 0.20."""
    u, j, _ = _owners_epoch(e)
    assert j.min() >= 0 and j.max() == I_SMALL - 1  # the last item is drawn
    for owned, sel in ((0, u < 100), (5, u >= 100)):
        c = np.bincount(j[sel], minlength=I_SMALL)
        assert c[:owned].sum() == 0  # owners never draw an owned item
        res = stats.chisquare(c[owned:])
        print(f"epoch {e}, {owned} owned: p {res.pvalue:.3f}")
        assert res.pvalue > P_BAR, (e, owned, res)


def test_shuffle_and_negatives_are_independent():
    """The shuffle keys and the negatives hash the same seed.  Joint table of a
    triplet's place in the shuffle (decile of its output position, and decile of
    the source index the shuffle put there) against its negative (8 bins of 5
    items), users without a list: independence at the same bar."""
    u, j, perm = _owners_epoch(0)
    x = np.arange(len(u))
    sel = u < 100
    # these users' pairs are source indices 0 .. 49,999 (the pairs are sorted by user)
    for name, rank, span in (("position", x, len(u)), ("source", perm[:len(u)], 100 * PER)):
        table = np.zeros((10, 8))
        np.add.at(table, (rank[sel] * 10 // span, j[sel] // 5), 1)
        res = stats.chi2_contingency(table)
        print(f"{name} decile x negative: p {res[1]:.3f}")
        assert res[1] > P_BAR, (name, res[0], res[1])


def test_forced_negative_and_give_up():
    """A user owning 63 of 64 items: with 1,024 tries nothing gives up and every
    negative is the one admissible item; with 64 tries (a draw succeeds with
    probability 1 - (63/64)^64 = 0.635) some draws end at -1 with the give-up
    bit, and the others still find item 17 at the same attempt."""
    items = np.array([k for k in range(64) if k != 17], np.int32)
    off = np.array([0, 63], np.int64)
    users = np.zeros(4096, np.int32)
    seed = ref.device_seed(3, 0)
    j, err = ref.negatives(users, 64, off, items, seed, max_tries=1024)
    assert err == 0 and (j == 17).all()
    j64, err64 = ref.negatives(users, 64, off, items, seed, max_tries=64)
    gave_up = int((j64 == -1).sum())
    print(f"gave up within 64 tries: {gave_up} of 4096")
    assert err64 == 2 and gave_up > 0
    assert set(np.unique(j64)) == {-1, 17}
    # the chunking of attempts is not part of the result
    j1, e1 = ref.negatives(users, 64, off, items, seed, max_tries=64, work=1)
    np.testing.assert_array_equal(j1, j64)
    assert e1 == 2


def test_restatement_flags_users_outside_the_lists():
    off = np.array([0, 1, 1], np.int64)
    items = np.array([0], np.int32)
    j, err = ref.negatives(np.array([0, 2, 1, -1]), 2, off, items, seed=5)
    assert err == 1 and j[1] == -1 and j[3] == -1 and j[0] == 1 and j[2] in (0, 1)


# ---------------------------------------------------------------------------
# alias table (acf_alias_build through ops.alias_table)
# ---------------------------------------------------------------------------
def _columns_ok(prob, alias, n):
    assert prob.dtype == np.float32 and alias.dtype == np.int32
    assert ((prob >= 0) & (prob <= 1)).all() and ((alias >= 0) & (alias < n)).all()


def _table_mass(prob, alias):
    n = len(prob)
    p = prob.astype(np.float64) / n
    np.add.at(p, alias, (1.0 - prob.astype(np.float64)) / n)
    return p


def _spanning():
    return np.logspace(-30, 30, 61).astype(np.float32)


ALIAS_CASES = {
    "one_item": lambda: np.array([3.0], np.float32),
    "one_nonzero": lambda: np.r_[np.zeros(3), 2.5, np.zeros(3)].astype(np.float32),
    "spanning_1e-30_1e30": _spanning,
    "equal": lambda: np.full(40, 0.7, np.float32),
    "gamma": lambda: (np.random.default_rng(0).gamma(0.7, size=40) + 0.01).astype(np.float32),
    # zero weights first, last and in between; the low indices are the last the builder pairs up
    "zeros_among_gamma": lambda: np.where(np.arange(41) % 4 == 0, 0.0,
                                          np.random.default_rng(1).gamma(0.7, size=41) + 0.01).astype(np.float32),
}


@pytest.mark.parametrize("case", sorted(ALIAS_CASES))
def test_alias_table_columns(ops, case):
    w = ALIAS_CASES[case]()
    n = len(w)
    prob, alias = ops.alias_table(w)
    _columns_ok(prob, alias, n)
    np.testing.assert_allclose(_table_mass(prob, alias), w.astype(np.float64) / w.astype(np.float64).sum(), atol=1e-6)
    zero = np.flatnonzero(w == 0)
    # a zero-weight item keeps nothing and is nobody's alias: r >= 0 always yields its alias
    assert (prob[zero] == 0).all()
    assert not np.isin(alias[w > 0], zero).any()
    assert not np.isin(alias[zero], zero).any()
    if case == "one_item":
        assert prob[0] == 1 and alias[0] == 0
    if case == "one_nonzero":
        assert (alias == 3).all() and prob[3] == 1
    if case == "equal":
        assert (prob == 1).all()
        np.testing.assert_array_equal(alias, np.arange(n))


def test_alias_table_zero_weights_at_the_builder_s_last_columns(ops):
    """Vose's builder pairs small columns from the highest index down, so
    zero-weight items at the lowest indices are met last, when rounding may have
    used the large columns up: they must still keep nothing.  (They do: the
    columns still to pair sum to their count, so the last large column stays
    above 1 - rounding until the last zero has been paired with it.)"""
    rng = np.random.default_rng(2)
    for trial in range(300):
        n = int(rng.integers(2, 60))
        w = rng.gamma(0.5, size=n).astype(np.float32) + np.float32(1e-3)
        w[:int(rng.integers(1, max(2, n // 2)))] = 0
        if not (w > 0).any():
            w[-1] = 1
        prob, alias = ops.alias_table(w)
        zero = np.flatnonzero(w == 0)
        assert (prob[zero] == 0).all(), (trial, w, prob)
        assert not np.isin(alias, zero).any(), (trial, w, alias)


@pytest.mark.parametrize("bad", [[1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0], [1.0, float("-inf")],
                                 [0.0, 0.0, 0.0], [-0.0]])
def test_alias_table_refuses(ops, bad):
    from importlib import import_module
    from conftest import PKG
    native = import_module(PKG + "._native")
    with pytest.raises(native.NativeError):
        ops.alias_table(np.array(bad, np.float32))


@pytest.mark.parametrize("case", sorted(ALIAS_CASES))
def test_alias_draws_follow_the_weights(ops, case):
    """2M draws of the restatement per table, users without a list: chi-square
    against w / sum(w) over the items with an expected count of at least 5 (the
    validity rule of the test; the spanning table has 54 items below it).  The
    items below it share one bin when that bin reaches 5; otherwise their total,
    a Poisson count of mean < 5, must stay below 30 (probability < 1e-13 above).
    Zero-weight items are never drawn."""
    w = ALIAS_CASES[case]()
    n, draws = len(w), 2_000_000
    prob, alias = ops.alias_table(w)
    j, err = ref.negatives(np.zeros(draws, np.int32), n, np.zeros(2, np.int64), np.zeros(0, np.int32),
                           ref.device_seed(11, 0), alias=(prob, alias))
    assert err == 0 and j.min() >= 0 and j.max() < n
    c = np.bincount(j, minlength=n).astype(np.float64)
    assert c[w == 0].sum() == 0
    expect = w.astype(np.float64) / w.astype(np.float64).sum() * draws
    big = expect >= 5
    obs, exp = list(c[big]), list(expect[big])
    rest_o, rest_e = c[~big].sum(), expect[~big].sum()
    if rest_e >= 5:
        obs.append(rest_o)
        exp.append(rest_e)
    else:
        assert rest_o < 30, (rest_o, rest_e)
        exp = list(np.array(exp) * (sum(obs) / sum(exp)))
    if len(obs) > 1:
        res = stats.chisquare(obs, exp)
        print(f"{case}: {len(obs)} bins, p {res.pvalue:.3f}")
        assert res.pvalue > P_BAR, (case, res)
    else:
        assert obs[0] == draws


def test_equal_weights_are_the_uniform_path(ops):
    prob, alias = ops.alias_table(np.ones(40, np.float32))
    users = np.zeros(5000, np.int32)
    off, items = np.array([0, 3], np.int64), np.array([0, 7, 39], np.int32)
    a = ref.negatives(users, 40, off, items, 9, alias=(prob, alias))
    b = ref.negatives(users, 40, off, items, 9)
    np.testing.assert_array_equal(a[0], b[0])


# ---------------------------------------------------------------------------
# host sampler (sampler.py)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ds(acf):
    return acf.synthetic_dataset(400, 250, 12000, seed=5)


def _pair_keys(u, i, num_items):
    return np.asarray(u, np.int64).reshape(-1) * num_items + np.asarray(i, np.int64).reshape(-1)


@pytest.mark.parametrize("B", [100, 512, 12001])
def test_host_shuffle_obeys_the_restatement_s_rule(acf, small_ds, B):
    from importlib import import_module
    from conftest import PKG
    sampler = import_module(PKG + ".sampler")
    ds = small_ds
    n = len(ds.pair_user)
    ul, il, udl, jl = sampler.shuffle(sampler.sampling(ds), B, ds, rng=np.random.RandomState(4))
    assert len(ul) == len(il) == len(udl) == len(jl) == n // B  # drop-last
    if n // B == 0:
        return
    u, i, j = (np.concatenate(x).reshape(-1) for x in (ul, il, jl))
    assert all(b.shape == (B, 1) for b in ul + il + jl)
    np.testing.assert_array_equal(np.concatenate(udl).reshape(-1), u)
    # positives: real pairs, none used twice
    keys = _pair_keys(u, i, ds.num_items)
    assert len(np.unique(keys)) == len(keys)
    assert np.isin(keys, _pair_keys(ds.pair_user, ds.pair_item, ds.num_items)).all()
    # negatives: in range and outside the user's sorted_lists() entry, the set the restatement rejects on
    off, items = ds.sorted_lists()
    assert j.min() >= 0 and j.max() < ds.num_items
    member = ref._member_keys(ds.num_items, off, items)
    assert not np.isin(u.astype(np.int64) * (ds.num_items + 1) + j, member).any()


def test_host_negatives_reject_list_edges(acf, small_ds):
    """sample_negatives_host against every user's first and last list entry: 200
    draws per user, none inside the list, and both neighbours of the list's
    ends are reachable."""
    from importlib import import_module
    from conftest import PKG
    sampler = import_module(PKG + ".sampler")
    ds = small_ds
    off, items = ds.sorted_lists()
    users = np.repeat(np.arange(ds.num_users), 200)
    j = sampler.sample_negatives_host(users, ds, np.random.RandomState(1))
    member = ref._member_keys(ds.num_items, off, items)
    assert not np.isin(users.astype(np.int64) * (ds.num_items + 1) + j, member).any()
    assert j.min() == 0 and j.max() == ds.num_items - 1
    with pytest.raises(IndexError):
        sampler.sample_negatives_host(np.array([ds.trainlist_len()]), ds, np.random.RandomState(1))
    with pytest.raises(IndexError):
        sampler.sample_negatives_host(np.array([-1]), ds, np.random.RandomState(1))
