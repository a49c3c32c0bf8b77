"""The numpy yardstick of the epoch sampler (ops.sample_epoch, DeviceSampler):
k_perm_keys, the stable 64-bit sort and k_negatives of csrc/acf_apr.hip restated
plainly on uint64 arrays.  The sampler is a counter-based function of
(seed, x, attempt), so this reproduces it bit for bit; no GPU, no tolerance.

Lists are sets here (np.isin on (user, item) keys): the kernel's binary search
over a sorted list must agree with plain membership."""
import numpy as np

MASK64 = (1 << 64) - 1
_U = np.uint64


def mix64(z):
    """mix64 of csrc/acf_rows.h (splitmix64's finaliser, the increment first) on
    uint64 arrays; arithmetic wraps modulo 2^64."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def device_seed(seed, epoch):
    """The 64-bit seed DeviceSampler.epoch(epoch) hands to ops.sample_epoch."""
    return (int(seed) * 0x9E3779B1 + int(epoch) * 0x85EBCA77 + 1) & MASK64


def perm_keys(n_pos, seed):
    """k_perm_keys: the sort key of positive x."""
    x = np.arange(n_pos, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix64(_U(int(seed) & MASK64) ^ mix64(x + _U(0x5bd1e995)))


def epoch_perm(n_pos, seed):
    """The permutation of ALL n_pos positives: a stable sort of their keys (equal
    keys keep the order of x).  An epoch uses its first (n_pos // B) * B entries."""
    return np.argsort(perm_keys(n_pos, seed), kind="stable").astype(np.int64)


def _member_keys(num_items, list_off, list_items):
    off = np.asarray(list_off, dtype=np.int64)
    items = np.asarray(list_items, dtype=np.int64)[:off[-1]]
    owner = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    return np.unique(owner * np.int64(num_items + 1) + items)


def propose(h, num_items, alias=None):
    """The proposal of one hash word: multiply-high of its upper half into
    [0, num_items); with an alias table, column j keeps j unless the float32 of
    the low 24 bits times 2^-24 is >= prob[j] (compared in float32)."""
    h = np.asarray(h, dtype=np.uint64)
    j = (((h >> _U(32)) * _U(num_items)) >> _U(32)).astype(np.int64)  # < 2^32 * 2^31: no wrap
    if alias is not None:
        prob, al = np.asarray(alias[0], dtype=np.float32), np.asarray(alias[1], dtype=np.int64)
        r = (h & _U(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)
        j = np.where(r >= prob[j], al[j], j)
    return j


def attempt_words(x, seed, a):
    """The hash word of attempt a (array, broadcast against x) at output position x."""
    x = np.asarray(x, dtype=np.uint64)
    a = np.asarray(a, dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = mix64(_U(int(seed) & MASK64) ^ _U(0xA0761D6478BD642F)) ^ mix64(x)
        return mix64(base + a * _U(0x9E3779B97F4A7C15))


def _unshift(y, s):
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def unmix64(z):
    """The inverse of mix64 (a bijection of 64-bit words), on Python ints."""
    z = _unshift(int(z), 31) * pow(0x94D049BB133111EB, -1, 1 << 64) & MASK64
    z = _unshift(z, 27) * pow(0xBF58476D1CE4E5B9, -1, 1 << 64) & MASK64
    return (_unshift(z, 30) - 0x9E3779B97F4A7C15) & MASK64


def seed_for_word(h, x, a=0):
    """The seed under which attempt a at output position x hashes to the word h:
    places a chosen word, such as one on the edge of the alias compare, where
    chance would take 2^24 draws to put one."""
    base = (unmix64(h) - a * 0x9E3779B97F4A7C15) & MASK64
    return unmix64(base ^ int(mix64(np.uint64(x)))) ^ 0xA0761D6478BD642F


def negatives(users, num_items, list_off, list_items, seed, max_tries=1 << 20, alias=None, work=1 << 18):
    """k_negatives over output positions x = 0 .. len(users) - 1: the first attempt
    a in [0, max_tries) whose proposal is not in the user's list; -1 and error bit
    2 when there is none; -1 and error bit 1 for a user outside [0, num_lists).
    Returns (item_neg int32, err_bits).  Attempts are evaluated `work` words at a
    time, which changes nothing but the speed."""
    users = np.asarray(users, dtype=np.int64)
    n, num_lists = len(users), len(list_off) - 1
    neg = np.full(n, -1, dtype=np.int64)
    member = _member_keys(num_items, list_off, list_items)
    valid = (users >= 0) & (users < num_lists)
    err = 0 if valid.all() else 1
    todo = np.flatnonzero(valid)
    a0 = 0
    while len(todo) and a0 < max_tries:
        na = int(min(max_tries - a0, max(1, work // len(todo))))
        a = np.arange(a0, a0 + na, dtype=np.uint64)[None, :]
        j = propose(attempt_words(todo[:, None], seed, a), num_items, alias)
        ok = ~np.isin(users[todo][:, None] * np.int64(num_items + 1) + j, member)
        hit = ok.any(axis=1)
        first = ok.argmax(axis=1)
        neg[todo[hit]] = j[hit, first[hit]]
        todo = todo[~hit]
        a0 += na
    if len(todo):
        err |= 2
    return neg.astype(np.int32), err


def sample_epoch(pos_user, pos_item, batch_size, num_items, list_off, list_items, seed, max_tries=1 << 20,
                 alias=None):
    """ops.sample_epoch: (user, item_pos, item_neg, err_bits) of one epoch."""
    pos_user = np.asarray(pos_user, dtype=np.int32).reshape(-1)
    pos_item = np.asarray(pos_item, dtype=np.int32).reshape(-1)
    n_pos = len(pos_user)
    n_out = (n_pos // batch_size) * batch_size
    src = epoch_perm(n_pos, seed)[:n_out]
    user, item_pos = pos_user[src], pos_item[src]
    neg, err = negatives(user, num_items, list_off, list_items, seed, max_tries, alias)
    return user, item_pos, neg, err
