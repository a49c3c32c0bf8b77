"""The streamed step's slot task at every instance it has, against the two-kernel
step (set_stream(False)) on the same plan: tables, Adagrad slots and both loss
arrays bit for bit, step_errors() == 0 and stream_recoveries() == 0.

A slot of at most TEAM occurrences runs the one-occurrence-per-member instance,
TEAM < count <= 2 TEAM the two-occurrence body, more the hot path.  A user
occurrence whose two items occur once in the batch (solo) forms one delta and
mirrors it for the other item.

Tables are 40 users x 60 items.  d = 8 / 64 / 100 / 256 are TEAM 32 / 4 / 2 / 1
(d = 100 is a padded row).

Slot counts (B = 32, 7 batches): user 0 and item 0 recur in every batch, so
their versions hand over, with 1, TEAM, TEAM + 1, 2 TEAM and 2 TEAM + 1
occurrences in turn.  A user cannot occur more than B times and an item not
more than 2 B times, so d = 8 (TEAM 32) has user counts 1 and 32 only and item
counts 1, 32, 33 and 64 (an item past B occurrences is positive and negative
of the same triplets).

Mirrored delta (B = 16, 6 batches): user 0 occurs twice in every batch; see
_mirror_stream.  Every table has -0.0 elements and eps is 0.5, so a delta zero
of the wrong sign would show in q + delta."""
import numpy as np
import pytest
import torch

U1, I1 = 40, 60
DIMS = [8, 64, 100, 256]
TEAM = {8: 32, 64: 4, 100: 2, 256: 1}
NAMES = ("P", "Q", "accP", "accQ", "loss_clean", "loss_adv")
B_CNT, NB_CNT = 32, 7
B_MIR, NB_MIR = 16, 6
VARIANTS = ("solo", "mixed", "ieqj", "saturated")


def _wanted_counts(T, B):
    want = [1, T, T + 1, 2 * T, 2 * T + 1]
    users = sorted({c for c in want if c <= B})
    items = sorted({c for c in want if c <= 2 * B})
    return users, items


def _count_stream(T, seed):
    """user 0 occurs cu(t) times and item 0 ci(t) times in batch t; the rest is random among the others."""
    rng = np.random.default_rng(seed)
    B = B_CNT
    users, items = _wanted_counts(T, B)
    u, i, j = [], [], []
    for t in range(NB_CNT):
        cu, ci = users[t % len(users)], items[t % len(items)]
        bu = rng.integers(1, U1, B)
        bi, bj = rng.integers(1, I1, B), rng.integers(1, I1, B)
        bu[:cu] = 0
        bi[B - min(ci, B):] = 0  # from the end, away from user 0's triplets where there is room
        if ci > B:
            bj[2 * B - ci:] = 0  # positive and negative of the same triplet
        u.append(bu), i.append(bi), j.append(bj)
    return tuple(np.concatenate(x).astype(np.int32) for x in (u, i, j))


def _mirror_stream(variant, seed):
    """User 0 occurs twice in every batch, with items (1, 2) and (3, 4), which no
    other triplet uses: four solo partners.  The other 14 triplets have distinct
    users and distinct items, drawn anew per batch so that their rows recur.
    mixed: the third triplet's positive is item 1, so user 0's first occurrence
    has one published and one solo partner and its second has two solo ones.
    ieqj: user 0's first triplet is (0, 1, 1): its gradient terms cancel exactly.
    saturated: the stream of solo; the tables make user 0's scores clip (_tables)."""
    rng = np.random.default_rng(seed)
    B = B_MIR
    u, i, j = [], [], []
    for _ in range(NB_MIR):
        bu = np.concatenate([[0, 0], 1 + rng.permutation(U1 - 1)[:B - 2]])
        it = 5 + rng.permutation(I1 - 5)[:2 * (B - 2)]
        bi = np.concatenate([[1, 3], it[:B - 2]])
        bj = np.concatenate([[2, 4], it[B - 2:]])
        if variant == "mixed":
            bi[2] = 1
        if variant == "ieqj":
            bj[0] = 1
        u.append(bu), i.append(bi), j.append(bj)
    return tuple(np.concatenate(x).astype(np.int32) for x in (u, i, j))


def _batch_counts(stream, B, t):
    u, i, j = (x[t * B:(t + 1) * B] for x in stream)
    return np.bincount(u, minlength=U1), np.bincount(np.concatenate([i, j]), minlength=I1)


@pytest.mark.parametrize("d", DIMS)
def test_count_stream_has_its_counts(d):
    """Plain counting: every reachable count of the list occurs for user 0 and for item 0."""
    T = TEAM[d]
    stream = _count_stream(T, d)
    users, items = _wanted_counts(T, B_CNT)
    got = [_batch_counts(stream, B_CNT, t) for t in range(NB_CNT)]
    assert {int(cu[0]) for cu, _ in got} == set(users)
    assert {int(ci[0]) for _, ci in got} == set(items)
    if T < 32:
        assert set(users) == set(items) == {1, T, T + 1, 2 * T, 2 * T + 1}
    else:
        assert (users, items) == ([1, 32], [1, 32, 33, 64])


@pytest.mark.parametrize("variant", VARIANTS)
def test_mirror_stream_has_its_structure(variant):
    stream = _mirror_stream(variant, 3)
    for t in range(NB_MIR):
        cu, ci = _batch_counts(stream, B_MIR, t)
        u, i, j = (x[t * B_MIR:(t + 1) * B_MIR] for x in stream)
        assert cu[0] == 2 and (u[:2] == 0).all()
        want = {"solo": (1, 1, 1, 1), "saturated": (1, 1, 1, 1), "mixed": (2, 1, 1, 1), "ieqj": (2, 0, 1, 1)}[variant]
        assert tuple(ci[1:5]) == want
        assert (i[0] == j[0]) == (variant == "ieqj")
        assert ci[5:].max() <= 1 and cu[1:].max() <= 1


def _tables(d, dev, saturated=False):
    rng = np.random.default_rng(d)
    P = (rng.standard_normal((U1, d)) * 0.2).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.2).astype(np.float32)
    P[::3, 1] = -0.0
    Q[::2, 0] = -0.0
    Q[1::2, 3] = -0.0
    if saturated:  # x = p.(q_i - q_j) = -18 (d - 1) < clip_lo = -80: the clip passes no gradient, G = 0
        P[0] = 3.0
        Q[[1, 3]] = -3.0
        Q[[2, 4]] = 3.0
        Q[1:5, 0] = -0.0
    return [torch.tensor(P, device=dev), torch.tensor(Q, device=dev),
            torch.full((U1, d), 0.1, device=dev), torch.full((I1, d), 0.1, device=dev)]


def _run(ops, dev, stream, B, d, hp, streamed, graph=False, poll=None, saturated=False):
    u, i, j = stream
    nb = len(u) // B
    ctx = ops.APRContext(U1, I1, d, B, nb, dev)
    if poll is not None:
        ctx.set_poll_sleep(poll)
    ctx.set_stream(streamed)
    ctx.plan(torch.tensor(u, device=dev), torch.tensor(i, device=dev), torch.tensor(j, device=dev), B)
    tabs = _tables(d, dev, saturated)
    ctx.train_planned(tabs, hp, 0, nb, graph=graph)
    lc, la = ctx.losses()
    out = tabs + [lc.clone(), la.clone()]
    torch.cuda.synchronize()
    assert ctx.step_errors() == 0
    assert ctx.stream_recoveries() == 0
    return out


def _same(want, got, what):
    for x, y, n in zip(want, got, NAMES):
        # bytes, not values: -0.0 == +0.0 and nan != nan as floats
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, n)


_WANT = {}


def _want(ops, dev, key, stream, B, d, hp, **kw):
    """The two-kernel result of a case, computed once and shared."""
    if key not in _WANT:
        _WANT[key] = _run(ops, dev, stream, B, d, hp, False, **kw)
    return _WANT[key]


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("d", DIMS)
def test_slot_counts_bit_identical(ops, dev, d, graph):
    stream = _count_stream(TEAM[d], d)
    hp = ops.StepHParams(adver=1, eps=0.5, reg=0.01, seed=5)
    want = _want(ops, dev, ("cnt", d), stream, B_CNT, d, hp)
    assert float(want[4].abs().sum()) > 0 and float(want[5].abs().sum()) > 0
    _same(want, _run(ops, dev, stream, B_CNT, d, hp, True, graph=graph), "streamed")


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_slot_counts_general_instance(ops, dev, d):
    """A non-default poll sleep runs k_stream_any: both instances give the two-kernel bits."""
    stream = _count_stream(TEAM[d], d)
    hp = ops.StepHParams(adver=1, eps=0.5, reg=0.01, seed=5)
    want = _want(ops, dev, ("cnt", d), stream, B_CNT, d, hp)
    _same(want, _run(ops, dev, stream, B_CNT, d, hp, True, poll=4), "k_stream_any")


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_mirrored_delta_bit_identical(ops, dev, d, variant):
    stream = _mirror_stream(variant, d + 1)
    sat = variant == "saturated"
    hp = ops.StepHParams(adver=1, eps=0.5, reg=0.0, seed=5)
    want = _want(ops, dev, ("mir", variant, d), stream, B_MIR, d, hp, saturated=sat)
    got = _run(ops, dev, stream, B_MIR, d, hp, True, saturated=sat)
    _same(want, got, variant)
    if sat:  # G = 0 for user 0 and its four items in every batch: nothing moves them
        first = _tables(d, dev, True)
        assert torch.equal(got[0][0].view(torch.int32), first[0][0].view(torch.int32))
        assert torch.equal(got[1][1:5].view(torch.int32), first[1][1:5].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_random_delta_still_draws_per_row(ops, dev, d):
    """adv = "random" (k_stream_any) keeps one delta per solo partner, keyed on its row
    (a mirrored pair would give the second item the negated delta of the first):
    the bits are the two-kernel step's."""
    stream = _mirror_stream("solo", d + 1)
    hp = ops.StepHParams(adver=1, adv="random", eps=0.5, reg=0.0, seed=5)
    want = _run(ops, dev, stream, B_MIR, d, hp, False)
    _same(want, _run(ops, dev, stream, B_MIR, d, hp, True), "random delta")
