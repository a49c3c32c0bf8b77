"""The streamed step's two instances (k_stream: the default mode with its
launch-constant switches folded; k_stream_any: every other mode) and the losses
it evaluates behind its version stores, against the two-kernel step
(set_stream(False)) on the same plan: tables, Adagrad slots and both loss arrays
bit for bit, in one call and in two piecewise calls.

Shapes: B = 64, 6 batches.  d = 8 / 64 / 100 / 256 are LPR 2 (TEAM 32), LPR 16
(TEAM 4), a padded last chunk (LPR 32, TEAM 2) and LPR 64 with TEAM 1.  The hot
stream (40 users x 24 items, every positive one of 2 items) gives an item far
more than 2 TEAM occurrences at every d but 8 (where 2 TEAM = B), so the
multi-pass path runs with its CSR records.  The sparse stream lets every row
occur at most twice in a batch; 24 items cannot do that at B = 64 (128 item
occurrences a batch), so it has 80 users x 160 items."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NB = 64, 6
DIMS = [8, 64, 100, 256]
NAMES = ("P", "Q", "accP", "accQ", "loss_clean", "loss_adv")


def _hot_stream(seed):
    """40 x 24: every positive is item 0 (3 in 4) or item 1; negatives among the other 22."""
    rng = np.random.default_rng(seed)
    n = B * NB
    u = rng.integers(0, 40, n)
    i = (rng.random(n) < 0.25).astype(np.int64)
    j = rng.integers(2, 24, n)
    return 40, 24, u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)


def _sparse_stream(seed):
    """80 x 160: in every batch each user and each item occurs at most twice (most once)."""
    rng = np.random.default_rng(seed)
    u, i, j = [], [], []
    for _ in range(NB):
        users = np.concatenate([rng.permutation(80)[:56], rng.permutation(80)[:8]])  # 64, each <= 2
        items = rng.permutation(160)[:112]  # 112 distinct items, the first 16 used twice
        slots = rng.permutation(np.concatenate([items, items[:16]]))  # 128 item occurrences
        u.append(users)
        i.append(slots[:B])
        j.append(slots[B:])
    cat = [np.concatenate(x).astype(np.int32) for x in (u, i, j)]
    for t in range(NB):
        s = slice(t * B, (t + 1) * B)
        assert np.bincount(cat[0][s]).max() <= 2 and np.bincount(np.concatenate([cat[1][s], cat[2][s]])).max() <= 2
    return 80, 160, cat[0], cat[1], cat[2]


def _loss_stream(seed):
    """40 x 24: in every batch user 0 occurs once, user 1 twice, user 2 five times, and
    (user 39, item 22, item 23) is a triplet whose three rows occur once: a fused triplet."""
    rng = np.random.default_rng(seed)
    u, i, j = [], [], []
    for _ in range(NB):
        users = np.concatenate([[0], [1] * 2, [2] * 5, rng.integers(3, 39, B - 9)])
        pos, neg = rng.integers(0, 22, B - 1), rng.integers(0, 22, B - 1)
        perm = rng.permutation(B - 1)
        u.append(np.concatenate([users[perm], [39]]))
        i.append(np.concatenate([pos, [22]]))
        j.append(np.concatenate([neg, [23]]))
    return (40, 24) + tuple(np.concatenate(x).astype(np.int32) for x in (u, i, j))


STREAMS = {"hot": _hot_stream, "sparse": _sparse_stream, "loss": _loss_stream}


def _tables(U1, I1, d, dev):
    rng = np.random.default_rng(d)
    P = (rng.standard_normal((U1, d)) * 0.2).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.2).astype(np.float32)
    return [torch.tensor(P, device=dev), torch.tensor(Q, device=dev),
            torch.full((U1, d), 0.1, device=dev), torch.full((I1, d), 0.1, device=dev)]


def _run(ops, dev, stream_data, d, hp, stream, pieces, fuse=True, poll=None):
    """Train a fresh context (so every run starts at the same call counter); tables + losses."""
    U1, I1, u, i, j = stream_data
    ctx = ops.APRContext(U1, I1, d, B, NB, dev)
    ctx.set_fusion(fuse)
    if poll is not None:
        ctx.set_poll_sleep(poll)
    ctx.set_stream(stream)
    ctx.plan(torch.tensor(u, device=dev), torch.tensor(i, device=dev), torch.tensor(j, device=dev), B)
    tabs = _tables(U1, I1, d, dev)
    for first, n in pieces:
        ctx.train_planned(tabs, hp, first, n, graph=False)
    lc, la = ctx.losses()
    out = tabs + [lc.clone(), la.clone()]
    assert ctx.step_errors() == 0
    assert ctx.stream_recoveries() == 0
    return out


def _same(want, got, what):
    for x, y, n in zip(want, got, NAMES):
        assert torch.equal(x, y), (what, n)


ONE, TWO = [(0, NB)], [(0, 2), (2, NB - 2)]

# the default instance at both values of reg, then the general one through each of its selectors
MODES = {
    "default_reg0": (dict(reg=0.0), {}),
    "default_reg": (dict(reg=0.01), {}),
    "zero_delta": (dict(reg=0.01, zero_delta=1), {}),
    "fusion_off": (dict(reg=0.01), dict(fuse=False)),
    "poll_sleep": (dict(reg=0.0), dict(poll=4)),
}


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", ["hot", "sparse", "loss"])
@pytest.mark.parametrize("mode", list(MODES))
def test_stream_instances_bit_identical_to_two_kernels(ops, dev, d, shape, mode):
    data = STREAMS[shape](d + 11)
    hpk, ctxk = MODES[mode]
    hp = ops.StepHParams(adver=1, seed=5, **hpk)
    want = _run(ops, dev, data, d, hp, False, ONE, **{k: v for k, v in ctxk.items() if k != "poll"})
    torch.cuda.synchronize()
    assert float(want[4].abs().sum()) > 0 and float(want[5].abs().sum()) > 0  # both loss arrays are written
    _same(want, _run(ops, dev, data, d, hp, True, ONE, **ctxk), "one call")
    _same(want, _run(ops, dev, data, d, hp, True, TWO, **ctxk), "two calls")


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", ["hot", "sparse", "loss"])
@pytest.mark.parametrize("reg", [0.0, 0.01])
def test_stream_random_delta_bit_identical(ops, dev, d, shape, reg):
    """adv = "random" (the general instance): the call counter is a key of the noise, so
    every run is one call of a fresh context; two streamed runs agree with each other
    and with the two-kernel step."""
    data = STREAMS[shape](d + 12)
    hp = ops.StepHParams(adver=1, adv="random", reg=reg, seed=5)
    want = _run(ops, dev, data, d, hp, False, ONE)
    a = _run(ops, dev, data, d, hp, True, ONE)
    b = _run(ops, dev, data, d, hp, True, ONE)
    _same(a, b, "streamed twice")
    _same(want, a, "two kernels")


def test_loss_stream_has_its_cases(ops, dev):
    """The loss stream is what its name says: users with 1, 2 and 5 occurrences in a
    batch and a triplet whose rows occur once (fused when fusion is on)."""
    _, _, u, i, j = _loss_stream(3)
    for t in range(NB):
        s = slice(t * B, (t + 1) * B)
        cu, ci = np.bincount(u[s], minlength=40), np.bincount(np.concatenate([i[s], j[s]]), minlength=24)
        assert (cu[0], cu[1], cu[2], cu[39], ci[22], ci[23]) == (1, 2, 5, 1, 1, 1)


def test_default_whole_plan_call_is_one_stream_launch(ops, dev):
    """A default-mode call over the whole plan is still ONE k_stream launch, its
    write-back in the tail (time_kernels' launch counts), and trains as train_planned."""
    d = 64
    U1, I1, u, i, j = _hot_stream(1)
    hp = ops.StepHParams(adver=1)
    ctx = ops.APRContext(U1, I1, d, B, NB, dev)
    ctx.plan(torch.tensor(u, device=dev), torch.tensor(i, device=dev), torch.tensor(j, device=dev), B)
    ta, tb = _tables(U1, I1, d, dev), _tables(U1, I1, d, dev)
    t = ctx.time_kernels(ta, hp)
    assert {k: v[1] for k, v in t.items()} == {"clean": 0, "adv": 0, "flush": 0, "stream": 1, "hot": 0}
    ctx.train_planned(tb, hp)
    for x, y in zip(ta, tb):
        assert torch.equal(x, y)
    assert ctx.step_errors() == 0
