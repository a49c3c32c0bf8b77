"""The streamed step's two default-mode instances -- k_stream with the row width a
constant (a full row: d = 4 LPR) and k_stream_pad (a padded one) -- and its
waits, which read table rows once in front of the attempts and poll versions
only.  Every case against the two-kernel step (set_stream(False)) on the same
plan: tables, Adagrad slots and both loss arrays bit for bit, step_errors() == 0,
stream_recoveries() == 0.

Full rows d = 8 ... 256 are (LPR, TEAM) = (2, 32) (4, 16) (8, 8) (16, 4) (32, 2)
(64, 1); the padded d = 36 / 60 / 132 share (16, 4) / (16, 4) / (64, 1).  A width
run by the other width's instance strides its versions wrongly: the bits guard
the host's choice.

Streams (48 users and 40 items recur; a stream that needs first touches in every
batch takes its fresh rows from ids past them):
  hot     item 0 in every triplet of a batch of 64, and negative of its first 8
          too: 72 occurrences > 2 TEAM at every TEAM (stream_slot_hot)
  two     item 0 occurs 2 TEAM and TEAM + 1 times in turn (batch of 64)
  sparse  no row occurs twice in the whole plan: every source is a table row,
          the attempts have nothing to wait for
  mixed   user 0 occurs min(B, 2 TEAM) times in every batch (its own row is a
          version from the second batch on); its partners alternate between
          items that recur and items first touched here, so the lanes of its
          wave hold version and table sources side by side
"""
import numpy as np
import pytest
import torch

U0, I0 = 48, 40
FULL = [8, 16, 32, 64, 128, 256]
PADDED = [36, 60, 132]
NB = 6
NAMES = ("P", "Q", "accP", "accQ", "loss_clean", "loss_adv")


def _team(d):
    lpr = 1
    while lpr < d // 4:
        lpr <<= 1
    return 64 // lpr


def _cat(u, i, j):
    return tuple(np.concatenate(x).astype(np.int32) for x in (u, i, j))


def _hot(T, seed):
    rng = np.random.default_rng(seed)
    B = 64
    u, i, j = [], [], []
    for _ in range(NB):
        bj = rng.integers(1, I0, B)
        bj[:8] = 0
        u.append(rng.integers(0, U0, B)), i.append(np.zeros(B, np.int64)), j.append(bj)
    return (U0, I0, B) + _cat(u, i, j)


def _two(T, seed):
    rng = np.random.default_rng(seed)
    B = 64
    u, i, j = [], [], []
    for t in range(NB):
        c = 2 * T if t % 2 == 0 else T + 1
        bi = rng.integers(1, I0, B)
        bi[B - c:] = 0
        u.append(rng.integers(0, U0, B)), i.append(bi), j.append(rng.integers(1, I0, B))
    return (U0, I0, B) + _cat(u, i, j)


def _sparse(T, seed):
    B = 32
    rng = np.random.default_rng(seed)
    n = NB * B
    items = rng.permutation(2 * n)
    return (n, 2 * n, B, rng.permutation(n).astype(np.int32), items[:n].astype(np.int32), items[n:].astype(np.int32))


def _mixed(T, seed):
    rng = np.random.default_rng(seed)
    B = 32
    m = min(B, 2 * T)
    fresh = I0  # ids from here on are touched once in the plan
    u, i, j = [], [], []
    for _ in range(NB):
        bu = rng.integers(1, U0, B)
        bi, bj = rng.integers(4, I0, B), rng.integers(4, I0, B)
        bu[:m] = 0
        for x in range(m):  # recurring items 0..3 on one side, a first touch on the other
            old, new = x % 4, fresh
            fresh += 1
            bi[x], bj[x] = (old, new) if x % 2 == 0 else (new, old)
        u.append(bu), i.append(bi), j.append(bj)
    return (U0, fresh, B) + _cat(u, i, j)


STREAMS = {"hot": _hot, "two": _two, "sparse": _sparse, "mixed": _mixed}


def _counts(data, t):
    U1, I1, B, u, i, j = data
    s = slice(t * B, (t + 1) * B)
    return np.bincount(u[s], minlength=U1), np.bincount(np.concatenate([i[s], j[s]]), minlength=I1)


@pytest.mark.parametrize("d", FULL + PADDED)
def test_streams_have_their_structure(d):
    """Plain counting: each stream reaches the path it is named for at this d's TEAM."""
    T = _team(d)
    for t in range(NB):
        assert _counts(_hot(T, d), t)[1][0] == 72 > 2 * T
        assert _counts(_two(T, d), t)[1][0] == (2 * T if t % 2 == 0 else T + 1)
    sp = _sparse(T, d)
    assert np.bincount(sp[3]).max() == 1 and np.bincount(np.concatenate([sp[4], sp[5]])).max() == 1
    mx = _mixed(T, d)
    seen = np.zeros(mx[1], bool)
    for t in range(NB):
        cu, ci = _counts(mx, t)
        m = min(32, 2 * T)
        assert cu[0] == m
        s = slice(t * 32, t * 32 + m)
        first = np.concatenate([mx[4][s], mx[5][s]])
        new = first[first >= I0]
        assert len(new) == m and not seen[new].any() and (ci[new] == 1).all()  # one first touch per occurrence
        if t > 0:
            assert seen[first[first < 4]].all()  # and one item an earlier batch updated
        seen[np.concatenate([mx[4][t * 32:(t + 1) * 32], mx[5][t * 32:(t + 1) * 32]])] = True


def _tables(U1, I1, d, dev):
    rng = np.random.default_rng(d)
    P = (rng.standard_normal((U1, d)) * 0.2).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.2).astype(np.float32)
    return [torch.tensor(P, device=dev), torch.tensor(Q, device=dev),
            torch.full((U1, d), 0.1, device=dev), torch.full((I1, d), 0.1, device=dev)]


def _run(ops, dev, data, d, hp, streamed, pieces=None, fuse=True, graph=False, poll=None, timed=False):
    """Train a fresh context (every run starts at the same call counter); tables + losses."""
    U1, I1, B, u, i, j = data
    ctx = ops.APRContext(U1, I1, d, B, NB, dev)
    ctx.set_fusion(fuse)
    if poll is not None:
        ctx.set_poll_sleep(poll)
    ctx.set_stream(streamed)
    ctx.plan(torch.tensor(u, device=dev), torch.tensor(i, device=dev), torch.tensor(j, device=dev), B)
    tabs = _tables(U1, I1, d, dev)
    for first, n in pieces or [(0, NB)]:
        if timed:  # the launch sequence of train_planned, by kind
            kinds = {k: v[1] for k, v in ctx.time_kernels(tabs, hp, first, n).items()}
            whole = (first, n) == (0, NB)  # the whole plan writes back in the launch's tail
            assert kinds == {"clean": 0, "adv": 0, "flush": 0 if whole else 1, "stream": 1, "hot": 0}
        else:
            ctx.train_planned(tabs, hp, first, n, graph=graph)
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


def _want(ops, dev, shape, d, hp, hpkey="default"):
    """The two-kernel result of a case, computed once and shared (fusion changes no bit)."""
    key = (shape, d, hpkey)
    if key not in _WANT:
        _WANT[key] = _run(ops, dev, STREAMS[shape](_team(d), d), d, hp, False)
        assert float(_WANT[key][4].abs().sum()) > 0 and float(_WANT[key][5].abs().sum()) > 0
    return _WANT[key]


def _hp(ops, **kw):
    return ops.StepHParams(adver=1, eps=0.5, reg=0.01, seed=5, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape", list(STREAMS))
@pytest.mark.parametrize("d", FULL + PADDED)
def test_streamed_bits_at_every_width(ops, dev, d, shape, fuse):
    """Full rows run k_stream, padded ones k_stream_pad (fusion off: k_stream_any at both)."""
    hp = _hp(ops)
    data = STREAMS[shape](_team(d), d)
    _same(_want(ops, dev, shape, d, hp), _run(ops, dev, data, d, hp, True, fuse=fuse), (shape, d, fuse))


@pytest.mark.gpu
@pytest.mark.parametrize("d", FULL + PADDED)
def test_launch_sequence_is_one_streamed_launch(ops, dev, d):
    """The default call is one launch of the stream kind and nothing else, at both widths'
    instances (time_kernels runs train_planned's sequence), whole and in two pieces."""
    hp = _hp(ops)
    data = _mixed(_team(d), d)
    want = _want(ops, dev, "mixed", d, hp)
    _same(want, _run(ops, dev, data, d, hp, True, timed=True), ("timed", d))
    _same(want, _run(ops, dev, data, d, hp, True, pieces=[(0, 2), (2, NB - 2)], timed=True), ("timed pieces", d))


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("shape", ["mixed", "hot"])
@pytest.mark.parametrize("d", [8, 64, 60, 256])
def test_piecewise_calls(ops, dev, d, shape, graph):
    """Two calls over the plan: the second call's first touches are table rows the first wrote back."""
    hp = _hp(ops)
    data = STREAMS[shape](_team(d), d)
    got = _run(ops, dev, data, d, hp, True, pieces=[(0, 3), (3, NB - 3)], graph=graph)
    _same(_want(ops, dev, shape, d, hp), got, (shape, d, graph))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(STREAMS))
@pytest.mark.parametrize("mode", ["random", "zero_delta", "poll_sleep"])
def test_general_instance_unchanged(ops, dev, shape, mode):
    """d = 64 through the modes k_stream_any serves: same bits as the two-kernel step."""
    d = 64
    hp = _hp(ops, **{"random": dict(adv="random"), "zero_delta": dict(zero_delta=1), "poll_sleep": {}}[mode])
    data = STREAMS[shape](_team(d), d)
    want = _want(ops, dev, shape, d, hp, "default" if mode == "poll_sleep" else mode)
    _same(want, _run(ops, dev, data, d, hp, True, poll=4 if mode == "poll_sleep" else None), (shape, mode))
