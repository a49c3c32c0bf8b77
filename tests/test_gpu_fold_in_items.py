"""Fold-in of new items against frozen user and item tables (ops.fold_in_items,
acf_fold_in_items).

The yardstick is the C oracle's training_batch step, driven per item and per
slice on a throw-away copy of P and on [Q ; q_r] with fresh 0.1 accumulators for
the frozen rows and i = num_item_rows for every triplet (`oracle_fold_items`).
An item with a single step in total is held to rtol 1e-5 / atol 1e-6 outright;
items with several dependent steps to the fp32_parity bar.

As for users, one item's fold-in is a sensitive map (the adversarial gradient of
q_r is close to (sum of |g_adv|) * q_r / |q_r|), so the seeds of every multi-step
fixture are ones for which the C oracle and apr_oracle.tf_graph_step, driven the
same way, agree to a TENTH of the bar with no outlier
(tests/test_fold_in_items_host.py::test_fixture_seeds_leave_headroom_on_the_cpu).
"""
import glob
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

U1 = 300
I1 = 300
LENS = [1, 2, 63, 64, 65, 200]  # batch 64: single slices, exact multiples, ragged tails, four dependent slices


# ---- fixtures (pure numpy: the CPU seed check builds the same ones) -----------
def make_lists(rng, lens, num_users):
    return [np.sort(rng.choice(num_users, size=n, replace=False)).astype(np.int32) for n in lens]


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate(lists).astype(np.int32) if len(lists) and off[-1] else np.zeros(0, np.int32)
    return off, flat


def tables(rng, d, users=U1, items=I1):
    P = rng.normal(0, 0.1, size=(users, d)).astype(np.float32)
    Q = rng.normal(0, 0.1, size=(items, d)).astype(np.float32)
    return P, Q


def draw_negatives(rng, T, num_items, epochs):
    """uniform on [0, num_items): the new item has no row there, so nothing is rejected"""
    return rng.randint(num_items, size=(epochs, T)).astype(np.int32)


STEP_SEEDS = {8: 1, 48: 1, 64: 1, 128: 1, 512: 1}


def step_case(d, seed=None):
    rng = np.random.RandomState((STEP_SEEDS[d] if seed is None else seed) + d)
    P, Q = tables(rng, d)
    off, flat = csr(make_lists(rng, LENS, U1))
    return P, Q, off, flat, draw_negatives(rng, len(flat), I1, 1)


EPOCH_SEED = 1


def epochs_case(seed=None, d=64, E=8):
    rng = np.random.RandomState(EPOCH_SEED if seed is None else seed)
    P, Q = tables(rng, d)
    off, flat = csr(make_lists(rng, [3, 40, 64, 100, 130], U1))
    neg = draw_negatives(rng, len(flat), I1, E)
    init = rng.normal(0, 0.05, size=(len(off) - 1, d)).astype(np.float32)
    acc = rng.uniform(0.05, 0.5, size=init.shape).astype(np.float32)
    return P, Q, off, flat, neg, init, acc


PADDED_SEEDS = {48: 1, 100: 1, 260: 1}


def padded_case(d, seed=None, E=2):
    """d whose row geometry is padded: a continued fit (init and a non-default
    acc_init), every item with at least two dependent steps (E = 2, batch 64)"""
    rng = np.random.RandomState((PADDED_SEEDS[d] if seed is None else seed) + d)
    P, Q = tables(rng, d)
    off, flat = csr(make_lists(rng, [2, 65, 130], U1))
    neg = draw_negatives(rng, len(flat), I1, E)
    init = rng.normal(0, 0.05, size=(len(off) - 1, d)).astype(np.float32)
    acc = rng.uniform(0.05, 0.5, size=init.shape).astype(np.float32)
    return P, Q, off, flat, neg, init, acc


GRID_SEED = 3


def grid_case(seed=None, n=4096, d=64, E=4):
    """4,096 items, lists of 1-100 users, one slice per epoch (batch 512), started
    from a non-zero init: this case is about the grid, not about cold starts."""
    rng = np.random.RandomState(GRID_SEED if seed is None else seed)
    P, Q = tables(rng, d)
    lens = rng.randint(1, 101, size=n)
    lens[0], lens[-1] = 100, 37
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    start = rng.randint(0, U1 - 100, size=n)  # an item's list: consecutive users from a random start
    owner = np.repeat(np.arange(n), lens)
    within = np.arange(off[-1]) - np.repeat(off[:-1], lens)
    flat = (start[owner] + within).astype(np.int32)
    neg = draw_negatives(rng, len(flat), I1, E)
    init = rng.normal(0, 0.1, size=(n, d)).astype(np.float32)
    return P, Q, off, flat, neg, init


def grid_picks(n=4096):
    return np.unique(np.r_[0, n - 1, np.linspace(0, n - 1, 64).astype(np.int64)])[:64]


PLANTED_SEED = 1


def planted_case(seed=None, n=12, d=32, users=400, items=350, per=30):
    """hidden item vectors; each new item's users are the top `per` by P . hidden"""
    rng = np.random.RandomState(PLANTED_SEED if seed is None else seed)
    P = rng.normal(0, 0.2, size=(users, d)).astype(np.float32)
    Q = rng.normal(0, 0.2, size=(items, d)).astype(np.float32)
    hidden = rng.normal(0, 1.0, size=(n, d)).astype(np.float32)
    top = np.argsort(-(hidden @ P.T), axis=1)[:, :per]
    return P, Q, [row.tolist() for row in top]


def hparams(ops_mod, oracle_mod, **kw):
    base = dict(lr=0.05, eps=0.5, reg=0.0, reg_adv=1.0, adver=1)
    base.update(kw)
    return ops_mod.StepHParams(**base), oracle_mod.HParams(**base)


def c_step(oracle):
    return lambda Pc, Qx, aP, aQ, u, i, j, hp: oracle.apr_batch(Pc, Qx, aP, aQ, u, i, j, hp)[0]


def oracle_fold_items(step, P, Q, off, flat, neg, ohp, batch, init=None, acc_init=None, items=None):
    """The yardstick: per item and slice one training_batch step on a copy of P and
    on [Q ; q_r] (fresh 0.1 accumulators for the frozen rows), i = num_item_rows
    for every triplet; row num_item_rows, its accumulator and sum(loss_clean)
    kept, everything else thrown away."""
    n, d, E = len(off) - 1, Q.shape[1], neg.shape[0]
    rows = Q.shape[0]
    items = range(n) if items is None else items
    Qn = np.zeros((n, d), np.float32) if init is None else init.copy()
    A = np.full((n, d), 0.1, np.float32) if acc_init is None else acc_init.copy()
    loss = np.zeros((E, n), np.float64)
    for r in items:
        for e in range(E):
            for s0 in range(int(off[r]), int(off[r + 1]), batch):
                s1 = min(s0 + batch, int(off[r + 1]))
                Pc, aP = P.copy(), np.full_like(P, 0.1)
                Qx = np.concatenate([Q, Qn[r:r + 1]])
                aQ = np.concatenate([np.full_like(Q, 0.1), A[r:r + 1]])
                lc = step(Pc, Qx, aP, aQ, flat[s0:s1].copy(), np.full(s1 - s0, rows, np.int32),
                          neg[e, s0:s1].copy(), ohp)
                Qn[r], A[r] = Qx[rows], aQ[rows]
                loss[e, r] += float(np.sum(lc, dtype=np.float64))
    return Qn, A, loss


def gpu_fold(ops, dev, P, Q, off, flat, neg, hp, batch, init=None, acc_init=None, **kw):
    T = lambda a: None if a is None else torch.tensor(a, device=dev)  # noqa: E731
    out = ops.fold_in_items(T(P), T(Q), off, flat, neg, hp, neg.shape[0], batch, init=T(init), acc_init=T(acc_init),
                            **kw)
    return [x.cpu().numpy() for x in out]


def compare(fp32_parity, got, want, off, batch, E, name):
    """single-step items outright, the others on the fp32_parity bar"""
    steps = E * -(-np.diff(off) // batch)
    one, many = np.flatnonzero(steps <= 1), np.flatnonzero(steps > 1)
    for g, w, what in zip(got, want, ("Q_new", "acc_new", "loss")):
        g2, w2 = (g.T, w.T) if what == "loss" else (g, w)
        np.testing.assert_allclose(g2[one], w2[one], rtol=1e-5, atol=1e-6, err_msg=f"{name} {what} (single step)")
        if len(many):
            fp32_parity(g2[many], w2[many].astype(np.float64), f"{name} {what} (dependent steps)")


# ---- parity -------------------------------------------------------------------
STEP_CASES = ([(d, adver, 0.0) for d in (8, 64, 128, 512) for adver in (0, 1)] + [(64, 1, 0.01)]
              + [(48, 0, 0.0), (48, 1, 0.0)])  # 48: a padded row geometry (12 float4 on 16 lanes)


@pytest.mark.parametrize("d,adver,reg", STEP_CASES)
def test_step_parity(ops, oracle, dev, fp32_parity, d, adver, reg):
    import apr_oracle
    P, Q, off, flat, neg = step_case(d)
    hp, ohp = hparams(ops, apr_oracle, adver=adver, reg=reg)
    want = oracle_fold_items(c_step(oracle), P, Q, off, flat, neg, ohp, 64)
    got = gpu_fold(ops, dev, P, Q, off, flat, neg, hp, 64)
    compare(fp32_parity, got, want, off, 64, 1, f"d={d} adver={adver} reg={reg}")


def test_many_epochs(ops, oracle, dev, fp32_parity):
    import apr_oracle
    P, Q, off, flat, neg, init, acc = epochs_case()
    hp, ohp = hparams(ops, apr_oracle)
    want = oracle_fold_items(c_step(oracle), P, Q, off, flat, neg, ohp, 64, init, acc)
    got = gpu_fold(ops, dev, P, Q, off, flat, neg, hp, 64, init, acc)
    for g, w, what in zip(got, want, ("Q_new", "acc_new", "loss")):
        fp32_parity(g, w.astype(np.float64), what)


@pytest.mark.parametrize("d", [48, 100, 260])
def test_padded_rows_continue_a_fit(ops, oracle, dev, fp32_parity, d):
    """a padded row geometry with init and acc_init, two dependent steps and more"""
    import apr_oracle
    P, Q, off, flat, neg, init, acc = padded_case(d)
    hp, ohp = hparams(ops, apr_oracle)
    want = oracle_fold_items(c_step(oracle), P, Q, off, flat, neg, ohp, 64, init, acc)
    got = gpu_fold(ops, dev, P, Q, off, flat, neg, hp, 64, init, acc)
    for g, w, what in zip(got, want, ("Q_new", "acc_new", "loss")):
        assert np.isfinite(g).all(), what
        fp32_parity(g, w.astype(np.float64), what)
    # continuing from the outputs equals one longer run (the documented use of init / acc_init)
    T = lambda x: torch.tensor(x, device=dev)  # noqa: E731
    half = ops.fold_in_items(T(P), T(Q), off, flat, neg[:1], hp, 1, 64, init=T(init), acc_init=T(acc))
    rest = ops.fold_in_items(T(P), T(Q), off, flat, neg[1:], hp, 1, 64, init=half[0], acc_init=half[1])
    assert np.array_equal(rest[0].cpu().numpy(), got[0]) and np.array_equal(rest[1].cpu().numpy(), got[1])


def awkward_case():
    """one slice per item (E = 1, batch 64), d = 8; op level, so lists are not de-duplicated"""
    rng = np.random.RandomState(21)
    d = 8
    P, Q = tables(rng, d)
    lists = [
        np.array([3, 9, 3, 41, 77], np.int32),       # 0: a user repeated inside one slice
        np.array([5, 6, 7, 8, 20], np.int32),        # 1: one negative repeated three times
        np.array([10, 11, 12], np.int32),            # 2: a negative shared by two triplets of different users
        np.array([100, 101, 102, 103, 104, 105], np.int32),  # 3: clip mask active (user rows scaled up below)
        np.array([50], np.int32),                    # 4: a list of length 1
        np.zeros(0, np.int32),                       # 5: an empty list between two non-empty ones
        np.array([60, 61], np.int32),                # 6
    ]
    negs = [[30, 31, 32, 33, 34], [200, 150, 200, 151, 200], [210, 211, 210], [110, 111, 112, 113, 114, 115], [51],
            [], [62, 63]]
    off, flat = csr(lists)
    neg = np.array([sum(negs, [])], np.int32)
    init = rng.normal(0, 0.3, size=(len(lists), d)).astype(np.float32)
    P[100:103] = np.float32(-1500.0) * np.sign(init[3]) * np.abs(P[100:103])  # p . q_r << 0 for three of the six
    return P, Q, off, flat, neg, init


def test_awkward_slices(ops, oracle, dev, fp32_parity):
    import apr_oracle
    P, Q, off, flat, neg, init = awkward_case()
    u3, j3 = flat[off[3]:off[4]], neg[0, off[3]:off[4]]
    x3 = (P[u3] * init[3]).sum(1) - (P[u3] * Q[j3]).sum(1)
    assert (x3 < -80).any() and (x3 > -80).any(), "the clip mask must be active for some triplets of this fixture"
    for adver in (0, 1):
        hp, ohp = hparams(ops, apr_oracle, adver=adver)
        want = oracle_fold_items(c_step(oracle), P, Q, off, flat, neg, ohp, 64, init)
        got = gpu_fold(ops, dev, P, Q, off, flat, neg, hp, 64, init)
        compare(fp32_parity, got, want, off, 64, 1, f"awkward adver={adver}")
        np.testing.assert_array_equal(got[0][5], init[5])            # the empty list keeps its inits
        np.testing.assert_array_equal(got[1][5], np.full(8, 0.1, np.float32))
        assert got[2][0, 5] == 0.0


# ---- independence, determinism, frozen tables -----------------------------------
def test_independence_and_determinism(ops, dev):
    P, Q, off, flat, neg, init, acc = epochs_case(E=2)
    n = len(off) - 1
    hp = ops.StepHParams(adver=1)
    tP, tQ = torch.tensor(P, device=dev), torch.tensor(Q, device=dev)
    p_before, q_before = tP.clone(), tQ.clone()

    def run(items):
        lists = [flat[off[r]:off[r + 1]] for r in items]
        o, f = csr(lists)
        ng = np.concatenate([neg[:, off[r]:off[r + 1]] for r in items], axis=1)
        return ops.fold_in_items(tP, tQ, o, f, ng, hp, 2, 64, init=torch.tensor(init[items], device=dev),
                                 acc_init=torch.tensor(acc[items], device=dev))

    together = run(list(range(n)))
    again = run(list(range(n)))
    rev = run(list(range(n))[::-1])
    for a, b in zip(together, again):
        assert torch.equal(a, b)
    for a, b, ax in zip(together, rev, (0, 0, 1)):
        assert torch.equal(a, b.flip(ax))
    for r in range(n):
        alone = run([r])
        assert torch.equal(alone[0][0], together[0][r]) and torch.equal(alone[1][0], together[1][r])
        assert torch.equal(alone[2][:, 0], together[2][:, r])
    assert torch.equal(tP, p_before) and torch.equal(tQ, q_before)  # bit-identical before and after


def test_zero_epochs_and_no_items(ops, dev):
    P, Q, off, flat, neg, init, acc = epochs_case(E=2)
    tP, tQ = torch.tensor(P, device=dev), torch.tensor(Q, device=dev)
    hp = ops.StepHParams(adver=1)
    Qn, A, loss = ops.fold_in_items(tP, tQ, off, flat, neg[:0], hp, 0, 64, init=torch.tensor(init, device=dev),
                                    acc_init=torch.tensor(acc, device=dev))
    np.testing.assert_array_equal(Qn.cpu().numpy(), init)
    np.testing.assert_array_equal(A.cpu().numpy(), acc)
    assert loss.shape == (0, len(off) - 1)
    Qn, A, loss = ops.fold_in_items(tP, tQ, off, flat, neg[:0], hp, 0)
    assert not Qn.any() and torch.equal(A, torch.full_like(A, 0.1))
    Qn, A, loss = ops.fold_in_items(tP, tQ, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((3, 0), np.int32),
                                    hp, 3)
    assert Qn.shape == (0, 64) and A.shape == (0, 64) and loss.shape == (3, 0)


def test_grid_larger_than_the_device(ops, oracle, dev, fp32_parity):
    import apr_oracle
    P, Q, off, flat, neg, init = grid_case()
    hp, ohp = hparams(ops, apr_oracle)
    got = gpu_fold(ops, dev, P, Q, off, flat, neg, hp, 512, init)
    picks = grid_picks()
    assert picks[0] == 0 and picks[-1] == len(off) - 2
    want = oracle_fold_items(c_step(oracle), P, Q, off, flat, neg, ohp, 512, init, items=picks)
    for g, w, what in zip(got, want, ("Q_new", "acc_new", "loss")):
        g2, w2 = (g.T, w.T) if what == "loss" else (g, w)
        fp32_parity(g2[picks], w2[picks].astype(np.float64), what)
    assert all(np.isfinite(g).all() for g in got)


# ---- errors -------------------------------------------------------------------
def test_errors(ops, dev):
    native = importlib.import_module(PKG + "._native")
    ev = importlib.import_module(PKG + ".evaluate")
    P, Q, off, flat, neg = step_case(8)
    tP, tQ = torch.tensor(P, device=dev), torch.tensor(Q[:280].copy(), device=dev)  # 300 users, 280 items
    neg = neg % 280
    hp = ops.StepHParams(adver=1)
    bad = flat.copy()
    bad[70] = U1
    with pytest.raises(native.NativeIndexError):
        ops.fold_in_items(tP, tQ, off, bad, neg, hp, 1, 64)
    for value in (-1, 280):  # 280: a row of P, not of Q
        badn = neg.copy()
        badn[0, 3] = value
        with pytest.raises(native.NativeIndexError):
            ops.fold_in_items(tP, tQ, off, flat, badn, hp, 1, 64)
    for bad_off in (off + 1, off[::-1].copy(), np.r_[off[:-1], off[-1] - 1]):
        with pytest.raises(ValueError, match="item_off"):
            ops.fold_in_items(tP, tQ, bad_off, flat, neg, hp, 1, 64)
    with pytest.raises(ValueError, match="item_neg"):
        ops.fold_in_items(tP, tQ, off, flat, neg[:, :-1], hp, 1, 64)
    with pytest.raises(ValueError, match="item_neg"):
        ops.fold_in_items(tP, tQ, off, flat, neg, hp, 2, 64)
    with pytest.raises(ValueError, match="batch"):
        ops.fold_in_items(tP, tQ, off, flat, neg, hp, 1, 513)
    with pytest.raises(ValueError, match="epochs"):
        ops.fold_in_items(tP, tQ, off, flat, neg[:0], hp, -1, 64)
    with pytest.raises(ValueError, match="adv"):
        ops.fold_in_items(tP, tQ, off, flat, neg, ops.StepHParams(adver=1, adv="random"), 1, 64)
    with pytest.raises(ValueError, match="zero_delta"):
        ops.fold_in_items(tP, tQ, off, flat, neg, ops.StepHParams(adver=1, zero_delta=1), 1, 64)
    with pytest.raises(ValueError, match="StepHParams"):
        ops.fold_in_items(tP, tQ, off, flat, neg, None, 1, 64)
    with pytest.raises(ValueError, match="init"):
        ops.fold_in_items(tP, tQ, off, flat, neg, hp, 1, 64, init=torch.zeros(2, 8, device=dev))
    with pytest.raises(ValueError, match="acc_init"):
        ops.fold_in_items(tP, tQ, off, flat, neg, hp, 1, 64, acc_init=torch.zeros(6, 4, device=dev))
    with pytest.raises(ValueError, match="2-D"):
        ops.fold_in_items(tP, tQ[0], off, flat, neg, hp, 1, 64)
    with pytest.raises(ValueError, match="differ in dim"):
        ops.fold_in_items(tP, torch.zeros(280, 12, device=dev), off, flat, neg, hp, 1, 64)
    with pytest.raises(ValueError, match="dim"):
        ops.fold_in_items(tP[:, :6].contiguous(), tQ[:, :6].contiguous(), off, flat, neg, hp, 1, 64)
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.fold_in_items(tP, tQ, off, flat.astype(np.float32), neg, hp, 1, 64)
    with pytest.raises(ValueError, match="float32"):
        ops.fold_in_items(tP.double(), tQ, off, flat, neg, hp, 1, 64)
    with pytest.raises(ValueError, match="HIP device"):
        ops.fold_in_items(tP.cpu(), tQ, off, flat, neg, hp, 1, 64)
    with pytest.raises(ValueError, match="outside"):  # the evaluate layer: a user that is no row of P
        ev.fold_in_items((tP, tQ), [[1, 2, U1]], epochs=1)
    # the C ABI refuses what the front end refuses
    import ctypes
    c = hp.to_c()
    o = torch.tensor(off, device=dev)
    f, ng = torch.tensor(flat, device=dev), torch.tensor(neg, device=dev)
    out = torch.full((len(off) - 1, 8), 7.0, device=dev)
    acc_out = torch.full_like(out, 7.0)

    def abi(batch, hpc, users=f, negs=ng):
        native.call("acf_fold_in_items", tP.data_ptr(), U1, tQ.data_ptr(), 280, 8, o.data_ptr(), len(off) - 1,
                    users.data_ptr(), negs.data_ptr(), len(flat), 1, batch, ctypes.byref(hpc), None, None,
                    out.data_ptr(), acc_out.data_ptr(), None, 1, None)

    with pytest.raises(native.NativeError, match="batch"):
        abi(513, c)
    with pytest.raises(native.NativeError, match="adv_mode"):
        abi(64, ops.StepHParams(adver=1, adv="random").to_c())
    with pytest.raises(native.NativeIndexError):
        abi(64, c, users=torch.tensor(bad, device=dev))
    with pytest.raises(native.NativeIndexError):
        abi(64, c, negs=torch.tensor(badn, device=dev))
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (acc_out == 7.0).all()  # nothing was written


def test_torch_op_gives_the_same_bits(ops, dev):
    acf_ops = importlib.import_module(PKG + ".torch_ops").load()
    P, Q, off, flat, neg, init, acc = epochs_case(E=2)
    T = lambda a: torch.tensor(a, device=dev)  # noqa: E731
    hp = ops.StepHParams(adver=1, reg=0.01, eps=0.3)
    want = ops.fold_in_items(T(P), T(Q), off, flat, neg, hp, 2, 64, init=T(init), acc_init=T(acc))
    got = acf_ops.fold_in_items(T(P), T(Q), T(off), T(flat), T(neg), 2, 64, T(init), T(acc), reg=0.01, eps=0.3)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    want = ops.fold_in_items(T(P), T(Q), off, flat, neg, ops.StepHParams(adver=0), 2)
    got = acf_ops.fold_in_items(T(P), T(Q), T(off), T(flat), T(neg).long(), 2, adver=False)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    with pytest.raises(Exception, match="batch"):
        acf_ops.fold_in_items(T(P), T(Q), T(off), T(flat), T(neg), 2, 513)
    with pytest.raises(Exception, match="item_off"):
        acf_ops.fold_in_items(T(P), T(Q), T(off) + 1, T(flat), T(neg), 2)


# ---- end to end ------------------------------------------------------------------
def test_end_to_end_on_a_planted_model(ops, oracle, dev, fp32_parity):
    import apr_oracle
    ev = importlib.import_module(PKG + ".evaluate")
    P, Q, lists = planted_case()
    tP, tQ = torch.tensor(P, device=dev), torch.tensor(Q, device=dev)
    n, E, K = len(lists), 10, 10
    f = ev.fold_in_items((tP, tQ), lists, epochs=E, batch=512, seed=4)
    loss = f.loss.cpu().numpy()
    assert f.keys == list(range(n)) and loss.shape == (E, n)
    assert (loss[E - 1] < loss[0]).all()
    neg = ev.fold_item_negatives(f.item_off, f.user_pos, Q.shape[0], E, 4)
    _, ohp = hparams(ops, apr_oracle)
    wantQ, _, want_loss = oracle_fold_items(c_step(oracle), P, Q, f.item_off, f.user_pos, neg, ohp, 512)
    fp32_parity(loss.T, want_loss.T, "loss")
    fp32_parity(f.Q, wantQ.astype(np.float64), "Q_new")
    users, scores = ev.audience_new((tP, tQ), lists, K, epochs=E, seed=4)
    assert users.shape == (n, K) and users.dtype == np.int32 and scores.dtype == np.float32
    for r, own in enumerate(lists):
        assert not set(users[r].tolist()) & set(own)
    us, sc = ops.recommend_topk(f.Q, tP, np.arange(n, dtype=np.int32), K, P.shape[0], f.item_off, f.user_pos)
    np.testing.assert_array_equal(users, us.cpu().numpy())
    np.testing.assert_array_equal(scores.view(np.uint32), sc.cpu().numpy().view(np.uint32))
    again, _ = ev.audience_new((tP, tQ), {k: v[::-1] + v[:2] for k, v in enumerate(lists)}, K, epochs=E, seed=4)
    np.testing.assert_array_equal(users, again)  # same seed, same lists (order and repeats do not matter)
    # a folded-in item scores its own users above the rest on average
    s = f.Q.cpu().numpy() @ P.T
    for r, own in enumerate(lists):
        rest = np.setdiff1d(np.arange(P.shape[0]), own)
        assert s[r, own].mean() > s[r, rest].mean()
    # the extended tables: the new items are items num_items + r
    ext = ev.extend_items((tP, tQ), f)
    assert ext.num_items == Q.shape[0] + n and ext.num_users == P.shape[0]
    assert torch.equal(ext.embedding_Q[:Q.shape[0]], tQ) and torch.equal(ext.embedding_Q[Q.shape[0]:], f.Q)
    own0 = np.asarray(lists[0], dtype=np.int64)
    items, _ = ev.recommend(ext, users=own0, k=K)
    assert (items >= Q.shape[0]).any() and items.max() < ext.num_items
    ids, _ = ev.similar_items(ext, [Q.shape[0]], k=5)  # a new item as a query of the extended table
    assert ids.shape == (1, 5) and Q.shape[0] not in ids[0]
    # the folded rows as queries against the real items
    got_ids, got_sc = ev.similar_items((tP, tQ), np.arange(n), k=5, rows=f)
    w_ids, w_sc = ops.neighbors_topk(tQ, np.arange(n, dtype=np.int32), 5, "cosine", X=f.Q,
                                     num_candidates=Q.shape[0], exclude_self=False)
    np.testing.assert_array_equal(got_ids, w_ids.cpu().numpy())
    np.testing.assert_array_equal(got_sc.view(np.uint32), w_sc.cpu().numpy().view(np.uint32))


def test_cli_writes_both_files(acf, tmp_path, monkeypatch):
    cli = importlib.import_module(PKG + ".cli")
    monkeypatch.chdir(tmp_path)
    rng = np.random.RandomState(0)
    keys = [907, 15, 300000, 42]
    fold = tmp_path / "new_items.rating"
    with open(fold, "w") as fh:
        for key in keys:
            for u in rng.choice(300, size=12, replace=False):
                fh.write("%d\t%d\t1\t0\n" % (u, key))
    lists = cli.read_fold_items_file(str(fold))
    for flavor, model in (("ori", "bpr"), ("adv", "apr")):
        rc = cli.main(["--path", str(tmp_path) + "/", "--opath", flavor + "/", "--dataset", "synthetic:300:200:8000",
                       "--model", model, "--epochs", "1", "--adv_epoch", "1", "--verbose", "1", "--embed_size", "16",
                       "--topk", "5", "--fold_in_items", str(fold)], flavor)
        assert rc == 0
        topk = glob.glob(str(tmp_path / "out" / flavor / "*.folditems.topk"))
        items = glob.glob(str(tmp_path / "out" / flavor / "*.folditems.items"))
        assert len(topk) == 1 and len(items) == 1
        assert [int(x) for x in open(items[0]).read().split()] == sorted(keys)
        users = cli.read_topk(topk[0])
        assert users.shape == (len(keys), 5)
        assert (users >= 0).all() and (users < 300).all()
        for row, key in zip(users, sorted(keys)):
            assert not set(row.tolist()) & set(lists[key])
