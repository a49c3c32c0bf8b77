"""The certified radius on the GPU (ops.eval_radius, torch.ops.acf.eval_radius,
evaluate.certified_radius, the CLI's --certify_radius).

The yardstick is the existing ops.eval_positions_worst, compared as integers, no
tolerance: eps[r][j] must be exactly the budget at which entry r's worst-case
position reaches j + 1.  For every entry r and every j with a finite e =
eps[r][j], with worst_x = eval_positions_worst at eps = x read at entry r:
  worst_e >= j + 1;  worst_prev(e) <= j when e > 0;
  worst_e == #{i : eps[r][i] <= e} when e is below the list's last finite value or
  the list is not full (the list then holds every candidate that counts at e).
The items are distinct candidates of the entry (never t, never excluded), ids
ascending inside a run of equal eps; padding is +inf / -1 exactly past the entry's
candidates; the number of zeros is min(K, eval_positions_all's position)."""
import functools
import importlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIDES = ("user", "item")


def _ops():
    return importlib.import_module(PKG + ".ops")


def _ev():
    return importlib.import_module(PKG + ".evaluate")


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return off, flat.astype(np.int32)


class Case:
    """Tables on the device once, and the two calls on them."""

    def __init__(self, P, Q, users, tests, num_cand, elists):
        self.P, self.Q = torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV)
        self.users, self.tests = np.asarray(users, np.int32), np.asarray(tests, np.int32)
        self.num_cand, self.elists = int(num_cand), elists
        self.excl = csr(elists) if elists is not None else (None, None)

    def radius(self, k, side, check=True, rows=slice(None)):
        eo, ef = csr(self.elists[rows]) if self.elists is not None else (None, None)
        eps, items = _ops().eval_radius(self.P, self.Q, self.users[rows], self.tests[rows], self.num_cand, eo, ef,
                                        k=k, side=side, check=check)
        n = len(self.users[rows])
        assert eps.dtype == torch.float32 and items.dtype == torch.int32
        assert tuple(eps.shape) == (n, k) and tuple(items.shape) == (n, k)
        return eps.cpu().numpy(), items.cpu().numpy()

    def worst(self, eps8, side):
        return _ops().eval_positions_worst(self.P, self.Q, self.users, self.tests, self.num_cand, *self.excl,
                                           eps=eps8, side=side).cpu().numpy()

    def positions(self):
        """ops.eval_positions_all(kernel="valu") with every entry's test item added to its exclusions."""
        elists = self.elists if self.elists is not None else [[] for _ in self.users]
        off, flat = csr([list(e) + [t] for e, t in zip(elists, self.tests)])
        return _ops().eval_positions_all(self.P, self.Q, self.users, self.tests, self.num_cand, off, flat,
                                         kernel="valu").cpu().numpy()

    def candidates(self):
        cand = np.ones((len(self.users), self.num_cand), bool)
        for r, t in enumerate(self.tests):
            if self.elists is not None:
                e = np.asarray(self.elists[r], np.int64)
                cand[r, e[(e >= 0) & (e < self.num_cand)]] = False
            if 0 <= t < self.num_cand:
                cand[r, t] = False
        return cand


def lift_tests(P, Q, users, tests, num_cand):
    """Move every entry's test-item row along its user row until it scores like the (r mod 7)-th best
    candidate (r mod 7 = 0: above the best, position 0): random tables would rank it in the middle, and
    the K smallest eps_c would all be 0."""
    for r, (u, t) in enumerate(zip(users, tests)):
        p = P[u].astype(np.float64)
        if not p.any():
            continue
        s = Q.astype(np.float64) @ p
        best = np.sort(s[:num_cand])[::-1]
        target = best[min(r % 7, num_cand) - 1] if r % 7 else best[0] + 0.01
        Q[t] = (Q[t].astype(np.float64) + (target - s[t]) * p / (p @ p)).astype(np.float32)


def check_case(case, k, side):
    """Every property of the module docstring for one call; returns (eps, items)."""
    eps, items = case.radius(k, side)
    n = len(case.users)
    assert not np.isnan(eps).any() and (eps >= 0).all() and (eps[:, 1:] >= eps[:, :-1]).all()
    # the worst-case positions at every finite list value and at its predecessor, 8 eps a call
    fin = eps[np.isfinite(eps)]
    prev = np.nextafter(fin[fin > 0], np.float32(0)).astype(np.float32)
    asked = np.unique(np.concatenate([fin, prev]))
    assert np.isfinite(asked).all()
    at = {}
    for a in range(0, len(asked), 8):
        chunk = asked[a:a + 8]
        got = case.worst([float(e) for e in chunk], side)
        for e, row in zip(chunk, got):
            at[e.tobytes()] = row
    cand = case.candidates()
    n_checked = 0
    for r in range(n):
        finite = np.isfinite(eps[r])
        full = bool(finite.all())
        last = eps[r][finite][-1] if finite.any() else None
        for j in range(k):
            e = eps[r, j]
            if not np.isfinite(e):
                continue
            w = int(at[e.tobytes()][r])
            assert w >= j + 1, (side, r, j, e, w)
            if e > 0:
                wp = int(at[np.nextafter(e, np.float32(0)).astype(np.float32).tobytes()][r])
                assert wp <= j, (side, r, j, e, wp)
            if e < last or not full:
                assert w == int((eps[r] <= e).sum()), (side, r, j, e, w)
            n_checked += 1
        # the items
        nc = int(cand[r].sum())
        live = items[r] >= 0
        assert live.sum() == min(k, nc) and live[:live.sum()].all(), (r, items[r], nc)
        assert np.isposinf(eps[r][~live]).all()
        ids = items[r][live]
        assert len(set(ids.tolist())) == len(ids) and (ids < case.num_cand).all() and cand[r][ids].all(), (r, ids)
        same = eps[r][live][1:] == eps[r][live][:-1]
        assert (np.diff(ids)[same] > 0).all(), (r, ids, eps[r])
    assert ((eps == 0).sum(axis=1) == np.minimum(k, case.positions())).all()
    print(side, "d", case.P.shape[1], "n", n, "cand", case.num_cand, "K", k, "checked", n_checked, "eps asked",
          len(asked), "zeros", int((eps == 0).sum()), "inf", int(np.isinf(eps).sum()))
    return eps, items


# ---- mixed entries -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_case(d, n=13, scale=1.0):
    """n entries (13: not a multiple of 8; one user twice), 1,500 candidates of 1,507 item rows, sigma =
    0.1 tables.  Exclusion lists unsorted, with repeats, -1 and ids >= num_cand; entry 2 excludes its
    own test item; entry 5's test item is an item row but no candidate; entry 6's user row is 0 (the
    item-side base is 0, every m is 0); row 9 of Q is a copy of entry 0's test item (D = 0, m = 0) and
    row 10 differs from it only where entry 0's user row is 0 (m = 0, D > 0): both have eps_c = 0."""
    rng = np.random.default_rng(1900 + d)
    U1, I1, num_cand = 40, 1507, 1500
    P = (0.1 * rng.standard_normal((U1, d))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((I1, d))).astype(np.float32)
    users = rng.permutation(U1)[:13].astype(np.int32)
    users[11] = users[3]
    tests = rng.choice(np.arange(20, num_cand), 13, replace=False).astype(np.int32)
    tests[5] = 1503
    P[users[6]] = 0.0
    P[users[0], 1] = 0.0
    lift_tests(P, Q, users, tests, num_cand)
    Q[9] = Q[tests[0]]
    Q[10] = Q[tests[0]]
    Q[10, 1] += np.float32(0.25)
    elists = []
    for r in range(13):
        e = rng.integers(20, num_cand, 20)
        e = np.concatenate([e, e[:4], [-1, num_cand + 5, num_cand]])
        elists.append(rng.permutation(e).astype(np.int32))
    elists[2] = np.concatenate([elists[2], [tests[2]]]).astype(np.int32)
    if scale != 1.0:
        P, Q = (P * np.float32(scale)).astype(np.float32), (Q * np.float32(scale)).astype(np.float32)
    return Case(P, Q, users[:n], tests[:n], num_cand, elists[:n])


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("d", [4, 8, 64, 100])
def test_mixed_entries(d, side):
    case = mixed_case(d)
    eps, items = check_case(case, 10, side)
    assert np.isfinite(eps).all() and (eps > 0).any()
    # the twin of entry 0's test item and the candidate that ties with it in score: eps_c = 0, in id order
    zeros = items[0][eps[0] == 0].tolist()
    assert 9 in zeros and 10 in zeros and zeros == sorted(zeros)
    assert (eps[6] == 0).all()  # p = 0: every margin is 0, and on the item side the base too
    # equal calls give equal bits
    again = case.radius(10, side)
    assert eps.tobytes() == again[0].tobytes() and items.tobytes() == again[1].tobytes()
    # an entry alone gets the list it gets among others (tile position and neighbours do not matter)
    for r in (0, 5, 8, 12):
        alone = case.radius(10, side, rows=slice(r, r + 1))
        assert alone[0].tobytes() == eps[r].tobytes() and alone[1].tobytes() == items[r].tobytes()
    # radius@k for k <= K is a prefix: a smaller K gives the head of the list
    head = case.radius(3, side)
    assert head[0].tobytes() == eps[:, :3].tobytes() and head[1].tobytes() == items[:, :3].tobytes()


def test_null_exclusion_lists():
    case = mixed_case(8)
    bare = Case(case.P.cpu().numpy(), case.Q.cpu().numpy(), case.users, case.tests, case.num_cand, None)
    for side in SIDES:
        eps, _ = check_case(bare, 10, side)
        assert (eps <= case.radius(10, side)[0]).all()  # more candidates: no radius grows


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_entry_tile_edges(n):
    for side in SIDES:
        check_case(mixed_case(8, n=n), 10, side)


@pytest.mark.parametrize("k", [1, 2, 128])
def test_selection_sizes(k):
    for side in SIDES:  # entry 7 is at position 0 without a twin: its first radius is positive
        eps, _ = check_case(mixed_case(8, n=8), k, side)
        assert eps[7, 0] > 0


def test_denormal_tables_take_the_bisection():
    """Tables scaled by 1e-20 at d = 4: the margins are denormal (about 1e-42) and eps * D moves in
    steps of the denormal spacing, so the neighbour steps do not settle and the bisection finishes."""
    case = mixed_case(4, n=3, scale=1e-20)
    assert float(case.P.abs().max()) < 1e-19
    for side in SIDES:
        eps, _ = check_case(case, 10, side)
        assert (eps[np.isfinite(eps)] > 0).any()


# ---- window and bitmap edges, few candidates ------------------------------------------------
@pytest.mark.parametrize("num_cand", [1, 255, 256, 257, 2049, 2053])
def test_window_edges(num_cand):
    """The edges of the 256-candidate window and of the 2,048-candidate bitmap; K = 10 is above the
    candidate count at num_cand = 1 (padding), and entry 2's test item is outside the range."""
    rng = np.random.default_rng(num_cand)
    P = (0.1 * rng.standard_normal((12, 8))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((num_cand + 3, 8))).astype(np.float32)
    users = rng.permutation(12)[:9].astype(np.int32)
    tests = rng.integers(0, num_cand, 9).astype(np.int32)
    tests[0], tests[1], tests[2] = num_cand - 1, 0, num_cand + 1
    elists = [np.concatenate([rng.integers(0, num_cand, 10), [num_cand - 1, num_cand, 0, -1]]).astype(np.int32)
              for _ in users]
    elists[3] = np.zeros(0, np.int32)
    elists[2] = np.array([-1, num_cand + 1], np.int32)  # nothing inside the range: t >= num_cand, all candidates
    lift_tests(P, Q, users, tests, num_cand)
    case = Case(P, Q, users, tests, num_cand, elists)
    for side in SIDES:
        eps, items = check_case(case, 10, side)
        assert (items[2] >= 0).sum() == min(10, num_cand)


def test_k_above_the_candidate_count():
    rng = np.random.default_rng(5)
    P = (0.1 * rng.standard_normal((4, 8))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((40, 8))).astype(np.float32)
    elists = [np.arange(3, 40, dtype=np.int32), np.zeros(0, np.int32), np.arange(40, dtype=np.int32)]
    lift_tests(P, Q, [0, 1, 2], [1, 5, 7], 40)
    case = Case(P, Q, [0, 1, 2], [1, 5, 7], 40, elists)
    for side in SIDES:
        eps, items = check_case(case, 64, side)
        assert (items[0] >= 0).sum() == 2 and (items[1] >= 0).sum() == 39 and (items[2] == -1).all()
        assert np.isposinf(eps[2]).all() and set(items[0][:2].tolist()) == {0, 2}


# ---- tile switch, large d ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [512, 516])
def test_tile_threshold(d):
    """d = 512 is the last size with 8 entries per workgroup (the LDS opt-in), 516 the first with 4."""
    rng = np.random.default_rng(d)
    n_cand = 260
    P = (0.1 * rng.standard_normal((10, d))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((n_cand, d))).astype(np.float32)
    tests = rng.choice(n_cand, 9, replace=False)
    lift_tests(P, Q, np.arange(9), tests, n_cand)
    case = Case(P, Q, np.arange(9), tests, n_cand, None)
    for side in SIDES:
        check_case(case, 10, side)


def test_large_d():
    rng = np.random.default_rng(74)
    d, n_cand = 1024, 300
    P = (0.1 * rng.standard_normal((5, d))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((n_cand + 2, d))).astype(np.float32)
    elists = [np.concatenate([rng.integers(0, n_cand, 12), [-1, n_cand]]).astype(np.int32) for _ in range(3)]
    tests = rng.choice(n_cand, 3, replace=False)
    lift_tests(P, Q, [4, 0, 2], tests, n_cand)
    case = Case(P, Q, [4, 0, 2], tests, n_cand, elists)
    for side in SIDES:
        check_case(case, 10, side)


# ---- strips and merge ------------------------------------------------------------------------
def test_strips_and_merge():
    """3 entries x 70,000 candidates at d = 8: 274 strips of one window, their partial lists and the
    merge.  The reference comes from the same call with ONE strip (2,048 tiles of 8 entries: the 3
    entries repeated) on each half of the candidates, the second half moved to the front of a copy
    of Q with the test items' rows behind it, merged on the host by (eps, id)."""
    ops = _ops()
    rng = np.random.default_rng(73)
    n_cand, half, k, reps = 70000, 35000, 10, 16384
    P = (0.1 * rng.standard_normal((5, 8))).astype(np.float32)
    Q = (0.1 * rng.standard_normal((n_cand, 8))).astype(np.float32)
    users = np.array([4, 0, 2], np.int32)
    tests = np.array([123, 35000 + 77, 69999], np.int32)
    elists = [np.concatenate([rng.integers(0, n_cand, 50), [-1, n_cand + 5]]).astype(np.int32) for _ in users]
    lift_tests(P, Q, users, tests, n_cand)
    case = Case(P, Q, users, tests, n_cand, elists)
    assert ops.eval_radius_workspace(3, n_cand, k) == 16 + 3 * 274 * k * 8
    assert ops.eval_radius_workspace(reps, half, k) == 16 + reps * k * 8  # one strip
    ru, rt = np.tile(users, reps // 3 + 1)[:reps], np.tile(tests, reps // 3 + 1)[:reps]
    rl = (elists * (reps // 3 + 1))[:reps]
    QB = np.concatenate([Q[half:], Q[tests]])  # candidate c of the second half is row c - half; t of entry r is row half + r
    tB = np.tile(half + np.arange(3), reps // 3 + 1)[:reps]
    # ids below `half` turn negative and are ignored; a test item of the second half must not count there
    lB = [np.concatenate([e.astype(np.int64) - half, [int(t) - half]]).astype(np.int32) for e, t in zip(rl, rt)]
    first, second = Case(P, Q, ru, rt, half, rl), Case(P, QB, ru, tB, half, lB)
    for side in SIDES:
        eps, items = check_case(case, k, side)
        ea, ia = first.radius(k, side)
        eb, ib = second.radius(k, side)
        for r in range(3):
            e2 = np.concatenate([ea[r], eb[r]])
            i2 = np.concatenate([ia[r], np.where(ib[r] >= 0, ib[r] + half, -1)])
            keep = i2 >= 0
            order = np.lexsort((i2[keep], e2[keep]))[:k]
            assert e2[keep][order].tobytes() == eps[r].tobytes(), (side, r)
            assert (i2[keep][order] == items[r]).all(), (side, r)
        again = case.radius(k, side)
        assert again[0].tobytes() == eps.tobytes() and again[1].tobytes() == items.tobytes()


# ---- the prune path --------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 128])
def test_every_candidate_passes_the_threshold(k):
    """1,500 candidates whose eps_c falls with the id: p = e_0, q_t = (2, 0, ..), q_c = (1 + c / 2048,
    1, ..), so m_c = 1 - c / 2048 exactly and D_c = sqrt(m_c^2 + 1): each candidate beats every
    earlier one, is appended, and the buffers are pruned at every step."""
    n_cand = 1500
    P = np.zeros((2, 4), np.float32)
    P[:, 0] = 1.0
    Q = np.zeros((n_cand + 1, 4), np.float32)
    Q[:n_cand, 0] = 1.0 + np.arange(n_cand, dtype=np.float32) / np.float32(2048.0)
    Q[:n_cand, 1] = 1.0
    Q[n_cand, 0] = 2.0
    case = Case(P, Q, [0, 1], [n_cand, n_cand], n_cand, [np.array([1499, -1], np.int32), np.zeros(0, np.int32)])
    for side in SIDES:
        eps, items = check_case(case, k, side)
        assert items[1].tolist() == list(range(1499, 1499 - k, -1))
        assert items[0].tolist() == list(range(1498, 1498 - k, -1))
        assert (np.diff(eps, axis=1) > 0).all() and (eps > 0).all()


# ---- range check, arguments, torch op ----------------------------------------------------------
def test_range_check():
    nat = importlib.import_module(PKG + "._native")
    case = mixed_case(8)
    for bad_u, bad_t in ((40, None), (-1, None), (None, 1507), (None, -2)):
        u, t = case.users.copy(), case.tests.copy()
        if bad_u is not None:
            u[4] = bad_u
        if bad_t is not None:
            t[4] = bad_t
        broken = Case(case.P.cpu().numpy(), case.Q.cpu().numpy(), u, t, case.num_cand, case.elists)
        with pytest.raises(nat.NativeIndexError):
            broken.radius(10, "user")
        got = broken.radius(10, "user", check=False)  # read as row 0: no error
        u[4], t[4] = (0, t[4]) if bad_u is not None else (u[4], 0)
        want = Case(case.P.cpu().numpy(), case.Q.cpu().numpy(), u, t, case.num_cand, case.elists).radius(10, "user")
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    ops = _ops()
    nat = importlib.import_module(PKG + "._native")
    case = mixed_case(8)
    ok = dict(P=case.P, Q=case.Q, users=case.users, test_items=case.tests, num_candidates=case.num_cand)
    need = ops.eval_radius_workspace(len(case.users), case.num_cand, 10)
    short = torch.empty(need // 8 - 1, dtype=torch.int64, device=DEV)
    # the native entry refuses them too (ACF_E_INVALID), before any launch: the outputs stay as they were
    eps = torch.full((len(case.users), 10), -7.0, device=DEV)
    items = torch.full((len(case.users), 10), -7, dtype=torch.int32, device=DEV)
    u, t = torch.tensor(case.users, device=DEV), torch.tensor(case.tests, device=DEV)
    work = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
    def native(k=10, side=0, nbytes=need):  # noqa: E306
        nat.call("acf_eval_radius", case.P.data_ptr(), case.Q.data_ptr(), case.P.shape[0], case.Q.shape[0], 8,
                 u.data_ptr(), t.data_ptr(), len(case.users), case.num_cand, None, None, k, side, eps.data_ptr(),
                 items.data_ptr(), work.data_ptr(), nbytes, 0, None)
    for bad in (dict(k=0), dict(k=129), dict(side=2), dict(nbytes=need - 8)):
        with pytest.raises(nat.NativeError, match="k must|side must|workspace too small"):
            native(**bad)
    torch.cuda.synchronize()
    assert (eps == -7.0).all() and (items == -7).all()

    # a caller's workspace is measured against the host-only query, in Python
    for bad in (dict(workspace=short), dict(workspace=short.cpu()), dict(workspace=work.reshape(1, -1))):
        with pytest.raises(ValueError, match="workspace"):
            ops.eval_radius(**{**ok, **bad})
    with pytest.raises(TypeError, match="workspace"):
        ops.eval_radius(**ok, workspace=torch.empty(need, dtype=torch.int32, device=DEV))

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(ops, "call", boom)
    for bad in (dict(k=0), dict(k=129), dict(k=2.5), dict(side="both"), dict(side=1),
                dict(test_items=case.tests[:-1])):
        with pytest.raises(ValueError):
            ops.eval_radius(**{**ok, **bad})


def test_caller_workspace():
    ops = _ops()
    case = mixed_case(8)
    need = ops.eval_radius_workspace(len(case.users), case.num_cand, 10)
    work = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    eo, ef = case.excl
    for side in SIDES:
        got = ops.eval_radius(case.P, case.Q, case.users, case.tests, case.num_cand, eo, ef, k=10, side=side,
                              workspace=work)
        want = case.radius(10, side)
        assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and (got[1].cpu().numpy() == want[1]).all()


def test_torch_op():
    ops = _ops()
    tops = importlib.import_module(PKG + ".torch_ops").load()
    case = mixed_case(8)
    tu, tt = torch.tensor(case.users, device=DEV), torch.tensor(case.tests, device=DEV)
    teo, tef = (torch.tensor(a, device=DEV) for a in case.excl)
    for side in SIDES:
        want = ops.eval_radius(case.P, case.Q, tu, tt, case.num_cand, teo, tef, k=10, side=side)
        got = tops.eval_radius(case.P, case.Q, tu, tt, case.num_cand, teo, tef, 10, side)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        none = tops.eval_radius(case.P, case.Q, tu, tt, case.num_cand, teo[:0], tef[:0], 4, side)
        bare = ops.eval_radius(case.P, case.Q, tu, tt, case.num_cand, k=4, side=side)
        assert torch.equal(none[0], bare[0]) and torch.equal(none[1], bare[1])
    dflt = tops.eval_radius(case.P, case.Q, tu, tt, case.num_cand, teo, tef)
    want = ops.eval_radius(case.P, case.Q, tu, tt, case.num_cand, teo, tef)
    assert tuple(dflt[0].shape) == (13, 10) and torch.equal(dflt[0], want[0]) and torch.equal(dflt[1], want[1])
    with pytest.raises(IndexError):
        tops.eval_radius(case.P, case.Q, tu + 1000, tt, case.num_cand, teo, tef, 10, "user")
    for bad in (dict(k=0), dict(k=129), dict(side="both")):
        with pytest.raises(RuntimeError):
            tops.eval_radius(case.P, case.Q, tu, tt, case.num_cand, teo, tef, bad.get("k", 10), bad.get("side", "user"))


# ---- end to end ---------------------------------------------------------------------------------
def test_radius_curve_is_certified_end_to_end(acf, tmp_path, monkeypatch):
    """A small MF trained for two BPR epochs and an all-items plan: radius_curve(eps, K, E) is
    certified(..., E, cutoffs=(K,))'s hr_lb, on both sides; the model layers return the same arrays."""
    ev = _ev()
    data = importlib.import_module(PKG + ".data")
    monkeypatch.chdir(tmp_path)
    ds = data.get_dataset("synthetic:60:200:1500")
    plan = ev.init_eval_model(ds, Namespace(eval_mode="all"))
    args = Namespace(path=str(tmp_path) + "/", opath="t/", dataset="synthetic", model="bpr", verbose=1,
                     batch_size=512, epochs=1, adv_epoch=0, embed_size=16, dns=1, reg=0.0, lr=0.05, reg_adv=1.0,
                     restore=None, ckpt=0, task="", adv="grad", eps=0.5, eval_mode="all", seed=11, adver=0)
    m = acf.MF(ds.num_users, ds.num_items, args).build_graph(device=torch.device(DEV))
    before = m.embedding_P.clone()
    acf.training(m, ds, args, "run", 0, args.epochs, "TS")
    assert not torch.equal(before, m.embedding_P)
    E, K = [0.0, 0.05, 0.5], 10
    curves = {}
    for side in SIDES:
        eps, items = m.certified_radius(plan, k=K, side=side)
        assert tuple(eps.shape) == (len(plan.users), K) and items.dtype == torch.int32
        rows = ev.certified(m, plan, E, side=side, cutoffs=(K,))
        curves[side] = ev.radius_curve(eps.cpu().numpy(), K, E)
        print(side, "hr_lb", [r[3] for r in rows], "radius_curve", curves[side])
        np.testing.assert_allclose(curves[side], [r[3] for r in rows], rtol=0, atol=1e-12)
        # every smaller cutoff from the same arrays
        rows3 = ev.certified(m, plan, E, side=side, cutoffs=(3,))
        np.testing.assert_allclose(ev.radius_curve(eps.cpu().numpy(), 3, E), [r[3] for r in rows3], rtol=0, atol=1e-12)
        again = ev.certified_radius((m.embedding_P, m.embedding_Q), plan, k=K, side=side)
        assert torch.equal(again[0], eps) and torch.equal(again[1], items)
        via_apr = acf.APR.certified_radius.__get__(Namespace(_ensure=lambda: None, model=m))(plan, k=K, side=side)
        assert torch.equal(via_apr[0], eps)
        summary = ev.radius_summary(eps.cpu().numpy(), (1, K))
        assert [r[0] for r in summary] == [1, K] and all(0.0 <= r[1] <= 1.0 and 0.0 <= r[2] <= 1.0 for r in summary)
    assert curves["user"][0] == curves["item"][0]  # eps = 0 is the same ranking on either side
    assert tuple(m.certified_radius(plan)[0].shape) == (len(plan.users), plan.K)  # k defaults to plan.K


def test_cli_writes_radius_file(acf, tmp_path, monkeypatch):
    import glob
    cli = importlib.import_module(PKG + ".cli")
    monkeypatch.chdir(tmp_path)
    rc = cli.main(["--path", str(tmp_path) + "/", "--opath", "t/", "--dataset", "synthetic:300:200:8000",
                   "--model", "bpr", "--epochs", "1", "--verbose", "1", "--embed_size", "16",
                   "--certify_radius", "1,10", "--certify_side", "both"])
    assert rc == 0
    files = glob.glob(str(tmp_path / "out" / "t" / "*.radius"))
    assert len(files) == 1
    rows = cli.read_radius(files[0])
    assert [(r[0], r[1]) for r in rows] == [(s, K) for s in SIDES for K in (1, 10)]
    assert all(0.0 <= r[2] <= 1.0 and 0.0 <= r[3] <= 1.0 for r in rows)
    assert rows[0][2] == rows[2][2] and rows[1][2] == rows[3][2]  # radius 0 is the same ranking on either side
    for r in rows:
        qs = [q for q in r[4:] if not np.isnan(q)]
        assert qs == sorted(qs) and all(q >= 0 for q in qs)
    assert rows[1][2] <= rows[0][2]  # missing the top 10 implies missing the top 1
