"""Certified worst-case positions without a GPU: the header and the binding, the
host-only workspace query, the checks that fire before any launch, the CLI flags
and file, and the float64 restatement (the yardstick of the GPU tests): its
eps = 0 row, its monotonicity and the soundness of the bound under sampled
perturbations of the budget."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, REPO

NAMES = ("acf_eval_positions_worst_workspace", "acf_eval_positions_worst")


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".evaluate")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module(PKG + ".cli")


@pytest.fixture(scope="module")
def native():
    return importlib.import_module(PKG + "._native")


def test_header_binding_and_exports(native):
    text = open(os.path.join(REPO, "include", "acf_apr.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in native.SIGNATURES
    assert set(NAMES) <= native.exported_symbols()
    build_native = importlib.import_module(PKG + ".build_native")
    assert any(h.endswith("csrc/acf_eval_worst.h") for h in build_native.LIBS["apr"]["headers"])
    assert "eval_positions_worst" in importlib.import_module(PKG + ".torch_ops").OPS


def _ws(native, n_users, num_cand, n_eps):
    size = ctypes.c_size_t(0)
    rc = native.load().acf_eval_positions_worst_workspace(n_users, num_cand, n_eps, ctypes.byref(size))
    return rc, size.value


def test_workspace_query_is_host_only(native):
    # (no device in this process: the query must not need one)
    rc, one = _ws(native, 6040, 3706, 8)
    assert rc == native.ACF_OK
    assert one < 6040 * 3706 * 4 // 8  # far below the U x I score array
    rc, few = _ws(native, 3, 70000, 4)
    assert rc == native.ACF_OK and few >= 16 + 2 * 4 * 3 * 4  # several strips' counts
    assert few < 3 * 70000 * 4 // 8
    rc, single = _ws(native, 100000, 1000, 8)
    assert rc == native.ACF_OK and single < 1 << 20  # enough tiles: one strip, no partial counts
    assert _ws(native, 0, 1, 1)[0] == native.ACF_OK
    for bad in ((-1, 100, 1), (3, 0, 1), (3, -7, 1), (3, 100, 0), (3, 100, 9), (3, 100, -1)):
        assert _ws(native, *bad)[0] == native.ACF_E_INVALID, bad
    assert native.load().acf_eval_positions_worst_workspace(3, 100, 1, None) == native.ACF_E_INVALID
    ops = importlib.import_module(PKG + ".ops")
    assert ops.eval_positions_worst_workspace(3, 70000, 4) == few


def test_bad_arguments_are_invalid_before_any_launch(native):
    lib = native.load()
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)  # a non-NULL pointer that is never dereferenced
    eps = (ctypes.c_float * 9)(0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0)
    names = ("P", "Q", "U1", "I1", "d", "users", "tests", "n", "cand", "eoff", "ex", "eps", "ne", "side", "out", "ws",
             "wsb", "check", "stream")
    ok = dict(P=p, Q=p, U1=10, I1=100, d=8, users=p, tests=p, n=2, cand=100, eoff=None, ex=None, eps=eps, ne=3,
              side=0, out=p, ws=p, wsb=1 << 20, check=0, stream=None)
    worst = lambda **k: lib.acf_eval_positions_worst(*[{**ok, **k}[a] for a in names])  # noqa: E731
    f = lambda *v: (ctypes.c_float * len(v))(*v)  # noqa: E731
    for bad in (dict(ne=0), dict(ne=9), dict(eps=f(0.5, -0.25), ne=2), dict(eps=f(float("nan")), ne=1),
                dict(eps=f(0.5, float("inf")), ne=2), dict(eps=None), dict(side=2), dict(side=-1), dict(wsb=8),
                dict(n=-1), dict(cand=0), dict(cand=101), dict(out=None), dict(ws=None), dict(d=6), dict(eoff=p),
                dict(users=None), dict(tests=None)):
        assert worst(**bad) == native.ACF_E_INVALID, bad
    assert worst(n=0) == native.ACF_OK  # nothing to do: no launch, no device


def test_checks_fire_before_any_native_call(monkeypatch):
    ops = importlib.import_module(PKG + ".ops")
    nat = importlib.import_module(PKG + "._native")

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(ops, "call", boom)
    monkeypatch.setattr(nat, "call", boom)
    P, Q = torch.zeros(6, 8), torch.zeros(20, 8)
    ok = dict(P=P, Q=Q, users=np.array([0, 3], np.int32), test_items=np.array([1, 2], np.int32), num_candidates=20,
              eps=(0.0, 0.5))

    def fails(match, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            ops.eval_positions_worst(**{**ok, **kw})

    fails("eps", eps=(0.5, -0.1))
    fails("eps", eps=(float("nan"),))
    fails("eps", eps=(float("inf"),))
    fails("eps", eps=())
    fails("eps", eps=tuple(0.1 * k for k in range(9)))
    fails("eps", eps=0.5)
    fails("side", side="both")
    fails("side", side=0)
    fails("test_items", test_items=np.array([1.0, 2.0]))
    fails("test_items", test_items=np.array([1, 2, 3], np.int32))
    fails("users", users=np.array([0.5, 3.0]))
    fails("go together", excl_off=np.array([0, 0, 0]))
    fails("excl_off", excl_off=np.array([0, 1]), excl_items=np.array([4], np.int32))
    fails(r"excl_off\[-1\]", excl_off=np.array([0, 1, 3]), excl_items=np.array([4, 5], np.int32))
    fails("excl_items", excl_off=np.array([0, 1, 2]), excl_items=np.array([4.0, 5.0]))
    fails("num_candidates", num_candidates=0)
    fails("num_candidates", num_candidates=21)
    fails("num_candidates", num_candidates=20.0)
    fails("float32", exc=TypeError, Q=Q.double())
    fails("float32", exc=TypeError, P=P.half())
    fails("HIP device")  # CPU tables: there is no CPU path


@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_cli_flags_and_file(cli, flavor, tmp_path):
    a = cli.parse_args([], flavor)
    assert a.certify_eps == [] and a.certify_side == "user"
    a = cli.parse_args(["--certify_eps", "0.1, 0.5,1", "--certify_side", "both"], flavor)
    assert a.certify_eps == [0.1, 0.5, 1.0] and a.certify_side == "both"
    assert cli.parse_args(["--certify_side", "item"], flavor).certify_side == "item"
    for bad in (["--certify_eps", "-1"], ["--certify_eps", "x"], ["--certify_eps", "inf"],
                ["--certify_side", "joint"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad, flavor)
    rows = [("user", 0.0, 100, 0.75, 1.0 / 3, 0.9), ("user", 0.1, 100, 0.5, 0.2, 0.8),
            ("item", 1e-3, 10, 0.0, 0.0, 1.0 / 7)]
    cli.write_certified(str(tmp_path / "o"), "run.certified", rows)
    lines = (tmp_path / "o" / "run.certified").read_text().splitlines()
    assert len(lines) == 3 and all(len(ln.split("\t")) == 6 for ln in lines)
    got = cli.read_certified(str(tmp_path / "o" / "run.certified"))
    assert got == rows and isinstance(got[0][2], int)
    (tmp_path / "bad.certified").write_text("user\t0.5\t100\t0.1\t0.2\n")
    with pytest.raises(ValueError):
        cli.read_certified(str(tmp_path / "bad.certified"))


def test_model_layers_expose_certified(acf):
    model = importlib.import_module(PKG + ".model")
    rec = importlib.import_module(PKG + ".recommender")
    for cls in (model.MF, rec.APR):
        assert callable(cls.certified)


def test_certified_refuses_a_sampled_plan_and_bad_arguments(ev):
    sampled = ev.EvalPlan("sample", np.arange(2), np.arange(2), np.ones(2), 10)
    tables = (torch.zeros(2, 4), torch.zeros(5, 4))
    with pytest.raises(ValueError, match="all-items"):
        ev.certified(tables, sampled, [0.5])
    plan = ev.EvalPlan("all", np.arange(2), np.arange(2), np.ones(2), 100, excl_off=np.zeros(3, np.int64),
                       excl=np.zeros(0, np.int32), num_candidates=5)
    with pytest.raises(ValueError, match="side"):
        ev.certified(tables, plan, [0.5], side="both")
    with pytest.raises(ValueError, match="eps"):
        ev.certified(tables, plan, [-0.5])


# ---- the float64 restatement ---------------------------------------------------
N_USERS, N_ITEMS, N_CAND = 13, 1500, 1493


def _case(d, sigma, seed):
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((N_USERS, d)) * sigma).astype(np.float32)
    Q = (rng.standard_normal((N_ITEMS, d)) * sigma).astype(np.float32)
    users = np.arange(N_USERS)
    tests = rng.integers(0, N_CAND, N_USERS)
    excl = [rng.integers(-1, N_ITEMS, rng.integers(0, 40)) for _ in range(N_USERS)]
    return P, Q, users, tests, excl


def _cand(tests, excl):
    cand = np.ones((N_USERS, N_CAND), bool)
    for r in range(N_USERS):
        e = np.asarray(excl[r])
        cand[r, e[(e >= 0) & (e < N_CAND)]] = False
        cand[r, tests[r]] = False
    return cand


def _radius(ev, P, Q, users, tests, excl, side):
    """Per entry, the median over its candidates of the eps at which the candidate flips."""
    m, base, cand = ev.worst_margins_host(P, Q, users, tests, N_CAND, excl, side)
    return np.array([np.median(np.abs(m[r][cand[r]]) / np.maximum(base[r][cand[r]], 1e-300)) for r in range(N_USERS)])


@pytest.mark.parametrize("side", ["user", "item"])
@pytest.mark.parametrize("d", [4, 8, 64, 100])
def test_restatement_eps0_monotone_and_sound(ev, d, side):
    """eps = 0 is #{score >=}; rows do not decrease in eps; and for random delta
    with |delta| = eps (user side: on p; item side: an independent one per item
    row) the float64 position of t never exceeds the float64 worst position.
    Per user four eps: 0 and 0.25x, 1x, 4x the median pairwise radius."""
    rng = np.random.default_rng(100 + d)
    for sigma in (0.01, 0.1, 1.0):
        P, Q, users, tests, excl = _case(d, sigma, seed=d * 7 + int(sigma * 100))
        cand = _cand(tests, excl)
        P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
        scores = P64[users] @ Q64[:N_CAND].T
        st = np.einsum("nd,nd->n", P64[users], Q64[tests])
        zero = ev.worst_positions_host(P, Q, users, tests, N_CAND, excl, [0.0], side)
        assert zero.shape == (1, N_USERS) and zero.dtype == np.int64
        assert (zero[0] == ((scores >= st[:, None]) & cand).sum(1)).all()
        radius = _radius(ev, P, Q, users, tests, excl, side)
        for r in range(N_USERS):
            eps = [0.0, 0.25 * radius[r], radius[r], 4.0 * radius[r]]
            worst = ev.worst_positions_host(P, Q, users[r:r + 1], tests[r:r + 1], N_CAND, [excl[r]], eps, side)[:, 0]
            assert worst[0] == zero[0, r]
            assert (np.diff(worst) >= 0).all()
            assert worst[-1] > worst[0] or worst[0] == cand[r].sum()  # the scale is the right one: counts move
            for e, w in zip(eps, worst):
                for _ in range(3):
                    if side == "user":
                        delta = rng.standard_normal(d)
                        p = P64[r] + e * delta / np.linalg.norm(delta)
                        s, t = Q64[:N_CAND] @ p, Q64[tests[r]] @ p
                    else:
                        delta = rng.standard_normal((N_ITEMS, d))
                        Qd = Q64 + e * delta / np.linalg.norm(delta, axis=1, keepdims=True)
                        s, t = Qd[:N_CAND] @ P64[r], Qd[tests[r]] @ P64[r]
                    assert ((s >= t) & cand[r]).sum() <= w, (sigma, r, e)


def test_restatement_reaches_the_bound_for_one_candidate(ev):
    """The inequality is tight: for a single candidate the delta along q_c - q_t
    (user side) at the threshold eps puts it at t's score, and a smaller one does not."""
    P, Q, users, tests, excl = _case(8, 0.1, seed=5)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    m, base, cand = ev.worst_margins_host(P, Q, users, tests, N_CAND, excl, "user")
    r = 0
    c = int(np.flatnonzero(cand[r] & (m[r] > 0))[0])
    e = m[r, c] / base[r, c]
    direction = (Q64[c] - Q64[tests[r]]) / base[r, c]
    for scale, reached in ((1.0 + 1e-9, True), (1.0 - 1e-6, False)):
        p = P64[r] + scale * e * direction
        assert (Q64[c] @ p >= Q64[tests[r]] @ p) == reached


def test_restatement_identical_rows_count_at_every_eps(ev):
    P, Q, users, tests, _ = _case(8, 0.1, seed=6)
    tests[0], dup = 11, 7
    Q[dup] = Q[tests[0]]
    m, base, cand = ev.worst_margins_host(P, Q, users, tests, N_CAND, None, "user")
    assert m[0, dup] == 0.0 and base[0, dup] == 0.0 and cand[0, dup]
    for side in ("user", "item"):
        eps = [0.0, 0.01, 1.0]
        a = ev.worst_positions_host(P, Q, users[:1], tests[:1], N_CAND, None, eps, side)
        b = ev.worst_positions_host(P, Q, users[:1], tests[:1], N_CAND, [[dup]], eps, side)
        assert (a == b + 1).all()  # the twin counts at every eps, 0 included
