"""The certified radius without a GPU: the header, the binding and the checks that
fire before any launch; evaluate.min_eps_f32 (the per-candidate minimum in numpy
float32, with the kernel's operations) is minimal; evaluate.radius_host (float64)
agrees with it within the bound that follows from the rounding band of
tests/test_gpu_eval_worst.py; radius_curve is the hit rate of the worst-case
positions; the .radius file round-trips."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, REPO

NAMES = ("acf_eval_radius_workspace", "acf_eval_radius")
F32_MAX = np.float32(np.finfo(np.float32).max)


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
    assert any(h.endswith("csrc/acf_eval_radius.h") for h in build_native.LIBS["apr"]["headers"])
    assert "eval_radius" in importlib.import_module(PKG + ".torch_ops").OPS
    rank = open(os.path.join(REPO, PKG, "csrc", "acf_rank.hip")).read()
    assert rank.index('#include "acf_eval_worst.h"') < rank.index('#include "acf_eval_radius.h"')


def test_workspace_query_is_host_only(native):
    def ws(*a):
        size = ctypes.c_size_t(0)
        return native.load().acf_eval_radius_workspace(*a, ctypes.byref(size)), size.value
    rc, one = ws(6040, 3706, 100)
    assert rc == native.ACF_OK and 16 + 6040 * 100 * 8 <= one < 6040 * 3706 * 4
    rc, few = ws(3, 70000, 10)
    assert rc == native.ACF_OK and few >= 16 + 2 * 3 * 10 * 8  # several strips' partial lists
    assert ws(0, 1, 1)[0] == native.ACF_OK
    for bad in ((-1, 100, 1), (3, 0, 1), (3, -7, 1), (3, 100, 0), (3, 100, 129), (3, 100, -1)):
        assert ws(*bad)[0] == native.ACF_E_INVALID, bad
    assert native.load().acf_eval_radius_workspace(3, 100, 1, None) == native.ACF_E_INVALID
    assert importlib.import_module(PKG + ".ops").eval_radius_workspace(3, 70000, 10) == few


def test_bad_arguments_are_invalid_before_any_launch(native):
    lib = native.load()
    one = (ctypes.c_int64 * 2)()
    p = ctypes.addressof(one)  # a non-NULL, 8-byte aligned pointer that is never dereferenced
    names = ("P", "Q", "U1", "I1", "d", "users", "tests", "n", "cand", "eoff", "ex", "k", "side", "eps", "items", "ws",
             "wsb", "check", "stream")
    ok = dict(P=p, Q=p, U1=10, I1=100, d=8, users=p, tests=p, n=2, cand=100, eoff=None, ex=None, k=10, side=0,
              eps=p, items=p, ws=p, wsb=1 << 20, check=0, stream=None)
    radius = lambda **k: lib.acf_eval_radius(*[{**ok, **k}[a] for a in names])  # noqa: E731
    for bad in (dict(k=0), dict(k=129), dict(k=-3), dict(side=2), dict(side=-1), dict(wsb=8), dict(ws=p + 4),
                dict(n=-1), dict(cand=0), dict(cand=101), dict(eps=None), dict(items=None), dict(ws=None),
                dict(d=6), dict(eoff=p), dict(users=None), dict(tests=None), dict(P=None), dict(Q=None)):
        assert radius(**bad) == native.ACF_E_INVALID, bad
    assert radius(n=0) == native.ACF_OK  # nothing to do: no launch, no device


def test_checks_fire_before_any_native_call(monkeypatch):
    ops = importlib.import_module(PKG + ".ops")
    nat = importlib.import_module(PKG + "._native")

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(ops, "call", boom)
    monkeypatch.setattr(nat, "call", boom)
    P, Q = torch.zeros(6, 8), torch.zeros(20, 8)
    ok = dict(P=P, Q=Q, users=np.array([0, 3], np.int32), test_items=np.array([1, 2], np.int32), num_candidates=20)

    def fails(match, exc=ValueError, **kw):
        with pytest.raises(exc, match=match):
            ops.eval_radius(**{**ok, **kw})

    for k in (0, 129, -1, 2.0, True, None):
        fails("k must", k=k)
    fails("side", side="both")
    fails("side", side=0)
    fails("test_items", test_items=np.array([1.0, 2.0]))
    fails("test_items", test_items=np.array([1, 2, 3], np.int32))
    fails("users", users=np.array([0.5, 3.0]))
    fails("go together", excl_off=np.array([0, 0, 0]))
    fails(r"excl_off\[-1\]", excl_off=np.array([0, 1, 3]), excl_items=np.array([4, 5], np.int32))
    fails("num_candidates", num_candidates=0)
    fails("num_candidates", num_candidates=21)
    fails("float32", exc=TypeError, Q=Q.double())
    fails("HIP device")  # CPU tables: there is no CPU path


def test_model_layers_expose_certified_radius(acf):
    model = importlib.import_module(PKG + ".model")
    rec = importlib.import_module(PKG + ".recommender")
    for cls in (model.MF, rec.APR):
        assert callable(cls.certified_radius)
    assert callable(acf.certified_radius)


def test_certified_radius_refuses_a_sampled_plan_and_bad_arguments(ev):
    sampled = ev.EvalPlan("sample", np.arange(2), np.arange(2), np.ones(2), 10)
    tables = (torch.zeros(2, 4), torch.zeros(5, 4))
    with pytest.raises(ValueError, match="all-items"):
        ev.certified_radius(tables, sampled)
    plan = ev.EvalPlan("all", np.arange(2), np.arange(2), np.ones(2), 100, excl_off=np.zeros(3, np.int64),
                       excl=np.zeros(0, np.int32), num_candidates=5)
    with pytest.raises(ValueError, match="side"):
        ev.certified_radius(tables, plan, side="both")
    with pytest.raises(ValueError, match="k must"):
        ev.certified_radius(tables, plan, k=129)


# ---- min_eps_f32: minimality ---------------------------------------------------------
def _pred(m, e, base, side):
    with np.errstate(all="ignore"):
        e = np.asarray(e, np.float32)
        return m <= (e * base if side == "user" else (np.float32(2) * e) * base)


def _assert_minimal(ev, m, base, side):
    """pred(e) and (e == 0 or not pred(prev(e))); +inf exactly where FLT_MAX fails too."""
    e, fb = ev.min_eps_f32(m, base, side, return_fallback=True)
    assert e.dtype == np.float32 and e.shape == m.shape and not np.isnan(e).any() and (e >= 0).all()
    fin = np.isfinite(e)
    assert _pred(m, e, base, side)[fin].all()
    prev = np.nextafter(e, np.float32(0)).astype(np.float32)
    pos = fin & (e > 0)
    assert not _pred(m, prev, base, side)[pos].any()
    assert not _pred(m, np.full_like(m, F32_MAX), base, side)[~fin].any()
    return e, fb


@pytest.mark.parametrize("side", ["user", "item"])
def test_min_eps_is_minimal(ev, side):
    rng = np.random.default_rng(31)
    n = 40000
    # normal range: sigma = 0.1 scores, distances of order 0.1 .. 1
    m = (0.05 * rng.standard_normal(n)).astype(np.float32)
    base = np.abs(0.3 * rng.standard_normal(n)).astype(np.float32) + np.float32(1e-3)
    e, fb = _assert_minimal(ev, m, base, side)
    assert (e[m <= 0] == 0).all() and (e[m > 0] > 0).all() and np.isfinite(e).all()
    print(side, "normal range: settled by the bisection", int(fb.sum()), "of", n)
    # tables scaled by 1e-20: m of the order 1e-40 (denormal), base 1e-20: denormal products
    s = np.float32(1e-20)
    md = ((m * s) * s).astype(np.float32)
    bd = (base * s).astype(np.float32)
    assert (np.abs(md[md != 0]) < np.finfo(np.float32).tiny).all()
    e, fb = _assert_minimal(ev, md, bd, side)
    assert (e[md <= 0] == 0).all() and np.isfinite(e).all() and fb.any()  # the steps do not settle these
    # bases near 1e-38: the quotient overflows; +inf exactly where no finite eps works
    bt = (np.abs(rng.standard_normal(n)) * 1e-38).astype(np.float32)
    mt = np.abs(rng.standard_normal(n)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, n).astype(np.float32)
    e, fb = _assert_minimal(ev, mt, bt, side)
    if side == "user":
        assert np.isinf(e).any() and np.isfinite(e).any()
    else:  # fl(2 e) overflows to +inf from FLT_MAX / 2 on, and +inf times a positive Np passes
        assert np.isfinite(e).all() and (e == e.max()).sum() > 1 and e.max() > F32_MAX / np.float32(2)
    # base 0: +inf for m > 0, 0 otherwise
    e = ev.min_eps_f32(np.array([1.0, 0.0, -1.0, 1e-45], np.float32), np.float32(0.0), side)
    assert e.tolist() == [np.inf, 0.0, 0.0, np.inf]
    # scalars, broadcasting and a bad side
    assert ev.min_eps_f32(-1.0, 2.0, side) == 0.0 and ev.min_eps_f32(np.ones((2, 3)), np.ones(3), side).shape == (2, 3)
    with pytest.raises(ValueError, match="side"):
        ev.min_eps_f32(m, base, "both")


# ---- radius_host against the fp32 restatement --------------------------------------------
N_USERS, N_ITEMS, N_CAND, K = 11, 700, 693, 20


def _case(d, seed):
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((N_USERS, d)) * 0.1).astype(np.float32)
    Q = (rng.standard_normal((N_ITEMS, d)) * 0.1).astype(np.float32)
    users = np.arange(N_USERS)
    tests = rng.integers(0, N_CAND, N_USERS)
    excl = [rng.integers(-1, N_ITEMS, rng.integers(0, 40)) for _ in range(N_USERS)]
    return P, Q, users, tests, excl


def _f32_margins(P, Q, users, tests, side):
    """m, base [n, N_CAND] in float32 by the kernel's chains: sequential round-then-add."""
    n, d = len(users), P.shape[1]
    p, qt, qc = P[users], Q[tests], Q[:N_CAND]
    st, sc = np.zeros(n, np.float32), np.zeros((n, N_CAND), np.float32)
    d2, n2 = np.zeros((n, N_CAND), np.float32), np.zeros(n, np.float32)
    for k in range(d):
        st = st + p[:, k] * qt[:, k]
        sc = sc + p[:, k, None] * qc[None, :, k]
        diff = qt[:, k, None] - qc[None, :, k]
        d2 = d2 + diff * diff
        n2 = n2 + p[:, k] * p[:, k]
    m = st[:, None] - sc
    base = np.sqrt(d2) if side == "user" else np.repeat(np.sqrt(n2)[:, None], N_CAND, axis=1)
    assert m.dtype == np.float32 and base.dtype == np.float32
    return m, base


@pytest.mark.parametrize("side", ["user", "item"])
@pytest.mark.parametrize("d", [4, 8, 64, 100])
def test_radius_host_agrees_with_the_fp32_restatement(ev, d, side):
    """Per candidate, by the band of the fp32 predicate (m and eps * base each within
    2^-23 ((d + 2) |p| (|q_t| + |q_c|) + (d + 4) eps base) of their real values),
      |eps_c(fp32) - eps_c(float64)| <= 2^-23 ((d + 2) |p| (|q_t| + |q_c|) / base_c + (d + 4) eps_c),
    and an order statistic is 1-Lipschitz in the sup norm, so every sorted entry is
    within the largest per-candidate bound of the entry."""
    P, Q, users, tests, excl = _case(d, seed=50 + d)
    m64, base64, cand = ev.worst_margins_host(P, Q, users, tests, N_CAND, excl, side)
    m32, b32 = _f32_margins(P, Q, users, tests, side)
    e32 = ev.min_eps_f32(m32, b32, side).astype(np.float64)
    want, want_items = ev.radius_host(P, Q, users, tests, N_CAND, excl, N_CAND, side)  # every candidate's
    assert want.shape == (N_USERS, N_CAND) and want_items.shape == (N_USERS, N_CAND)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    pn, qn = np.linalg.norm(P64[users], axis=1), np.linalg.norm(Q64, axis=1)
    scale = pn[:, None] * (qn[tests][:, None] + qn[None, :N_CAND])
    with np.errstate(divide="ignore", invalid="ignore"):
        e64 = np.where(m64 <= 0, 0.0, m64 / base64)
        bound = 2.0 ** -23 * ((d + 2) * scale / base64 + (d + 4) * e64)
    worst_ratio = 0.0
    for r in range(N_USERS):
        c = cand[r]
        assert np.isfinite(bound[r][c]).all()
        lim = bound[r][c].max()
        nc = int(c.sum())
        got = np.sort(e32[r][c])
        err = np.abs(got - want[r, :nc])
        worst_ratio = max(worst_ratio, float(err.max() / lim))
        assert (err <= lim).all(), (r, err.max(), lim)
        # the lists themselves: ascending, never t, never excluded, zeros first, padded past the candidates
        assert (np.diff(want[r, :nc]) >= 0).all() and c[want_items[r, :nc]].all()
        assert len(set(want_items[r, :nc].tolist())) == nc
        assert np.isposinf(want[r, nc:]).all() and (want_items[r, nc:] == -1).all() and nc < N_CAND
        assert (want[r] == 0).sum() == ((m64[r] <= 0) & c).sum()
        short, _ = ev.radius_host(P, Q, users[r:r + 1], tests[r:r + 1], N_CAND, [excl[r]], K, side)
        assert (short[0] == want[r, :K]).all()
    print(side, "d", d, "largest error / bound", worst_ratio)


def test_radius_host_pads_and_breaks_ties_by_id(ev):
    P = np.array([[1.0, 0.0], [0.0, 0.0]], np.float32)
    Q = np.array([[3.0, 0.0], [1.0, 0.0], [1.0, 0.0], [5.0, 0.0], [2.0, 0.0]], np.float32)
    eps, items = ev.radius_host(P, Q, [0, 1], [0, 0], 5, [[4, -1, 9], []], 6, "user")
    assert items[0].tolist() == [3, 1, 2, -1, -1, -1]  # item 3 scores above t; 1 and 2 tie: the lower id first
    assert eps[0].tolist() == [0.0, 1.0, 1.0, np.inf, np.inf, np.inf]
    assert eps[1].tolist()[:4] == [0.0] * 4 and items[1].tolist() == [1, 2, 3, 4, -1, -1]  # p = 0: every m is 0
    eps, _ = ev.radius_host(P, Q, [1], [0], 5, None, 2, "item")
    assert eps.tolist() == [[0.0, 0.0]]
    eps, _ = ev.radius_host(P, Q[:, ::-1].copy(), [0], [0], 5, None, 4, "item")  # p . q = 0 for all: m = 0
    assert eps.tolist() == [[0.0] * 4]


# ---- summary and curve ---------------------------------------------------------------
def test_radius_curve_is_the_hit_rate_of_the_worst_positions(ev):
    """A grid of eps halfway between neighbouring flip points of the lists (so every
    margin is well separated from its threshold): the float64 worst positions give
    exactly the hit rates radius_curve reads off the float64 radii."""
    P, Q, users, tests, excl = _case(8, seed=77)
    for side in ("user", "item"):
        eps, _ = ev.radius_host(P, Q, users, tests, N_CAND, excl, K, side)
        flips = np.unique(eps[np.isfinite(eps) & (eps > 0)])
        grid = [0.0] + [float(x) for x in (flips[:-1] + flips[1:])[:: max(1, len(flips) // 12)] / 2.0] + [1e3]
        worst = ev.worst_positions_host(P, Q, users, tests, N_CAND, excl, grid, side)
        for k in (1, 5, K):
            want = [float((worst[e] < k).mean()) for e in range(len(grid))]
            assert ev.radius_curve(eps, k, grid) == want
        assert ev.radius_curve(eps, K, grid)[0] >= ev.radius_curve(eps, K, grid)[-1]
    with pytest.raises(ValueError, match="K must"):
        ev.radius_curve(eps, K + 1, [0.0])


def test_radius_summary_rows(ev):
    eps = np.array([[0.0, 0.0, 1.0], [0.0, 0.5, np.inf], [0.25, 2.0, np.inf], [np.inf, np.inf, np.inf]])
    rows = ev.radius_summary(eps, [1, 3])
    assert [r[0] for r in rows] == [1, 3] and all(len(r) == 8 for r in rows)
    assert rows[0][1:3] == (0.5, 0.25) and rows[1][1:3] == (0.0, 0.75)
    assert rows[0][3:] == tuple(float(q) for q in np.quantile([0.0, 0.0, 0.25], [0.1, 0.25, 0.5, 0.75, 0.9]))
    assert rows[1][3:] == (1.0,) * 5
    none = ev.radius_summary(np.full((2, 1), np.inf), [1])
    assert none[0][:3] == (1, 0.0, 1.0) and all(np.isnan(v) for v in none[0][3:])
    with pytest.raises(ValueError, match="K must"):
        ev.radius_summary(eps, [4])


# ---- CLI -------------------------------------------------------------------------------
@pytest.mark.parametrize("flavor", ["ori", "adv"])
def test_cli_flag_and_file(cli, flavor, tmp_path):
    assert cli.parse_args([], flavor).certify_radius == []
    a = cli.parse_args(["--certify_radius", "1, 10,50", "--certify_side", "both"], flavor)
    assert a.certify_radius == [1, 10, 50] and a.certify_side == "both"
    for bad in (["--certify_radius", "0"], ["--certify_radius", "129"], ["--certify_radius", "x"],
                ["--certify_radius", ""], ["--certify_radius", "1.5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad, flavor)
    rows = [("user", 1, 0.75, 0.0, 0.0, 1.0 / 3, 0.1, 0.2, 0.7), ("user", 10, 0.5, 0.25, 1e-3, 0.01, 0.02, 0.5, 2.0),
            ("item", 10, 0.0, 1.0, float("nan"), float("nan"), float("nan"), float("nan"), float("nan"))]
    cli.write_radius(str(tmp_path / "o"), "run.radius", rows)
    lines = (tmp_path / "o" / "run.radius").read_text().splitlines()
    assert len(lines) == 3 and all(len(ln.split("\t")) == 9 for ln in lines)
    got = cli.read_radius(str(tmp_path / "o" / "run.radius"))
    assert got[:2] == rows[:2] and isinstance(got[0][1], int)
    assert got[2][:4] == rows[2][:4] and all(np.isnan(v) for v in got[2][4:])
    (tmp_path / "bad.radius").write_text("user\t10\t0.1\t0.2\n")
    with pytest.raises(ValueError):
        cli.read_radius(str(tmp_path / "bad.radius"))
    with pytest.raises(ValueError):
        cli.write_radius(str(tmp_path / "o"), "short.radius", [("user", 1, 0.5, 0.5, 1.0)])
