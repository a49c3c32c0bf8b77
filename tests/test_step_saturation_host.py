"""saturation_fixture.py checked without a GPU: its conditions on the float64
trajectory (population of every regime in every batch, upper tail <= 60, the
margin of every score to both bounds, rows that only clipped triplets touch,
the crossings of the adversarial pass), and the fp32 oracle against float64 in
every regime, including that it takes float64's branch for every triplet."""
import numpy as np
import pytest

import saturation_fixture as sf
from saturation_fixture import ABOVE, BELOW, CENTRAL, LOWER, UPPER
from test_gpu_step_geometry import ATOL, RTOL, _few_step_scale, _parity_allowance

CASES = [(d, s, a) for d in sf.DIMS for s in sf.BOUNDS for a in (0, 1)]


@pytest.mark.parametrize("d,setting,adver", CASES)
def test_fixture_conditions(d, setting, adver):
    fx = sf.problem(d, setting, adver)
    out = sf.conditions(fx)
    print(d, setting, adver, {k: v.tolist() for k, v in out["populations"].items()}, out["crossings"],
          f"smallest margin {out['min_margin']:.1f} bounds")
    assert len(fx["u"]) == sf.B * sf.NB and fx["u"].max() < sf.U1 and max(fx["i"].max(), fx["j"].max()) < sf.I1
    # scores64 restates the first half of _step64: the losses it implies are _step64's, to the bit
    for x, loss in ((fx["x"], fx["lc"]),) + (((fx["xa"], fx["la"]),) if adver else ()):
        assert np.array_equal(np.logaddexp(0, -np.clip(x, fx["lo"], fx["hi"])), loss)
    # three per-row scales in each table
    for W in (fx["P"], fx["Q"]):
        rms = np.sqrt((W[:-4].astype(np.float64) ** 2).mean(1)) / (64.0 / d) ** 0.25
        assert (rms < 0.5).any() and ((rms > 0.6) & (rms < 1.5)).any() and (rms > 1.5).any()


def _one_value(v):
    return len(np.unique(v.view(np.int32))) == 1


@pytest.mark.parametrize("d,setting,adver", CASES)
def test_oracle_takes_the_float64_branch_in_every_regime(oracle, d, setting, adver):
    """The oracle's loss tells its branch: a clipped triplet's is one constant per
    bound (-clip_lo = 80 exactly under the default bounds), a lower-tail one's is
    -x > 13.94, an upper-tail one's e^-x < e^-13.94.  Then the distances: tables
    and Adagrad slots within half the project's bar in every summation order
    tried (so _few_step_scale is 1 in every case), upper-tail losses relatively
    (upper_rtol), the rest at the bar."""
    fx = sf.problem(d, setting, adver)
    want, lc, la, deltas = sf.oracle_run(oracle, fx)
    k, kd, ur = sf.bars(oracle, fx, _few_step_scale)
    print(d, setting, adver, f"k = {k:.2f}, delta k = {kd:.2f}, upper-tail rtol = {ur:.2e}")
    assert k == 1.0 and kd == 1.0 and 1e-5 <= ur < 2e-4
    # the seed's second condition: every oracle sample within half a bar of float64
    for tabs, lc_s, la_s, deltas_s in sf.oracle_samples(oracle, fx):
        got = list(tabs) + [lc_s, la_s] + [a for pair in deltas_s for a in pair]
        ref = list(fx["f64"]) + [a for pair in fx["deltas"] for a in pair]
        for o, w in zip(got, ref):
            assert (np.abs(o.astype(np.float64) - w) <= sf.HALF_BAR * (ATOL + RTOL * np.abs(w))).all()
    lo, hi = fx["lo"], fx["hi"]
    for x, got, ref in ((fx["x"], lc, fx["lc"]),) + (((fx["xa"], la, fx["la"]),) if adver else ()):
        r = sf.regimes(x, lo, hi)
        below, above = got[r == BELOW], got[r == ABOVE]
        assert _one_value(below) and (setting == "default" or _one_value(above))
        if setting == "default":
            assert below[0] == np.float32(-lo)
        consts = [below[0]] + ([above[0]] if setting == "tight" else [])
        free = got[(r != BELOW) & (r != ABOVE)]
        assert not np.isin(free.view(np.int32), np.array(consts).view(np.int32)).any()
        assert (got[r == LOWER] > sf.T).all() and (got[r == UPPER] < np.exp(-sf.T)).all()
        mid = got[r == CENTRAL]
        assert ((mid > 0.5 * np.exp(-sf.T)) & (mid <= sf.T + 1e-5)).all()  # log(y + 1) moves in steps of 2^-23
        up = r == UPPER
        np.testing.assert_allclose(got[up], ref[up], rtol=ur, atol=0)
        np.testing.assert_allclose(got[~up], ref[~up], rtol=k * RTOL, atol=k * ATOL)
    for o, w in zip(want, fx["f64"]):
        np.testing.assert_allclose(o, w, rtol=k * RTOL, atol=k * ATOL)
    # the oracle lets no gradient through a clipped triplet: rows, slots and deltas
    for rows, tabs, n in ((fx["clipped_users"], (want[0], want[2]), 0), (fx["clipped_items"], (want[1], want[3]), 1)):
        rows = list(rows)
        assert np.array_equal(tabs[0][rows], (fx["P"], fx["Q"])[n][rows]) and (tabs[1][rows] == np.float32(0.1)).all()
        for t in range(fx["nb"]):
            assert not deltas[t][n][rows].any() and not fx["deltas"][t][n][rows].any()


@pytest.mark.parametrize("setting", list(sf.BOUNDS))
@pytest.mark.parametrize("d", sf.DIMS)
def test_exact_bound_case(oracle, d, setting):
    """x == bound exactly passes gradient, the next float outside does not: in
    float64 and in the oracle; the exact rows are used by one triplet each."""
    fx, at_bound, outside = sf.exact_problem(d, setting)
    assert len(at_bound) == len(outside) == (1 if setting == "default" else 2)
    f32 = np.float32
    for b, bound in at_bound:
        assert fx["x"][b] == bound
    for b, bound in outside:
        assert f32(fx["x"][b]) == fx["x"][b] == np.nextafter(f32(bound), f32(np.sign(bound) * np.inf))
    for b, _ in at_bound + outside:
        for col, row in ((fx["u"], fx["u"][b]), (np.concatenate([fx["i"], fx["j"]]), fx["i"][b]),
                         (np.concatenate([fx["i"], fx["j"]]), fx["j"][b])):
            assert (col == row).sum() == 1
    for adver in (0, 1):
        want = sf.oracle_run(oracle, dict(fx, adver=adver))[0]
        for b, bound in at_bound + outside:
            moved = [not np.array_equal(want[0][fx["u"][b]], fx["P"][fx["u"][b]]),
                     not np.array_equal(want[1][fx["i"][b]], fx["Q"][fx["i"][b]]),
                     not np.array_equal(want[1][fx["j"][b]], fx["Q"][fx["j"][b]])]
            assert moved == [(b, bound) in at_bound] * 3, (b, moved)


@pytest.mark.parametrize("adver", [0, 1])
def test_large_batch_fixture(oracle, adver):
    fx = sf.large_problem(adver)
    out = sf.conditions(fx)
    B = fx["B"]
    print("large", adver, {k: v.tolist() for k, v in out["populations"].items()},
          f"smallest margin {out['min_margin']:.1f} bounds")
    for t in range(fx["nb"]):  # some slot has more than ACF_HOT_MIN = 8 occurrences
        s = slice(t * B, (t + 1) * B)
        assert np.bincount(fx["u"][s]).max() > 8 and np.bincount(np.concatenate([fx["i"][s], fx["j"][s]])).max() > 8
    want, lc, la, _ = sf.oracle_run(oracle, fx)
    smp = sf.oracle_samples(oracle, fx)
    allow = _parity_allowance([a for s in smp for a in s[0]], list(fx["f64"][:4]) * len(smp))
    k, _, ur = sf.bars(oracle, fx, _few_step_scale, tables=False)
    print(f"elements allowed outside 1e-5: {allow}; loss bar x {k:.2f}; upper-tail rtol {ur:.2e}")
    assert allow is None or allow <= 400
    assert k < 32.0
