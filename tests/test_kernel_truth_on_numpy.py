"""The kernel truth table (tests/golden/kernel_truth.json) and its bounds, without a GPU: the table is what 60-digit
arithmetic gives, it visits the regions it is meant to visit, and the plain NumPy restatement of the formulas
(np_terms._kern: libm's exp and a correctly rounded sqrt) stays inside the bounds of tests/kernel_truth.py on EVERY grid
point -- the condition under which holding the device to them asks for nothing a straightforward implementation lacks."""
import os

import numpy as np
import pytest

import kernel_truth as kt
import np_terms

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_table_is_consistent_and_covers_its_regions():
    grids = kt.load()
    assert os.path.getsize(os.path.join(GOLDEN, "kernel_truth.json")) <= os.path.getsize(os.path.join(GOLDEN, "sklearn_gpr.json"))
    for name, g in grids.items():
        assert 250 <= len(g) <= 512
        with np.errstate(over="ignore"):
            assert np.array_equal(g.d2, g.t * g.t)               # the stored d2 is the device's single product
        assert np.array_equal(g.t[:g.n_common], grids["se"].t[:g.n_common])
        assert np.all((g.k >= 0) & (g.k <= 1))
        assert all(float(s) == k or abs(float(s) - k) <= np.spacing(k) for s, k in zip(g.k_dec, g.k))
        d2 = g.d2
        assert d2[0] == 0.0 and g.k[0] == 1.0 and 5e-324 in d2 and 1e-300 in d2 and np.any((d2 < 1e-300) & (d2 > 9e-301))
        assert np.isinf(d2).sum() == 1 and g.k[np.isinf(d2)][0] == 0.0 and g.k_dec[int(np.argmax(np.isinf(d2)))] == "0.0"
        assert np.any(np.abs(d2 / 1e300 - 1) < 1e-15) and np.any((d2 > 1.7e308) & np.isfinite(d2))
        lg = np.log2(d2[(d2 > 0) & np.isfinite(d2)])
        assert np.sum((lg > -60) & (lg < 20)) >= 200
        a = 0.5 * d2 if name == "se" else kt.C_OF[name] * np.sqrt(d2)          # minus the argument of exp
        x = a * 1.4426950408889634
        for n in (1, 10, 100, 1000):                                            # both sides of every half-integer
            near = x[np.abs(x - (n + 0.5)) < 1e-3 * n]
            assert np.any(near < n + 0.5) and np.any(near > n + 0.5), (name, n)
        tiny = np.finfo(np.float64).tiny
        assert np.sum((g.k > 0) & (g.k < tiny)) >= 30                           # subnormal results
        assert np.any((a > 746) & (a < 800)) and np.any(np.abs(a - 800) < 1e-9) and np.any(a > 800) and np.any(a > 9e9)
        assert np.any(g.must_zero & np.isfinite(d2)) and not np.any(g.must_zero & (g.k != 0))
        # fp32: the truth at the rounded offsets
        assert np.all(np.isfinite(g.t32)) and g.k32[0] == 1.0 and np.all((g.k32 >= 0) & (g.k32 <= 1))


def test_table_matches_a_fresh_mpmath_evaluation():
    mp = pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_kernel_truth", os.path.join(GOLDEN, "make_kernel_truth.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert mp.mp.dps == 60
    fresh = gen.build()
    import json
    with open(os.path.join(GOLDEN, "kernel_truth.json")) as fh:
        assert json.load(fh) == fresh


@pytest.mark.parametrize("name", kt.KERNELS)
def test_numpy_restatement_is_inside_the_bounds_on_every_grid_point(name):
    g = kt.load()[name]
    with np.errstate(under="ignore", over="ignore"):
        got = np_terms._kern(kt.KIND[name], g.d2, 0.0)
    bad = kt.violations(g, got)
    print(name, "NumPy, largest error in ulps per band:", kt.band_maxima(g, got))
    assert bad.size == 0, kt.describe(g, got, bad)
    assert got[0] == 1.0


def test_the_metric_notices_what_it_is_for():
    """one ulp is np.spacing(truth) -- 2^-1074 for subnormal truths --, NaN / out-of-range values and a non-zero where the
    truth is far below half the smallest subnormal are violations"""
    g = kt.load()["se"]
    ok = g.k.copy()
    assert kt.violations(g, ok).size == 0
    i = int(np.flatnonzero((g.k > 1e-3) & (g.k < 0.5))[0])
    for ulps, bad in ((2, False), (3, True)):
        v = ok.copy()
        v[i] += ulps * np.spacing(g.k[i])
        assert (kt.violations(g, v).tolist() == [i]) == bad and kt.err_ulps(g, v)[i] == ulps
    j = int(np.flatnonzero((g.k > 0) & (g.k < 1e-310))[0])
    v = ok.copy()
    v[j] += 3 * 5e-324
    assert kt.violations(g, v).tolist() == [j] and kt.err_ulps(g, v)[j] == 3
    z = int(np.flatnonzero(g.must_zero)[0])
    for wrong in (5e-324, np.nan, -0.1):
        v = ok.copy()
        v[z] = wrong
        assert kt.violations(g, v).tolist() == [z]
    v = ok.copy()
    v[0] = np.nextafter(1.0, 2.0)
    assert kt.violations(g, v).tolist() == [0]
