"""The committed 60-digit truth table of the RationalQuadratic kernel and its two derivatives
(tests/golden/kprod_truth.json, written by tests/golden/make_kprod_truth.py) and the error model the tests hold the device's
formula to.  TEST INFRASTRUCTURE ONLY.  Metric and conventions as in tests/kernel_truth.py: errors in ulps of the truth
(np.spacing(truth), so a subnormal truth counts in units of 2^-1074); below 2^-1076 the result must be exactly 0.

The formula (csrc/kprod.hip: rq_eval):   k = exp(-a),  a = fl(alpha * L),  L = log1p(u),  u = fl(d2 / (2 alpha)).
Its roundings, each relative to the quantity it produces, in units of eps = 2^-53:
    u        one division (2 alpha is exact)                                                  1
    L        log1p passes a relative error of u on times u / ((1 + u) L) <= 1, and is itself
             accurate to 2 ulp = 4 eps (the OpenCL / OCML bound for double log1p; glibc: under 1 ulp)   1 + 4
    a        one product                                                                      1
a carries at most 7 eps relative, i.e. 7 eps a absolute, which exp turns into 7 eps a RELATIVE on k: at most 7 a ulps of the
truth (an ulp is at least eps |k|; a subnormal truth has larger ulps and the same count holds a fortiori).  exp itself and
the final rounding: 2 ulp, the bound tests/kernel_truth.py derives for SE, whose argument is exact.  Hence
    bound = 2 + 7 a ulp,   a = alpha log1p(d2 / (2 alpha)).
A finite d2 whose u overflows (alpha < 1/2, d2 beyond 2 alpha DBL_MAX) takes L = fl(fl(log d2) - fl(log 2 alpha)): the two
logarithms have opposite signs there, so their errors, 4 eps each relative to themselves, add up to at most 4 eps L, and the
subtraction adds 1: the same 5 eps on L, the same bound.
At d2 = 0 the formula is exact: log1p(0) = 0 and exp(-0) = 1.  Where d2 overflowed a = inf: the bound is infinite there, and
the separate must-be-zero condition applies (the truth is 0).
The derivatives are held on the host only (the device's gradient contraction is compared with NumPy sums of them):
    dk/dg = -2 alpha r k, r = u / (1 + u):       k's error (the bound above, absolute) times 2 alpha r, plus four roundings
    dk/dalpha = k (r - L): the difference cancels (it is -u^2 / 2 for small u), so its error is bounded by the operands':
             (3 eps r + 4 eps L) k for r and L, plus k's own error times |r - L| and two roundings on the result.
"""
import json
import os

import numpy as np

ALPHAS = (0.1, 1.3, 50.0)
EPS = 2.0 ** -53
BANDS = ("d2 < 1", "d2 >= 1, normal", "subnormal")


def exp_arg(alpha, d2):
    """a = alpha log1p(d2 / (2 alpha)), the argument the bound is a function of (+inf where d2 is)"""
    d2 = np.asarray(d2, dtype=np.float64)
    with np.errstate(over="ignore", divide="ignore"):
        u = d2 / (2.0 * alpha)
        return alpha * np.where(np.isinf(u) & np.isfinite(d2), np.log(d2) - np.log(2.0 * alpha), np.log1p(u))


def bound_ulps(alpha, d2):
    return 2.0 + 7.0 * exp_arg(alpha, d2)


class Grid:
    """one alpha's grid: t, d2 = fl(t t), k / dk / dp (the truths as doubles), must_zero, bound (ulp)"""

    def __init__(self, alpha, t, d2, e):
        unhex = lambda xs: np.array([float.fromhex(s) for s in xs])      # noqa: E731
        self.alpha, self.t, self.d2 = alpha, t, d2
        self.k, self.dk, self.dp = unhex(e["k"]), unhex(e["dk"]), unhex(e["dp"])
        self.must_zero = np.zeros(len(self.k), dtype=bool)
        self.must_zero[list(e["must_zero"])] = True
        self.ulp = np.spacing(self.k)
        self.bound = bound_ulps(alpha, d2)
        self.a = exp_arg(alpha, d2)
        self.band = np.where(self.k < np.finfo(np.float64).tiny, 2, np.where(d2 < 1.0, 0, 1))

    def __len__(self):
        return len(self.t)


_cache = {}


def load():
    """{alpha: Grid}"""
    if not _cache:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kprod_truth.json")) as fh:
            g = json.load(fh)
        unhex = lambda xs: np.array([float.fromhex(s) for s in xs])      # noqa: E731
        tc, dc = unhex(g["common"]["t"]), unhex(g["common"]["d2"])
        for alpha in ALPHAS:
            e = g["alphas"][repr(alpha)]
            _cache[alpha] = Grid(alpha, np.concatenate([tc, unhex(e["t"])]), np.concatenate([dc, unhex(e["d2"])]), e)
    return _cache


def err_ulps(grid, got):
    got = np.asarray(got, dtype=np.float64).ravel()
    assert got.shape == grid.k.shape
    with np.errstate(over="ignore"):
        return np.abs(got - grid.k) / grid.ulp


def violations(grid, got, fraction=1.0):
    """indices where `got` is NaN, outside [0, 1], not 0 where it must be, or beyond fraction * bound"""
    got = np.asarray(got, dtype=np.float64).ravel()
    e = err_ulps(grid, got)
    bad = ~(e <= fraction * grid.bound) | ~((got >= 0.0) & (got <= 1.0)) | (grid.must_zero & (got != 0.0))
    return np.flatnonzero(bad)


def band_maxima(grid, got):
    e = err_ulps(grid, got)
    return {BANDS[b]: (float(np.max(e[grid.band == b])) if np.any(grid.band == b) else 0.0) for b in range(3)}


def describe(grid, got, idx, limit=8):
    got = np.asarray(got, dtype=np.float64).ravel()
    e = err_ulps(grid, got)
    return "; ".join(f"[{i}] t={grid.t[i]!r} d2={grid.d2[i]!r} got={got[i]!r} truth={grid.k[i]!r} err={e[i]:.3g} ulp "
                     f"(bound {grid.bound[i]:.3g})" for i in idx[:limit])


def _k_abs_error(grid):
    """the model's bound on |k - truth|, absolute (0 where the truth is exactly 0 because d2 overflowed)"""
    with np.errstate(invalid="ignore"):
        e = grid.bound * grid.ulp
    return np.where(np.isfinite(e), e, 0.0)


def _r_and_l(grid):
    with np.errstate(over="ignore", invalid="ignore"):
        u = grid.d2 / (2.0 * grid.alpha)
        r = np.where(u < 1e300, u / (1.0 + u), 1.0)
    return r, np.where(np.isfinite(grid.a), grid.a / grid.alpha, 0.0)


def dscale_tolerance(grid):
    """absolute tolerance of the host formula of dk/dg = -2 alpha r k (kprod_np.rq_dscale) per grid point: k's error times
    2 alpha r, four more roundings, the final one counted in the spacing of the truth (which may be subnormal); u itself
    underflows for a subnormal d2 (an absolute error of up to 2^-1074 on u, times 2 alpha)"""
    r, _ = _r_and_l(grid)
    return (_k_abs_error(grid) * 2.0 * grid.alpha * r + 4.0 * EPS * np.abs(grid.dk) + np.spacing(np.abs(grid.dk)) +
            max(1.0, 2.0 * grid.alpha) * 5e-324)


def dparam_tolerance(grid):
    """absolute tolerance of the host formula of dk/dalpha = k (r - L) (kprod_np.rq_dparam) per grid point: k's error times
    |r - L|, the operands' errors (3 eps r, 4 eps L) times k, two roundings on the result"""
    r, l = _r_and_l(grid)
    return (_k_abs_error(grid) * np.abs(r - l) + EPS * grid.k * (3.0 * r + 4.0 * l) + 2.0 * EPS * np.abs(grid.dp) +
            np.spacing(np.abs(grid.dp)))
