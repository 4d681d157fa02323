"""The committed 60-digit truth table of the Cosine and GammaExponential kinds and their derivatives
(tests/golden/kinds_truth.json, written by tests/golden/make_kinds_truth.py) and the error models the tests hold the formulas
of csrc/kprod.hip to.  TEST INFRASTRUCTURE ONLY.  eps = 2^-53 throughout.

The constants come from documented bounds, not from what a device returned.  ROCm's device-library documentation is not
shipped with the toolchain the suite runs on, so they are the OpenCL C specification's limits for double precision, which the
device library implements: cospi, sinpi <= 4 ulp, pow <= 16 ulp, log <= 3 ulp, sqrt correctly rounded; 1 ulp <= 2 eps
relative.  glibc (the NumPy mirror in tests/kinds_np.py) stays under 1 ulp for all of them.

COSINE (cosine_eval):  k = cospi(dh),  dh = fl(sqrt(d2)).
|k| <= 1 and k has zeros, so ulps of the truth mean nothing: the bound is ABSOLUTE, in units of eps.
    dh       sqrt is correctly rounded: dh = d (1 + e), |e| <= eps, so |dh - d| <= eps d
    cos(pi dh) - cos(pi d)
             Taylor around d: at most |sin(pi d)| pi |dh - d| + (pi |dh - d|)^2 / 2
                                                                    pi d |sin(pi d)|  +  (pi d)^2 eps / 2       (units of eps)
             The second term is below 1e-3 for d <= 1e6; it is what keeps the bound true at integers (sin = 0) once d is
             large, e.g. the table's d2 = 1e300, where dh is an even integer and the true d is not.
    cospi    argument reduction is exact (that is why the formula uses it); 4 ulp of a result of magnitude <= 1, an ulp of
             which is at most eps                                                                       4
    table    the stored truth is rounded to a double of magnitude <= 1                                  1/2
Hence   bound = c0 + pi d |sin(pi d)| + (pi d)^2 eps / 2,   c0 = 4.5,   capped at 2 / eps (|k| <= 1 on both sides).
At d2 = 0 the formula is exact (cospi(0) = 1); at d2 = +inf the library returns exactly 1 and the table says 1.
A NumPy evaluation must reduce first, cos(pi remainder(d, 2)): its argument then carries pi |r| eps with |r| <= 1, and
|r sin(pi r)| pi <= 1.83, so it needs 1.83 + 1 (glibc) + 1/2 < c0; the naive cos(pi d) carries pi d eps UNMULTIPLIED by
|sin| and breaks the bound at the integers.

The derivatives are held on the host only (the device's contractions are compared with NumPy sums of them).  With
E_s = s0 + pi d |cos(pi d)| + (pi d)^2 eps / 2 the same bound for sinpi(dh) (s0 = 6: the mirror's reduced argument costs up
to pi |r cos(pi r)| <= pi there, plus 1 + 1/2, and the device's 4.5 is below it):
    dk/dg = -(pi dh) s:     pi d E_s eps  +  5 eps |dk|  (pi's own rounding, dh, two products, the table)  +  one spacing
    kx = -pi s / (2 dh):    pi / (2 d) E_s eps  +  5 eps |kx|  +  one spacing;   the constant -pi^2 / 2 at d = 0: 2 eps |kx|

GAMMAEXP (gexp_eval):  k = exp_nonpos(-ah),  ah = pow(d2, h),  h = fl(gamma / 2) (exact: a halving).
In ulps of the truth (np.spacing(truth): a subnormal truth counts in units of 2^-1074; below 2^-1076 the result must be 0).
    ah       pow: 16 ulp = 32 eps relative, i.e. 32 eps a absolute; -ah is exact
    exp      turns an absolute error of 32 eps a on its argument into 32 eps a RELATIVE on k: at most 32 a ulps of the
             truth (an ulp is at least eps |k|; a subnormal truth has larger ulps and the same count holds a fortiori)
    exp_nonpos and the final rounding: 2 ulp, the bound tests/kernel_truth.py derives for SE, whose argument is exact
Hence   bound = 2 + c a ulp,   c = 32,   a = d2^(gamma / 2)       (glibc's pow, under 1 ulp, stays within 2 + 2 a).
At d2 = 0 the formula is exact: pow(0, h) = 0 and exp(-0) = 1.  Where a = inf the bound is infinite and the must-be-zero
condition applies instead.  Derivatives, on the host only, with E_k = bound * ulp(k) the absolute bound on k:
    dk/dg = -gamma a k:            gamma a E_k  +  (32 + 3) eps |dk|  +  one spacing
    kx = -(gamma / 2) a k / d2:    (gamma / 2) a / d2 E_k  +  (32 + 4) eps |kx|  +  one spacing
    dp = -k a log(d2) / 2:         a |log d2| / 2 E_k  +  (32 + 6 + 3) eps |dp|  (log: 3 ulp = 6 eps)  +  one spacing
Near the underflow of k the product a k is subnormal and loses up to half a unit of 2^-1074, which the factors behind it
carry on (gamma <= 2; |log d2| / 2), and a k that comes out as 0 makes the library return exact zeros for derivatives whose
truth is that many units of 2^-1074 at most (E_k covers it: it is at least 2 units there).  Each tolerance therefore adds
2^-1074 times its factor: 2, 2 and 1 + |log d2| / 2.
"""
import json
import os

import numpy as np

GAMMAS = (0.3, 1.0, 1.7, 2.0)
EPS = 2.0 ** -53
C0, S0, C_POW = 4.5, 6.0, 32.0
COS_BANDS = ("d < 1", "1 <= d < 1e3", "1e3 <= d <= 1e6", "d > 1e6")
GEXP_BANDS = ("d2 < 1", "d2 >= 1, normal", "subnormal")


def _unhex(xs):
    return np.array([float.fromhex(s) for s in xs])


class Grid:
    """one kind's grid: t, d2 = fl(t t), the truths k / dk / kx / dp as doubles, must_zero"""

    def __init__(self, t, d2, e, gamma=None):
        self.gamma, self.t, self.d2 = gamma, t, d2
        self.k, self.dk, self.kx, self.dp = (_unhex(e[key]) for key in ("k", "dk", "kx", "dp"))
        self.must_zero = np.zeros(len(self.k), dtype=bool)
        self.must_zero[list(e.get("must_zero", ()))] = True
        with np.errstate(over="ignore", invalid="ignore"):
            self.d = np.sqrt(d2)
            if gamma is None:
                self.band = np.where(self.d < 1.0, 0, np.where(self.d < 1e3, 1, np.where(self.d <= 1e6, 2, 3)))
            else:
                self.a = np.power(d2, 0.5 * gamma)
                self.ulp = np.spacing(self.k)
                self.band = np.where(self.k < np.finfo(np.float64).tiny, 2, np.where(d2 < 1.0, 0, 1))

    def __len__(self):
        return len(self.t)


_cache = {}


def load():
    """{"cosine": Grid, gamma: Grid for gamma in GAMMAS}"""
    if not _cache:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kinds_truth.json")) as fh:
            g = json.load(fh)
        tc, dc = _unhex(g["common"]["t"]), _unhex(g["common"]["d2"])
        e = g["cosine"]
        _cache["cosine"] = Grid(np.concatenate([tc, _unhex(e["t"])]), np.concatenate([dc, _unhex(e["d2"])]), e)
        for gamma in GAMMAS:
            e = g["gammaexp"][repr(gamma)]
            _cache[gamma] = Grid(np.concatenate([tc, _unhex(e["t"])]), np.concatenate([dc, _unhex(e["d2"])]), e, gamma)
    return _cache


# ---- Cosine: absolute, in units of eps ------------------------------------------------------------------------------------
def _cos_bound_units(d, trig, c0):
    """c0 + pi d |trig| + (pi d)^2 eps / 2, capped at 2 / eps; trig = sin(pi d) for the value, cos(pi d) for sinpi"""
    with np.errstate(over="ignore", invalid="ignore"):
        b = c0 + np.pi * d * np.abs(trig) + (np.pi * d) ** 2 * (0.5 * EPS)
    return np.where(np.isfinite(b), np.minimum(b, 2.0 / EPS), 2.0 / EPS)


def _sin_cos_of_truth(grid):
    """(|sin(pi d)|, |cos(pi d)|) at the grid's d = fl(sqrt(d2)), reduced exactly first (remainder is exact).  d is off the
    true square root by eps d, which moves either by at most pi d eps: (pi d)^2 eps on the bound, twice the Taylor term and
    as negligible where the bound is not capped anyway"""
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(grid.d), np.remainder(np.where(np.isfinite(grid.d), grid.d, 0.0), 2.0), 0.0)
    return np.abs(np.sin(np.pi * r)), np.abs(np.cos(np.pi * r))


def cosine_bound_units(grid):
    s, _ = _sin_cos_of_truth(grid)
    b = _cos_bound_units(grid.d, s, C0)
    return np.where(np.isinf(grid.d2) | (grid.d2 == 0.0), 0.0, b)       # exact at both ends


def cosine_err_units(grid, got):
    got = np.asarray(got, dtype=np.float64).ravel()
    assert got.shape == grid.k.shape
    return np.abs(got - grid.k) / EPS


def cosine_violations(grid, got, fraction=1.0):
    """indices where `got` is NaN, outside [-1, 1] or beyond fraction * bound"""
    got = np.asarray(got, dtype=np.float64).ravel()
    bad = ~(cosine_err_units(grid, got) <= fraction * cosine_bound_units(grid)) | ~(np.abs(got) <= 1.0)
    return np.flatnonzero(bad)


def cosine_band_maxima(grid, got):
    """largest error per band, as (units of eps, fraction of the bound)"""
    e, b = cosine_err_units(grid, got), cosine_bound_units(grid)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(b > 0.0, e / np.where(b > 0.0, b, 1.0), np.where(e == 0.0, 0.0, np.inf))
    return {COS_BANDS[q]: ((float(np.max(e[grid.band == q])), float(np.max(frac[grid.band == q]))) if np.any(grid.band == q)
                           else (0.0, 0.0)) for q in range(4)}


def cosine_dscale_tolerance(grid):
    _, c = _sin_cos_of_truth(grid)
    es = _cos_bound_units(grid.d, c, S0) * EPS
    with np.errstate(over="ignore", invalid="ignore"):
        tol = np.pi * grid.d * es + 5.0 * EPS * np.abs(grid.dk) + np.spacing(np.abs(grid.dk))
    return np.where(np.isinf(grid.d2), 0.0, tol)


def cosine_dd2_tolerance(grid):
    _, c = _sin_cos_of_truth(grid)
    es = _cos_bound_units(grid.d, c, S0) * EPS
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        tol = np.pi / (2.0 * grid.d) * es + 5.0 * EPS * np.abs(grid.kx) + np.spacing(np.abs(grid.kx))
    return np.where(np.isinf(grid.d2), 0.0, np.where(grid.d2 == 0.0, 2.0 * EPS * np.abs(grid.kx), tol))


# ---- GammaExponential: ulps of the truth ----------------------------------------------------------------------------------
def gexp_bound_ulps(grid):
    with np.errstate(over="ignore"):
        return 2.0 + C_POW * grid.a


def gexp_err_ulps(grid, got):
    got = np.asarray(got, dtype=np.float64).ravel()
    assert got.shape == grid.k.shape
    with np.errstate(over="ignore"):
        return np.abs(got - grid.k) / grid.ulp


def gexp_violations(grid, got, fraction=1.0):
    """indices where `got` is NaN, outside [0, 1], not 0 where it must be, or beyond fraction * bound"""
    got = np.asarray(got, dtype=np.float64).ravel()
    bad = (~(gexp_err_ulps(grid, got) <= fraction * gexp_bound_ulps(grid)) | ~((got >= 0.0) & (got <= 1.0)) |
           (grid.must_zero & (got != 0.0)))
    return np.flatnonzero(bad)


def gexp_band_maxima(grid, got):
    e = gexp_err_ulps(grid, got)
    return {GEXP_BANDS[q]: (float(np.max(e[grid.band == q])) if np.any(grid.band == q) else 0.0) for q in range(3)}


def gexp_abs_error(grid):
    """E_k: the model's bound on |k - truth|, absolute (0 where the truth is exactly 0 because a overflowed)"""
    with np.errstate(invalid="ignore", over="ignore"):
        e = gexp_bound_ulps(grid) * grid.ulp
    return np.where(np.isfinite(e), e, 0.0)


def _gexp_tol(grid, truth, sens, roundings, tiny_factor):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lead = gexp_abs_error(grid) * sens
        lead = np.where(np.isfinite(lead), lead, 0.0)           # (a = inf: the truth and the formula are exact zeros)
        tol = lead + roundings * EPS * np.abs(truth) + np.spacing(np.abs(truth)) + 5e-324 * tiny_factor
    return np.where(np.isfinite(tol), tol, np.inf)


def gexp_dscale_tolerance(grid):
    with np.errstate(over="ignore"):
        sens = grid.gamma * grid.a
    return _gexp_tol(grid, grid.dk, sens, C_POW + 3.0, 2.0)


def gexp_dd2_tolerance(grid):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sens = np.where(grid.d2 > 0.0, 0.5 * grid.gamma * grid.a / grid.d2, 0.0)
    return _gexp_tol(grid, grid.kx, sens, C_POW + 4.0, 2.0)


def gexp_dparam_tolerance(grid):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        half_log = np.where((grid.d2 > 0.0) & np.isfinite(grid.d2), 0.5 * np.abs(np.log(grid.d2)), 0.0)
        sens = grid.a * half_log
    return _gexp_tol(grid, grid.dp, sens, C_POW + 9.0, 1.0 + half_log)


def describe(grid, got, idx, truth=None, limit=8):
    got = np.asarray(got, dtype=np.float64).ravel()
    truth = grid.k if truth is None else truth
    return "; ".join(f"[{i}] t={grid.t[i]!r} d2={grid.d2[i]!r} got={got[i]!r} truth={truth[i]!r}" for i in idx[:limit])
