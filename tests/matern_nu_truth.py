"""The committed 60-digit truth table of the general-nu Matern kind (tests/golden/matern_nu_truth.json, written by
tests/golden/make_matern_nu_truth.py) and the error model the tests hold csrc/kprod.hip's matern_nu_derivs to, on the host
through its NumPy restatement (tests/matern_nu_np.py, within HALF the bound) and on the device (within the bound).
TEST INFRASTRUCTURE ONLY.  eps = 2^-53 throughout; one ulp is at most 2 eps relative.

    |k - truth| <= (A + 4 x + C n) eps |truth|  +  2^-1074        x = sqrt(2 nu) d,   n = floor(nu + 1/2) (0 for nu < 1/2)

The constants come from documented bounds and from counting the routine's operations, not from what any implementation
returned.  The library limits are the OpenCL C specification's for double precision, which the device library implements
(pow <= 16 ulp, log, exp, expm1 <= 3 ulp, sqrt correctly rounded); glibc stays under 1 ulp for all of them.

4 x   the argument's own rounding, as tests/kernel_truth.py charges the closed-form Matern kinds: x^ = fl(c fl(sqrt(d2))),
      c = fl(sqrt(2 nu)), carries 3 eps (the root, the rounded constant, the product) and
      |d log k / d log x| = x K_(nu-1)(x) / K_nu(x) <= x + 1  (Segura's bound x K_(v+1) / K_v < v + 1/2 + sqrt(x^2 + (v + 1/2)^2) at
      v = nu - 1 >= -1; for nu >= 1/2 the ratio is <= 1 and the "+ 1" is not needed).  3 (x + 1) <= 4 x + 3: the 3 goes into A.
C n   the recurrence Q_(j+1) = x^2 Q_(j-1) + 2 (mu + j) Q_j: every term is positive, 2 (mu + j) is exact, so a step costs
      the rounding of x^2, of the two products and of the sum, and the error of a sum of positive terms is at most the larger
      of its terms' errors plus its own rounding: max(e_(j-1) + 2, e_j + 1) + 1 <= max(e) + 3.   C = 3,  n - 1 steps.
A     = 128, the sum of
        32   pow, 16 ulp: (x / 2)^(2 mu) in the series (it multiplies the leading terms), (x / 2)^mu behind the fraction
         6   log, 3 ulp: -log(x / 2) multiplies Temme's second starting term
         6   expm1, 3 ulp, in the same term where |2 mu log(x / 2)| < 1
         4   exp: e^-x through exp_nonpos, 2 ulp (tests/kernel_truth.py: SE), x > 2 only
         2   truncation: the series and the fraction stop at the first term below eps times its sum; the terms fall at
             least like 1 / 2 from there on, so the tail is below 2 eps
        14   the seven constants of nu the host computes (1 / Gamma(1 +- mu), Gamma_1, Gamma_2, pi mu / sin(pi mu),
             2^(1-n) / Gamma(nu), nu times it), 2 eps each on average: the library rounds long double values once (1 eps);
             the NumPy restatement's float64 Horner sums carry 2 and its math.gamma up to 2 ulp = 4 eps
         3   the argument, from above
        48   the starting values.  Temme's K_mu begins with f_0 = fact (Gamma_1 cosh(e) + Gamma_2 sinh(e) / e log(2 / x)),
             whose two parts have opposite signs; at x = 2 the first term is -0.58 (mu = 0) to -0.89 (mu = 1/2) against
             K_mu(2) = 0.11 .. 0.12, so the roundings of f_0 (6: three products, two sums, the constant factor) weigh up to
             8 times in K_mu: 48.  K_(mu+1) has a positive leading term and no such factor.
        13   the sums themselves.  Term i of the series carries about 4 i roundings (f_i, p_i, q_i, c_i by recurrence) and
             weighs (x^2 / 4)^i / i! <= 1 / i!: sum 4 i / i! = 4 e < 11, plus one rounding per addition while the partial
             sum still changes by more than eps / 2 of itself, 2 in all.  The fraction's terms fall faster.
      Nothing here grows with x or nu.
2^-1074  the last product, ca Q_n e^-x, is rounded once into the subnormal range (e^-x is applied as e^-600 e^-(x-600)
      beyond x = 600 so that no factor is subnormal before it).
Where the truth is below 2^-1076 the result must be exactly 0; at d2 = 0 it must be exactly 1; never NaN.

The derivatives share everything up to the last products: kx = -nu ca Q_(n-1) [e^-x] is the same chain one step shorter,
with |d log kx / d log x| <= x + 3 (x^(nu-1) K_(nu-1) in place of x^nu K_nu, for nu < 1 times the x^(2 nu - 2) it diverges
with: 2 |nu - 1| <= 2 more) and dk = 2 d2 kx two more roundings:
    |kx - truth| <= (A + 6 + 4 x + C n) eps |truth| + 2 * 2^-1074        |dk - truth| <= (A + 8 + 4 x + C n) eps |truth| + (2 + x) 2^-1074
(the subnormal terms: where k comes out as 0 the library returns exact zeros for derivatives whose truth is at most
k nu / x resp. k x, k < 2^-1075).  At d2 = 0: kx = -nu / (2 (nu - 1)), two roundings, 2 eps.
"""
import json
import math
import os

import numpy as np

EPS = 2.0 ** -53
A, C = 128.0, 3.0
TINY = 2.0 ** -1074


def _unhex(xs):
    return np.array([float.fromhex(s) for s in xs])


class Grid:
    """one nu's grid: t, d2 = fl(t t), x = sqrt(2 nu) sqrt(d2), the truths k / kx / dk as doubles, must_zero"""

    def __init__(self, nu, e):
        self.nu = nu
        self.n = 0 if nu < 0.5 else int(math.floor(nu + 0.5))
        self.t, self.d2 = _unhex(e["t"]), _unhex(e["d2"])
        self.k, self.kx, self.dk = _unhex(e["k"]), _unhex(e["kx"]), _unhex(e["dk"])
        self.must_zero = np.zeros(len(self.k), dtype=bool)
        self.must_zero[list(e["must_zero"])] = True
        with np.errstate(over="ignore"):
            self.x = math.sqrt(2.0 * nu) * np.sqrt(self.d2)

    def __len__(self):
        return len(self.t)


_cache = {}


def load():
    """{nu: Grid}"""
    if not _cache:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matern_nu_truth.json")) as fh:
            g = json.load(fh)
        for s in g["nus"]:
            _cache[float(s)] = Grid(float(s), g["grid"][s])
    return _cache


NUS = (0.1, 0.3, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 2.5, 3.7, 7.5, 12.0, 25.0, 32.0)


def bound_units(nu, x, extra=0.0):
    """A + 4 x + C n (+ extra), in units of eps relative to the truth; x = sqrt(2 nu) d"""
    n = 0 if nu < 0.5 else int(math.floor(nu + 0.5))
    with np.errstate(over="ignore"):
        return A + extra + 4.0 * np.asarray(x, dtype=np.float64) + C * n


def _tol(grid, truth, extra, tiny_factor, fraction):
    with np.errstate(over="ignore", invalid="ignore"):
        rel = fraction * bound_units(grid.nu, grid.x, extra) * EPS * np.abs(truth)
        rel = np.where(np.isfinite(rel), rel, 0.0)        # (x = inf: the truth and the routine are exact zeros)
        tiny = TINY * np.where(np.isfinite(tiny_factor), tiny_factor, 0.0)
    return np.where((grid.d2 == 0.0) & (truth != 1.0), 2.0 * EPS * np.abs(truth), rel + tiny)


def k_tolerance(grid, fraction=1.0):
    return _tol(grid, grid.k, 0.0, np.ones(len(grid)), fraction)


def kx_tolerance(grid, fraction=1.0):
    return _tol(grid, grid.kx, 6.0, 2.0 * np.ones(len(grid)), fraction)


def dk_tolerance(grid, fraction=1.0):
    return _tol(grid, grid.dk, 8.0, 2.0 + grid.x, fraction)


def err_units(grid, got, truth=None):
    """|got - truth| in units of eps |truth| (0 where both are 0)"""
    truth = grid.k if truth is None else truth
    got = np.asarray(got, dtype=np.float64).ravel()
    assert got.shape == truth.shape
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.abs(got - truth) / (EPS * np.abs(truth))
    return np.where(got == truth, 0.0, e)


def violations(grid, got, fraction=1.0):
    """indices where the value is NaN, outside [0, 1], not 0 where it must be, not 1 at d2 = 0, or beyond fraction * bound"""
    got = np.asarray(got, dtype=np.float64).ravel()
    bad = (~(np.abs(got - grid.k) <= k_tolerance(grid, fraction)) | ~((got >= 0.0) & (got <= 1.0)) |
           (grid.must_zero & (got != 0.0)) | ((grid.d2 == 0.0) & (got != 1.0)))
    return np.flatnonzero(bad)


def deriv_violations(grid, got, which, fraction=1.0):
    got = np.asarray(got, dtype=np.float64).ravel()
    truth, tol = (grid.kx, kx_tolerance(grid, fraction)) if which == "kx" else (grid.dk, dk_tolerance(grid, fraction))
    bad = ~(np.abs(got - truth) <= tol) | (grid.must_zero & (got != 0.0)) | (np.isinf(grid.d2) & (got != 0.0))
    return np.flatnonzero(bad)


def describe(grid, got, idx, truth=None, limit=8):
    got = np.asarray(got, dtype=np.float64).ravel()
    truth = grid.k if truth is None else truth
    e = err_units(grid, got, truth)
    return "; ".join(f"[{i}] nu={grid.nu} t={grid.t[i]!r} x={grid.x[i]:.6g} got={got[i]!r} truth={truth[i]!r} err={e[i]:.4g} eps "
                     f"(A + 4x + Cn = {bound_units(grid.nu, grid.x[i]):.4g})" for i in idx[:limit])
