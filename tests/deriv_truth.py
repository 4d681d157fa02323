"""The 80-digit table of the derivative kinds (tests/golden/deriv_truth.json, written by tests/golden/make_deriv_truth.py) and
the first-order rounding bounds the formulas are held to, on the device (tests/test_gpu_deriv.py) and in their NumPy
restatement (tests/test_deriv_truth_on_numpy.py).  TEST INFRASTRUCTURE ONLY.

Bounds: units of 2^-53 times the sum of the absolute addends of the entry (the table's `*_sabs`), as in
tests/wienerpp_truth.py.  The units, from the operation count of csrc/deriv_eval.h at input dimension D (one unit = one
rounding to nearest, relative 2^-53):
  * a coordinate difference u_d: 1.  s = sum_d u_d^2 by fma: 2 per square, 1 per fma, D terms: s is right to D + 3 units.
  * the exponential's argument x (s / 2 for SE; l = c sqrt(s) for the Matern kinds: (D + 3) / 2 from s, 2 for the square root
    step, 2 for c and its product): at most D + 7 units RELATIVE, so x (D + 7) units ABSOLUTE in the exponent, which is the
    relative error of E; exp_nonpos itself is good to 2 ulp = 4 units:               U_E(x) = 4 + x (D + 7)
  * the pair's coefficients from E: a constant and its product (2 units), (1 + l) of Matern-5/2 (1 unit and l's own D + 7), the
    reciprocal root of Matern-3/2 (two Newton steps from the hardware seed: 8 units, and (D + 3) / 2 from s): at most 2 D + 20
  * the entry: two coordinate differences (2), two products and the fma (3), the entry's own final rounding (1), and the
    table's value rounded to float64 (1): 7.                                         U_value(x) = U_E(x) + 2 D + 32  (rounded up)
  * the input-scale coefficients multiply by s or l once more and subtract a constant: D + 8 on top.
                                                                                     U_inscale(x) = U_value(x) + D + 8
An absolute floor of 16 x 2^-1074 covers results in the subnormal range (an exponential that underflowed is flushed to an
exact 0 by the library: `must_zero` lists where the table demands exact zeros, `exact` the exact coincident values)."""
import json
import os

import numpy as np

EPS = 2.0 ** -53
FLOOR = 16 * 2.0 ** -1074
HERE = os.path.dirname(os.path.abspath(__file__))
_C = {"se": None, "m32": np.sqrt(3.0), "m52": np.sqrt(5.0)}


def load():
    """base -> D -> dict(X, Y (D x n), s, terms: (a, b) -> dict(value, value_sabs, inscale, inscale_sabs, must_zero, exact))"""
    with open(os.path.join(HERE, "golden", "deriv_truth.json")) as fh:
        raw = json.load(fh)
    out = {}
    for base, per_d in raw.items():
        out[base] = {}
        for D, G in per_d.items():
            g = dict(X=np.asfortranarray(np.array(G["X"], dtype=np.float64).reshape(int(D), -1)),
                     Y=np.asfortranarray(np.array(G["Y"], dtype=np.float64).reshape(int(D), -1)),
                     s=np.array(G["s"]), distance=np.array(G["distance"]), terms={})
            for ab, rec in G["terms"].items():
                r = {k: np.array(rec[k], dtype=np.float64) for k in ("value", "value_sabs", "inscale", "inscale_sabs")}
                r["must_zero"] = np.array(rec["must_zero"], dtype=int)
                r["exact"] = np.array(rec["exact"], dtype=np.float64).reshape(-1, 2)
                g["terms"][tuple(int(v) for v in ab.split(","))] = r
            out[base][int(D)] = g
    return out


def exponent(base, s):
    """x: the magnitude of the exponential's argument, clamped where the library clamps it (E is then an exact 0)"""
    x = 0.5 * s if base == "se" else _C[base] * np.sqrt(s)
    return np.minimum(x, 800.0)


def units_value(base, D, s):
    return 4.0 + exponent(base, s) * (D + 7) + 2 * D + 32


def units_inscale(base, D, s):
    return units_value(base, D, s) + D + 8


def value_bound(base, D, G, rec):
    return units_value(base, D, G["s"]) * EPS * rec["value_sabs"] + FLOOR


def inscale_bound(base, D, G, rec):
    return units_inscale(base, D, G["s"]) * EPS * rec["inscale_sabs"] + FLOOR


# ---- long-double linear algebra for the truths of whole models ----------------------------------------------------------
def cholesky_ld(A):
    """lower Cholesky factor of A in A's own dtype (long double), None if a pivot is not positive"""
    A = np.array(A)
    n = A.shape[0]
    Lc = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not d > 0:
            return None
        Lc[j, j] = np.sqrt(d)
        Lc[j + 1:, j] = (A[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    return Lc


def solve_lower_ld(Lc, b):
    x = np.array(b, dtype=Lc.dtype)
    for i in range(Lc.shape[0]):
        x[i] = (x[i] - Lc[i, :i] @ x[:i]) / Lc[i, i]
    return x


def solve_upper_ld(U, b):
    x = np.array(b, dtype=U.dtype)
    for i in range(U.shape[0] - 1, -1, -1):
        x[i] = (x[i] - U[i, i + 1:] @ x[i + 1:]) / U[i, i]
    return x
