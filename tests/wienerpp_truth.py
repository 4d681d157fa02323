"""The committed 60-digit truth table of the Wiener and PiecewisePolynomial kinds and their derivatives
(tests/golden/wienerpp_truth.json, written by tests/golden/make_wienerpp_truth.py) and the error models the tests hold the
formulas of csrc/kprod.hip to.  TEST INFRASTRUCTURE ONLY.  eps = 2^-53 throughout; every bound is ABSOLUTE, per entry, and no
pair of the table is excluded from any comparison.

Only +, x, / by constants, fma and sqrt occur, all correctly rounded (relative eps each), so the bounds are a first-order
rounding analysis of the formulation chosen; none is fitted to what a device returned.

The scalars (kp_dot_scalars; the NumPy mirror forms them with separately rounded products, which the same bounds cover):
    a = x'x, b = y'y   a chain of D fma's over positive terms:   relative (D + 1) eps
    d2                 D differences (eps each, twice in the square) and D fma's:   relative (D + 3) eps
    X, Y, d            their correctly rounded square roots: half the relative error plus eps / 2, so each of the three has
                       relative error at most  er = (D / 2 + 2) eps

WIENER i.  k is a sum of positive terms, each a product of 2 i + 1 factors out of {X, Y, d, m, M} (it is homogeneous of that
degree), min and max are exact selections.  The one difference, T = (X + Y) - m / 2 >= 3 m / 2, amplifies the relative error
of its operands by at most (X + Y + m / 2) / T <= 5 / 3: it counts as one more factor.  Every term takes at most 12 rounded
operations, the sum one, the table's own rounding one:
    |dk| <= ((2 i + 2) er + 16 eps) |k|  =  wiener_rel(i, D) |k|            dg = (2 i + 1) k:  (wiener_rel + 2 eps) |dg|
  dx_d = c1 x_d + c2 (x_d - y_d),  c1 = kX / X,  c2 = kd / d:  kX and kd are sums of positive terms of degree 2 i (the
  difference 3 (X + Y) - 2 m >= 4 m in d k / d m of i = 2 amplifies by at most 2: one more factor), the quotient adds a factor,
  the difference x_d - y_d is rounded once, at most 20 operations per coefficient and 4 in the combination:
    |d dx_d| <= ((2 i + 2) er + 28 eps) (|c1 x_d| + |c2 (x_d - y_d)|) + ulp
  The two parts are taken in absolute value: they have opposite signs where x_d lies beyond y_d, and the bound stays absolute.
  At a tie X == Y the half-and-half rule is part of the truth; the table's ties are exact in float64 (integer coordinates), and
  its nearly equal norms differ by 1e-13, 400 times er: the order of X and Y is never in doubt.  Exact zeros (the origin, d == 0)
  are exact on both sides.
PIECEWISE q, j.  k = t^n p_q(r), n = j + q, t = 1 - r.  r carries er relatively, so t carries the ABSOLUTE error
    dt = er r + eps t      (the subtraction is exact for r >= 1/2; near r = 1 the cancellation leaves er, not er t)
  and the power t^e, e >= 1, taken by at most 2 log2(66) < 14 multiplications:
    |d t^e| <= e (t + 2 dt)^(e - 1) dt  =: P(e)     (first order, evaluated at the far end of the interval; covers t = 0, where
                                                    a computed r just below 1 against a true r >= 1 leaves dt^e)
  P(0) is 0, except within 2 dt of r = 1, where t^0 jumps from 1 to 0 (the kink of max(1 - r, 0) itself): there P(0) = 1.
  p_q has positive coefficients and degree q: r |p_q'| <= q p_q, at most 12 operations with the coefficients' roundings.
    |dk| <= p_q(r) P(n) + (q er + 32 eps) |k|
  kx = d k / d (d2) = t^(n-1) g(r),  g = -pt_q / 2 (q >= 1: degree q - 1, positive coefficients),  g = -j / (2 r) (q = 0):
    |d kx| <= |g| P(n - 1) + (3 er + 32 eps) |kx|  =: E
    dx_d = 2 kx (x_d - y_d):  2 |x_d - y_d| E + 4 eps |dx_d| + ulp          dg = 2 d2 kx:  2 d2 E + (D + 7) eps |dg| + ulp
  Beyond r = 1 + 2 er the computed r is beyond 1 too: value and derivatives are exact zeros and every bound is 0.
`ulp` above is one spacing of the truth (its own rounding and the last operation's).
"""
import json
import os

import numpy as np

EPS = 2.0 ** -53
IS = (0, 1, 2, 3)


def _unhex(xs):
    return np.array([float.fromhex(s) for s in xs])


class Group:
    """the pairs of one family, parameter and dimension: X, Y (D x n, pair i = column i of each), cat, truth[name] (k, dg: n;
    dx, dy: D x n)"""

    def __init__(self, D, pairs, ents):
        self.D, self.n = D, len(pairs)
        self.cat = [p["cat"] for p in pairs]
        self.integral = np.array([bool(p.get("integral", False)) for p in pairs])
        self.X = np.asfortranarray(np.array([_unhex(p["x"]) for p in pairs]).T.reshape(D, -1))
        self.Y = np.asfortranarray(np.array([_unhex(p["y"]) for p in pairs]).T.reshape(D, -1))
        self.truth = {"k": _unhex([e["k"] for e in ents]), "dg": _unhex([e["dg"] for e in ents]),
                      "dx": np.array([_unhex(e["dx"]) for e in ents]).T.reshape(D, -1),
                      "dy": np.array([_unhex(e["dy"]) for e in ents]).T.reshape(D, -1)}

    def is_cat(self, name):
        return np.array([c == name for c in self.cat])


_cache = {}


def load():
    """{("w", i): {D: Group}, ("p", q, j): {D: Group}}"""
    if not _cache:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wienerpp_truth.json")) as fh:
            g = json.load(fh)
        for D in sorted({p["D"] for p in g["pairs"]}):
            ps = [p for p in g["pairs"] if p["D"] == D]
            for i in IS:
                sel = [p for p in ps if str(i) in p.get("wiener", ())]
                _cache.setdefault(("w", i), {})[D] = Group(D, sel, [p["wiener"][str(i)] for p in sel])
            for key in sorted({k for p in ps for k in p.get("pp", ())}):
                q, j = (int(v) for v in key.split(","))
                sel = [p for p in ps if key in p.get("pp", ())]
                _cache.setdefault(("p", q, j), {})[D] = Group(D, sel, [p["pp"][key] for p in sel])
    return _cache


def _sp(v):
    return np.spacing(np.abs(v))


def eps_r(D):
    return (0.5 * D + 2.0) * EPS


def wiener_rel(i, D):
    return (2 * i + 2) * eps_r(D) + 16.0 * EPS


def wiener_tolerances(i, g):
    import wienerpp_np as wn
    t = g.truth
    rel = wiener_rel(i, g.D)
    out = {"k": rel * np.abs(t["k"]), "dg": (rel + 2.0 * EPS) * np.abs(t["dg"])}
    drel = (2 * i + 2) * eps_r(g.D) + 28.0 * EPS
    a, b, d2 = np.sum(g.X * g.X, 0), np.sum(g.Y * g.Y, 0), np.sum((g.X - g.Y) ** 2, 0)
    c = wn.wiener(i, a, b, d2)        # elementwise on the pairs: magnitudes to a few digits
    df = np.abs(g.X - g.Y)
    out["dx"] = drel * (np.abs(c["c1"])[None] * np.abs(g.X) + np.abs(c["c2"])[None] * df) + _sp(t["dx"])
    out["dy"] = drel * (np.abs(c["c1y"])[None] * np.abs(g.Y) + np.abs(c["c2"])[None] * df) + _sp(t["dy"])
    return out


def pp_poly(q, j, r):
    """(p_q(r), |g(r)|) in float64: g = pt_q / 2 for q >= 1, j / (2 r) for q = 0 (0 at r = 0)"""
    j = float(j)
    r = np.asarray(r, dtype=np.float64)
    if q == 0:
        return np.ones_like(r), np.where(r > 0.0, j / (2.0 * np.where(r > 0.0, r, 1.0)), 0.0)
    if q == 1:
        return 1.0 + (j + 1.0) * r, 0.5 * (j + 1.0) * (j + 2.0) + 0.0 * r
    if q == 2:
        return (1.0 + (j + 2.0) * r + (j + 1.0) * (j + 3.0) / 3.0 * r * r,
                0.5 * (j + 3.0) * (j + 4.0) / 3.0 * (1.0 + (j + 1.0) * r))
    n, c2, c3 = j + 3.0, (6.0 * j * j + 36.0 * j + 45.0) / 15.0, (j + 1.0) * (j + 3.0) * (j + 5.0) / 15.0
    return (1.0 + n * r + c2 * r * r + c3 * r ** 3,
            0.5 * ((n * n + n - 2.0 * c2) + ((n + 2.0) * c2 - 3.0 * c3) * r + (n + 3.0) * c3 * r * r))


def _pow_err(t, e, dt):
    """P(e) of the docstring"""
    if e == 0:
        return np.where(t <= 2.0 * dt, 1.0, 0.0)
    return e * (t + 2.0 * dt) ** (e - 1) * dt


def _pp_setup(D, r):
    r = np.asarray(r, dtype=np.float64)
    er = eps_r(D)
    with np.errstate(invalid="ignore", over="ignore"):
        outside = ~((r - 1.0) <= 2.0 * er * r) | ~np.isfinite(r)          # (an overflowed or NaN r is outside)
        rr = np.where(outside, 1.0, r)
    t = np.maximum(1.0 - rr, 0.0)
    return rr, t, er * rr + EPS * t, er, outside


def pp_value_bound(q, j, D, r, k):
    rr, t, dt, er, outside = _pp_setup(D, r)
    p, _ = pp_poly(q, j, rr)
    return np.where(outside, 0.0, p * _pow_err(t, int(j) + q, dt) + (q * er + 32.0 * EPS) * np.abs(k))


def pp_kx_bound(q, j, D, r, kx):
    rr, t, dt, er, outside = _pp_setup(D, r)
    _, gm = pp_poly(q, j, rr)
    return np.where(outside, 0.0, gm * _pow_err(t, int(j) + q - 1, dt) + (3.0 * er + 32.0 * EPS) * np.abs(kx))


def pp_tolerances(q, j, g):
    t = g.truth
    with np.errstate(over="ignore"):
        d2 = np.sum((g.X - g.Y) ** 2, 0)
    r = np.sqrt(d2)
    # |kx| from the truth: dg = 2 d2 kx
    kx = np.where((d2 > 0.0) & np.isfinite(d2), np.abs(t["dg"]) / (2.0 * np.where((d2 > 0.0) & np.isfinite(d2), d2, 1.0)), 0.0)
    E = pp_kx_bound(q, j, g.D, r, kx)
    with np.errstate(over="ignore", invalid="ignore"):
        d2f = np.where(np.isfinite(d2), d2, 0.0)
        out = {"k": pp_value_bound(q, j, g.D, r, t["k"]),
               "dg": 2.0 * d2f * E + (g.D + 7.0) * EPS * np.abs(t["dg"]) + _sp(t["dg"])}
        df = np.where(np.isfinite(g.X - g.Y), np.abs(g.X - g.Y), 0.0)
        for name in ("dx", "dy"):
            out[name] = 2.0 * df * E[None] + 4.0 * EPS * np.abs(t[name]) + _sp(t[name])
    return out


def tolerances(key, g):
    return wiener_tolerances(key[1], g) if key[0] == "w" else pp_tolerances(key[1], key[2], g)


def violations(got, truth, tol):
    """flat indices where `got` is NaN or further than tol from the truth"""
    got, truth, tol = np.asarray(got, dtype=np.float64), np.asarray(truth), np.asarray(tol)
    with np.errstate(invalid="ignore"):
        ok = (got == truth) | (np.abs(got - truth) <= tol)
    return np.flatnonzero(~ok.ravel())


def worst(got, truth, tol):
    """the largest |got - truth| / tol (0 where both are equal)"""
    got, truth, tol = np.asarray(got, dtype=np.float64), np.asarray(truth), np.asarray(tol)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(got == truth, 0.0, np.abs(got - truth) / tol)
    return float(np.max(r)) if r.size else 0.0
