"""The committed 60-digit truth table of the NeuralNetwork, FBM and Exponentiated kinds and their derivatives
(tests/golden/dotkinds_truth.json, written by tests/golden/make_dotkinds_truth.py) and the error models the tests hold the
formulas of csrc/kprod.hip to.  TEST INFRASTRUCTURE ONLY.  eps = 2^-53 throughout; every bound is ABSOLUTE, per entry.

The constants come from documented bounds, not from what a device returned: the OpenCL C specification's limits for double
precision, which the device library implements -- atan2 <= 6 ulp, asin <= 4 ulp, pow <= 16 ulp, log <= 3 ulp, exp <= 3 ulp,
sqrt and fma correctly rounded; 1 ulp <= 2 eps relative.  glibc (the NumPy mirror, tests/dotkinds_np.py) stays under 1 ulp
for all of them.  All bounds are first order in eps (the second-order terms are below eps times the first).

The scalars (kp_dot_scalars; the mirror forms them with separately rounded products, which the same bounds cover with D + 1):
    s  = x'y     a chain of D fma's:                    |ds| <= (D + 1) eps S,   S = sum_d |x_d y_d|  (>= |s|)
    a, b         the same chain over positive terms:    relative (D + 1) eps
    d2           D differences (eps each, twice in the square) and D fma's:   relative (D + 3) eps
    L  = sum_{i<j} c_ij^2,  c = p - q,  p = fl(x_i y_j),  q = fl(x_j y_i):    |dc| <= eps (|p| + |q| + |c|), so
                 |dL| <= eps (sum 2 |c| (|p| + |q| + |c|) + (P + 1) L),   P = D (D - 1) / 2  -- no term is as large as a b
    R2 = ((a + b) + 1) + L:   |dR2| <= (D + 1) eps (a + b) + 3 eps R2 + |dL|;   R = sqrt(R2):  |dR| <= |dR2| / (2 R) + eps R

NEURALNET   k = atan2(s, R).  With Q = s^2 + R^2 = (1 + a)(1 + b):  dk/ds = R / Q,  dk/dR = -s / Q, so
    |dk| <= (R |ds| + |s| |dR|) / Q  +  12 eps |k| (atan2)  +  eps |k| (the table's rounding)
  the first term is the conditioning of R and of s: the bound is in units of max(|k|, that conditioning), as it must be --
  |k| itself can be 1e-16 (orthogonal points) or pi / 2 - 1e-6 (parallel points at norm 1e6) under the same formula.
  The textbook asin(u), u = s / sqrt((1 + a)(1 + b)), has d asin / du = sqrt(Q) / R, which is 1e6 and more on nearly
  parallel points at large norms, times the 3 eps |u| of u's own roundings: it breaks this bound there, and the tests say so.
    dg = s (1/(1+a) + 1/(1+b)) / R:   |dg| (|dR| / R + (D + 8) eps) + (1/(1+a) + 1/(1+b)) |ds| / R + ulp
    dx_d = c1 x_d + c3 y_d,  c1 = -s / ((1 + a) R),  c3 = 1 / R:
                                      T (|dR| / R + (D + 8) eps) + |x_d| |ds| / ((1 + a) R) + ulp,   T = |c1 x_d| + |c3 y_d|
FBM         k = ((pa + pb) - pd) / 2,  pv = pow(v, h): 32 eps from pow, h times the relative error of its base
    |dk| <= eps / 2 ((34 + h (D + 1)) (pa + pb) + (33 + h (D + 3)) pd) + eps |k|;   pd <= 2 (pa + pb) for h <= 1
  hence   bound = (50 + h (1.5 D + 3.5)) eps (a^h + b^h) + eps |k|:  absolute in units of a^h + b^h, because the value cancels
    dg = 2 h k:     2 h bound_k + 3 eps |dg|
    dp = ((la + lb) - ld) / 2,  lv = pv log v (log: 6 eps of |log v|, and the base's relative error absolutely):
                    eps / 2 sum_v pv (|log v| (41 + h D_v) + D_v) + eps (|la| + |lb| + |ld|) + ulp,   D_v = D + 1, D + 1, D + 3
    dx_d = c1 x_d + c2 (x_d - y_d),  c1 = h pa / a,  c2 = -h pd / d2:
                    eps ((38 + (h + 1)(D + 1)) |c1 x_d| + (39 + (h + 1)(D + 3)) |c2 (x_d - y_d)|) + ulp
  A power term whose base is exactly 0 is exactly 0 in the table and in the formula: it contributes no error.
EXPONENTIATED  k = exp(s):  the error of s is RELATIVE on k
    |dk| <= |k| ((D + 1) eps S + 6 eps (exp) + eps)
    dg = 2 s k:     |dg| (rel_k + 3 eps) + 2 |k| |ds| + ulp           dx_d = k y_d:   |dx_d| (rel_k + 2 eps) + ulp
  An overflowed truth (2 s k beyond s = 700) is +-inf on both sides.
`ulp` above is one spacing of the truth (its own rounding and the last operation's).
"""
import json
import os

import numpy as np

EPS = 2.0 ** -53
HS = (0.1, 0.25, 0.5, 0.75, 1.0)
KINDS = ("nn", "fbm", "exp")


def _unhex(xs):
    return np.array([float.fromhex(s) for s in xs])


class Group:
    """the pairs of one kind and one dimension: X, Y (D x n, pair i = column i of each), cat, truth[name] (k, dg, dp: n;
    dx, dy: D x n)"""

    def __init__(self, D, pairs, key, h=None):
        self.D, self.h, self.n = D, h, len(pairs)
        self.cat = [p["cat"] for p in pairs]
        self.X = np.asfortranarray(np.array([_unhex(p["x"]) for p in pairs]).T.reshape(D, -1))
        self.Y = np.asfortranarray(np.array([_unhex(p["y"]) for p in pairs]).T.reshape(D, -1))
        ent = [p[key] if h is None else p[key][repr(h)] for p in pairs]
        self.truth = {"k": _unhex([e["k"] for e in ent]), "dg": _unhex([e["dg"] for e in ent]),
                      "dp": _unhex([e["dp"] for e in ent]) if h is not None else np.zeros(len(ent)),
                      "dx": np.array([_unhex(e["dx"]) for e in ent]).T.reshape(D, -1),
                      "dy": np.array([_unhex(e["dy"]) for e in ent]).T.reshape(D, -1)}

    def is_cat(self, name):
        return np.array([c == name for c in self.cat])


_cache = {}


def load():
    """{"nn": {D: Group}, ("fbm", h): {D: Group}, "exp": {D: Group}}"""
    if not _cache:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dotkinds_truth.json")) as fh:
            g = json.load(fh)
        assert tuple(float(h) for h in g["hs"]) == HS
        dims = sorted({p["D"] for p in g["pairs"]})
        _cache["nn"] = {D: Group(D, [p for p in g["pairs"] if p["D"] == D and "nn" in p], "nn") for D in dims}
        for h in HS:
            _cache[("fbm", h)] = {D: Group(D, [p for p in g["pairs"] if p["D"] == D and repr(h) in p.get("fbm", ())], "fbm", h) for D in dims}
        _cache["exp"] = {D: Group(D, [p for p in g["pairs"] if p["D"] == D and p["exp"] is not None], "exp") for D in dims}
    return _cache


def _pair_scalars(X, Y):
    """per pair, in float64 (the bounds need them to a few digits only): s, S, a, b, d2, L, dL"""
    D = X.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        s, S = np.sum(X * Y, 0), np.sum(np.abs(X * Y), 0)
        a, b, d2 = np.sum(X * X, 0), np.sum(Y * Y, 0), np.sum((X - Y) ** 2, 0)
        lag, dl = np.zeros_like(s), np.zeros_like(s)
        for i in range(D):
            for j in range(i + 1, D):
                p, q = X[i] * Y[j], X[j] * Y[i]
                c = p - q
                lag = lag + c * c
                dl = dl + 2.0 * np.abs(c) * (np.abs(p) + np.abs(q) + np.abs(c))
        dl = EPS * (dl + (D * (D - 1) / 2 + 1) * lag)
    return s, S, a, b, d2, lag, dl


def _sp(v):
    return np.spacing(np.abs(v))


def nn_tolerances(g):
    D = g.D
    s, S, a, b, _, lag, dl = _pair_scalars(g.X, g.Y)
    t = g.truth
    ds = (D + 1) * EPS * S
    R2 = ((a + b) + 1.0) + lag
    R = np.sqrt(R2)
    dR = ((D + 1) * EPS * (a + b) + 3.0 * EPS * R2 + dl) / (2.0 * R) + EPS * R
    Q = (1.0 + a) * (1.0 + b)
    ia, ib = 1.0 / (1.0 + a), 1.0 / (1.0 + b)
    out = {"k": (R * ds + np.abs(s) * dR) / Q + 13.0 * EPS * np.abs(t["k"]),
           "dg": np.abs(t["dg"]) * (dR / R + (D + 8) * EPS) + (ia + ib) * ds / R + _sp(t["dg"]),
           "dp": np.zeros(g.n)}
    for name, P_, Q_, inv in (("dx", g.X, g.Y, ia), ("dy", g.Y, g.X, ib)):
        T = np.abs(s * inv / R)[None] * np.abs(P_) + np.abs(Q_) / R[None]
        out[name] = T * (dR / R + (D + 8) * EPS)[None] + np.abs(P_) * (inv * ds / R)[None] + _sp(t[name])
    return out


def _pw(v, h):
    return np.where(v > 0.0, np.power(np.where(v > 0.0, v, 1.0), h), 0.0)


def fbm_tolerances(g):
    D, h = g.D, g.h
    _, _, a, b, d2, _, _ = _pair_scalars(g.X, g.Y)
    t = g.truth
    pa, pb, pd = _pw(a, h), _pw(b, h), _pw(d2, h)
    bk = (50.0 + h * (1.5 * D + 3.5)) * EPS * (pa + pb) + EPS * np.abs(t["k"])
    out = {"k": bk, "dg": 2.0 * h * bk + 3.0 * EPS * np.abs(t["dg"])}
    dp, mag = np.zeros(g.n), np.zeros(g.n)
    for v, pv, Dv in ((a, pa, D + 1), (b, pb, D + 1), (d2, pd, D + 3)):
        lg = np.abs(np.log(np.where(v > 0.0, v, 1.0)))
        dp = dp + pv * (lg * (41.0 + h * Dv) + Dv)
        mag = mag + pv * lg
    out["dp"] = 0.5 * EPS * dp + EPS * mag + _sp(t["dp"])
    c2 = np.where(d2 > 0.0, h * pd / np.where(d2 > 0.0, d2, 1.0), 0.0)
    for name, P_, Q_, v, pv in (("dx", g.X, g.Y, a, pa), ("dy", g.Y, g.X, b, pb)):
        c1 = np.where(v > 0.0, h * pv / np.where(v > 0.0, v, 1.0), 0.0)
        out[name] = EPS * ((38.0 + (h + 1.0) * (D + 1)) * c1[None] * np.abs(P_) +
                           (39.0 + (h + 1.0) * (D + 3)) * c2[None] * np.abs(P_ - Q_)) + _sp(t[name])
    return out


def exp_tolerances(g):
    D = g.D
    s, S, _, _, _, _, _ = _pair_scalars(g.X, g.Y)
    t = g.truth
    ds = (D + 1) * EPS * S
    rel = ds + 7.0 * EPS
    with np.errstate(over="ignore", invalid="ignore"):
        out = {"k": np.abs(t["k"]) * rel, "dg": np.abs(t["dg"]) * (rel + 3.0 * EPS) + 2.0 * np.abs(t["k"]) * ds + _sp(t["dg"]),
               "dp": np.zeros(g.n)}
        for name in ("dx", "dy"):
            out[name] = np.abs(t[name]) * (rel + 2.0 * EPS)[None] + _sp(t[name])
    return {k: np.where(np.isfinite(v), v, 0.0) for k, v in out.items()}     # (an overflowed truth: both sides are +-inf)


def tolerances(kind, g):
    return {"nn": nn_tolerances, "fbm": fbm_tolerances, "exp": exp_tolerances}[kind](g)


def violations(got, truth, tol):
    """flat indices where `got` is NaN or further than tol from the truth (an infinite truth must be met exactly)"""
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
