#!/usr/bin/env python3
"""Writes tests/golden/deriv_truth.json: the derivative kinds (include/sthenomi.h: SGP_DERIV_*) at 80 digits.

    python tests/golden/make_deriv_truth.py

The truth does not re-type the device formulas: kappa(s) of each base kind is written down once, SymPy differentiates it
with respect to s three times, and mpmath evaluates the derivatives at 80 digits at the EXACT difference of the float64
points.  The entries are then the definitions of include/sthenomi.h,
    value:    (p+1, 0): 2 kappa' u_p;  (0, q+1): -2 kappa' u_q;  (p+1, q+1): -4 kappa'' u_p u_q - 2 kappa' delta_pq
    inscale:  d / dg of the value at points scaled by g, g = 1 -- SymPy again: the value as a function of g u, differentiated
and, with each, the sum of the absolute values of its addends (what a first-order rounding bound multiplies).  At an exactly
coincident pair the definitions are limits: the one-sided entries and every input-scale derivative are 0, the two-sided entry
is -2 kappa'(0+) delta_pq (SymPy's limit).

Cases: every base kind, D in {1, 3, 16}, (a, b) in {(1,0), (0,2), (1,1), (1,2)} (those whose coordinates exist at D), and
pairs at distance 0, 1e-160, 1e-8, 1, 40 and 1e200, two directions each.  Tiny and huge distances sit at the origin, so that
the float64 difference is the distance itself; s = 1e400 overflows in float64."""
import json
import os

import mpmath as mp
import numpy as np
import sympy as sp

mp.mp.dps = 500      # far more than the 80 digits kept: nothing that cancels near s = 1e-320 can reach them
HERE = os.path.dirname(os.path.abspath(__file__))
DISTANCES = (0.0, 1e-160, 1e-8, 1.0, 40.0, 1e200)
TERMS = ((1, 0), (0, 2), (1, 1), (1, 2))

s_, g_ = sp.symbols("s g", positive=True)
KAPPA = {
    "se": sp.exp(-s_ / 2),
    "m32": (1 + sp.sqrt(3 * s_)) * sp.exp(-sp.sqrt(3 * s_)),
    "m52": (1 + sp.sqrt(5 * s_) + sp.Rational(5, 3) * s_) * sp.exp(-sp.sqrt(5 * s_)),
}


def _forms(base):
    """mpmath functions (s, u_p, u_q) -> addends of the value and of its input-scale derivative, per shape of term"""
    k = KAPPA[base]
    k1, k2 = sp.simplify(sp.diff(k, s_)), sp.simplify(sp.diff(k, s_, 2))      # (closed forms without cancelling quotients)
    up, uq = sp.symbols("up uq", real=True)
    shapes = {"row": [2 * k1 * up], "col": [-2 * k1 * uq], "both": [-4 * k2 * up * uq], "both_same": [-4 * k2 * up * uq, -2 * k1]}
    out = {}
    for name, addends in shapes.items():
        # scaled by g: s -> g^2 s, u -> g u; the derivative at g = 1, addend by addend after expansion into monomials of kappa^(n)
        grads = []
        for a in addends:
            scaled = a.subs({s_: g_ ** 2 * s_, up: g_ * up, uq: g_ * uq}, simultaneous=True)
            d = sp.diff(scaled, g_).subs(g_, 1)
            grads.extend(sp.Add.make_args(sp.expand(sp.simplify(d))))
        out[name] = ([sp.lambdify((s_, up, uq), a, "mpmath") for a in addends],
                     [sp.lambdify((s_, up, uq), a, "mpmath") for a in grads])
    lim = sp.limit(-2 * k1, s_, 0, "+")
    return out, mp.mpf(sp.N(lim, 80))


def _points(D, rng):
    X, Y, R = [], [], []
    for r in DISTANCES:
        for rep in range(2):
            d = rng.standard_normal(D)
            d = d / np.linalg.norm(d) if D > 1 else np.array([1.0 if rep == 0 else -1.0])
            x = rng.standard_normal(D) if r in (0.0, 1e-8, 1.0, 40.0) else np.zeros(D)
            y = x - r * d
            X.append(x), Y.append(y), R.append(r)
    return np.array(X).T, np.array(Y).T, R


def main():
    rng = np.random.default_rng(20240607)
    table = {}
    for base in KAPPA:
        forms, at0 = _forms(base)
        table[base] = {}
        for D in (1, 3, 16):
            X, Y, R = _points(D, rng)
            n = X.shape[1]
            U = [[mp.mpf(float(X[d, i])) - mp.mpf(float(Y[d, i])) for d in range(D)] for i in range(n)]
            S = [mp.fsum(u * u for u in ui) for ui in U]
            with np.errstate(over="ignore"):
                s64 = ((X - Y) ** 2).sum(0)
            G = {"X": X.tolist(), "Y": Y.tolist(), "distance": R, "s": [float(min(s, mp.mpf("1e308"))) for s in S],
                 "s_overflows": [bool(np.isinf(v)) for v in s64], "terms": {}}
            for (a, b) in TERMS:
                if max(a, b) > D:
                    continue
                shape = "row" if b == 0 else "col" if a == 0 else "both_same" if a == b else "both"
                fv, fg = forms[shape]
                rec = {k: [] for k in ("value", "value_sabs", "inscale", "inscale_sabs")}
                rec["must_zero"], rec["exact"] = [], []
                for i in range(n):
                    up, uq = U[i][max(a, 1) - 1], U[i][max(b, 1) - 1]
                    if S[i] == 0:
                        v = [at0] if shape == "both_same" else [mp.mpf(0)]
                        gr = [mp.mpf(0)]
                        if shape == "both_same":
                            rec["exact"].append([i, float(at0)])
                        else:
                            rec["must_zero"].append(i)
                    else:
                        v = [f(S[i], up, uq) for f in fv]
                        gr = [f(S[i], up, uq) for f in fg]
                        if G["s_overflows"][i]:
                            rec["must_zero"].append(i)
                    rec["value"].append(float(mp.fsum(v)))
                    rec["value_sabs"].append(float(mp.fsum(abs(t) for t in v)))
                    rec["inscale"].append(float(mp.fsum(gr)))
                    rec["inscale_sabs"].append(float(mp.fsum(abs(t) for t in gr)))
                G["terms"][f"{a},{b}"] = rec
            table[base][str(D)] = G
    with open(os.path.join(HERE, "deriv_truth.json"), "w") as fh:
        json.dump(table, fh)
    print("wrote deriv_truth.json:", {b: {D: len(G["terms"]) for D, G in t.items()} for b, t in table.items()})


if __name__ == "__main__":
    main()
