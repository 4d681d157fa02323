"""Generate tests/golden/dotkinds_truth.json: 60-digit (mpmath) values of the three kinds of the product path that are
functions of s = x'y, a = x'x, b = y'y and d2 = |x - y|^2 (include/sthenomi_kprod.h)
    NeuralNetwork    k = asin(s / sqrt((1 + a)(1 + b)))
    FBM              k = (a^h + b^h - d2^h) / 2,          h in {0.1, 0.25, 0.5, 0.75, 1.0}
    Exponentiated    k = exp(s)
and of the derivatives the gradient contractions use, with R^2 = (1 + a)(1 + b) - s^2:
                     d k / d x (row point)                  d k / d g (both inputs scaled by g, at g = 1)   d k / d param
    NeuralNetwork    (y - s x / (1 + a)) / R                s (1 / (1 + a) + 1 / (1 + b)) / R                0
    FBM              h a^(h-1) x - h d2^(h-1) (x - y)       2 h k                                            (a^h ln a + b^h ln b - d2^h ln d2) / 2
    Exponentiated    k y                                    2 s k                                            0
d k / d y is the same formula with x and y exchanged.  FBM's convention where a formula has no value: a power term whose
base is exactly 0 contributes exactly 0 to the value and to every derivative (0^h ln 0 := 0; 0^(h-1) := 0 for h < 1 too).

The truth is the function AT THE STORED DOUBLES: the points are hex doubles and every scalar is formed from them in 60
digits (more where the cancellation in R^2 or in FBM's value needs it: the working precision is raised until two successive
precisions agree to 40 digits).

Pairs, per dimension D in {1, 2, 3, 8, 16} (fewer at 8 and 16; beyond D = 1 each pair carries two of the five h, in turn, to keep the file small),
norms from 1e-8 to 1e6:
    random        independent directions, equal and unequal norms
    parallel      y = c (x + angle * perpendicular), relative angle 1e-3 .. 1e-8 (D = 1: y = c x)
    antiparallel  y = -c x (rounded)
    equal         y == x bit for bit
    origin        x = 0 or y = 0
    onecoord      both points on one coordinate axis
    exps          Exponentiated only: pairs scaled so that s runs from -700 to 708
Exponentiated is tabulated on every pair whose |s| <= 709.

    python tests/golden/make_dotkinds_truth.py      (a few seconds; needs mpmath)

Layout: {"digits", "hs", "pairs": [{"D", "cat", "x": [hex], "y": [hex], "nn": {k, dg, dx, dy}, "fbm": {repr(h): {k, dg, dp,
dx, dy}}, "exp": {k, dg, dx, dy} | null}]}, every number a hex double, correctly rounded.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_kprod_truth import signed_double  # noqa: E402

HS = (0.1, 0.25, 0.5, 0.75, 1.0)
DIMS = (1, 2, 3, 8, 16)


def _scalars(x, y):
    xs, ys = [mp.mpf(v) for v in x], [mp.mpf(v) for v in y]
    s = mp.fsum(p * q for p, q in zip(xs, ys))
    a = mp.fsum(p * p for p in xs)
    b = mp.fsum(q * q for q in ys)
    d2 = mp.fsum((p - q) ** 2 for p, q in zip(xs, ys))
    return xs, ys, s, a, b, d2


def nn_truths(x, y):
    xs, ys, s, a, b, _ = _scalars(x, y)
    R = mp.sqrt((1 + a) * (1 + b) - s * s)
    k = mp.asin(s / mp.sqrt((1 + a) * (1 + b)))
    dg = s * (1 / (1 + a) + 1 / (1 + b)) / R
    dx = [(q - s * p / (1 + a)) / R for p, q in zip(xs, ys)]
    dy = [(p - s * q / (1 + b)) / R for p, q in zip(xs, ys)]
    return k, dg, dx, dy


def _pw(v, h):
    return mp.power(v, h) if v > 0 else mp.mpf(0)


def _pwlog(v, h):
    return mp.power(v, h) * mp.log(v) if v > 0 else mp.mpf(0)


def _pwm1(v, h):
    return mp.power(v, h - 1) if v > 0 else mp.mpf(0)


def fbm_truths(h, x, y):
    xs, ys, s, a, b, d2 = _scalars(x, y)
    h = mp.mpf(h)
    k = (_pw(a, h) + _pw(b, h) - _pw(d2, h)) / 2
    dp = (_pwlog(a, h) + _pwlog(b, h) - _pwlog(d2, h)) / 2
    dx = [h * _pwm1(a, h) * p - h * _pwm1(d2, h) * (p - q) for p, q in zip(xs, ys)]
    dy = [h * _pwm1(b, h) * q - h * _pwm1(d2, h) * (q - p) for p, q in zip(xs, ys)]
    return k, 2 * h * k, dp, dx, dy


def exp_truths(x, y):
    xs, ys, s, _, _, _ = _scalars(x, y)
    k = mp.exp(s)
    return k, 2 * s * k, [k * q for q in ys], [k * p for p in xs]


def settled(fn, *args):
    """fn(*args) flattened to mpf's, at a working precision raised until two successive ones agree to 40 digits"""
    def flat(v):
        out = []
        for e in v:
            out.extend(e if isinstance(e, list) else [e])
        return out
    prev = None
    for dps in (60, 120, 240, 480):
        with mp.workdps(dps):
            cur = [+e for e in flat(fn(*args))]
        # (a derivative that is exactly 0 by cancellation, FBM's d / dx at D = 1 for instance, comes out as rounding noise of
        # the working precision: it settles against the largest value of the pair, 1e-50 of which is far below a double's ulp)
        big = max(abs(c) for c in cur)
        if prev is not None and all(abs(p - c) <= abs(c) * mp.mpf(10) ** -40 + big * mp.mpf(10) ** -50
                                    for p, c in zip(prev, cur)):
            return cur
        prev = cur
    raise AssertionError("the truth does not settle")


def hx(v):
    return float(signed_double(v)).hex()


def pack(vals, D, with_dp):
    """the flat list of settled() -> a dict of hex doubles"""
    out = {"k": hx(vals[0]), "dg": hx(vals[1])}
    at = 2
    if with_dp:
        out["dp"] = hx(vals[2])
        at = 3
    out["dx"] = [hx(v) for v in vals[at:at + D]]
    out["dy"] = [hx(v) for v in vals[at + D:at + 2 * D]]
    return out


def unit(rng, D):
    v = rng.standard_normal(D)
    return v / np.linalg.norm(v)


def pairs_for(D, rng):
    """[(category, x, y)] as float64 arrays"""
    norms = (1e-8, 1e-4, 1e-2, 1.0, 1e2, 1e4, 1e6)
    step = 2 if D < 8 else 3      # fewer pairs where each one is long
    few = D >= 8
    out = []
    for i, nx in enumerate(norms[::step]):
        ny = norms[(3 * i + 2) % len(norms)]
        if not few or i % 2 == 0:
            out.append(("random", nx * unit(rng, D), nx * unit(rng, D)))
        if not few or i % 2 == 1:
            out.append(("random", nx * unit(rng, D), ny * unit(rng, D)))
    for nx, ang in ((1e-2, 1e-3), (1.0, 1e-5), (1.0, 1e-8), (1e3, 1e-3), (1e3, 1e-6), (1e6, 1e-4), (1e6, 1e-8))[::step]:
        u = unit(rng, D)
        if D > 1:
            p = unit(rng, D)
            p = p - (p @ u) * u
            p = p / np.linalg.norm(p)
        else:
            p = np.zeros(1)
        out.append(("parallel", nx * u, (1.7 * nx) * (u + ang * p)))
    for nx in (1e-4, 1.0, 1e3, 1e6)[::step]:
        x = nx * unit(rng, D)
        out.append(("antiparallel", x, -0.6 * x))
    for nx in (1e-8, 1.0, 1e3, 1e6)[::step]:
        x = nx * unit(rng, D)
        out.append(("equal", x, x.copy()))
    for nx in (1e-8, 1.0, 1e6)[::2 if few else 1]:
        out.append(("origin", nx * unit(rng, D), np.zeros(D)))
    out.append(("origin", np.zeros(D), 3.0 * unit(rng, D)))
    if not few:
        out.append(("origin", np.zeros(D), np.zeros(D)))
    for nx in (1e-3, 2.0, 1e5)[::step]:
        x, y = np.zeros(D), np.zeros(D)
        x[D - 1], y[D - 1] = nx, -0.37 * nx
        out.append(("onecoord", x, y))
        y2 = np.zeros(D)
        y2[0] = nx
        if D > 1:
            out.append(("onecoord", x, y2))       # two axes: s = 0 exactly
    if D in (1, 3, 16):
        for s in (-700.0, -100.0, -1.0, 1e-10, 1.0, 100.0, 700.0, 708.0)[::2 if D == 16 else 1] + ((708.0,) if D == 16 else ()):
            x = unit(rng, D) * np.sqrt(abs(s)) * 1.3
            yd = unit(rng, D) if D > 1 else np.ones(1)
            if abs(x @ yd) < 0.05 * np.linalg.norm(x):
                yd = yd + x / np.linalg.norm(x)
            y = yd * (s / (x @ yd))
            while x @ y > 709.7:                  # (the rounded dot product must stay below the overflow of exp)
                y = y * (1 - 2.0 ** -40)
            out.append(("exps", x, y))
    return out


def build():
    rng = np.random.default_rng(20250304)
    out = {"digits": 60, "hs": [repr(h) for h in HS], "pairs": []}
    for D in DIMS:
        for i, (cat, x, y) in enumerate(pairs_for(D, rng)):
            x, y = [float(v) for v in x], [float(v) for v in y]
            e = {"D": D, "cat": cat, "x": [v.hex() for v in x], "y": [v.hex() for v in y]}
            s = sum(mp.mpf(p) * mp.mpf(q) for p, q in zip(x, y))
            if cat != "exps":
                e["nn"] = pack(settled(nn_truths, x, y), D, False)
                hs = HS if D == 1 else (HS[i % 5], HS[(i + 2) % 5])      # beyond D = 1: two of the five h per pair, in turn
                e["fbm"] = {repr(h): pack(settled(fbm_truths, h, x, y), D, True) for h in hs}
            e["exp"] = pack(settled(exp_truths, x, y), D, False) if abs(s) <= 709 else None
            out["pairs"].append(e)
    return out


def main():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dotkinds_truth.json")
    with open(path, "w") as f:
        json.dump(build(), f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
