"""Generate tests/golden/kprod_truth.json: 60-digit (mpmath) values of the RationalQuadratic kernel
    k = (1 + d2 / (2 alpha))^-alpha
and of the two derivatives the gradient contraction of product chains uses (include/sthenomi_kprod.h)
    dk/dg     = -d2 (1 + d2 / (2 alpha))^(-alpha - 1)            both inputs scaled by g, at g = 1
    dk/dalpha = k (u / (1 + u) - log1p(u)),  u = d2 / (2 alpha)
at alpha in {0.1, 1.3, 50}, on the offsets of make_kernel_truth.py that every kernel shares (d2 = 0, subnormal, 1e-300,
1e+300, the largest finite square, +inf, and 25 of its 200 points over 2^-60 .. 2^20) followed by offsets chosen per alpha by the
argument -a = -alpha log1p(u) of the formula's exp.  As there, d2 = fl(t t) is stored: the table's d2 is bit for bit the
argument the device's formula sees, and the truth is the function AT THAT DOUBLE.

    python tests/golden/make_kprod_truth.py      (a few seconds; needs mpmath)

Layout (hex floats): common {t, d2}; alphas[str(alpha)]: {t, d2} the alpha's own offsets, {k, dk, dp} the truths at the
common offsets followed by those at its own, must_zero: the indices whose truth is below 2^-1076.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_kernel_truth import common_offsets, hexes, to_double  # noqa: E402

mp.mp.dps = 60
ALPHAS = (0.1, 1.3, 50.0)
ZERO_BELOW = mp.mpf(2) ** -1076          # below half of what still rounds up to the smallest subnormal: must be 0


def signed_double(v):
    return -to_double(-v) if v < 0 else to_double(v)


def truths_at(alpha, d2):
    """(k, dk/dg, dk/dalpha) as mpf at the double d2 (or +inf) for the double alpha"""
    if d2 == np.inf:
        return mp.mpf(0), mp.mpf(0), mp.mpf(0)
    a, d = mp.mpf(alpha), mp.mpf(d2)
    u = d / (2 * a)
    l = mp.log1p(u)
    k = mp.exp(-a * l)
    return k, -d * mp.exp(-(a + 1) * l), k * (u / (1 + u) - l)


def own_offsets(alpha):
    """offsets t with alpha log1p(t^2 / (2 alpha)) = a for arguments a that matter to a hand-written exp"""
    ln2 = mp.log(2)
    args = [(n + mp.mpf(1) / 2) * ln2 for n in (1, 10, 100, 1000)]
    args += [mp.mpf(v) for v in (700, 708.4, 720, 740, 744.5, 745.13, 745.14, 746.5, 775, 790, 799.999, 800, 800.001, 1e4)]
    ts = []
    for a in args:
        u = mp.expm1(a / mp.mpf(alpha))
        t = mp.sqrt(2 * mp.mpf(alpha) * u)
        if t < mp.mpf(1.3e154):                      # (alpha = 0.1 never gets there: its exp argument stays above -72)
            t0 = float(t)
            ts += [float(np.nextafter(t0, 0)), t0, float(np.nextafter(t0, np.inf))]
    return ts


def thinned(ts):
    """the shared offsets with every eighth of their 200 random points (the special ones in front and behind all stay)"""
    n_front, n_back = len(ts) - 203, 3
    assert n_front > 10
    return ts[:n_front] + ts[n_front:len(ts) - n_back:8] + ts[len(ts) - n_back:]


def build():
    tc = thinned(common_offsets())
    out = {"digits": 60, "common": {"t": hexes(tc)}, "alphas": {}}
    for alpha in ALPHAS:
        to = own_offsets(alpha)
        with np.errstate(over="ignore"):
            d2 = [float(np.float64(t) * np.float64(t)) for t in tc + to]
        vals = [truths_at(alpha, v) for v in d2]
        out["common"]["d2"] = hexes(d2[:len(tc)])
        out["alphas"][repr(alpha)] = {"t": hexes(to), "d2": hexes(d2[len(tc):]), "k": hexes([to_double(v[0]) for v in vals]),
                                      "must_zero": [i for i, v in enumerate(vals) if v[0] < ZERO_BELOW],
                                      "dk": hexes([signed_double(v[1]) for v in vals]),
                                      "dp": hexes([signed_double(v[2]) for v in vals])}
    return out


def main():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kprod_truth.json")
    with open(path, "w") as f:
        json.dump(build(), f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
