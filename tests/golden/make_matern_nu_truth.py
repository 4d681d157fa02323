"""Generate tests/golden/matern_nu_truth.json: 60-digit (mpmath) values of the general-nu Matern kind (SGP_MATERN_NU,
include/sthenomi_kprod.h)
    k = 2^(1 - nu) / Gamma(nu) x^nu K_nu(x),   x = sqrt(2 nu) d,   d = sqrt(d2)
and of the two derivatives the gradient contractions use
    kx = dk / d(d2) = -(nu / x) 2^(1 - nu) / Gamma(nu) x^nu K_(nu-1)(x)          dk = 2 d2 kx  (both inputs scaled by g, at g = 1)
with the library's conventions where the formula has no value: at d2 = 0, k = 1, dk = 0 and kx = -nu / (2 (nu - 1)) for
nu > 1 (the limit) and 0 for nu <= 1 (where it diverges: the subgradient Matern-1/2 has there); at d2 = +inf all three are 0.

Grid, for every nu of NUS: the offsets D; the three d at which x = 2 (1 - 2^-20), 2, 2 (1 + 2^-20) (the routine changes
from Temme's series to the continued fraction at x = 2); one d past the underflow of k (the first x on a grid of 5 from 700
at which k < 2^-1080); d = 1e160, whose square overflows.  As in make_kernel_truth.py, d2 = fl(d d) is stored and the truth
is the function AT THAT DOUBLE (and at the double nu).

    python tests/golden/make_matern_nu_truth.py      (a few seconds; needs mpmath)

Layout (hex floats): nus; grid[repr(nu)] {t, d2, k, kx, dk, must_zero}: must_zero the indices whose k is below 2^-1076.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_kernel_truth import hexes  # noqa: E402
from make_kprod_truth import signed_double  # noqa: E402

mp.mp.dps = 60
NUS = (0.1, 0.3, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 2.5, 3.7, 7.5, 12.0, 25.0, 32.0)
D = (0.0, 1e-160, 1e-30, 1e-8, 1e-3, 0.05, 0.3, 1.0, 1.4, 2.5, 6.0, 20.0, 100.0, 400.0)
ZERO_BELOW = mp.mpf(2) ** -1076


def truths(nu, d2):
    """(k, kx, dk) as mpf at the doubles nu and d2 (or +inf)"""
    v = mp.mpf(nu)
    if d2 == np.inf:
        return mp.mpf(0), mp.mpf(0), mp.mpf(0)
    if d2 == 0.0:
        return mp.mpf(1), (-v / (2 * (v - 1)) if nu > 1.0 else mp.mpf(0)), mp.mpf(0)
    s = mp.mpf(d2)
    x = mp.sqrt(2 * v * s)
    c = mp.power(2, 1 - v) / mp.gamma(v) * mp.power(x, v)
    k = c * mp.besselk(v, x)
    kx = -(v / x) * c * mp.besselk(v - 1, x)
    return k, kx, 2 * s * kx


def offsets(nu):
    v = mp.mpf(nu)
    r = mp.sqrt(2 * v)
    ts = [float(d) for d in D]
    ts += [float(mp.mpf(2) * (1 + sgn * mp.mpf(2) ** -20) / r) for sgn in (-1, 0, 1)]
    x = mp.mpf(700)
    while truths(nu, float((x / r) ** 2))[0] >= mp.mpf(2) ** -1080:
        x += 5
    ts += [float(x / r), 1e160]
    return ts


def build():
    out = {"digits": 60, "nus": [repr(nu) for nu in NUS], "grid": {}}
    for nu in NUS:
        ts = offsets(nu)
        with np.errstate(over="ignore"):
            d2 = [float(np.float64(t) * np.float64(t)) for t in ts]
        vals = [truths(nu, v) for v in d2]
        out["grid"][repr(nu)] = {"t": hexes(ts), "d2": hexes(d2), "k": hexes([signed_double(v[0]) for v in vals]),
                                 "kx": hexes([signed_double(v[1]) for v in vals]),
                                 "dk": hexes([signed_double(v[2]) for v in vals]),
                                 "must_zero": [i for i, v in enumerate(vals) if v[0] < ZERO_BELOW]}
    return out


def main():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "matern_nu_truth.json")
    with open(path, "w") as f:
        json.dump(build(), f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
