"""Generate tests/golden/kinds_truth.json: 60-digit (mpmath) values of the two kinds the product path evaluates beside
RationalQuadratic and Linear (include/sthenomi_kprod.h)
    Cosine             k = cos(pi d),      d = sqrt(d2)
    GammaExponential   k = exp(-a),        a = d2^(gamma / 2),   gamma in {0.3, 1.0, 1.7, 2.0}
and of the three derivatives the gradient contractions use
    dk/dg   both inputs scaled by g, at g = 1:   -pi d sin(pi d)          -gamma a k
    kx      = dk / d(d2):                        -pi sin(pi d) / (2 d)    -(gamma / 2) a k / d2
    dp      = dk / d param:                      0                        -k a log(d2) / 2
with the library's conventions where a formula has no value: Cosine at d2 = 0 has kx = -pi^2 / 2 (the limit) and at
d2 = +inf is 1 with zero derivatives (every double >= 2^53 is an even integer); GammaExponential at d2 = 0 has kx = dp = 0
(the subgradient / the limit) and at d2 = +inf is 0 with zero derivatives.

The offsets are those of make_kernel_truth.py that every kernel shares, thinned as make_kprod_truth.py thins them (d2 = 0,
subnormal, 1e-300, 1e+300, the largest finite square, +inf, and 25 points over 2^-60 .. 2^20), followed by offsets of the
kind's own.  As there, d2 = fl(t t) is stored: the table's d2 is bit for bit the argument the device's formula sees, and the
truth is the function AT THAT DOUBLE.  Where d is large the working precision grows with it (cos(pi d) at d = 1e150 needs
150 digits of d before the first of the result).

    python tests/golden/make_kinds_truth.py      (a few seconds; needs mpmath)

Layout (hex floats): common {t, d2}; cosine {t, d2, k, dk, kx, dp}; gammaexp[str(gamma)] {t, d2, k, dk, kx, dp, must_zero}:
{t, d2} the kind's own offsets, the truths at the common offsets followed by those at its own, must_zero the indices whose
truth is below 2^-1076.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_kernel_truth import common_offsets, hexes, to_double  # noqa: E402
from make_kprod_truth import signed_double, thinned  # noqa: E402

mp.mp.dps = 60
GAMMAS = (0.3, 1.0, 1.7, 2.0)
ZERO_BELOW = mp.mpf(2) ** -1076


def cosine_truths(d2):
    """(k, dk/dg, kx, dp) as mpf at the double d2 (or +inf)"""
    if d2 == np.inf:
        return mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)
    if d2 == 0.0:
        return mp.mpf(1), mp.mpf(0), -mp.pi ** 2 / 2, mp.mpf(0)
    digits = 60 + max(0, int(np.ceil(0.5 * np.log10(d2))) + 2)
    with mp.workdps(digits):
        d = mp.sqrt(mp.mpf(d2))
        c, s = mp.cospi(d), mp.sinpi(d)
        return +c, -mp.pi * d * s, -mp.pi * s / (2 * d), mp.mpf(0)


def gammaexp_truths(gamma, d2):
    if d2 == np.inf or d2 == 0.0:
        return mp.mpf(0 if d2 else 1), mp.mpf(0), mp.mpf(0), mp.mpf(0)
    g, v = mp.mpf(gamma), mp.mpf(d2)
    a = mp.power(v, g / 2)
    k = mp.exp(-a)
    return k, -g * a * k, -(g / 2) * a * k / v, -k * a * mp.log(v) / 2


def around(t0):
    t0 = float(t0)
    return [float(np.nextafter(t0, 0)), t0, float(np.nextafter(t0, np.inf))]


def cosine_offsets():
    """d at and one ulp either side of half-integers (the zeros) and of integers, and 60 random d over 1e-8 .. 1e6"""
    ts = []
    for n in (0, 1, 2, 7, 100, 12345, 10 ** 6):
        ts += around(n + 0.5)
        if n:
            ts += around(float(n))
    rng = np.random.default_rng(20250116)
    ts += [float(10.0 ** e) for e in np.sort(rng.uniform(-8.0, 6.0, 60))]
    ts += [1e-8, 1e6]
    return ts


def gammaexp_offsets(gamma):
    """offsets t = a^(1 / gamma) for arguments a of the formula's exp that matter to a hand-written exp: where the
    reduction's n flips, where k is subnormal (a over 708.4 .. 745.13), beyond where it underflows (must be zero)"""
    ln2 = mp.log(2)
    args = [(n + mp.mpf(1) / 2) * ln2 for n in (1, 10, 100, 1000)]
    args += [mp.mpf(v) for v in (1e-3, 1.0, 700, 708.4, 720, 740, 744.5, 745.13, 745.14, 746.5, 775, 790, 799.999, 800, 800.001, 1e4)]
    ts = []
    for a in args:
        ts += around(mp.power(a, 1 / mp.mpf(gamma)))
    return ts


def table(truths, ts):
    with np.errstate(over="ignore"):
        d2 = [float(np.float64(t) * np.float64(t)) for t in ts]
    vals = [truths(v) for v in d2]
    return d2, {"k": hexes([signed_double(v[0]) for v in vals]), "dk": hexes([signed_double(v[1]) for v in vals]),
                "kx": hexes([signed_double(v[2]) for v in vals]), "dp": hexes([signed_double(v[3]) for v in vals]),
                "must_zero": [i for i, v in enumerate(vals) if abs(v[0]) < ZERO_BELOW]}


def build():
    tc = thinned(common_offsets())
    out = {"digits": 60, "common": {"t": hexes(tc)}, "gammaexp": {}}
    to = cosine_offsets()
    d2, e = table(cosine_truths, tc + to)
    del e["must_zero"]          # (the zeros of the cosine are not representable: no entry is an exact 0)
    out["common"]["d2"] = hexes(d2[:len(tc)])
    out["cosine"] = dict(t=hexes(to), d2=hexes(d2[len(tc):]), **e)
    for gamma in GAMMAS:
        to = gammaexp_offsets(gamma)
        d2, e = table(lambda v: gammaexp_truths(gamma, v), tc + to)
        out["gammaexp"][repr(gamma)] = dict(t=hexes(to), d2=hexes(d2[len(tc):]), **e)
    return out


def main():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kinds_truth.json")
    with open(path, "w") as f:
        json.dump(build(), f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
