"""Generate tests/golden/kernel_truth.json: 60-digit (mpmath) values of the four stationary kernels
    SE exp(-d2 / 2),  Matern-1/2 exp(-d),  Matern-3/2 (1 + l) exp(-l), l = sqrt(3) d,  Matern-5/2 (1 + l + l^2 / 3) exp(-l), l = sqrt(5) d
on a grid of offsets t that visits the places where hand-written exp / sqrt go wrong.  With one point at 0 and the other
at t, the device's squared distance is the single product fl(t * t), which is stored: the table's d2 is bit for bit the
argument the kernel formulas see, and the truth is the kernel AT THAT DOUBLE.

    python tests/golden/make_kernel_truth.py      (a few seconds; needs mpmath)

File layout (hex floats, so nothing depends on decimal parsing or an RNG implementation):
    common: {t, d2}                        offsets shared by all kernels
    kernels[name]: {k, k_dec, k32}         truths at the common offsets followed by those at the kernel's own offsets
                   {t, d2}                 the kernel's own offsets (chosen by the argument of its exp)
k = the truth rounded to the nearest double (subnormals included), k_dec = its first 25 digits, k32 = the truth at the
offset rounded to float32 (clipped to the largest finite float32), rounded to double, for the fp32 assembly.
"""
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
KERNELS = ("se", "matern12", "matern32", "matern52")
F32_MAX = float(np.finfo(np.float32).max)


def kappa(name, d2):
    """the kernel at squared distance d2 (mpf, or +inf)"""
    if d2 == mp.inf:
        return mp.mpf(0)
    d = mp.sqrt(d2)
    if name == "se":
        return mp.exp(-d2 / 2)
    if name == "matern12":
        return mp.exp(-d)
    if name == "matern32":
        l = mp.sqrt(3) * d
        return (1 + l) * mp.exp(-l)
    l = mp.sqrt(5) * d
    return (1 + l + l * l / 3) * mp.exp(-l)


def to_double(v):
    """mpf >= 0 -> the nearest double, subnormals included (ties cannot occur at 60 digits for these values)"""
    if v == 0:
        return 0.0
    e = int(mp.floor(mp.log(v, 2)))
    q = max(e - 52, -1074)
    n = int(mp.nint(mp.ldexp(v, -q)))
    return float(np.ldexp(float(n), q))          # n < 2^53 + 1: exact


def offset_for_exp_arg(name, a):
    """the offset t at which the kernel's exp is evaluated at -a (a > 0), in 60 digits"""
    a = mp.mpf(a)
    if name == "se":
        return mp.sqrt(2 * a)
    return a / mp.sqrt({"matern12": 1, "matern32": 3, "matern52": 5}[name])


def common_offsets():
    """offsets whose squared distance is what matters: the same for every kernel"""
    tiny = 5e-324
    d2s = [0.0, tiny, 2 * tiny, np.nextafter(1e-300, 0), 1e-300, np.nextafter(1e-300, 1), 1e-200, 1e-100]
    ts = [0.0] + [float(np.sqrt(v)) for v in d2s[1:]]
    ts += [float(np.nextafter(1e-150, 0)), float(np.nextafter(1e-150, 1))]      # d2 two ulps either side of the 1e-300 clamp
    for c in (1e-16, 2.0 ** -26):                # d2 = 1e-32 and 2^-52 with their neighbours
        ts += [float(np.nextafter(c, 0)), c, float(np.nextafter(c, 1))]
    rng = np.random.default_rng(20240917)
    e = np.linspace(-30.0, 10.0, 200)            # d2 over 2^-60 .. 2^20
    ts += [float(np.ldexp(1.0 + rng.random(), int(np.floor(v)))) for v in e]
    tmax = float(np.sqrt(np.finfo(np.float64).max))
    while np.isinf(np.float64(tmax) * np.float64(tmax)):
        tmax = float(np.nextafter(tmax, 0))
    ts += [1e150, tmax, 1.5e154]                 # d2 = 1e300, the largest finite square (DBL_MAX to an ulp), +inf
    return ts


def own_offsets(name):
    """offsets chosen by the argument -a of the kernel's exp"""
    rng = np.random.default_rng(7 + KERNELS.index(name))
    ln2 = mp.log(2)
    ts = []
    for n in (1, 10, 100, 1000):                 # a log2(e) on both sides of n + 1/2, where the reduction's n flips
        t0 = float(offset_for_exp_arg(name, (n + mp.mpf(1) / 2) * ln2))
        ts += [t0 * (1 - 1e-6), float(np.nextafter(t0, 0)), t0, float(np.nextafter(t0, np.inf)), t0 * (1 + 1e-6)]
    # the RESULT is subnormal for exp arguments -705 .. -746, moved out by the log of the polynomial factor there
    shift = {"se": 0.0, "matern12": 0.0, "matern32": float(np.log(726.0)), "matern52": float(np.log(726.0 + 725.0 ** 2 / 3))}[name]
    for a in np.sort(rng.uniform(705.0, 746.0, 34)):      # (rounds to 0 at the very end)
        ts.append(float(offset_for_exp_arg(name, a + shift)))
    for a in (745.0 + shift, 745.13 + shift, 745.14 + shift, 746.5 + shift, 775.0, 790.0, 799.999):
        ts.append(float(offset_for_exp_arg(name, a)))
    t800 = float(offset_for_exp_arg(name, 800))
    ts += [float(np.nextafter(t800, 0)), t800, float(np.nextafter(t800, np.inf))]
    ts += [float(offset_for_exp_arg(name, 1e4)), float(offset_for_exp_arg(name, 1e10))]
    return ts


def hexes(vals):
    return [float(v).hex() for v in vals]


def truths(name, ts):
    with np.errstate(over="ignore"):
        d2 = [float(np.float64(t) * np.float64(t)) for t in ts]
        t32 = [min(float(np.float32(t)), F32_MAX) for t in ts]
    kv = [kappa(name, mp.inf if v == np.inf else mp.mpf(v)) for v in d2]
    k32 = [kappa(name, mp.mpf(t) ** 2) for t in t32]
    return d2, [to_double(v) for v in kv], [mp.nstr(v, 25) for v in kv], [to_double(v) for v in k32]


def build():
    tc = common_offsets()
    out = {"digits": 60, "common": {"t": hexes(tc)}, "kernels": {}}
    for name in KERNELS:
        to = own_offsets(name)
        d2, k, kd, k32 = truths(name, tc + to)
        out["common"]["d2"] = hexes(d2[:len(tc)])
        out["kernels"][name] = {"t": hexes(to), "d2": hexes(d2[len(tc):]), "k": hexes(k), "k_dec": kd, "k32": hexes(k32)}
    return out


def main():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_truth.json")
    with open(path, "w") as f:
        json.dump(build(), f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
