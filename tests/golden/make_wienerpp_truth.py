"""Generate tests/golden/wienerpp_truth.json: 60-digit (mpmath) values of the Wiener and PiecewisePolynomial kinds of the product
path (include/sthenomi_kprod.h: SGP_WIENER, SGP_PIECEWISE0 .. 3) and of the derivatives the gradient contractions use.

    WIENER i        X = |x|, Y = |y|, m = min(X, Y), M = max(X, Y), d = |x - y|
                    i = 0  m      i = 1  m^3 / 3 + m^2 d / 2      i = 2  m^5 / 20 + m^3 d (X + Y - m / 2) / 12
                    i = 3  m^7 / 252 + m^4 d (5 M^2 + 2 X Y + 3 m^2) / 720
    PIECEWISE q, j  max(1 - r, 0)^(j + q) p_q(r),  r = d   (Rasmussen & Williams eq. 4.21; the coefficients of p_q below)
Per pair and parameter the table holds k, dg = d k(g x, g y) / dg at g = 1, dx = d k / d x and dy = d k / d y.

Conventions where a formula has no value (the library's rules, include/sthenomi_kprod.h):
    dX / dx = 0 at X = 0,  dd / dx = 0 at d = 0;  at a tie X == Y (every coincident pair included) dm and dM go half to each
    side, so that dx + dy of a coincident pair is the true d k(x, x) / dx;
    PIECEWISE is 0 with every derivative 0 for r >= 1; q = 0 has dx = 0 at r = 0 (the subgradient).

Two independent routes for WIENER: every pair goes through the closed form above, differentiated symbolically with respect
to X, Y and d.  At D = 1 on the half line (x, y >= 0) the truth of i >= 1 is formed WITHOUT the closed form, as the iterated
integral  k_i(s, t) = int_0^s int_0^t k_(i-1)(u, v) dv du,  k_0 = min, carried out exactly on polynomials with rational
coefficients (sympy) for s <= t and evaluated, with its partial derivatives, at the stored doubles; the generator asserts that
the two routes agree to 50 digits and stores the integral's.  PIECEWISE's derivative is k' = t^(n-1) (t p' - n p), n = j + q,
t = 1 - r, from the coefficients of p_q alone (not the factored form the library uses).

The truth is the function AT THE STORED DOUBLES.  Pairs, per dimension D in {1, 2, 3, 8, 16} (w: WIENER, p: PIECEWISE):
    equal (w p)      y == x bit for bit                     origin_x, origin_y, origin_both (w p)   the origin on either side
    near (w p)       |x - y| = 0.3, inside the support      tie (w)       X == Y exactly (integer coordinates), x != y
    nearnorm (w)     norms 1 and 1 + 1e-13                  opposite (w)  D = 1: x > 0 > y;  half (w)  D = 1: 0 < x < y
    huge (w)         norms 1e60 and 3e59: tabulated for every i whose values stay below 1e300 (i <= 2)
    huge3 (w)        norms 1e40 and 2e40 (m^7 = 1e280)      tiny (w)      norms 1e-30 and 2e-30
    r1 (p)           x = 0, y = e_1: r exactly 1            below1, below3, above1 (p)   y = e_1 (1 -+ ulps)
    far (p)          y = -x, r = 2                          overflow (p)  d^2 beyond the doubles
    tinyr (p)        r = 1e-9                               mid, mid9 (p) r = 0.5 and 0.9
PIECEWISE parameters: D = 1, 3: q in 0 .. 3, j in {1, floor(D / 2) + q + 1, 64}; D = 2, 8, 16: j = floor(D / 2) + q + 1 for
every q (D = 2: and (q, j) = (0, 1), (3, 64); D = 8, 16: origin_y and tinyr are left to the smaller dimensions), to keep the
file small.

    python tests/golden/make_wienerpp_truth.py      (a few seconds; needs mpmath and sympy)

Layout: {"digits", "pairs": [{"D", "cat", "x": [hex], "y": [hex], "wiener": {"i": {k, dg, dx, dy}}, "pp": {"q,j": {k, dg, dx,
dy}}, "integral": bool}]}, every number a hex double, correctly rounded.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_kprod_truth import signed_double  # noqa: E402

mp.mp.dps = 60
DIMS = (1, 2, 3, 8, 16)


def _norms(x, y):
    xs, ys = [mp.mpf(v) for v in x], [mp.mpf(v) for v in y]
    X = mp.sqrt(mp.fsum(p * p for p in xs))
    Y = mp.sqrt(mp.fsum(q * q for q in ys))
    d = mp.sqrt(mp.fsum((p - q) ** 2 for p, q in zip(xs, ys)))
    return xs, ys, X, Y, d


_sym = {}


def _wiener_sym(i):
    """the closed form and its partial derivatives as functions of (X, Y, d) for X <= Y (m = X, M = Y)"""
    if i not in _sym:
        import sympy as sp
        X, Y, d = sp.symbols("X Y d", positive=True)
        m, M = X, Y
        k = [m, m ** 3 / 3 + m ** 2 * d / 2, m ** 5 / 20 + m ** 3 * d * (X + Y - m / 2) / 12,
             m ** 7 / 252 + m ** 4 * d * (5 * M ** 2 + 2 * X * Y + 3 * m ** 2) / 720][i]
        _sym[i] = tuple(sp.lambdify((X, Y, d), e, "mpmath") for e in (k, sp.diff(k, X), sp.diff(k, Y), sp.diff(k, d)))
    return _sym[i]


def wiener_truths(i, x, y):
    xs, ys, X, Y, d = _norms(x, y)
    f = _wiener_sym(i)
    if X < Y:
        k, kX, kY, kd = (g(X, Y, d) for g in f)
    elif X > Y:
        k, kY, kX, kd = (g(Y, X, d) for g in f)
    else:       # a tie: the mean of the two one-sided derivatives
        k, a, b, kd = (g(X, Y, d) for g in f)
        kX = kY = (a + b) / 2
    c1 = kX / X if X > 0 else mp.mpf(0)
    c1y = kY / Y if Y > 0 else mp.mpf(0)
    c2 = kd / d if d > 0 else mp.mpf(0)
    dx = [c1 * p + c2 * (p - q) for p, q in zip(xs, ys)]
    dy = [c1y * q + c2 * (q - p) for p, q in zip(xs, ys)]
    return k, (2 * i + 1) * k, dx, dy


_int = {}


def _wiener_integral(i):
    """k_i(s, t) for s <= t as a sympy polynomial, by the iterated integral of k_(i-1)"""
    import sympy as sp
    s, t, u, v = sp.symbols("s t u v", positive=True)
    if i == 0:
        return s
    if i not in _int:
        A = _wiener_integral(i - 1)                 # k_(i-1)(first, second) for first <= second
        low = A.subs({s: v, t: u}, simultaneous=True)    # v <= u
        up = A.subs({s: u, t: v}, simultaneous=True)     # u <= v
        inner = sp.integrate(low, (v, 0, u)) + sp.integrate(up, (v, u, t))
        _int[i] = sp.expand(sp.integrate(inner, (u, 0, s)))
    return _int[i]


def wiener_integral_truths(i, x, y):
    """D = 1, x, y >= 0: k, dg, dx, dy from the iterated integral"""
    import sympy as sp
    s, t = sp.symbols("s t", positive=True)
    A = _wiener_integral(i)
    fs = [sp.lambdify((s, t), e, "mpmath") for e in (A, sp.diff(A, s), sp.diff(A, t))]
    xv, yv = mp.mpf(x[0]), mp.mpf(y[0])
    lo, hi = (xv, yv) if xv <= yv else (yv, xv)
    k, ds, dt = (mp.mpf(g(lo, hi)) for g in fs)
    if xv == yv:
        ds = dt = (ds + dt) / 2
    dx, dy = (ds, dt) if xv <= yv else (dt, ds)
    return k, xv * dx + yv * dy, [dx], [dy]


def pp_coeffs(q, j):
    """the coefficients of p_q, lowest power first"""
    j = mp.mpf(j)
    return [[mp.mpf(1)], [1, j + 1], [1, j + 2, (j * j + 4 * j + 3) / 3],
            [1, j + 3, (6 * j * j + 36 * j + 45) / 15, (j ** 3 + 9 * j * j + 23 * j + 15) / 15]][q]


def pp_truths(q, j, x, y):
    xs, ys, _, _, r = _norms(x, y)
    z = [mp.mpf(0)] * len(xs)
    if r >= 1:
        return mp.mpf(0), mp.mpf(0), z, z
    c, n, t = pp_coeffs(q, j), j + q, 1 - r
    p = mp.fsum(cv * r ** e for e, cv in enumerate(c))
    dp = mp.fsum(e * cv * r ** (e - 1) for e, cv in enumerate(c) if e >= 1)
    k = t ** n * p
    kr = t ** (n - 1) * (t * dp - n * p)         # k'(r)
    if r == 0:
        return k, mp.mpf(0), z, z
    dx = [kr * (a - b) / r for a, b in zip(xs, ys)]
    return k, r * kr, dx, [-v for v in dx]


def pp_params(D):
    jd = lambda q: D // 2 + q + 1      # noqa: E731
    if D in (1, 3):
        return sorted({(q, j) for q in range(4) for j in (1, jd(q), 64)})
    return sorted({(q, jd(q)) for q in range(4)} | ({(0, 1), (3, 64)} if D == 2 else set()))


def make_pairs(D):
    rng = np.random.RandomState(2100 + D)

    def vec(norm):
        v = rng.standard_normal(D)
        return v / np.sqrt(np.sum(v * v)) * norm

    e1, zero = np.eye(D)[0], np.zeros(D)
    out = []

    def add(cat, x, y, fams):
        out.append((cat, np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), fams))

    x = np.abs(vec(0.7)) if D == 1 else vec(0.7)
    add("equal", x, x.copy(), "wp")
    add("origin_x", zero, np.abs(vec(0.4)), "wp")
    add("origin_y", np.abs(vec(0.3)), zero, "wp" if D <= 3 else "w")
    if D <= 3:
        add("origin_both", zero, zero, "wp")
    x = vec(0.5)
    add("near", x, x + vec(0.3), "wp")
    # WIENER
    if D == 1:
        add("tie", [2.0], [-2.0], "w")
        add("opposite", [0.75], [-1.25], "w")
        add("half", [0.6], [1.7], "w")
        add("half", [2.5], [0.375], "w")
        add("nearnorm", [1.0], [1.0 + 1e-13], "w")
    else:
        t1, t2 = np.zeros(D), np.zeros(D)
        t1[:2], t2[0] = (3.0, 4.0), 5.0
        add("tie", t1, t2, "w")
        add("nearnorm", vec(1.0), vec(1.0 + 1e-13), "w")
    add("huge", np.abs(vec(1e60)), np.abs(vec(3e59)), "w")
    add("huge3", np.abs(vec(1e40)), np.abs(vec(2e40)), "w")
    add("tiny", np.abs(vec(1e-30)), np.abs(vec(2e-30)), "w")
    # PIECEWISE
    add("r1", zero, e1, "p")
    add("below1", zero, e1 * (1.0 - 2.0 ** -53), "p")
    if D <= 3:
        add("below3", zero, e1 * (1.0 - 3 * 2.0 ** -53), "p")
        add("above1", zero, e1 * (1.0 + 2.0 ** -52), "p")
        x = vec(1.0)
        add("far", x, -x, "p")
        add("overflow", 1e200 * e1, -1e200 * e1, "p")
        add("mid9", x, x + vec(0.9), "p")
    x = vec(0.5)
    if D <= 3:
        add("tinyr", x, x + vec(1e-9), "p")
    add("mid", x, x + vec(0.5), "p")
    return out


def _hex(v):
    return signed_double(mp.mpf(v)).hex()


def _entry(k, dg, dx, dy):
    return {"k": _hex(k), "dg": _hex(dg), "dx": [_hex(v) for v in dx], "dy": [_hex(v) for v in dy]}


def main():
    pairs = []
    for D in DIMS:
        for cat, x, y, fams in make_pairs(D):
            rec = {"D": D, "cat": cat, "x": [float(v).hex() for v in x], "y": [float(v).hex() for v in y]}
            if "w" in fams:
                half = D == 1 and x[0] >= 0.0 and y[0] >= 0.0
                rec["integral"] = bool(half)
                rec["wiener"] = {}
                for i in range(4):
                    tr = wiener_truths(i, x, y)
                    if half and i >= 1:
                        ti = wiener_integral_truths(i, x, y)
                        for a, b in zip([tr[0], tr[1], tr[2][0], tr[3][0]], [ti[0], ti[1], ti[2][0], ti[3][0]]):
                            assert abs(a - b) <= mp.mpf(10) ** -50 * max(abs(a), abs(b)), (i, x, y, a, b)
                        tr = ti
                    if max(abs(v) for v in [tr[0], tr[1]] + list(tr[2]) + list(tr[3])) > mp.mpf(10) ** 300:
                        continue
                    rec["wiener"][str(i)] = _entry(*tr)
            if "p" in fams:
                rec["pp"] = {f"{q},{j}": _entry(*pp_truths(q, j, x, y)) for q, j in pp_params(D)}
            pairs.append(rec)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wienerpp_truth.json")
    with open(path, "w") as fh:
        json.dump({"digits": mp.mp.dps, "pairs": pairs}, fh, separators=(",", ":"))
    print(path, len(pairs), "pairs", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
