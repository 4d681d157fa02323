"""NumPy (float64) formulas of the Wiener and PiecewisePolynomial kinds (csrc/kprod.hip: wiener_parts / wiener_derivs /
pp_derivs) in the library's own formulation and operation order, and the evaluators of tests/kprod_np.py and
tests/kprod_grad_np.py extended to them.  TEST INFRASTRUCTURE ONLY (tests/test_wienerpp_on_numpy.py holds the formulas to the
60-digit table; tests/test_gpu_wienerpp.py holds the library to them).

Both families travel the route of the kinds of x'y (tests/dotkinds_np.py): scalars a = x'x, b = y'y and d2 from direct
differences, point derivatives as coefficients, d k / d x = c1 x + c2 (x - y) + c3 y with c3 = 0 (PIECEWISE: c1 = 0,
c2 = 2 d k / d (d2)).

install(monkeypatch) installs dotkinds_np first and then makes its coefficient route know kinds 10 .. 14, so kprod_np.factor,
kprod_grad_np.np_input_grads / np_diag_grads and kinds_np.factor_abs_bound know kinds 10 .. 14 and 24 .. 26;
factor_abs_bound also gets the value bound of general-nu Matern (kind 20; matern_nu_np.install makes the evaluators know it)."""
import numpy as np

import dotkinds_np as dk
import kinds_np
from stheno_jl_amd import lib as L

PP_KINDS = (L.PIECEWISE0, L.PIECEWISE1, L.PIECEWISE2, L.PIECEWISE3)
WPP_KINDS = (L.WIENER,) + PP_KINDS


def is_wpp(kind):
    return (int(kind) & L.KIND_MASK) in WPP_KINDS


def _div0(num, den):
    """num / den, 0 where den == 0"""
    ok = den > 0.0
    return np.where(ok, num / np.where(ok, den, 1.0), 0.0)


def wiener(i, a, b, d2):
    """dict(k, dk, dp, c1, c1y, c2, c3) from a (n x 1), b (1 x m), d2 (n x m)"""
    with np.errstate(over="ignore", invalid="ignore"):
        X, Y, d = np.sqrt(a) + 0.0 * b, np.sqrt(b) + 0.0 * a, np.sqrt(d2)
        m, M = np.minimum(X, Y), np.maximum(X, Y)
        m2 = m * m
        z = np.zeros_like(d)
        km, kM, kS, kP, kd = z, z, z, z, z
        if i == 0:
            k, km = m, z + 1.0
        elif i == 1:
            k = m2 * m / 3.0 + m2 * d * 0.5
            km, kd = m2 + m * d, 0.5 * m2
        elif i == 2:
            m3, S = m2 * m, X + Y
            T = S - 0.5 * m
            k = m3 * m2 / 20.0 + m3 * d * T / 12.0
            km = m2 * m2 / 4.0 + m2 * d * (3.0 * S - 2.0 * m) / 12.0
            kS, kd = m3 * d / 12.0, m3 * T / 12.0
        else:
            m3, m4 = m2 * m, m2 * m2
            Q = (5.0 * (M * M) + 2.0 * (X * Y)) + 3.0 * m2
            k = m4 * m3 / 252.0 + m4 * d * Q / 720.0
            km = (m4 * m2 / 36.0 + m3 * d * Q / 180.0) + m4 * m * d / 120.0
            kM, kP, kd = m4 * d * M / 72.0, m4 * d / 360.0, m4 * Q / 720.0
        wx = np.where(X < Y, 1.0, np.where(X > Y, 0.0, 0.5))
        wy = 1.0 - wx
        kX = ((wx * km + wy * kM) + kS) + kP * Y
        kY = ((wy * km + wx * kM) + kS) + kP * X
        return dict(k=k, dk=(2.0 * i + 1.0) * k, dp=z, c1=_div0(kX, X), c1y=_div0(kY, Y), c2=_div0(kd, d), c3=z)


def _pp_pow(t, e):
    pw = np.ones_like(t)
    while e > 0:
        if e & 1:
            pw = pw * t
        t = t * t
        e >>= 1
    return pw


def piecewise(q, j, d2):
    """dict(k, dk, kx) from d2, the library's square-and-multiply and polynomial forms"""
    j = float(j)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.sqrt(d2)
        inside = r < 1.0
        rr = np.where(inside, r, 0.5)
        t = 1.0 - rr
        pw = _pp_pow(t, int(j) + q - 1)
        p, pt = np.ones_like(rr), np.zeros_like(rr)
        if q == 1:
            p, pt = 1.0 + (j + 1.0) * rr, (j + 1.0) * (j + 2.0) + 0.0 * rr
        elif q == 2:
            p = 1.0 + rr * ((j + 2.0) + ((j + 1.0) * (j + 3.0) / 3.0) * rr)
            pt = ((j + 3.0) * (j + 4.0) / 3.0) * (1.0 + (j + 1.0) * rr)
        elif q == 3:
            n, n2, n3 = j + 3.0, 6.0 * j * j + 36.0 * j + 45.0, (j + 1.0) * (j + 3.0) * (j + 5.0)
            p = 1.0 + rr * (n + rr * (n2 / 15.0 + (n3 / 15.0) * rr))
            a0, a1, a2 = (15.0 * (n * n + n) - 2.0 * n2) / 15.0, ((n + 2.0) * n2 - 3.0 * n3) / 15.0, (n + 3.0) * n3 / 15.0
            pt = a0 + rr * (a1 + a2 * rr)
        k = (pw * t) * p
        kx = _div0(-(j * pw), 2.0 * rr) if q == 0 else -0.5 * (pw * pt)
        k, kx = np.where(inside, k, 0.0), np.where(inside, kx, 0.0)
        dk = np.where(inside, 2.0 * np.where(inside, d2, 0.0) * kx, 0.0)
    return dict(k=k, dk=dk, kx=kx)


def derivs(kind, Xr, Xc, param):
    code = int(kind) & L.KIND_MASK
    _, a, b, d2, _ = dk.scalars(Xr, Xc)
    if code == L.WIENER:
        return wiener(int(param), a, b, d2)
    r = piecewise(code - L.PIECEWISE0, param, d2)
    z = np.zeros_like(d2)
    return dict(k=r["k"], dk=r["dk"], dp=z, c1=z, c1y=z, c2=2.0 * r["kx"], c3=z)


def extended_derivs(before):
    def _derivs(kind, Xr, Xc, param):
        return derivs(kind, Xr, Xc, param) if is_wpp(kind) else before(kind, Xr, Xc, param)
    return _derivs


def extended_abs_bound(before):
    def factor_abs_bound(kind, Xr, Xc, param):
        """kinds_np.factor_abs_bound with the five kinds: (|k|, e), e the value bound of tests/wienerpp_truth.py per entry"""
        code = int(kind) & L.KIND_MASK
        if code == L.MATERN_NU:
            # chains here mix the kinds with general-nu Matern, which kinds_np has no bound for: its model
            # (tests/matern_nu_truth.py: (128 + 4 x + 3 n) eps relative, x = sqrt(2 nu) d) plus what the (D + 2) eps of d2 do
            # through |d k / d (d2)| d2 = |d k / d g| / 2
            import kprod_np as kn
            import matern_nu_truth as mt
            Xr, Xc = np.asarray(Xr, dtype=np.float64), np.asarray(Xc, dtype=np.float64)
            k, dg, _ = kn.factor(kind, Xr, Xc, param)
            x = np.sqrt(2.0 * param * dk.scalars(Xr, Xc)[3])
            return np.abs(k), mt.bound_units(param, x) * mt.EPS * np.abs(k) + 0.5 * (Xr.shape[0] + 2) * mt.EPS * np.abs(dg)
        if not is_wpp(kind):
            return before(kind, Xr, Xc, param)
        import wienerpp_truth as wt
        Xr, Xc = np.asarray(Xr, dtype=np.float64), np.asarray(Xc, dtype=np.float64)
        D = Xr.shape[0]
        k = np.abs(derivs(kind, Xr, Xc, param)["k"])
        if code == L.WIENER:
            return k, wt.wiener_rel(int(param), D) * k
        _, _, _, d2, _ = dk.scalars(Xr, Xc)
        return k, wt.pp_value_bound(code - L.PIECEWISE0, int(param), D, np.sqrt(d2), k)
    return factor_abs_bound


def install(monkeypatch):
    """teach the evaluators kinds 10 .. 14 (and, through dotkinds_np, 24 .. 26) for the duration of a test"""
    dk.install(monkeypatch)
    monkeypatch.setattr(dk, "DOT_KINDS", tuple(dk.DOT_KINDS) + WPP_KINDS)
    monkeypatch.setattr(dk, "derivs", extended_derivs(dk.derivs))
    monkeypatch.setattr(kinds_np, "factor_abs_bound", extended_abs_bound(kinds_np.factor_abs_bound))
