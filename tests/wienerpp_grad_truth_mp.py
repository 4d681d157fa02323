"""The pin problem of tests/wienerpp_grad_truth.py and its values at 40 digits (mpmath), written independently of that module.
TEST INFRASTRUCTURE ONLY.  The layout is tests/kprod_grad_truth_mp.py's (KM: N = 24, D = 3, M = 6, views 0 the points, 1 the
points x 0.7, 2 their first coordinate x 0.5, a function-scaled first head, logpdf, the ELBO in the dense Titsias form, the
diagonal on one view and on two); `long_double_run` and `pin_values` are KM's own code run on this module's problem, truth and
entry-by-entry spec.  What is written here:
  * the chains: one per kind pair, every WIENER i and PIECEWISE q, each beside a kind of kprod_grad_truth;
    the first coordinate is non-negative, so that the WIENER factors (view 2) sit on the half line and K is positive definite;
  * the two families in mpmath from the header's formulas (include/sthenomi_kprod.h), derivatives by mpmath.diff of polynomials:
    WIENER as k_A(X, Y, d), the header's expression with m := X, M := Y (valid for X <= Y), and k_B(X, Y, d) = k_A(Y, X, d);
    d k / d X = wx dk_A / dX + wy dk_B / dX with wx = 1, 0, 1/2 for X <, >, == Y (the one-sided derivatives, half of each at a
    tie), d k / d d from the branch in force (both agree at a tie); c1 = kX / X, c1y = kY / Y, c2 = kd / d, each 0 where its
    denominator is.  PIECEWISE as K(r) = (1 - r)^(j+q) p_q(r) for r < 1: kx = K'(r) / (2 r), at r = 0 its limit K''(0) / 2
    (q >= 1) or 0 (q = 0); zeros for r >= 1;
  * the contraction of a cotangent entry by entry with the coefficient form of the point derivatives."""
import types

import numpy as np

import kprod_grad_truth as KT
import kprod_grad_truth_mp as KM
import wienerpp_grad_truth as WG
from kprod_grad_truth_mp import DIGITS, M, N, NOISE, Z_NOISE  # noqa: F401

W, P0 = WG.WIENER, WG.PIECEWISE0


def _chains(row0, col0, rs, cs):
    r, c = (lambda v: row0 + v), (lambda v: col0 + v)
    spec = [(0.5, rs, cs, [(W, 2, 1.0), (KT.SE, 0, 0.0)]),
            (0.4, None, None, [(P0 + 1, 1, 2.0), (KT.RQ, 0, 0.9), (KT.LINEAR, 1, 0.4)]),
            (0.6, None, None, [(W, 2, 0.0), (P0, 1, 2.0)]),
            (0.8, None, None, [(W, 2, 2.0), (KT.MATERN32, 1, 0.0)]),
            (0.3, None, None, [(P0 + 2, 1, 4.0), (KT.GAMMAEXP, 1, 1.3)]),
            (0.9, None, None, [(W, 2, 3.0), (P0 + 3, 1, 5.0), (KT.MATERN_NU, 0, 1.25)]),
            (0.2, None, None, [(P0 + 2, 0, 3.0)])]
    chains, t = [], 0
    for coef, a, b, fac in spec:
        chains.append(dict(I=0, J=0, head=t, coef=coef, rs=a, cs=b,
                           factors=[(t + i, kind, r(v), c(v), param) for i, (kind, v, param) in enumerate(fac)]))
        t += len(fac)
    return chains


def pin_problem():
    rng = np.random.default_rng(81)
    X, Z = (rng.standard_normal((KM.D, k)) / np.sqrt(KM.D) * 1.5 for k in (N, M))
    X[0], Z[0] = np.abs(X[0]), np.abs(Z[0])
    X[:, 5], X[:, 11] = X[:, 3], 0.0          # a duplicate (ties, d == 0 off the diagonal) and the origin
    y, mean = rng.standard_normal(N), 0.1 * rng.standard_normal(N)
    sx, sz = 1.0 + 0.3 * np.sin(X.sum(0)), 1.0 + 0.3 * np.sin(Z.sum(0))
    w = rng.standard_normal(N)
    v = KM._views
    xx = KT.hand_spec(_chains(0, 0, sx, sx), v(X), [N], [N], True)
    zz = KT.hand_spec(_chains(0, 0, sz, sz), v(Z), [M], [M], True)
    xz = KT.hand_spec(_chains(0, 3, sx, sz), v(X) + v(Z), [N], [M], False)
    dg = KT.hand_spec(_chains(0, 3, sx, sx), v(X) + v(1.2 * X), [N], [N], True)
    return dict(xx=xx, zz=zz, xz=xz, dg=dg, y=y, mean=mean, w=w)


# ---- the two families in mpmath ----------------------------------------------------------------------------------------------------
def _wiener_a(mp, i, X, Y, d):
    """the header's expression with m := X, M := Y"""
    return (X, X ** 3 / 3 + X * X * d / 2, X ** 5 / 20 + X ** 3 * d * (X + Y - X / 2) / 12,
            X ** 7 / 252 + X ** 4 * d * (5 * Y * Y + 2 * X * Y + 3 * X * X) / 720)[i]


def _mp_factor(mp, kind, param, xr, xc):
    """KM._mp_factor's four numbers; for the coefficient kinds (kp None) followed by c1, c1y, c2, c3"""
    zero = mp.mpf(0)
    if kind not in WG.WPP:
        return KM._mp_factor(mp, kind, param, xr, xc)
    d = mp.sqrt(sum((u - v) ** 2 for u, v in zip(xr, xc)))
    if kind == W:
        i = int(param)
        X, Y = mp.sqrt(sum(v * v for v in xr)), mp.sqrt(sum(v * v for v in xc))
        kA = lambda X_, Y_, d_: _wiener_a(mp, i, X_, Y_, d_)                   # noqa: E731
        kB = lambda X_, Y_, d_: _wiener_a(mp, i, Y_, X_, d_)                   # noqa: E731
        wx = mp.mpf(1) if X < Y else (zero if X > Y else mp.mpf(1) / 2)
        wy = 1 - wx
        kX = wx * mp.diff(lambda t: kA(t, Y, d), X) + wy * mp.diff(lambda t: kB(t, Y, d), X)
        kY = wx * mp.diff(lambda t: kA(X, t, d), Y) + wy * mp.diff(lambda t: kB(X, t, d), Y)
        kd = mp.diff(lambda t: (kA if X <= Y else kB)(X, Y, t), d)
        k = (kA if X <= Y else kB)(X, Y, d)
        return (k, None, (2 * i + 1) * k, zero, kX / X if X > 0 else zero, kY / Y if Y > 0 else zero, kd / d if d > 0 else zero, zero)
    q, j = kind - P0, int(param)
    if d >= 1:
        return zero, None, zero, zero, zero, zero, zero, zero
    p = lambda r: (1, 1 + (j + 1) * r, 1 + (j + 2) * r + mp.mpf(j * j + 4 * j + 3) / 3 * r * r,        # noqa: E731
                   1 + (j + 3) * r + mp.mpf(6 * j * j + 36 * j + 45) / 15 * r * r
                   + mp.mpf(j ** 3 + 9 * j * j + 23 * j + 15) / 15 * r ** 3)[q]
    K = lambda r: (1 - r) ** (j + q) * p(r)                                    # noqa: E731
    if d > 0:
        kx = mp.diff(K, d) / (2 * d)
    else:
        kx = mp.diff(K, d, 2) / 2 if q >= 1 else zero
    return K(d), None, 2 * d * d * kx, zero, zero, zero, 2 * kx, zero


class _MpSpec(KM._MpSpec):
    def __init__(self, mp, S, diag=False):
        self.mp, self.S, self.diag = mp, S, diag
        self.X = [[[mp.mpf(float(a[d, i])) for d in range(a.shape[0])] for i in range(a.shape[1])] for a in S["inputs"]]
        self.nr, self.nc = S["row_len"][0], S["col_len"][0]
        self.F = [[[[(_mp_factor(mp, kind, param, self.X[ri][i], self.X[ci][j]) if (not diag or i == j) else None)
                     for j in range(self.nc)] for i in range(self.nr)] for (_, kind, ri, ci, param) in ch["factors"]]
                  for ch in S["chains"]]

    def contract(self, G, out, prefix, scales):
        """KM._MpSpec.contract with the coefficient form: the row point gets c1 x + c2 (x - y) + c3 y, the column point
        c1y y + c2 (y - x) + c3 x (a symmetric spec takes the row side twice; the diagonal gives each side its own)"""
        mp, S = self.mp, self.S
        sym = S["symmetric"] and not self.diag
        side = 2 if sym else 1
        nt = S["n_terms"]
        dc, ds, dp = [mp.mpf(0)] * nt, [mp.mpf(0)] * nt, [mp.mpf(0)] * nt
        gx = [[[mp.mpf(0)] * len(pts) for _ in range(len(pts[0]))] for pts in self.X]
        pairs = [(i, i) for i in range(self.nr)] if self.diag else [(i, j) for i in range(self.nr) for j in range(self.nc)]
        rsum, csum = [mp.mpf(0)] * self.nr, [mp.mpf(0)] * self.nc
        for c, ch in enumerate(S["chains"]):
            for (i, j) in pairs:
                coef, r, s = self.weights(c, i, j)
                g = G(i, j)
                full = self.prod(c, i, j)
                dc[ch["head"]] += g * r * s * full
                if c == 0:
                    rsum[i] += side * g * coef * s * full
                    csum[j] += g * coef * r * full
                for f, (t, kind, ri, ci, param) in enumerate(ch["factors"]):
                    e = self.F[c][f][i][j]
                    A = g * coef * r * s * self.prod(c, i, j, skip=f)
                    ds[t] += A * e[2]
                    dp[t] += A * e[3]
                    xr, xc = self.X[ri][i], self.X[ci][j]
                    for d in range(len(xr)):
                        if len(e) == 8:
                            row = e[4] * xr[d] + e[6] * (xr[d] - xc[d]) + e[7] * xc[d]
                            col = e[5] * xc[d] + e[6] * (xc[d] - xr[d]) + e[7] * xr[d]
                        elif kind == KT.LINEAR:
                            row, col = xc[d], xr[d]
                        else:
                            row = 2 * e[1] * (xr[d] - xc[d])
                            col = -row
                        gx[ri][d][i] += side * A * row
                        if not sym:
                            gx[ci][d][j] += A * col
        out[prefix + ".d_coef"], out[prefix + ".d_inscale"], out[prefix + ".d_param"] = dc, ds, dp
        for k, g in enumerate(gx):
            out[f"{prefix}.inputs.{k}"] = [v for row in g for v in row]
        if "rowscale" in scales:
            out[prefix + ".rowscale"] = rsum
        if "colscale" in scales:
            out[prefix + ".colscale"] = csum


# KM's own drivers on this module's problem: `KT` inside them is kprod_grad_truth with the three entry points of
# wienerpp_grad_truth in place of its own
_TRUTH = types.SimpleNamespace(**dict(vars(KT), logpdf_grad=WG.logpdf_grad, elbo_grad=WG.elbo_grad, diag_grad=WG.diag_grad))
long_double_run = WG.rebind(KM.long_double_run, KM, KT=_TRUTH, pin_problem=pin_problem)
pin_values = WG.rebind(KM.pin_values, KM, _MpSpec=_MpSpec, pin_problem=pin_problem)
