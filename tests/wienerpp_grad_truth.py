"""Extended-precision truth for the gradients through chains that hold the Wiener and PiecewisePolynomial kinds
(include/sthenomi_kprod.h: codes 10 .. 14; the mode-3 instantiations of csrc/kprod.hip).  TEST INFRASTRUCTURE ONLY.

A dtype-generic restatement of the five kinds on top of tests/dotkinds_grad_truth.py (imported as DG, not edited; it stands on
kprod_grad_truth, KT, and grad_truth, T, the same way): every other kind, the chain product, the factorisation, the ELBO's
cotangents and the units are theirs.  Written here, straight from the header's definitions in the working dtype:
    WIENER i     X = |x|, Y = |y|, d = |x - y| from direct differences, m = min, M = max.  X + Y = m + M and X Y = m M, so k
                 is stated in (m, M, d) alone:  m;  m^3 / 3 + m^2 d / 2;  m^5 / 20 + m^3 d (M + m / 2) / 12;
                 m^7 / 252 + m^4 d Q / 720, Q = 5 M^2 + 2 m M + 3 m^2, and km, kM, kd are its partial derivatives.
                 kX = wx km + wy kM, kY = wy km + wx kM, wx = 1, 0, 1/2 for X <, >, == Y, wy = 1 - wx;
                 c1 = kX / X (0 at X == 0), c1y = kY / Y (0 at Y == 0), c2 = kd / d (0 at d == 0), c3 = 0;
                 dk = (2 i + 1) k, dp = 0.
    PIECEWISE q  r = d, t = max(1 - r, 0), n = j + q, k = t^n p_q(r), p_q = sum_k a_k r^k the header's polynomial.
                 k' = -t^(n-1) (n p - (1 - r) p'), whose bracket has no constant term (a_1 = n), so
                 kx = d k / d (d^2) = k' / (2 r) = -t^(n-1) g(r) / 2,  g = sum_(k >= 1) ((n + k) a_k - (k + 1) a_(k+1)) r^(k-1)
                 -- a power times a polynomial; q = 0: kx = -j t^(j-1) / (2 r), 0 at r == 0.  The power is a plain repeated
                 product (t^0 = 1).  c2 = 2 kx, c1 = c1y = c3 = 0, dk = 2 d^2 kx, dp = 0; exact zeros for r >= 1.
`dense`, `diag_of` and `contract` are DG's, run with this module's `factor` and with kinds 10 .. 14 on DG's coefficient route
(d k / d x = c1 x + c2 (x - y) + c3 y; the column point's: c1y y + c2 (y - x) + c3 x).  Run in np.longdouble it is the truth,
twice in np.float64 (the column recurrence and LAPACK's blocked order) the yardstick.  tests/test_wienerpp_grad_truth_on_numpy.py
holds the long-double `factor` to the committed 60-digit table (tests/golden/wienerpp_truth.json), pair by pair.

The cases (CASES): data blocks (129, 1, 70), N = 200, two single blocks of 257; ELBO: inducing blocks (33, 1), Sigma_z = 1e-2
(scalar, once dense); noise 0.05 .. 0.3, scalar and diagonal; every case asks for inputs and scales.  Points are
standard_normal / sqrt(D) * 1.5 with coordinate 0 made non-negative (a WIENER factor reads it through SelectTransform([0]):
the half line, where i >= 1 is positive definite); the first block holds an exact duplicate (columns 3 and 5) and a point at
the origin (column 11), the last block ends with a copy of column 7 of the first.  `wp-wfull-D3` is the one case whose WIENER
factor reads the whole point (norms from kp_dot_scalars): the issue's coefficient 0.2 beside a unit SE term leaves K + Sigma_y
indefinite in the long-double run, and so does 0.1; WFULL_COEF = 0.05 (halved twice) is what the case uses.
Seeds are 9100 + the case's position.  All of them meet the conditions the CPU file asserts on the inputs (|r - 1| > 1e-12,
20 % .. 80 % of the pairs beyond each PIECEWISE support, equal float64 norms only between identical points, the conditioning
caps).  Three were moved by 100 for another reason: SEED_BUMP below.

The device's kp.* / kpelbo.* families are held to MARGIN * max(e_float64 of the case, the family's floor)
(tests/test_gpu_wienerpp_grad_truth.py), MARGIN from tests/grad_truth.py.  FLOORS: the medians of this reference's own float64
figures over CASES, printed by `python tests/wienerpp_grad_truth.py` and written down below.  Nothing is taken from a device.

The diagonal (DIAG_CASES, `diag_grad`) involves no factorisation; its bound is kprod_grad_truth's model,
    |device - truth| <= (D + 8 + sum_f amp_f) eps Sm,
with, for the kinds written here (every other kind: KT's amp and magnitudes),
    WIENER i     amp = (2 i + 2) (D / 2 + 2) + 28 = wienerpp_truth.wiener_rel(i, D) / eps + 12, the table's bound of the point
                 derivatives (the roundings of the norms and of d are inside it); Sm takes |c1 x| + |c2 (x - y)| part by part
    PIECEWISE q  amp = the largest of pp_value_bound / |k| and pp_kx_bound / |kx| over the case's entries inside the
                 support, in eps, plus 8 for the products that follow (the bounds are absolute and carry the rounding of r)."""
import os
import sys
import types

import numpy as np

import dotkinds_grad_truth as DG
import grad_truth as T
import kprod_grad_truth as KT
from kprod_grad_truth import EPS, MARGIN, NOISE_DENSE, NOISE_DIAG, NOISE_SCALAR  # noqa: F401

WIENER, PIECEWISE0 = 10, 11
PP = (11, 12, 13, 14)
WPP = (WIENER,) + PP
COEF_KINDS = DG.DOT + WPP            # the kinds whose point derivatives come as (c1, c1y, c2, c3)


def pp_coefficients(q, j, dt):
    """a_0 .. a_q of p_q (the header's polynomials), in dtype dt"""
    j = dt(j)
    a = [dt(1)]
    if q == 1:
        a += [j + dt(1)]
    elif q == 2:
        a += [j + dt(2), (j * j + dt(4) * j + dt(3)) / dt(3)]
    elif q == 3:
        a += [j + dt(3), (dt(6) * j * j + dt(36) * j + dt(45)) / dt(15), (j * j * j + dt(9) * j * j + dt(23) * j + dt(15)) / dt(15)]
    return a


def _horner(c, r):
    p = np.zeros_like(r)
    for v in reversed(c):
        p = p * r + v
    return p


def _quot(num, den, dt):
    """num / den, 0 where den == 0"""
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, dt(1)), dt(0))


def factor(kind, X, Y, param, dt, diag=False):
    """DG.factor with kinds 10 .. 14: dict(k, kp=None, dk, dp, c1, c1y, c2, c3)"""
    if kind not in WPP:
        return DG.factor(kind, X, Y, param, dt, diag)
    x, y = DG._outer(X, Y, diag)
    zero, one, two, half = dt(0), dt(1), dt(2), dt(1) / dt(2)
    d2 = ((x - y) ** 2).sum(0)
    z = zero * d2
    if kind == WIENER:
        i = int(param)
        assert i == param and 0 <= i <= 3
        Xn, Yn, d = np.sqrt((x * x).sum(0)) + z, np.sqrt((y * y).sum(0)) + z, np.sqrt(d2)
        m, M = np.minimum(Xn, Yn), np.maximum(Xn, Yn)
        kM = z
        if i == 0:
            k, km, kd = m, z + one, z
        elif i == 1:
            k = m ** 3 / dt(3) + m * m * d / two
            km, kd = m * m + m * d, m * m / two
        elif i == 2:
            U = M + m / two
            k = m ** 5 / dt(20) + m ** 3 * d * U / dt(12)
            km = m ** 4 / dt(4) + m * m * d * (dt(3) * M + two * m) / dt(12)
            kM, kd = m ** 3 * d / dt(12), m ** 3 * U / dt(12)
        else:
            Q = dt(5) * M * M + two * m * M + dt(3) * m * m
            k = m ** 7 / dt(252) + m ** 4 * d * Q / dt(720)
            km = m ** 6 / dt(36) + (dt(4) * m ** 3 * d * Q + m ** 4 * d * (two * M + dt(6) * m)) / dt(720)
            kM, kd = m ** 4 * d * (dt(10) * M + two * m) / dt(720), m ** 4 * Q / dt(720)
        wx = np.where(Xn < Yn, one, np.where(Xn > Yn, zero, half))
        wy = one - wx
        return dict(k=k, kp=None, dk=dt(2 * i + 1) * k, dp=z, c1=_quot(wx * km + wy * kM, Xn, dt),
                    c1y=_quot(wy * km + wx * kM, Yn, dt), c2=_quot(kd, d, dt), c3=z)
    q, j = kind - PIECEWISE0, int(param)
    assert j == param and j >= 1
    n = j + q
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.sqrt(d2)
        inside = r < one
    rr = np.where(inside, r, half)
    t = one - rr
    pw = z + one                       # t^(n-1)
    for _ in range(n - 1):
        pw = pw * t
    a = pp_coefficients(q, j, dt)
    if q == 0:
        kx = -_quot(dt(j) * pw, two * rr, dt)
    else:
        g = [dt(n + k) * a[k] - (dt(k + 1) * a[k + 1] if k + 1 <= q else zero) for k in range(1, q + 1)]
        kx = -(pw * _horner(g, rr)) / two
    k, kx = np.where(inside, pw * t * _horner(a, rr), zero), np.where(inside, kx, zero)
    return dict(k=k, kp=None, dk=two * np.where(inside, d2, zero) * kx, dp=z, c1=z, c1y=z, c2=two * kx, c3=z)


def rebind(fn, module, **names):
    """fn of `module` run with `names` in place of the module globals of those names.  It overrides only what fn itself looks
    up: a helper of `module` that fn calls keeps the module's own globals"""
    return types.FunctionType(fn.__code__, dict(vars(module), **names), fn.__name__, fn.__defaults__)


def _over(fn):
    """fn of dotkinds_grad_truth run with this module's `factor` and with kinds 10 .. 14 on its coefficient route.  This relies
    on DG's dense, diag_of and contract calling `factor` and testing `kind in DOT` themselves, not through a helper of DG;
    tests/test_wienerpp_grad_truth_on_numpy.py asserts that a kind-10 factor reaches this module's `factor` through all three"""
    return rebind(fn, DG, factor=factor, DOT=COEF_KINDS)


dense, diag_of, contract = _over(DG.dense), _over(DG.diag_of), _over(DG.contract)


class _Ops:
    dense, diag_of = staticmethod(dense), staticmethod(diag_of)

    @staticmethod
    def contract(S, G, dt, inputs=False, scales=True):
        return contract(S, G, dt, inputs=inputs, scales=scales)


def logpdf_grad(S, noise_kind, noise, mean, y, dt, inputs=False, scales=False, cholesky=None):
    return T.logpdf_grad(S, noise_kind, noise, mean, y, dt, inputs=inputs, scales=scales, cholesky=cholesky, ops=_Ops)


def elbo_grad(Szz, Sxz, Sxx, noise_kind, noise, z_noise_kind, z_noise, mean, y, dt, inputs=False, cholesky=None):
    """sgp_elbo_grad_param's zz and xz sides (the diagonal is held by DIAG_CASES with the caller's w)"""
    return T.elbo_grad(Szz, Sxz, Sxx, noise_kind, noise, z_noise_kind, z_noise, mean, y, dt, inputs=inputs, cholesky=cholesky, ops=_Ops)


# ---- sgp_kernelmatrix_diag_grad_param with the caller's w ----------------------------------------------------------------------
def _amp(kind, param, f, X, Y, dt):
    """amp_f of the module docstring for one factor over the diagonal's entries, as a float"""
    if kind not in COEF_KINDS:
        return KT._amp(kind, param, f, X, Y, dt)
    import wienerpp_truth as wt
    D = X.shape[0]
    if kind == WIENER:
        return (2.0 * param + 2.0) * (0.5 * D + 2.0) + 28.0
    assert kind in PP, "the diagonal cases hold no NEURALNET / FBM / EXPONENTIATED factor"
    q, j = kind - PIECEWISE0, int(param)
    k, kx = np.abs(f["k"]).astype(np.float64), np.abs(f["c2"]).astype(np.float64) / 2.0
    r = np.sqrt(KT._d2(X, Y, True).astype(np.float64))
    amp = 0.0
    for v, b in ((k, wt.pp_value_bound(q, j, D, r, k)), (kx, wt.pp_kx_bound(q, j, D, r, kx))):
        amp = max(amp, float(np.max(np.where(v > 0, b / np.where(v > 0, v, 1.0), 0.0), initial=0.0)) / EPS)
    return amp + 8.0


def diag_grad(S, w, dt):
    """KT.diag_grad (same outputs and conventions: the row input receives d k / d x, the column input d k / d y, both added
    when the two are one array) over chains that may hold the coefficient kinds; Sm takes their point derivatives part by part"""
    X_in = [a.astype(dt) for a in S["inputs"]]
    roff, _ = KT._offsets(S)
    w = np.asarray(w, np.float64).astype(dt)
    nt = S["n_terms"]
    out = dict(gx=[np.zeros(a.shape, dt) for a in X_in], S_gx=[np.zeros(a.shape, dt) for a in X_in],
               Sm_gx=[np.zeros(a.shape, dt) for a in X_in], amp_gx=[0.0] * len(X_in),
               diagonal=np.zeros(nt, bool), amp=np.zeros(nt), dim=np.zeros(nt, int),
               rowscale=[None] * nt, colscale=[None] * nt, Sm_rowscale=[None] * nt, Sm_colscale=[None] * nt)
    for key in ("coef", "inscale", "param"):
        out["d_" + key], out["S_" + key], out["Sm_" + key] = np.zeros(nt, dt), np.zeros(nt, dt), np.zeros(nt, dt)
    for ch in S["chains"]:
        if ch["I"] != ch["J"]:
            continue
        I, h, coef = ch["I"], ch["head"], dt(ch["coef"])
        rs, cs = KT._scale_vectors(ch, dt)
        rsv, csv = (1 if rs is None else rs), (1 if cs is None else cs)
        fs, mags, amp, dim = [], [], 0.0, 0
        for (t, kind, ri, ci, param) in ch["factors"]:
            f = factor(kind, X_in[ri], X_in[ci], param, dt, diag=True)
            fs.append(f)
            mags.append((np.abs(f["k"]), None, np.abs(f["dk"]), np.abs(f["dp"])) if kind in COEF_KINDS else
                        KT._magnitudes(kind, param, f, X_in[ri], X_in[ci], dt))
            amp += _amp(kind, param, f, X_in[ri], X_in[ci], dt)
            dim = max(dim, X_in[ri].shape[0])
        wb = w[roff[I]:roff[I + 1]]
        ww = wb * rsv * csv
        full = KT._product([f["k"] for f in fs], fs[0]["k"])
        mfull = KT._product([m[0] for m in mags], mags[0][0])
        out["d_coef"][h], out["S_coef"][h], out["Sm_coef"][h] = (ww * full).sum(), np.abs(ww * full).sum(), (np.abs(ww) * mfull).sum()
        if rs is not None:
            out["rowscale"][h], out["Sm_rowscale"][h] = wb * coef * csv * full, np.abs(wb * coef * csv) * mfull
        if cs is not None:
            out["colscale"][h], out["Sm_colscale"][h] = wb * coef * rsv * full, np.abs(wb * coef * rsv) * mfull
        for ia, (t, kind, ri, ci, param) in enumerate(ch["factors"]):
            out["diagonal"][t], out["amp"][t], out["dim"][t] = True, amp, dim
            A = coef * ww * KT._product([f["k"] for ib, f in enumerate(fs) if ib != ia], fs[0]["k"])
            mA = np.abs(coef * ww) * KT._product([m[0] for ib, m in enumerate(mags) if ib != ia], mags[0][0])
            for key, q, mq in (("inscale", fs[ia]["dk"], mags[ia][2]), ("param", fs[ia]["dp"], mags[ia][3])):
                out["d_" + key][t], out["S_" + key][t], out["Sm_" + key][t] = (A * q).sum(), np.abs(A * q).sum(), (mA * mq).sum()
            X, Y, f = X_in[ri], X_in[ci], fs[ia]
            for k in (ri, ci):
                out["amp_gx"][k] = max(out["amp_gx"][k], amp + dim)
            if kind in COEF_KINDS:
                rows, cols = (f["c1"] * X, f["c2"] * (X - Y), f["c3"] * Y), (f["c1y"] * Y, f["c2"] * (Y - X), f["c3"] * X)
            elif kind == KT.LINEAR:
                rows, cols = (Y,), (X,)
            else:
                rows = (dt(2) * f["kp"] * (X - Y),)
                cols = (-rows[0],)
            for k, parts in ((ri, rows), (ci, cols)):
                out["gx"][k] += A[None, :] * sum(parts)
                out["S_gx"][k] += np.abs(A[None, :] * sum(parts))
                # a distance kind's magnitude is its model's |kp| (COSINE: pi^2 / 2), not the value's
                mag = sum(np.abs(p) for p in parts) if f["kp"] is None else dt(2) * mags[ia][1] * np.abs(X - Y)
                out["Sm_gx"][k] += mA[None, :] * mag
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
LAYOUT, ONE_BLOCK, Z_LAYOUT = (129, 1, 70), (257,), (33, 1)
WFULL_COEF = 0.05         # wp-wfull-D3: 0.2 and 0.1 leave K + Sigma_y indefinite in the long-double run (smallest eigenvalue -1.1, -0.06)


def _w(i, D):
    """WIENER i on the half line: the input itself at D = 1, its first coordinate beyond"""
    import stheno_jl_amd as P
    return P.WienerKernel(i) if D == 1 else P.WienerKernel(i) @ P.SelectTransform([0])


def _kernels(D):
    import stheno_jl_amd as P
    wl = P.with_lengthscale
    W, PPK, SE, RQ = P.WienerKernel, P.PiecewisePolynomialKernel, P.SEKernel, P.RationalQuadraticKernel
    lp = {1: 0.75, 2: 1.4, 3: 1.65, 5: 1.8, 8: 1.9, 9: 1.95, 16: 2.03}[D]      # about the median distance of the data: the support edge cuts through it
    return {"w0": lambda: 0.5 * wl(_w(0, D), 2.0),
            "w1-se": lambda: 0.8 * wl(_w(1, D), 2.0) * wl(SE(), 1.3) + 0.2 * wl(P.Matern32Kernel(), 1.5),
            "w2-pp1": lambda: 1.5 * wl(_w(2, D), 2.0) + 0.6 * wl(PPK(1, dim=D), lp),
            "w3-se": lambda: 2.0 * wl(_w(3, D), 1.5) * wl(SE(), 1.4) + 0.3 * wl(SE(), 1.2),
            "wfull": lambda: WFULL_COEF * wl(W(1), 1.5) + 1.0 * wl(SE(), 1.3),
            "pp0": lambda: 0.8 * wl(PPK(0, dim=D), lp),
            "pp2": lambda: 0.8 * wl(PPK(2, dim=D), lp) + 0.1 * wl(SE(), 1.5),
            "pp3": lambda: 0.8 * wl(PPK(3, dim=D), lp) + 0.1 * wl(P.Matern52Kernel(), 1.5),
            "pp-rq-lin": lambda: 0.5 * wl(PPK(1, dim=D), lp) * RQ(0.9) * P.LinearKernel(0.4) + 0.3 * wl(SE(), 1.5),
            "w-fbm-mn": lambda: 0.7 * wl(_w(1, D), 1.5) * P.FBMKernel(0.6) * wl(P.GeneralMaternKernel(0.8), 1.2) + 0.2 * wl(SE(), 1.3),
            "scaled": lambda: 0.7 * wl(_w(1, D), 1.5) * wl(SE(), 1.2) + 0.3 * wl(PPK(2, dim=D), lp),
            "pp1-w0": lambda: 0.6 * wl(PPK(1, dim=D), lp) * wl(_w(0, D), 1.5) + 0.2 * wl(SE(), 1.4),
            "mixed": lambda: 0.7 * wl(_w(2, D), 1.2) * wl(SE(), 1.2) + 0.4 * wl(PPK(3, dim=D), lp) * RQ(1.1),
            "diag": lambda: (1.3 * SE() * wl(_w(2, D), 1.2) + 0.3 * P.LinearKernel(0.4) * PPK(1, dim=D) + 0.2 * wl(W(3), 2.0) +
                             0.5 * W(0) * wl(PPK(3, dim=D), 2.0) + 0.1 * W(1) + 0.4 * wl(PPK(0, dim=D), 1.5) * wl(PPK(2, dim=D), 3.0))}


# (id, kind of case, kernel, D, noise, layout, model): "diag" noise is a vector, "dense" (ELBO) a dense Sigma_z beside a scalar
# Sigma_y; model "scaled": blocks g f g of g = sigma(x) f (a head with a function-valued row scale)
CASES = [("wp-w0-D1", "lp", "w0", 1, "scalar", LAYOUT, "plain"), ("wp-w1-se-D2", "lp", "w1-se", 2, "diag", LAYOUT, "plain"),
         ("wp-w2-pp1-D3", "lp", "w2-pp1", 3, "scalar", LAYOUT, "plain"), ("wp-w3-se-D8", "lp", "w3-se", 8, "scalar", LAYOUT, "plain"),
         ("wp-wfull-D3", "lp", "wfull", 3, "scalar", LAYOUT, "plain"), ("wp-pp0-D1", "lp", "pp0", 1, "diag", LAYOUT, "plain"),
         ("wp-pp2-D5", "lp", "pp2", 5, "scalar", LAYOUT, "plain"), ("wp-pp3-D16", "lp", "pp3", 16, "scalar", ONE_BLOCK, "plain"),
         ("wp-pp-rq-lin-D2", "lp", "pp-rq-lin", 2, "scalar", LAYOUT, "plain"),
         ("wp-w-fbm-mn-D9", "lp", "w-fbm-mn", 9, "diag", LAYOUT, "plain"), ("wp-scaled-D3", "lp", "scaled", 3, "scalar", LAYOUT, "scaled"),
         ("wp-pp1-w0-D2", "lp", "pp1-w0", 2, "scalar", ONE_BLOCK, "plain"),
         ("wpelbo-w-D1", "elbo", "w1-se", 1, "scalar", LAYOUT, "plain"), ("wpelbo-pp-D3", "elbo", "pp2", 3, "scalar", LAYOUT, "plain"),
         ("wpelbo-mixed-D2", "elbo", "mixed", 2, "dense", LAYOUT, "plain"), ("wpelbo-D16", "elbo", "scaled", 16, "scalar", LAYOUT, "plain")]
# (id, kernel, D, model): "views" is var(f(a x) + f(b x)), "plain" var(f(x))
DIAG_CASES = [("wpdiag-D3-views", "diag", 3, "views"), ("wpdiag-D8-views", "diag", 8, "views"), ("wpdiag-D3-plain", "diag", 3, "plain")]


# seeds moved by 100: with the first seeds the NumPy double of the entry points (NumPy's own LAPACK routes; tests/
# test_wienerpp_grad_truth_on_numpy.py runs the GPU file's bodies on it under margin 2) missed margin 2 in kp.value / kp.noise,
# kp.value and kpelbo.inputs by factors 1.6, 1.1 and 1.1: the floors, medians of 12 and of 4 figures, are thin for margin 2
SEED_BUMP = {"wp-wfull-D3": 100, "wp-scaled-D3": 100, "wpelbo-w-D1": 100}


def _sigma(pt):
    return 1.0 + 0.3 * float(np.sin(np.sum(pt)))


def _model(kernel, model):
    import stheno_jl_amd as P
    if model == "scaled":
        return P.gppp(lambda GP: (lambda f: {"f": f, "g": _sigma * f})(GP(kernel))), ("g", "f", "g")
    if model == "views":
        return P.gppp(lambda GP: (lambda f: {"f": f, "g": P.stretch(f, 0.7) + P.stretch(f, 1.6)})(GP(kernel))), ("g", "g", "g")
    return P.gppp(lambda GP: {"f": GP(kernel)}), ("f", "f", "f")


def _blocks(rng, D, layout, names):
    import stheno_jl_amd as P
    X = rng.standard_normal((D, sum(layout))) / np.sqrt(D) * 1.5
    X[0] = np.abs(X[0])
    X[:, 5], X[:, 11] = X[:, 3], 0.0
    if len(layout) > 1:
        X[:, -1] = X[:, 7]
    off = np.concatenate([[0], np.cumsum(layout)])
    cols = [np.asfortranarray(X[:, off[i]:off[i + 1]]) for i in range(len(layout))]
    return P.BlockData([P.GPPPInput(nm, c[0].copy() if D == 1 else P.ColVecs(c)) for nm, c in zip(names, cols)])


def problem(case):
    """(F, x, z or None, noise, z_noise, y) of a case"""
    cid, what, kname, D, noise_kind, layout, model = case
    rng = np.random.default_rng(9100 + [c[0] for c in CASES].index(cid) + SEED_BUMP.get(cid, 0))
    F, names = _model(_kernels(D)[kname](), model)
    x = _blocks(rng, D, layout, names)
    z = _blocks(rng, D, Z_LAYOUT, names) if what == "elbo" else None
    n, m = sum(layout), sum(Z_LAYOUT)
    noise = 0.05 + 0.25 * rng.random(n) if noise_kind == "diag" else float(0.05 + 0.25 * rng.random())
    sz = 1e-2
    if noise_kind == "dense":
        Q = rng.standard_normal((m, m))
        sz = np.asfortranarray(1e-2 * np.eye(m) + 1e-2 * (Q @ Q.T) / m)
    return F, x, z, noise, sz, rng.standard_normal(n)


def diag_problem(case):
    """(spec, w) of a diagonal case"""
    import stheno_jl_amd as P
    cid, kname, D, model = case
    rng = np.random.default_rng(9200 + [c[0] for c in DIAG_CASES].index(cid))
    F, names = _model(_kernels(D)[kname](), model)
    spec, _, _ = P.build_spec(F, _blocks(rng, D, LAYOUT, names))
    return spec, np.ascontiguousarray(rng.standard_normal(spec.N))


def specs(case):
    """the specs of a case as the host builds them: (xx,) or (zz, xz, xx)"""
    import stheno_jl_amd as P
    F, x, z, *_ = problem(case)
    if z is None:
        return (P.build_spec(F, x)[0],)
    return P.build_spec(F, z)[0], P.build_spec(F, x, None, z)[0], P.build_spec(F, x)[0]


def launch_classes(spec):
    """{DMAX} over the chains of a spec that hold a WIENER or PIECEWISE factor: such a chain is of tier 4
    (csrc/kprod_kinds_table.h) and runs the mode-3 instantiations at DMAX = its largest factor dimension rounded up to a
    power of two"""
    out = set()
    for ch in KT.read_spec(spec)["chains"]:
        if any(kind in WPP for (_, kind, _, _, _) in ch["factors"]):
            dim = max(np.atleast_2d(spec.inputs[ri]).shape[0] for (_, _, ri, _, _) in ch["factors"])
            out.add(1 << (dim - 1).bit_length())
    return out


def _runs():
    return ((KT.require_extended(), None), (np.float64, None), (np.float64, KT.cholesky_blocked_order))


_TRUTH = {}


def truth(case):
    """(long double, float64, float64 in the blocked order): computed once per case, shared, never modified"""
    import stheno_jl_amd as P
    if case[0] not in _TRUTH:
        F, x, z, noise, sz, y = problem(case)
        mean = P.mean(F(x, noise))
        nk = NOISE_DIAG if np.ndim(noise) else NOISE_SCALAR
        Ss = [KT.read_spec(sp) for sp in specs(case)]
        if z is None:
            _TRUTH[case[0]] = tuple(logpdf_grad(Ss[0], nk, noise, mean, y, dt, inputs=True, scales=True, cholesky=ch) for dt, ch in _runs())
        else:
            zk = NOISE_DENSE if np.ndim(sz) else NOISE_SCALAR
            _TRUTH[case[0]] = tuple(elbo_grad(*Ss, nk, noise, zk, sz, mean, y, dt, inputs=True, cholesky=ch) for dt, ch in _runs())
    return _TRUTH[case[0]]


def diag_truth(case):
    if case[0] not in _TRUTH:
        spec, w = diag_problem(case)
        _TRUTH[case[0]] = diag_grad(KT.read_spec(spec), w, KT.require_extended())
    return _TRUTH[case[0]]


logpdf_units = DG.logpdf_units


def reference_figures(case):
    """e_float64 of a case: family by family the larger figure of the two float64 runs against the long-double run"""
    R, *R64 = truth(case)
    if case[1] == "lp":
        runs = [logpdf_units(KT.logpdf_reference_outputs(r), R) for r in R64]
    else:
        runs = [KT.elbo_units(dict(KT.elbo_reference_outputs(dict(r, xx=None))), R) for r in R64]
    return {fam: max(r[fam] for r in runs) for fam in runs[0]}


# the sorted lists of reference_figures over CASES and their medians, printed by `python tests/wienerpp_grad_truth.py`
MEASURED_FLOAT64 = {'kp.d_coef': [22.1, 27.0, 32.5, 42.2, 114.3, 201.8, 209.3, 334.3, 391.0, 579.5, 818.8, 9147.1],
 'kp.d_inscale': [2.8, 27.9, 36.7, 60.0, 168.5, 207.6, 208.7, 209.3, 273.7, 445.1, 648.7, 9136.2],
 'kp.d_param': [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 83.6, 1289.4],
 'kp.inputs': [16.0, 42.7, 51.7, 79.7, 81.5, 97.0, 102.2, 137.4, 153.9, 165.8, 690.2, 4732.2],
 'kp.noise': [1.4, 3.5, 4.7, 4.9, 8.1, 15.5, 23.8, 26.1, 29.4, 50.1, 52.6, 119.8],
 'kp.scales': [36.4],
 'kp.value': [0.4, 0.7, 1.2, 1.2, 1.5, 1.7, 1.8, 2.6, 4.0, 7.2, 8.1, 19.0],
 'kp.y': [10.5, 17.8, 17.8, 30.9, 34.4, 39.7, 43.8, 77.4, 82.9, 85.5, 88.3, 105.1],
 'kpelbo.d_coef': [323.5, 2231.3, 38595.0, 599408.2],
 'kpelbo.d_inscale': [663.3, 2237.3, 38594.2, 599408.7],
 'kpelbo.d_param': [0.0, 0.0, 0.0, 555.7],
 'kpelbo.inputs': [435.4, 1206.1, 1616.8, 8302.4],
 'kpelbo.noise': [0.4, 0.4, 1.0, 1.4],
 'kpelbo.value': [0.3, 1.3, 2.6, 3.2],
 'kpelbo.y': [1.5, 3.2, 4.0, 9.4],
 'kpelbo.z_noise': [2.8, 39.1, 49.3, 130.4]}
FLOORS = {fam: float(np.median(v)) for fam, v in MEASURED_FLOAT64.items()}


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    entry.load_package()
    figs = {}
    for case in CASES:
        for fam, v in reference_figures(case).items():
            figs.setdefault(fam, []).append(round(float(v), 1))
    print("MEASURED_FLOAT64 =", {k: sorted(v) for k, v in sorted(figs.items())})
    print("FLOORS =", {k: float(np.median(v)) for k, v in sorted(figs.items())})


if __name__ == "__main__":
    main()
