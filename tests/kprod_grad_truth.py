"""Extended-precision truth for the gradients through product chains (include/sthenomi_kprod.h, include/sthenomi_kprod_grad.h:
sgp_logpdf_grad_param, sgp_logpdf_grad_param_xs, sgp_kernelmatrix_diag_grad_param, sgp_elbo_grad_param).

TEST INFRASTRUCTURE ONLY.  A dtype-generic restatement of the two headers on top of tests/grad_truth.py: the factorisation,
the triangular inverse, the direct squared distance, the noise matrix, the four plain kinds, the ELBO's cotangents and the
units are that module's (its logpdf_grad / elbo_grad run with this module's `dense`, `diag_of` and `contract`); what is
written here are the kinds a chain can hold beyond them -- RQ, LINEAR, COSINE, GAMMAEXP and general-nu Matern (kind 20) --
each with k, d k / d (d^2), d k / d g and d k / d param in the working dtype, straight from the headers' definitions, the
chain product, every leave-one-out product (formed directly as the product over f != a: no prefix or suffix products, no
division), and the contractions with a head's row and column scale vectors.  Run in np.longdouble it is the truth, run in
np.float64 the yardstick.  Every sum is returned with the sum of the absolute values of its addends.

Kind 20 restates the device's algorithm (Temme's series, Steed's second continued fraction, the upward recurrence;
csrc/kprod.hip: matern_nu_derivs), generic in the dtype and stopped by the working dtype's own epsilon.  That is allowed to be
a truth because tests/test_kprod_grad_truth_on_numpy.py pins its long-double run to mpmath.besselk: the largest relative
error over the nu and x grid of tests/kprod_grad_truth_mp.py (that of tests/matern_nu_truth.py and more) is BESSEL_MEASURED
below, against the cap 2^-59 (1 / 64 of a float64 eps).  Two things differ from the device so that it stays under the cap,
both measured against mpmath before they were changed (47 and 1356 units of 2^-64; the cap is 32): the series hands over to
the fraction at x = 1, not 2 (Temme's first term cancels up to eightfold against K_mu at x = 2, |mu| -> 1/2; the fraction
then takes up to MN_CF2_MAXIT steps, the iteration limit that was raised for it), and the argument x = sqrt(2 nu d^2) is
carried with what its rounding misses (_mn_argument), because e^-x turns the rounding of x into x / 2 units.

Limits, as the headers document them: Matern-1/2 and GammaExponential have kappa' = 0 at coincident points, Cosine -pi^2 / 2,
kind 20 -nu / (2 (nu - 1)) for nu > 1 and 0 for nu <= 1.  Cosine is cos(pi d) with pi in the working dtype (no cospi: the
float64 run then shows what the plain formula costs).  Polynomial(n, c) and Periodic(r) are flattened on the host
(kernels.py: leaf_products / leaf_terms) into n LINEAR factors and into an SE factor on the embedded points: they arrive here
as those kinds.

The diagonal (`kpdiag.*`) involves no factorisation: its bound is a model, not a measurement,
    |device - truth| <= (D + 8 + sum_f amp_f) eps Sm
per sum and per entry.  (D + 8) eps S is the base term of diag_grad* (tests/test_gpu_grad_truth.py: the D-term distance, the
products, the accumulation); Sm is the sum of the absolute addends with a COSINE factor's value, dk and kappa' replaced by
what their error models are relative to (1, pi d and pi^2 / 2: the factor passes through zero) and a LINEAR factor's value by
sum_d |x_d y_d| + |c|; amp_f is the kind's own model, once per factor of the chain, the largest over the case's entries, in
eps relative to that magnitude:
    SE 4;  Matern-1/2, 3/2, 5/2  2 (6 + 4 l) + 8, l = sqrt(2 nu) d        (tests/kernel_truth.py, in ulp = 2 eps; 8: the
                                                                            derivative's own products)
    RQ  2 (2 + 7 a) + 8, a = alpha log1p(d^2 / (2 alpha))                  (tests/kprod_truth.py)
    COSINE  S0 + pi d + 4;  GAMMAEXP  2 (2 + C_POW a) + 8 + 6, a = d^gamma (tests/kinds_truth.py; 6: log d^2 in d / d gamma)
    kind 20  A + 8 + 4 x + C n                                             (tests/matern_nu_truth.py: the bound of dk)
    LINEAR  D + 1;  CONST, WHITE  0
plus (D + 2) max(1, arg_f) for what the roundings of the D-term d^2 do through the factor (arg_f: d^2 / 2, l, a, pi d, a, x:
the logarithmic slope of every quantity of the kind is at most that, or 1)."""
import math

import numpy as np

import grad_truth as T
from grad_truth import (EPS, MARGIN, NOISE_DENSE, NOISE_DIAG, NOISE_SCALAR, SELF_MARGIN, cholesky,  # noqa: F401
                        cholesky_blocked_order, noise_matrix, require_extended, scale_entries, scale_scalar, sqdist,
                        tri_inverse, units)

SE, MATERN12, MATERN32, MATERN52, WHITE, CONST = range(6)
RQ, LINEAR, COSINE, GAMMAEXP, MATERN_NU = 6, 7, 16, 17, 20
TIMES_PREV, KIND_MASK = 0x100, 0xff

# largest relative error of the long-double Bessel routine against mpmath at 40 digits over the grid of
# tests/kprod_grad_truth_mp.py (k and kappa'), printed by `python tests/test_kprod_grad_truth_on_numpy.py`; the cap is 2^-59
BESSEL_CAP = 2.0 ** -59
BESSEL_MEASURED = 1.157e-18      # 21.3 units of 2^-64 (nu = 32, x = 2.5)

# e_float64 of a case is the larger figure of two float64 runs of this reference (grad_truth.py: its own column recurrence and
# LAPACK's blocked order).  Floors, in units: the median of e_float64 over the final case list
# (tests/test_gpu_kprod_grad_truth.py's cases; printed by `python tests/test_kprod_grad_truth_on_numpy.py`), so that a lucky
# float64 draw does not make a bound vanish.  First the sorted measured lists, then their medians.
MEASURED_FLOAT64 = {'kp.d_coef': [11.4, 14.6, 19.4, 23.7, 35.3, 104.1, 173.4, 179.0, 188.8, 191.7, 192.5, 198.7, 199.7, 200.9, 212.2,
               213.1, 228.3, 273.8, 297.2, 377.5, 409.5, 425.4, 497.5, 650.2, 708.6, 735.0, 759.5, 958.1, 1037.6,
               1124.0, 1210.8, 1469.6, 1823.6, 2632.0, 120797.4],
 'kp.d_inscale': [0.0, 16.6, 22.6, 46.0, 54.4, 66.0, 68.5, 73.8, 77.3, 105.3, 165.8, 204.3, 213.4, 244.0, 244.3, 304.1,
                  425.5, 454.8, 550.2, 556.6, 667.6, 696.7, 762.2, 763.3, 791.2, 902.5, 929.7, 1053.8, 1255.2, 1285.9,
                  1701.9, 2109.4, 3258.3, 5418.2, 67681.9],
 'kp.d_param': [0.0, 0.0, 0.0, 11.7, 13.5, 29.1, 36.9, 37.6, 69.2, 71.5, 73.3, 81.1, 126.3, 154.6, 155.3, 155.9, 157.7,
                200.7, 201.1, 207.3, 221.6, 228.9, 275.6, 359.3, 389.6, 425.4, 459.7, 571.8, 655.3, 731.6, 963.3,
                1922.9, 2607.8, 2854.8, 270255.4],
 'kp.inputs': [0.0, 13.1, 15.1, 17.6, 38.2, 45.4, 45.9, 48.3, 49.0, 58.7, 75.1, 93.5, 97.1, 97.7, 101.5, 109.1, 112.4,
               139.2, 148.1, 153.3, 159.4, 169.6, 174.1, 210.6, 213.0, 224.0, 284.2, 291.5, 305.1, 322.1, 334.7, 478.9,
               507.3, 932.9, 9298.1],
 'kp.noise': [0.0, 0.2, 4.1, 4.6, 4.9, 5.1, 6.4, 6.9, 6.9, 9.2, 10.5, 10.9, 11.3, 11.7, 12.0, 14.2, 14.4, 14.7, 15.2,
              16.6, 18.1, 18.5, 20.0, 20.2, 21.4, 22.9, 24.3, 28.1, 29.1, 36.2, 36.6, 45.3, 46.1, 103.7, 295.4],
 'kp.scales': [83.9, 386.0, 827.2],
 'kp.value': [0.3, 0.4, 0.5, 0.6, 0.6, 0.7, 0.7, 0.9, 1.2, 1.2, 1.4, 1.7, 1.9, 1.9, 2.3, 2.3, 2.5, 2.5, 2.6, 3.0, 3.3,
              4.0, 4.0, 4.6, 5.1, 5.3, 5.4, 5.9, 7.1, 7.7, 13.0, 13.2, 13.5, 14.0, 42.4],
 'kp.y': [4.7, 4.9, 5.8, 6.1, 8.5, 14.7, 16.6, 17.5, 20.0, 21.5, 22.2, 25.5, 32.9, 33.2, 34.3, 47.7, 49.4, 50.0, 65.8,
          76.9, 80.2, 82.4, 84.9, 90.1, 107.0, 120.4, 124.2, 127.5, 146.8, 153.8, 154.6, 199.9, 216.0, 301.0, 413.4],
 'kpelbo.d_coef': [5.7, 77.1, 346.5, 502.4, 906.2, 1557.6, 19966.8],
 'kpelbo.d_inscale': [67.0, 158.3, 432.5, 796.0, 1327.7, 2583.9, 8138.2],
 'kpelbo.d_param': [80.0, 227.3, 990.5, 1023.6, 1602.9, 3390.9, 17992.1],
 'kpelbo.inputs': [41.9, 136.2, 243.1, 295.6, 1835.1, 5404.7, 7841.0],
 'kpelbo.noise': [0.1, 0.9, 0.9, 1.0, 1.2, 5.7, 8.7],
 'kpelbo.scales': [30.3, 188.8, 215.1, 425.9, 1105.0, 3402.3],
 'kpelbo.value': [0.3, 0.7, 2.2, 2.7, 3.2, 9.1, 12.4],
 'kpelbo.y': [4.1, 15.6, 16.5, 26.3, 37.6, 55.0, 75.4],
 'kpelbo.z_noise': [1.2, 3.5, 14.9, 48.7, 69.9, 113.5, 131.7]}
FLOORS = {'kp.d_coef': 273.8,
 'kp.d_inscale': 454.8,
 'kp.d_param': 200.7,
 'kp.inputs': 139.2,
 'kp.noise': 14.7,
 'kp.scales': 386.0,
 'kp.value': 2.5,
 'kp.y': 50.0,
 'kpelbo.d_coef': 502.4,
 'kpelbo.d_inscale': 796.0,
 'kpelbo.d_param': 1023.6,
 'kpelbo.inputs': 295.6,
 'kpelbo.noise': 1.0,
 'kpelbo.scales': 320.5,
 'kpelbo.value': 2.7,
 'kpelbo.y': 26.3,
 'kpelbo.z_noise': 48.7}

# the tolerance of the existing tests that each family's bound must undercut by a factor 100 (relative to the scale)
OLD_TOLERANCE = {"d_inscale": 2e-6, "other": 1e-8}


# ---- reading a spec --------------------------------------------------------------------------------------------
def read_spec(spec):
    """dict(chains, n_terms, inputs, row_len, col_len, symmetric) from a stheno_jl_amd.lib.Spec; a chain is
    dict(I, J, head, coef, rs, cs, factors=[(t, kind, row_input, col_input, param)]); a plain term is a chain of one"""
    from stheno_jl_amd import lib as L
    assert (L.RQ, L.LINEAR, L.COSINE, L.GAMMAEXP, L.MATERN_NU) == (RQ, LINEAR, COSINE, GAMMAEXP, MATERN_NU)
    assert (L.KIND_TIMES_PREV, L.KIND_MASK, L.CONST, L.WHITE) == (TIMES_PREV, KIND_MASK, CONST, WHITE)
    assert not spec.has_patch and not spec.has_stencil
    chains = []
    tp, nb = spec._term_ptr, len(spec.col_len)
    for I in range(len(spec.row_len)):
        for J in range(nb):
            p = I * nb + J
            t = int(tp[p])
            while t < int(tp[p + 1]):
                e = t + 1
                while e < int(tp[p + 1]) and (spec._terms[e].kind & TIMES_PREV):
                    e += 1
                rs, cs = spec.term_row_scale[t], spec.term_col_scale[t]
                chains.append(dict(I=I, J=J, head=t, coef=float(spec._terms[t].coef),
                                   rs=None if rs is None else np.array(rs, dtype=np.float64),
                                   cs=None if cs is None else np.array(cs, dtype=np.float64),
                                   factors=[(u, int(spec._terms[u].kind) & KIND_MASK, int(spec._terms[u].row_input),
                                             int(spec._terms[u].col_input), float(spec._terms[u].param)) for u in range(t, e)]))
                t = e
    return hand_spec(chains, spec.inputs, spec.row_len, spec.col_len, spec.symmetric)


def hand_spec(chains, inputs, row_len, col_len, symmetric):
    n_terms = sum(len(c["factors"]) for c in chains)
    return dict(chains=chains, n_terms=n_terms, inputs=[np.atleast_2d(np.array(a, dtype=np.float64)) for a in inputs],
                row_len=[int(v) for v in row_len], col_len=[int(v) for v in col_len], symmetric=bool(symmetric))


# ---- general-nu Matern: K_nu by Temme's series / Steed's continued fraction, generic in the dtype -----------------------------
# Taylor coefficients of 1 / Gamma(1 + z) at 0 (Abramowitz & Stegun 6.1.34), to 20 digits: 1e-20 relative, 1 / 50 of 2^-59
_RGAMMA = ("1.0", "0.57721566490153286061", "-0.65587807152025388108", "-0.042002635034095235529", "0.1665386113822914895",
           "-0.042197734555544336748", "-0.0096219715278769735621", "0.0072189432466630995424", "-0.0011651675918590651121",
           "-0.00021524167411495097282", "0.00012805028238811618615", "-0.000020134854780788238656", "-1.2504934821426706573e-6",
           "1.1330272319816958824e-6", "-2.0563384169776071035e-7", "6.1160951044814158179e-9", "5.0020076444692229301e-9",
           "-1.1812745704870201446e-9", "1.0434267116911005105e-10", "7.782263439905071254e-12", "-3.6968056186422057082e-12",
           "5.100370287454475979e-13", "-2.0583260535665067832e-14", "-5.3481225394230179824e-15", "1.2267786282382607902e-15",
           "-1.1812593016974587695e-16", "1.1866922547516003326e-18", "1.4123806553180317816e-18")
MN_X_SPLIT, MN_X_ZERO, MN_X_EXP_SPLIT = 1.0, 1000.0, 600.0
MN_TEMME_MAXIT, MN_CF2_MAXIT = 60, 1000          # the long-double run takes 17 and 124 at the most


def mn_constants(nu, dt):
    """what depends on nu alone, in dtype dt (nu itself is a double).  1 / Gamma(nu) from the series' 1 / Gamma(1 +- mu) and
    the functional equation: Gamma(mu + n) = (mu + n - 1) .. (mu + 1) Gamma(1 + mu); nu < 1/2: Gamma(nu) = Gamma(1 + nu) / nu"""
    nuf = float(nu)
    if not (0.0 < nuf <= 32.0):
        raise ValueError("nu must be finite and in (0, 32]")
    nu = dt(nuf)
    n = 0 if nuf < 0.5 else int(math.floor(nuf + 0.5))
    mu = -nu if n == 0 else nu - dt(n)
    m2 = mu * mu
    a = [dt(s) for s in _RGAMMA]
    g1 = g2 = dt(0)
    for j in range(13, -1, -1):
        g2 = g2 * m2 + a[2 * j]
        g1 = g1 * m2 - a[2 * j + 1]
    gampl, gammi = g2 - mu * g1, g2 + mu * g1             # 1 / Gamma(1 + mu), 1 / Gamma(1 - mu)
    pi = T._pi(dt)
    fact = dt(1) if mu == 0 else (pi * mu) / np.sin(pi * mu)
    if n == 0:
        rgam = nu * gammi
    else:
        rgam = gampl
        for j in range(1, n):
            rgam = rgam / (mu + dt(j))
    half = dt(1) / dt(2)
    ca = dt(2) ** (1 - n) * rgam
    return dict(nu=nu, n=n, mu=mu, fact=fact, gam1=g1, gam2=g2, ph=half / gampl, qh=half / gammi,
                a1=(half - mu) * (half + mu), ca=ca, ck=nu * ca, sq=np.sqrt(dt(2) * nu),
                kx0=(-nu / (dt(2) * (nu - dt(1))) if nuf > 1.0 else dt(0)), half_pi=pi / dt(2),
                eps=dt(np.finfo(dt).eps) / dt(2))


def _mn_temme(c, x, dt):
    """(Q0, Q1, E, iterations) for 0 < x <= 2;  Q_j = (x / 2)^mu x^j K_(mu+j)(x)"""
    mu, m2, eps = c["mu"], c["mu"] * c["mu"], c["eps"]
    one, two = dt(1), dt(2)
    xh = x / two
    dl = -np.log(xh)
    E = np.power(xh, two * mu)
    g = -(two * mu) * dl
    small = np.abs(g) < 1
    gs = np.where(small & (g != 0), g, one)
    t2 = np.where(small, np.where(g != 0, np.expm1(gs) / gs, one) * dl, (one - E) / (two * mu if mu != 0 else one))
    ff = c["fact"] * (c["gam1"] * ((one + E) / two) + c["gam2"] * t2)
    p = np.full(x.shape, c["ph"], dtype=dt)
    q = c["qh"] * E
    s0, s1, cc, dd = ff.copy(), p.copy(), np.ones(x.shape, dtype=dt), xh * xh
    live = np.ones(x.shape, dtype=bool)
    its = np.zeros(x.shape, dtype=int)
    for i in range(1, MN_TEMME_MAXIT + 1):
        di = dt(i)
        ff = (di * ff + p + q) / (di * di - m2)
        cc = cc * (dd / di)
        p = p / (di - mu)
        q = q / (di + mu)
        de0 = cc * ff
        de1 = cc * (p - di * ff)
        s0 = np.where(live, s0 + de0, s0)
        s1 = np.where(live, s1 + de1, s1)
        its += live
        live = live & ~((np.abs(de0) < np.abs(s0) * eps) & (np.abs(de1) < np.abs(s1) * eps))
        if not live.any():
            break
    return s0, two * s1, E, its


def _mn_cf2(c, x, dt):
    """(Q0, Q1, E, iterations) for x > 2, all times e^x"""
    mu, a1, eps = c["mu"], c["a1"], c["eps"]
    one, two, half = dt(1), dt(2), dt(1) / dt(2)
    b = two * (one + x)
    d = one / b
    h = d.copy()
    delh = d.copy()
    q1, q2 = np.zeros(x.shape, dtype=dt), np.ones(x.shape, dtype=dt)
    q = np.full(x.shape, a1, dtype=dt)
    cc, a = a1, -a1                                  # (the same for every x)
    s = one + q * delh
    h_out, s_out, its = h.copy(), s.copy(), np.zeros(x.shape, dtype=int)
    # the entries still iterating, kept packed: an entry leaves with the sums of the step that met the criterion
    idx = np.arange(x.size) if a1 != 0 else np.arange(0)          # (mu = -1/2: the fraction is 1, K_(1/2) is its closed form)
    for i in range(2, MN_CF2_MAXIT + 1):
        if idx.size == 0:
            break
        a = a - dt(2 * (i - 1))
        cc = -a * cc / dt(i)
        qn = (q1 - b * q2) / a
        q1, q2 = q2, qn
        q = q + cc * qn
        b = b + two
        dn = one / (b + a * d)
        delh = (-a * d * dn) * delh
        d = dn
        h = h + delh
        dels = q * delh
        s = s + dels
        done = np.abs(dels) < np.abs(s) * eps
        if i == MN_CF2_MAXIT:
            done = np.ones(done.shape, dtype=bool)
        if done.any():
            h_out[idx[done]], s_out[idx[done]], its[idx[done]] = h[done], s[done], i - 1
            keep = ~done
            idx, b, d, h, delh, q1, q2, q, s = (v[keep] for v in (idx, b, d, h, delh, q1, q2, q, s))
    h, s = h_out, s_out
    h = a1 * h
    ks0 = np.sqrt(c["half_pi"] / x) / s
    w = np.power(x / two, mu)
    q0 = w * ks0
    return q0, q0 * (mu + x + half - h), w * w, its


def _two_prod(a, b, dt):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker's product on Veltkamp's split; no fma in NumPy)"""
    split = dt(2.0 ** ((np.finfo(dt).nmant + 2) // 2) + 1.0)

    def halves(v):
        c = split * v
        hi = c - (c - v)
        return hi, v - hi
    p = a * b
    ah, al = halves(a)
    bh, bl = halves(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _mn_argument(nu, d2, dt):
    """x = sqrt(2 nu d2) as (x, x_lo): x the working dtype's rounding and x_lo what it misses, so that e^-x can be applied as
    e^-x (1 - x_lo).  k falls like e^-x: a rounding of x alone costs x / 2 units of the working epsilon, 500 of them at
    x = 1000 -- the 2^-59 of the pin is 32 -- and no iteration limit touches it.  2 nu d2 is formed exactly as p + e, then one
    Newton step on the square root's residual (exact: x^2 again as a two-term product)."""
    p, e = _two_prod(np.full(d2.shape, dt(2) * nu, dtype=dt), d2, dt)
    x = np.sqrt(p)
    q, qe = _two_prod(x, x, dt)
    safe = np.where(x > 0, x, dt(1))
    return x, np.where(x > 0, (((p - q) - qe) + e) / (dt(2) * safe), dt(0))


def matern_nu_derivs(d2, nu, dt, want_iterations=False):
    """(k, dk / d(d2), dk(g x, g x') / dg at g = 1) of kind 20 at squared distances d2, in dtype dt:
    k = C x^nu K_nu(x), x = sqrt(2 nu) d;  kx = -nu ca Q_(n-1) [e^-x];  dk = 2 d2 kx.
    d2 == 0: k = 1, kx = -nu / (2 (nu - 1)) (nu > 1) or 0;  x >= 1000: exact zeros."""
    c = mn_constants(nu, dt)
    n = c["n"]
    d2 = np.asarray(d2, dtype=dt)
    shape = d2.shape
    d2 = d2.ravel()
    k, kx = np.zeros(d2.shape, dtype=dt), np.zeros(d2.shape, dtype=dt)
    its = np.zeros(d2.shape, dtype=int)
    zero = ~(d2 > 0)
    k[zero], kx[zero] = dt(1), c["kx0"]
    with np.errstate(over="ignore", invalid="ignore"):
        x, x_lo = _mn_argument(c["nu"], d2, dt)
    for lo in (True, False):
        m = ~zero & (x < MN_X_ZERO) & ((x <= MN_X_SPLIT) if lo else (x > MN_X_SPLIT))
        if not m.any():
            continue
        xm = x[m]
        qa, qb, E, it = (_mn_temme if lo else _mn_cf2)(c, xm, dt)
        if n == 0:
            tk = c["ca"] * (qa / E)
            tx = c["ck"] * ((qb / (xm * E)) / xm)
        else:
            x2 = xm * xm
            for j in range(1, n):
                qa, qb = qb, x2 * qa + (dt(2) * (c["nu"] - dt(n - j))) * qb
            tk, tx = c["ca"] * qb, c["ck"] * qa
        if not lo:
            far = xm > MN_X_EXP_SPLIT
            e600 = np.exp(-dt(MN_X_EXP_SPLIT))
            tk, tx = np.where(far, tk * e600, tk), np.where(far, tx * e600, tx)
            ex = np.exp(-np.where(far, xm - dt(MN_X_EXP_SPLIT), xm))
            ex = ex - ex * x_lo[m]
            tk, tx = tk * ex, tx * ex
        tk = np.minimum(tk, dt(1))
        k[m], kx[m], its[m] = tk, np.where(tk == 0, dt(0), -tx), it
    with np.errstate(over="ignore", invalid="ignore"):
        dk = np.where(kx == 0, dt(0), dt(2) * d2 * kx)
    out = (k.reshape(shape), kx.reshape(shape), dk.reshape(shape))
    return out + (its.reshape(shape),) if want_iterations else out


# ---- one factor ------------------------------------------------------------------------------------------------------------
def _dot(X, Y, diag):
    s = np.zeros(X.shape[1] if diag else (X.shape[1], Y.shape[1]), dtype=X.dtype)
    for d in range(X.shape[0]):
        s += X[d] * Y[d] if diag else X[d][:, None] * Y[d][None, :]
    return s


def _d2(X, Y, diag):
    if not diag:
        return sqdist(X, Y)
    d2 = np.zeros(X.shape[1], dtype=X.dtype)
    for d in range(X.shape[0]):
        df = X[d] - Y[d]
        d2 += df * df
    return d2


def kappa(kind, d2, param, dt):
    """(k, d k / d (d^2), d k(g x, g x') / dg at g = 1, d k / d param) of a distance kind at squared distances d2"""
    d2 = np.asarray(d2, dtype=dt)
    zero, one, two, half = dt(0), dt(1), dt(2), dt(1) / dt(2)
    if kind <= CONST:
        k, kp, dk = T.kappa(kind, d2, param, dt)
        return k, kp, dk, (np.ones_like(d2) if kind == CONST else np.zeros_like(d2))
    if kind == RQ:
        al = dt(param)
        u = d2 / (two * al)
        l = np.log1p(u)
        k = np.exp(-al * l)
        kp = -half * np.exp(-(al + one) * l)
        return k, kp, two * d2 * kp, k * (u / (one + u) - l)
    if kind == COSINE:
        pi = T._pi(dt)
        d = np.sqrt(d2)
        sn = np.sin(pi * d)
        safe = np.where(d > 0, d, one)
        return np.cos(pi * d), np.where(d > 0, -pi * sn / (two * safe), -half * pi * pi), -(pi * d) * sn, np.zeros_like(d2)
    if kind == GAMMAEXP:
        gm = dt(param)
        pos = d2 > 0
        safe = np.where(pos, d2, one)
        a = np.where(pos, np.power(safe, half * gm), zero)
        k = np.exp(-a)
        ak = a * k
        return (k, np.where(pos, -(half * gm) * ak / safe, zero), -gm * ak,
                np.where(pos, -half * (ak * np.log(safe)), zero))
    if kind == MATERN_NU:
        k, kx, dk = matern_nu_derivs(d2, param, dt)
        return k, kx, dk, np.zeros_like(d2)
    raise ValueError(kind)


def factor(kind, X, Y, param, dt, diag=False):
    """dict(k, kp, dk, dp) of one factor between the columns of X and Y (every pair, or with diag=True pair i with pair i);
    LINEAR: k = x'y + c, dk = 2 x'y, dp = 1, kp None (d k / d x = x')"""
    if kind == LINEAR:
        s = _dot(X, Y, diag)
        return dict(k=s + dt(param), kp=None, dk=dt(2) * s, dp=np.ones_like(s))
    k, kp, dk, dp = kappa(kind, _d2(X, Y, diag), param, dt)
    return dict(k=k, kp=kp, dk=dk, dp=dp)


def _product(ks, like):
    """the product of the arrays in chain order; of none: ones"""
    if not ks:
        return np.ones_like(like)
    p = ks[0]
    for k in ks[1:]:
        p = p * k
    return p


def _offsets(S):
    return (np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int), np.concatenate([[0], np.cumsum(S["col_len"])]).astype(int))


def _scale_vectors(ch, dt):
    return (None if ch["rs"] is None else ch["rs"].astype(dt), None if ch["cs"] is None else ch["cs"].astype(dt))


# ---- the covariance of a spec, its diagonal, and the contraction of a cotangent with its chains --------------------------------
def dense(S, dt):
    X_in = [a.astype(dt) for a in S["inputs"]]
    roff, coff = _offsets(S)
    K = np.zeros((roff[-1], coff[-1]), dtype=dt)
    for ch in S["chains"]:
        ks = [factor(kind, X_in[ri], X_in[ci], param, dt)["k"] for (_, kind, ri, ci, param) in ch["factors"]]
        blk = dt(ch["coef"]) * _product(ks, ks[0])
        rs, cs = _scale_vectors(ch, dt)
        if rs is not None:
            blk = rs[:, None] * blk
        if cs is not None:
            blk = blk * cs[None, :]
        K[roff[ch["I"]]:roff[ch["I"] + 1], coff[ch["J"]]:coff[ch["J"] + 1]] += blk
    return K


def diag_of(S, dt):
    """var_i = sum over the chains of the diagonal block pairs of coef rs_i cs_i prod_f k_f(xr^f_i, xc^f_i)"""
    X_in = [a.astype(dt) for a in S["inputs"]]
    roff, _ = _offsets(S)
    v = np.zeros(roff[-1], dtype=dt)
    for ch in S["chains"]:
        if ch["I"] != ch["J"]:
            continue
        ks = [factor(kind, X_in[ri], X_in[ci], param, dt, diag=True)["k"] for (_, kind, ri, ci, param) in ch["factors"]]
        rs, cs = _scale_vectors(ch, dt)
        v[roff[ch["I"]]:roff[ch["I"] + 1]] += dt(ch["coef"]) * _product(ks, ks[0]) * (1 if rs is None else rs) * (1 if cs is None else cs)
    return v


def contract(S, G, dt, inputs=False, scales=False):
    """sum_ij G_ij d K_ij / d theta for every term of S (the documented results of sgp_logpdf_grad_param_xs), each with the sum
    of the absolute values of its addends; the layout of grad_truth.contract plus d_param / S_param, one entry per term:
    d_coef on heads (continuations: exact 0), d_inscale and d_param on every factor.  Symmetric spec: the row side carries the
    factor 2 of the mirror block (LINEAR included: k(x, y) = k(y, x))."""
    X_in = [a.astype(dt) for a in S["inputs"]]
    sym = S["symmetric"]
    roff, coff = _offsets(S)
    nt = S["n_terms"]
    out = dict(n_rows=np.ones(nt, dt))
    for key in ("coef", "inscale", "param"):
        out["d_" + key], out["S_" + key] = np.zeros(nt, dt), np.zeros(nt, dt)
    if inputs:
        out["gx"] = [np.zeros(a.shape, dt) for a in X_in]
        out["Sn_gx"] = [np.zeros(a.shape, dt) for a in X_in]
    if scales:
        out["rowscale"], out["Sn_rowscale"] = [None] * nt, [None] * nt
        out["colscale"], out["Sn_colscale"] = [None] * nt, [None] * nt
    two = dt(2)
    side = two if sym else dt(1)
    for ch in S["chains"]:
        I, J, h, coef = ch["I"], ch["J"], ch["head"], dt(ch["coef"])
        rs, cs = _scale_vectors(ch, dt)
        fs = [factor(kind, X_in[ri], X_in[ci], param, dt) for (_, kind, ri, ci, param) in ch["factors"]]
        g = G[roff[I]:roff[I + 1], coff[J]:coff[J + 1]]
        nr, nc = g.shape
        w = g
        if rs is not None:
            w = w * rs[:, None]
        if cs is not None:
            w = w * cs[None, :]
        full = _product([f["k"] for f in fs], fs[0]["k"])
        a = w * full
        out["d_coef"][h], out["S_coef"][h] = a.sum(), np.abs(a).sum()
        wc = coef * w
        for ia, (t, kind, ri, ci, param) in enumerate(ch["factors"]):
            out["n_rows"][t] = max(nr, 1)
            A = wc * _product([f["k"] for ib, f in enumerate(fs) if ib != ia], fs[0]["k"])
            for key, q in (("inscale", fs[ia]["dk"]), ("param", fs[ia]["dp"])):
                a = A * q
                out["d_" + key][t], out["S_" + key][t] = a.sum(), np.abs(a).sum()
            if not inputs:
                continue
            X, Y = X_in[ri], X_in[ci]
            if kind == LINEAR:
                absA = np.abs(A)
                for d in range(X.shape[0]):
                    c = side * A * Y[d][None, :]
                    out["gx"][ri][d] += c.sum(1)
                    out["Sn_gx"][ri][d] += (side * absA * np.abs(Y[d])[None, :]).sum(1) / max(nc, 1)
                    if not sym:
                        c = A * X[d][:, None]
                        out["gx"][ci][d] += c.sum(0)
                        out["Sn_gx"][ci][d] += (absA * np.abs(X[d])[:, None]).sum(0) / max(nr, 1)
                continue
            core = side * two * (A * fs[ia]["kp"])
            acore = np.abs(core)
            for d in range(X.shape[0]):
                df = X[d][:, None] - Y[d][None, :]
                c = core * df
                ac = acore * np.abs(df)
                out["gx"][ri][d] += c.sum(1)
                out["Sn_gx"][ri][d] += ac.sum(1) / max(nc, 1)
                if not sym:
                    out["gx"][ci][d] -= c.sum(0)
                    out["Sn_gx"][ci][d] += ac.sum(0) / max(nr, 1)
        if scales:
            base = coef * g * full
            if rs is not None:
                wcs = base if cs is None else base * cs[None, :]
                out["rowscale"][h] = side * wcs.sum(1)
                out["Sn_rowscale"][h] = side * np.abs(wcs).sum(1) / max(nc, 1)
            if cs is not None and not sym:
                wrs = base if rs is None else base * rs[:, None]
                out["colscale"][h] = wrs.sum(0)
                out["Sn_colscale"][h] = np.abs(wrs).sum(0) / max(nr, 1)
    return out


# ---- logpdf, the ELBO and their gradients: grad_truth's, with the three functions above --------------------------------------------
class _Ops:
    dense, diag_of = staticmethod(dense), staticmethod(diag_of)

    @staticmethod
    def contract(S, G, dt, inputs=False, scales=True):
        return contract(S, G, dt, inputs=inputs, scales=scales)


def logpdf_grad(S, noise_kind, noise, mean, y, dt, inputs=False, scales=False, cholesky=None):
    """sgp_logpdf_grad_param_xs as documented, in dtype dt (grad_truth.logpdf_grad on this module's chains)"""
    return T.logpdf_grad(S, noise_kind, noise, mean, y, dt, inputs=inputs, scales=scales, cholesky=cholesky, ops=_Ops)


def elbo_grad(Szz, Sxz, Sxx, noise_kind, noise, z_noise_kind, z_noise, mean, y, dt, inputs=False, cholesky=None):
    """sgp_elbo_grad_param as documented, in dtype dt: grad_truth.elbo_grad's cotangents contracted with the chains of zz and
    xz (row / column scale sums included), and `xx`: the diagonal's gradients under w = d elbo / d var"""
    R = T.elbo_grad(Szz, Sxz, Sxx, noise_kind, noise, z_noise_kind, z_noise, mean, y, dt, inputs=inputs, cholesky=cholesky,
                    ops=_Ops)
    R["xx"] = diag_grad(Sxx, np.asarray(R["var"], dtype=np.float64), dt)
    return R


# ---- sgp_kernelmatrix_diag_grad_param with the caller's w ----------------------------------------------------------------------
def _amp(kind, param, f, X, Y, dt):
    """amp_f of the module docstring for one factor over the diagonal's entries, as a float"""
    D = X.shape[0]
    if kind in (CONST, WHITE):
        return 0.0
    if kind == LINEAR:
        return D + 1.0
    d2 = _d2(X, Y, True).astype(np.float64)
    d = np.sqrt(d2)
    if kind == SE:
        model, arg = np.full(d2.shape, 4.0), d2 / 2.0
    elif kind in (MATERN12, MATERN32, MATERN52):
        arg = np.sqrt({MATERN12: 1.0, MATERN32: 3.0, MATERN52: 5.0}[kind]) * d
        model = 2.0 * (6.0 + 4.0 * arg) + 8.0
    elif kind == RQ:
        arg = param * np.log1p(d2 / (2.0 * param))
        model = 2.0 * (2.0 + 7.0 * arg) + 8.0
    elif kind == COSINE:
        arg = np.pi * d
        model = 6.0 + arg + 4.0
    elif kind == GAMMAEXP:
        arg = np.power(d2, 0.5 * param)
        model = 2.0 * (2.0 + 32.0 * arg) + 8.0 + 6.0
    else:
        arg = math.sqrt(2.0 * param) * d
        model = 128.0 + 8.0 + 4.0 * arg + 3.0 * (0 if param < 0.5 else math.floor(param + 0.5))
    return float(np.max(model + (D + 2.0) * np.maximum(1.0, arg), initial=0.0))


def _magnitudes(kind, param, f, X, Y, dt):
    """(|k|, |kp|, |dk|, |dp|) of a factor as the error models count them: COSINE against 1, pi^2 / 2 and pi d, LINEAR against
    sum_d |x_d y_d| + |c|"""
    if kind == COSINE:
        d = np.sqrt(_d2(X, Y, True))
        pi = T._pi(dt)
        return np.ones_like(d), np.full_like(d, pi * pi / dt(2)), pi * d, np.zeros_like(d)
    if kind == LINEAR:
        s = _dot(np.abs(X), np.abs(Y), True)
        return s + abs(dt(param)), None, dt(2) * s, np.ones_like(s)
    return np.abs(f["k"]), np.abs(f["kp"]), np.abs(f["dk"]), np.abs(f["dp"])


def diag_grad(S, w, dt):
    """per chain of the diagonal block pairs, with W_i = w_i coef rs_i cs_i and E^f_i = prod_{f' != f} k_f'(xr_i, xc_i):
    d_coef[h] = sum_i w_i rs_i cs_i prod_f k_f, d_inscale[f] = sum_i W_i E^f_i dk_f / dg, d_param[f] likewise,
    gx[row_input(f)] += 2 W E^f kappa'_f (xr - xc), gx[col_input(f)] -= the same (LINEAR: the row input gets W E^f xc, the column
    input W E^f xr), rowscale[h]_i = w_i coef cs_i prod_f k_f, colscale[h]_i = w_i coef rs_i prod_f k_f.
    Every sum and entry X with S_X (absolute addends) and Sm_X (the same with the magnitudes of the module docstring);
    `amp`: sum_f amp_f per term's chain; terms of other block pairs: exact zeros (`diagonal` False)."""
    X_in = [a.astype(dt) for a in S["inputs"]]
    roff, _ = _offsets(S)
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
        rs, cs = _scale_vectors(ch, dt)
        rsv, csv = (1 if rs is None else rs), (1 if cs is None else cs)
        fs, mags, amp, dim = [], [], 0.0, 0
        for (t, kind, ri, ci, param) in ch["factors"]:
            f = factor(kind, X_in[ri], X_in[ci], param, dt, diag=True)
            fs.append(f)
            mags.append(_magnitudes(kind, param, f, X_in[ri], X_in[ci], dt))
            amp += _amp(kind, param, f, X_in[ri], X_in[ci], dt)
            dim = max(dim, X_in[ri].shape[0])
        wb = w[roff[I]:roff[I + 1]]
        ww = wb * rsv * csv
        full = _product([f["k"] for f in fs], fs[0]["k"])
        mfull = _product([m[0] for m in mags], mags[0][0])
        out["d_coef"][h], out["S_coef"][h], out["Sm_coef"][h] = (ww * full).sum(), np.abs(ww * full).sum(), (np.abs(ww) * mfull).sum()
        if rs is not None:
            out["rowscale"][h], out["Sm_rowscale"][h] = wb * coef * csv * full, np.abs(wb * coef * csv) * mfull
        if cs is not None:
            out["colscale"][h], out["Sm_colscale"][h] = wb * coef * rsv * full, np.abs(wb * coef * rsv) * mfull
        for ia, (t, kind, ri, ci, param) in enumerate(ch["factors"]):
            out["diagonal"][t], out["amp"][t], out["dim"][t] = True, amp, dim
            A = coef * ww * _product([f["k"] for ib, f in enumerate(fs) if ib != ia], fs[0]["k"])
            mA = np.abs(coef * ww) * _product([m[0] for ib, m in enumerate(mags) if ib != ia], mags[0][0])
            for key, q, mq in (("inscale", fs[ia]["dk"], mags[ia][2]), ("param", fs[ia]["dp"], mags[ia][3])):
                out["d_" + key][t], out["S_" + key][t], out["Sm_" + key][t] = (A * q).sum(), np.abs(A * q).sum(), (mA * mq).sum()
            X, Y = X_in[ri], X_in[ci]
            for k in (ri, ci):
                out["amp_gx"][k] = max(out["amp_gx"][k], amp + dim)
            if kind == LINEAR:
                out["gx"][ri] += A[None, :] * Y
                out["gx"][ci] += A[None, :] * X
                for k, other in ((ri, Y), (ci, X)):
                    out["S_gx"][k] += np.abs(A)[None, :] * np.abs(other)
                    out["Sm_gx"][k] += mA[None, :] * np.abs(other)
                continue
            core = dt(2) * (A * fs[ia]["kp"])[None, :] * (X - Y)
            out["gx"][ri] += core
            out["gx"][ci] -= core
            for k in (ri, ci):
                out["S_gx"][k] += np.abs(core)
                out["Sm_gx"][k] += dt(2) * (mA * mags[ia][1])[None, :] * np.abs(X - Y)
    return out


# ---- units per output family ----------------------------------------------------------------------------------------------------
def _max_units(pairs):
    u = 0.0
    for a, e, s in pairs:
        if e is None:
            assert a is None
            continue
        assert a is not None and np.shape(a) == np.shape(e), (np.shape(a), np.shape(e))
        u = max(u, units(a, e, scale_entries(e, s)))
    return u


def _term_units(o, r, u, prefix):
    for key in ("coef", "inscale", "param"):
        assert len(o["d_" + key]) == len(r["d_" + key])
        fam = f"{prefix}.d_{key}"
        u[fam] = max(u.get(fam, 0.0), units(o["d_" + key], r["d_" + key], scale_scalar(r["d_" + key], r["S_" + key], r["n_rows"])))
    if r.get("gx") is not None and o.get("gx") is not None:
        assert len(o["gx"]) == len(r["gx"])
        u[prefix + ".inputs"] = max(u.get(prefix + ".inputs", 0.0), _max_units(zip(o["gx"], r["gx"], r["Sn_gx"])))
    for side in ("rowscale", "colscale"):
        if r.get(side) is not None and o.get(side) is not None and any(e is not None for e in r[side]):
            assert len(o[side]) >= len(r[side])
            u[prefix + ".scales"] = max(u.get(prefix + ".scales", 0.0), _max_units(zip(o[side], r[side], r["Sn_" + side])))


def logpdf_units(out, R):
    """largest error of each output family of a logpdf case against the truth R, in units.  out: value, y, mean, noise,
    d_coef, d_inscale, d_param, gx (or None), rowscale (or None)"""
    n = R["n"]
    u = {"kp.value": units(out["value"], R["value"], scale_scalar(R["value"], R["S_value"], n))}
    sc = scale_entries(R["alpha"], R["S_alpha"] / n)
    u["kp.y"] = max(units(out["y"], -R["alpha"], sc), units(out["mean"], R["alpha"], sc))
    u["kp.noise"] = units(out["noise"], R["noise"], scale_scalar(R["noise"], R["S_noise"], n))
    _term_units(out, R, u, "kp")
    return u


def logpdf_reference_outputs(R):
    return dict(value=R["value"], y=-R["alpha"], mean=R["alpha"], noise=R["noise"], d_coef=R["d_coef"], d_inscale=R["d_inscale"],
                d_param=R["d_param"], gx=R.get("gx"), rowscale=R.get("rowscale"))


def elbo_units(out, R):
    """the same for an ELBO case.  out: value, y, mean, noise, z_noise, zz / xz = dict(d_coef, d_inscale, d_param, gx,
    rowscale, colscale)"""
    n, m = R["n"], R["m"]
    u = {"kpelbo.value": units(out["value"], R["value"], scale_scalar(R["value"], R["S_value"], n))}
    sc = scale_entries(R["y"], R["S_y"] / m)
    u["kpelbo.y"] = max(units(out["y"], R["y"], sc), units(out["mean"], -R["y"], sc))
    for key, cnt in (("noise", n), ("z_noise", m)):
        if np.ndim(R[key]) == 0:
            u["kpelbo." + key] = units(out[key], R[key], scale_scalar(R[key], R["S_" + key], cnt))
        else:
            assert np.shape(out[key]) == np.shape(R[key])
            u["kpelbo." + key] = units(out[key], R[key], scale_entries(R[key], R["S_" + key]))
    for key in ("zz", "xz"):
        _term_units(out[key], R[key], u, "kpelbo")
    return u


def elbo_reference_outputs(R):
    return dict(value=R["value"], y=R["y"], mean=-R["y"], noise=R["noise"], z_noise=R["z_noise"], var=R["var"],
                zz=R["zz"], xz=R["xz"], xx=R["xx"])


def diag_model_figures(o, r, with_inputs=True):
    """error / ((D + 8 + sum_f amp_f) eps Sm) of every sum and entry of a diagonal case, as {family: largest figure}; asserts
    the exact zeros (terms of off-diagonal pairs; entries nothing contributes to)"""
    off = ~r["diagonal"]
    fig = {}
    bound = (r["dim"] + 8.0 + r["amp"]) * EPS
    for key in ("coef", "inscale", "param"):
        got, want, Sm = np.asarray(o["d_" + key], dtype=r["d_" + key].dtype), r["d_" + key], r["Sm_" + key]
        assert len(got) == len(want) and np.all(got[off] == 0.0), key
        assert np.all(got[Sm == 0] == 0.0), key
        fig["kpdiag.d_" + key] = float(np.max(np.abs(got - want) / np.where(Sm > 0, bound * Sm, 1.0), initial=0.0))
    if with_inputs:
        assert len(o["gx"]) == len(r["gx"])
        fig["kpdiag.inputs"] = 0.0
        for a, e, s, amp in zip(o["gx"], r["gx"], r["Sm_gx"], r["amp_gx"]):
            assert np.shape(a) == e.shape and not np.any(np.isnan(a))
            assert np.all(np.asarray(a)[s == 0] == 0.0)
            fig["kpdiag.inputs"] = max(fig["kpdiag.inputs"],
                                       float(np.max(np.abs(a - e) / np.where(s > 0, (8.0 + amp) * EPS * s, 1.0), initial=0.0)))
    for side in ("rowscale", "colscale"):
        if o.get(side) is None:
            continue
        for t, (e, s) in enumerate(zip(r[side], r["Sm_" + side])):
            if e is None:
                continue
            a = o[side][t]
            assert a is not None and np.shape(a) == e.shape
            b = (r["dim"][t] + 8.0 + r["amp"][t]) * EPS
            fig["kpdiag.scales"] = max(fig.get("kpdiag.scales", 0.0),
                                       float(np.max(np.abs(a - e) / np.where(s > 0, b * s, 1.0), initial=0.0)))
    return fig
