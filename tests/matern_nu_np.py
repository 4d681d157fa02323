"""NumPy (float64) restatement of the general-nu Matern routine of csrc/kprod.hip (matern_nu_derivs) and of the per-term
constants csrc/capi.hip computes when a spec is uploaded (matern_nu_constants), operation for operation.  TEST
INFRASTRUCTURE ONLY: tests/test_matern_nu_on_numpy.py holds it to the 60-digit table within half the bound of
tests/matern_nu_truth.py, tests/test_gpu_matern_nu.py holds the library to the same table and uses it as the evaluator's
formula for kind 20.

    k(d2) = C x^nu K_nu(x),   x = sqrt(2 nu) sqrt(d2),   C = 2^(1 - nu) / Gamma(nu)

nu = mu + n, n = floor(nu + 1/2) >= 1, mu in [-1/2, 1/2); for nu < 1/2 the routine takes mu = -nu and n = 0 instead (K is
even in its order, so the pair (K_mu, K_(mu+1)) it starts from is (K_nu, K_(nu-1)): the value and what the derivative needs,
without the cancelling downward step).  Everything is carried as
    Q_j = (x / 2)^mu x^j K_(mu+j)(x)      (x <= 2)          Q_j = the same times e^x      (x > 2)
so that the powers of x that K_(mu+j) ~ x^-(mu+j) brings at small x and the e^-x it brings at large x never meet an
overflow or an underflow: Q_0 and Q_1 come from Temme's series (x <= 2) or Steed's second continued fraction (x > 2), Q_n
from the upward recurrence Q_(j+1) = x^2 Q_(j-1) + 2 (mu + j) Q_j, and
    k = ca Q_n [e^-x],   kx = dk / d(d2) = -nu ca Q_(n-1) [e^-x],   dk = 2 d2 kx,   ca = 2^(1-n) / Gamma(nu)
(nu < 1/2:  k = ca Q_0 / E,  kx = -nu ca Q_1 / (E x^2),  E = (x / 2)^(2 mu)).
"""
import math

import numpy as np

NU_MAX = 32.0
EPS = 2.0 ** -53
X_SPLIT = 2.0            # Temme's series up to here, the continued fraction beyond
X_ZERO = 1000.0          # C x^nu K_nu(x) < 2^-1076 for every nu <= 32 from here on (nu = 32: 1e-384)
X_EXP_SPLIT = 600.0      # beyond it e^-x is applied as e^-600 e^-(x - 600): e^-x alone is subnormal from 708 on while
E600 = 2.6503965530043108e-261   # the product with x^nu still is a normal number
TEMME_MAXIT = 30
CF2_MAXIT = 200
HALF_PI = 1.5707963267948966

# Taylor coefficients of 1 / Gamma(1 + z) at 0 (Abramowitz & Stegun 6.1.34, here to 20 digits)
RGAMMA = (1.0, 0.57721566490153286061, -0.65587807152025388108, -0.042002635034095235529, 0.1665386113822914895,
          -0.042197734555544336748, -0.0096219715278769735621, 0.0072189432466630995424, -0.0011651675918590651121,
          -0.00021524167411495097282, 0.00012805028238811618615, -0.000020134854780788238656, -1.2504934821426706573e-6,
          1.1330272319816958824e-6, -2.0563384169776071035e-7, 6.1160951044814158179e-9, 5.0020076444692229301e-9,
          -1.1812745704870201446e-9, 1.0434267116911005105e-10, 7.782263439905071254e-12, -3.6968056186422057082e-12,
          5.100370287454475979e-13, -2.0583260535665067832e-14, -5.3481225394230179824e-15, 1.2267786282382607902e-15,
          -1.1812593016974587695e-16, 1.1866922547516003326e-18, 1.4123806553180317816e-18)


def constants(nu):
    """what depends on nu alone (csrc/capi.hip: matern_nu_constants)"""
    nu = float(nu)
    if not (0.0 < nu <= NU_MAX):
        raise ValueError("nu must be finite and in (0, 32]")
    n = 0 if nu < 0.5 else int(math.floor(nu + 0.5))
    mu = -nu if n == 0 else nu - n          # exact
    m2 = mu * mu
    g1 = g2 = 0.0
    for j in range(13, -1, -1):             # Horner in mu^2: Gamma_2 the even part, Gamma_1 minus the odd part over mu
        g2 = g2 * m2 + RGAMMA[2 * j]
        g1 = g1 * m2 - RGAMMA[2 * j + 1]
    gampl, gammi = g2 - mu * g1, g2 + mu * g1      # 1 / Gamma(1 + mu), 1 / Gamma(1 - mu)
    fact = 1.0 if mu == 0.0 else (math.pi * mu) / math.sin(math.pi * mu)
    ca = 2.0 ** (1 - n) / math.gamma(nu)
    return dict(nu=nu, n=n, mu=mu, fact=fact, gam1=g1, gam2=g2, ph=0.5 / gampl, qh=0.5 / gammi, a1=(0.5 - mu) * (0.5 + mu), ca=ca,
                ck=nu * ca, sq=math.sqrt(2.0 * nu), kx0=(-nu / (2.0 * (nu - 1.0)) if nu > 1.0 else 0.0))


def _temme(c, x):
    """(Q0, Q1, E, iterations) for 0 < x <= 2"""
    mu, m2 = c["mu"], c["mu"] * c["mu"]
    xh = 0.5 * x
    dl = -np.log(xh)
    E = np.power(xh, 2.0 * mu)
    g = -(2.0 * mu) * dl
    small = np.abs(g) < 1.0
    gs = np.where(small & (g != 0.0), g, 1.0)
    t2 = np.where(small, np.where(g != 0.0, np.expm1(gs) / gs, 1.0) * dl, (1.0 - E) / (2.0 * mu if mu != 0.0 else 1.0))
    ff = c["fact"] * (c["gam1"] * (0.5 * (1.0 + E)) + c["gam2"] * t2)
    p = np.full(x.shape, c["ph"])
    q = c["qh"] * E
    s0, s1, cc, dd = ff.copy(), p.copy(), np.ones(x.shape), xh * xh
    live = np.ones(x.shape, dtype=bool)
    its = np.zeros(x.shape, dtype=int)
    for i in range(1, TEMME_MAXIT + 1):
        ff = (i * ff + p + q) / (i * i - m2)
        cc = cc * (dd / i)
        p = p / (i - mu)
        q = q / (i + mu)
        de0 = cc * ff
        de1 = cc * (p - i * ff)
        s0 = np.where(live, s0 + de0, s0)
        s1 = np.where(live, s1 + de1, s1)
        its += live
        live = live & ~((np.abs(de0) < np.abs(s0) * EPS) & (np.abs(de1) < np.abs(s1) * EPS))
        if not live.any():
            break
    return s0, 2.0 * s1, E, its


def _cf2(c, x):
    """(Q0, Q1, E, iterations) for x > 2, all times e^x"""
    mu, a1 = c["mu"], c["a1"]
    b = 2.0 * (1.0 + x)
    d = 1.0 / b
    h = d.copy()
    delh = d.copy()
    q1, q2 = np.zeros(x.shape), np.ones(x.shape)
    q = np.full(x.shape, a1)
    cc = np.full(x.shape, a1)
    a = np.full(x.shape, -a1)
    s = 1.0 + q * delh
    live = np.full(x.shape, a1 != 0.0)          # (mu = -1/2: the fraction is 1, K_(1/2) is its closed form)
    its = np.zeros(x.shape, dtype=int)
    for i in range(2, CF2_MAXIT + 1):
        if not live.any():
            break
        a = a - 2.0 * (i - 1)
        cc = -a * cc / i
        qn = (q1 - b * q2) / a
        q1, q2 = q2, qn
        q = q + cc * qn
        b = b + 2.0
        dn = 1.0 / (b + a * d)
        delh = (-a * d * dn) * delh
        d = dn
        h = np.where(live, h + delh, h)
        dels = q * delh
        s = np.where(live, s + dels, s)
        its += live
        live = live & ~(np.abs(dels) < np.abs(s) * EPS)
    h = a1 * h
    ks0 = np.sqrt(HALF_PI / x) / s
    w = np.power(0.5 * x, mu)
    q0 = w * ks0
    return q0, q0 * (mu + x + 0.5 - h), w * w, its


def derivs(d2, nu, want_iterations=False):
    """(k, dk, kx) at squared distances d2: the value, d k(g x, g y) / dg at g = 1, and dk / d(d2)"""
    c = constants(nu) if not isinstance(nu, dict) else nu
    nu, n = c["nu"], c["n"]
    d2 = np.asarray(d2, dtype=np.float64)
    shape = d2.shape
    d2 = d2.ravel()
    k, kx = np.zeros(d2.shape), np.zeros(d2.shape)
    its = np.zeros(d2.shape, dtype=int)
    zero = ~(d2 > 0.0)
    k[zero], kx[zero] = 1.0, c["kx0"]
    with np.errstate(over="ignore", invalid="ignore"):
        x = c["sq"] * np.sqrt(d2)
    for lo in (True, False):
        m = ~zero & (x < X_ZERO) & ((x <= X_SPLIT) if lo else (x > X_SPLIT))
        if not m.any():
            continue
        xm = x[m]
        qa, qb, E, it = (_temme if lo else _cf2)(c, xm)
        if n == 0:
            tk = c["ca"] * (qa / E)
            tx = c["ck"] * ((qb / (xm * E)) / xm)
        else:
            x2 = xm * xm
            for j in range(1, n):
                qa, qb = qb, x2 * qa + (2.0 * (nu - (n - j))) * qb
            tk, tx = c["ca"] * qb, c["ck"] * qa
        if not lo:
            far = xm > X_EXP_SPLIT
            tk, tx = np.where(far, tk * E600, tk), np.where(far, tx * E600, tx)
            ex = np.exp(-np.where(far, xm - X_EXP_SPLIT, xm))
            tk, tx = tk * ex, tx * ex
        tk = np.minimum(tk, 1.0)
        k[m], kx[m], its[m] = tk, np.where(tk == 0.0, 0.0, -tx), it
    with np.errstate(over="ignore", invalid="ignore"):
        dk = np.where(kx == 0.0, 0.0, 2.0 * d2 * kx)
    out = (k.reshape(shape), dk.reshape(shape), kx.reshape(shape))
    return out + (its.reshape(shape),) if want_iterations else out


def matern_nu(d2, nu):
    return derivs(d2, nu)[0]


def matern_nu_dscale(d2, nu):
    return derivs(d2, nu)[1]


def matern_nu_dd2(d2, nu):
    return derivs(d2, nu)[2]


# ---- the evaluators of tests/kprod_np.py and tests/kprod_grad_np.py extended to kind 20 ------------------------------------
MATERN_NU = 20


def _sq_dists(Xr, Xc):
    with np.errstate(over="ignore"):
        return ((Xr[:, :, None] - Xc[:, None, :]) ** 2).sum(0)


def extended_factor(before):
    """kprod_np.factor with kind 20 in front of `before`: (k, d k / d inscale, d k / d param = 0)"""
    def factor(kind, Xr, Xc, param):
        if int(kind) & 0xff == MATERN_NU:
            k, dk, _ = derivs(_sq_dists(Xr, Xc), param)
            return k, dk, np.zeros_like(k)
        return before(kind, Xr, Xc, param)
    return factor


def extended_kappa_prime(before):
    """kprod_grad_np.kappa_prime with kind 20 in front of `before`"""
    def kappa_prime(kind, d2, param):
        if int(kind) & 0xff == MATERN_NU:
            return derivs(d2, param)[2]
        return before(kind, d2, param)
    return kappa_prime


def install(monkeypatch):
    """make np_spec_matrix, np_contract, np_input_grads and np_diag_grads take specs with kind 20 for one test"""
    import kinds_np  # noqa: F401  (installs kinds 16 and 17 first)
    import kprod_grad_np as kg
    import kprod_np as kn
    monkeypatch.setattr(kn, "factor", extended_factor(kn.factor))
    monkeypatch.setattr(kg, "kappa_prime", extended_kappa_prime(kg.kappa_prime))
