"""NumPy (float64) formulas of the Cosine and GammaExponential kinds (csrc/kprod.hip: cosine_eval / cosine_derivs, gexp_eval /
gexp_derivs) and the evaluators of tests/kprod_np.py and tests/kprod_grad_np.py extended to them.  TEST INFRASTRUCTURE ONLY
(tests/test_kinds_on_numpy.py holds the formulas to the 60-digit table; tests/test_gpu_kinds.py holds the library to them).

Importing this module makes kprod_np.factor and kprod_grad_np.kappa_prime know kinds 16 and 17: the two evaluators look their
per-kind formulas up by those names, and every other kind is passed on to the original definition untouched, so np_spec_matrix,
np_contract, np_input_grads and np_diag_grads take specs with the new kinds as they are."""
import numpy as np

import kprod_grad_np as kg
import kprod_np as kn
from stheno_jl_amd import lib as L

PI = np.pi


def _reduced(d2):
    """(d, r): d = sqrt(d2) and r = remainder(d, 2) in [-1, 1] (exact), 0 where d2 overflowed"""
    d2 = np.asarray(d2, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(d2)
        fin = np.isfinite(d)
        return d, np.where(fin, np.remainder(np.where(fin, d, 0.0), 2.0), 0.0), fin


def cosine(d2):
    """cos(pi d) with the argument reduced first; exactly 1 where d2 overflowed"""
    _, r, _ = _reduced(d2)
    return np.cos(PI * r)


def cosine_dscale(d2):
    """d k(g x, g y) / dg at g = 1 = -pi d sin(pi d); 0 where d2 overflowed"""
    d, r, fin = _reduced(d2)
    return np.where(fin, -(PI * np.where(fin, d, 0.0)) * np.sin(PI * r), 0.0)


def cosine_dd2(d2):
    """d k / d (d2) = -pi sin(pi d) / (2 d); its limit -pi^2 / 2 at d = 0; 0 where d2 overflowed"""
    d, r, fin = _reduced(d2)
    pos = fin & (d > 0.0)
    return np.where(pos, -PI * np.sin(PI * r) / (2.0 * np.where(pos, d, 1.0)), np.where(fin, -0.5 * PI * PI, 0.0))


def _gexp_a_k(d2, gamma):
    d2 = np.asarray(d2, dtype=np.float64)
    with np.errstate(over="ignore"):
        a = np.power(d2, 0.5 * gamma)
        return d2, a, np.exp(-a)


def gammaexp(d2, gamma):
    """exp(-d2^(gamma / 2)) through pow, as the library forms it"""
    return _gexp_a_k(d2, gamma)[2]


def _gexp_live(d2, k):
    return (k != 0.0) & (d2 > 0.0)


def gammaexp_dscale(d2, gamma):
    """-gamma a k; 0 where k is"""
    d2, a, k = _gexp_a_k(d2, gamma)
    live = _gexp_live(d2, k)
    return np.where(live, -gamma * (np.where(live, a, 0.0) * k), 0.0)


def gammaexp_dd2(d2, gamma):
    """-(gamma / 2) a k / d2; 0 at coincident points (the subgradient) and where k is 0"""
    d2, a, k = _gexp_a_k(d2, gamma)
    live = _gexp_live(d2, k)
    with np.errstate(over="ignore"):
        return np.where(live, -(0.5 * gamma) * (np.where(live, a, 0.0) * k) / np.where(live, d2, 1.0), 0.0)


def gammaexp_dparam(d2, gamma):
    """d k / d gamma = -k a log(d2) / 2; 0 at d2 = 0 (the limit) and where k is 0"""
    d2, a, k = _gexp_a_k(d2, gamma)
    live = _gexp_live(d2, k)
    return np.where(live, -0.5 * ((np.where(live, a, 0.0) * k) * np.log(np.where(live, d2, 1.0))), 0.0)


_factor_before, _kappa_prime_before = kn.factor, kg.kappa_prime


def _sq_dists(Xr, Xc):
    with np.errstate(over="ignore"):
        return ((Xr[:, :, None] - Xc[:, None, :]) ** 2).sum(0)


def factor(kind, Xr, Xc, param):
    """kprod_np.factor with the two kinds: (k, d k / d inscale, d k / d param)"""
    code = int(kind) & L.KIND_MASK
    if code == L.COSINE:
        d2 = _sq_dists(Xr, Xc)
        return cosine(d2), cosine_dscale(d2), np.zeros_like(d2)
    if code == L.GAMMAEXP:
        d2 = _sq_dists(Xr, Xc)
        return gammaexp(d2, param), gammaexp_dscale(d2, param), gammaexp_dparam(d2, param)
    return _factor_before(kind, Xr, Xc, param)


def kappa_prime(kind, d2, param):
    """kprod_grad_np.kappa_prime with the two kinds"""
    code = int(kind) & L.KIND_MASK
    if code == L.COSINE:
        return cosine_dd2(d2)
    if code == L.GAMMAEXP:
        return gammaexp_dd2(d2, param)
    return _kappa_prime_before(kind, d2, param)


if kn.factor is not factor and getattr(kn.factor, "__module__", "") != __name__:
    kn.factor, kg.kappa_prime = factor, kappa_prime


# ---- entrywise tolerance of a spec's matrix between two float64 evaluations that follow the documented formulas ------------
def factor_abs_bound(kind, Xr, Xc, param):
    """(|k|, e): e = the absolute bound of ONE evaluation of a factor on |k - truth| per entry: the kind's error model
    (tests/kinds_truth.py, tests/kprod_truth.py, tests/kernel_truth.py) at the entry's d2, plus what the roundings of d2
    itself (a sum of D squares: (D + 2) eps relative) do through |d k / d (d2)| d2.  LINEAR: a dot product of D terms,
    (D + 1) eps sum |x_d y_d|.  WHITE and CONST are exact."""
    import kernel_truth as kt0
    import kinds_truth as kt
    import kprod_truth as kpt
    code = int(kind) & L.KIND_MASK
    D = Xr.shape[0]
    if code == L.LINEAR:
        s = Xr.T @ Xc + param
        return np.abs(s), (D + 1) * kt.EPS * (np.abs(Xr).T @ np.abs(Xc) + abs(param))
    d2 = _sq_dists(Xr, Xc)
    k = factor(kind, Xr, Xc, param)[0]
    if code in (L.WHITE, L.CONST):
        return np.abs(k), np.zeros_like(k)
    with np.errstate(over="ignore", invalid="ignore"):
        if code == L.COSINE:
            d, r, _ = _reduced(d2)
            model = kt._cos_bound_units(d, np.sin(PI * r), kt.C0) * kt.EPS
        elif code == L.GAMMAEXP:
            model = (2.0 + kt.C_POW * np.power(d2, 0.5 * param)) * np.spacing(k)
        elif code == L.RQ:
            model = kpt.bound_ulps(param, d2) * np.spacing(k)
        else:
            name = {L.SE: "se", L.MATERN12: "matern12", L.MATERN32: "matern32", L.MATERN52: "matern52"}[code]
            model = kt0.bound_ulps(name, d2, np.spacing(k)) * np.spacing(k)
        model = np.where(np.isfinite(model), model, 0.0)             # (an overflowed argument: both sides are exact zeros)
        slope = np.abs(kappa_prime(kind, d2, param)) * np.where(np.isfinite(d2), d2, 0.0)
        slope = np.where(np.isfinite(slope), slope, 0.0)
    return np.abs(k), model + (D + 2) * kt.EPS * slope


def np_spec_tolerance(spec, sides=2):
    """entrywise bound on the difference between `sides` evaluations of the spec's matrix (the library's and np_spec_matrix:
    2): per chain |coef rs cs| (prod_f (|k_f| + e_f) - prod_f |k_f|), e_f = factor_abs_bound, plus one rounding per product
    and per accumulation of the chain"""
    import kinds_truth as kt
    T = np.zeros((spec.N, spec.M))
    roff = np.concatenate([[0], np.cumsum(spec.row_len)])
    coff = np.concatenate([[0], np.cumsum(spec.col_len)])
    for I, J, ts in kn.chains(spec):
        mag, up = 1.0, 1.0
        for t in ts:
            Tm = spec._terms[t]
            a, e = factor_abs_bound(Tm.kind, np.asarray(spec.inputs[Tm.row_input]), np.asarray(spec.inputs[Tm.col_input]), Tm.param)
            mag, up = mag * a, up * (a + e)
        coef, rs, cs = kn._weights(spec, ts[0])
        w = np.abs(coef * rs * cs)
        T[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += w * ((up - mag) + (len(ts) + 4) * kt.EPS * up)
    return sides * T
