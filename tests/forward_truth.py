"""Extended-precision truth for the forward posterior path: posterior moments, samples and updates (include/sthenomi.h:
sgp_posterior_create / _predict / _predict_explicit, sgp_rand, sgp_elbo, sgp_sparse_posterior_create / _predict;
include/sthenomi_extend.h: sgp_posterior_extend; include/sthenomi_vfe_update.h: sgp_sparse_posterior_update).

TEST INFRASTRUCTURE ONLY.  A dtype-generic restatement on top of tests/grad_truth.py (kernels, distances, Cholesky
recurrences, units) and tests/predgrad_truth.py (exact_core / sparse_core: the one computation of L^-1, alpha, Lz^-1, Le^-1
both modules share): run in np.longdouble it is the truth, run in np.float64 -- once with the column recurrence, once with
the factor taken in LAPACK's blocked order -- it is the yardstick.  Nothing here comes from np_capi.py, oracle/ or the
product.

  post.alpha    alpha = C^-1 (y - m), C = K + Sigma_y = L L'                               (sgp_posterior_create: alpha_out)
  post.mean     m*_i + sum_j K*_ij alpha_j                                                  (sgp_posterior_predict: mean_out)
  post.var      k**_ii - sum_j V_ji^2, V = L^-1 K*'; S = |k**_ii| + sum_j V_ji^2             (var_out)
  post.cov      K** - V' V, entry by entry; S = |K**| + |V|' |V|                             (cov_out)
  post.logpdf_y -1/2 (n log 2 pi + 2 sum log L_ii + |L^-1 (y - m)|^2)                       (sgp_posterior_extend: logpdf_out)
  spost.mean    m* + K*z alpha, alpha = Lz^-T Le^-T u                                        (sgp_sparse_posterior_predict)
  spost.var     k** - sum B'^2 + sum C'^2, B' = K*z Lz^-T, C' = B' Le^-T; S = |k**| + sum B'^2 + sum C'^2
  spost.cov     K** - B' B'' + C' C''; S = |K**| + |B'| |B'|' + |C'| |C'|'
  spost.elbo    -1/2 (n log 2 pi + sum log s2 + 2 sum log Le_ii + |delta|^2 - |Le^-1 A delta|^2 + sum var / s2 - |A|_F^2)
                                                                                             (sgp_elbo)
  rand          m + L Z for the caller's Z (N x S); scale entry by entry |m| + |L| |Z|       (sgp_rand)
  ext.*         the post.* families of the STACKED data, for the posterior update_posterior returns (sthenomi_extend.h: "what
                sgp_posterior_create on the stacked data leaves")
  vupd.*        the spost.* families of the STACKED data, for a VFE posterior after update_posterior; vupd.elbo is elbo_out
                less half the create call's trace term (sthenomi_vfe_update.h), which is the ELBO of the stacked data

The cross matrix, the prior variance and the prior covariance can be handed over as matrices (sgp_posterior_predict_explicit).
Every sum comes with the sum of the absolute values of its addends; the error unit is eps = 2^-53 times
grad_truth.scale_entries / scale_scalar of both (rand: the absolute sum itself).

Bounds, by the method of grad_truth.py: device <= MARGIN * max(e_float64 of the case, the family's floor), e_float64 the
larger figure of the two float64 runs, the floor the median of e_float64 over the final case list
(tests/test_gpu_forward_truth.py's cases; `python tests/test_forward_truth_on_numpy.py` prints them)."""
import numpy as np

import grad_truth as T
import predgrad_truth as PT
from grad_truth import require_extended, scale_entries, scale_scalar, units  # noqa: F401

MARGIN, SELF_MARGIN, EPS = T.MARGIN, T.SELF_MARGIN, T.EPS

# sorted float64 figures of the final case list, family by family, and their medians (the floors)
MEASURED_FLOAT64 = {'ext.alpha': [15.1, 31.9, 36.1, 64.7, 94.6, 101.0],
 'ext.cov': [2.2, 9.8, 19.8, 19.8, 21.0, 21.2],
 'ext.logpdf_y': [0.2, 1.3, 1.6, 2.4, 3.5, 12.3],
 'ext.mean': [15.2, 44.8, 74.3, 118.7, 178.7, 274.1],
 'ext.var': [5.1, 9.8, 16.1, 17.4, 18.5, 19.8],
 'post.alpha': [6.1, 64.6, 68.8, 101.2, 262.7, 273.8, 369.2, 1216.5],
 'post.cov': [1.4, 19.9, 20.2, 28.4, 80.2, 94.5, 129.3, 142.2],
 'post.mean': [13.3, 26.4, 118.9, 180.7, 285.2, 663.1, 673.7, 1091.6],
 'post.var': [2.3, 16.4, 19.7, 21.1, 94.5, 119.3, 134.2, 163.7],
 'rand': [33.2, 41.4, 79.6, 398.3],
 'spost.cov': [0.8, 6.2, 33.4, 117.9],
 'spost.elbo': [0.7, 2.0, 2.5, 17.4],
 'spost.mean': [32.1, 122.0, 211.9, 249.2],
 'spost.var': [0.8, 3.4, 29.8, 123.3],
 'vupd.cov': [5.4, 12.4, 13.0, 13.6, 102.1],
 'vupd.elbo': [0.2, 1.8, 2.8, 2.8, 7.4],
 'vupd.mean': [33.4, 40.7, 59.1, 60.4, 84.9],
 'vupd.var': [3.0, 10.7, 11.0, 13.1, 51.2]}
FLOORS = {'ext.alpha': 50.400000000000006,
 'ext.cov': 19.8,
 'ext.logpdf_y': 2.0,
 'ext.mean': 96.5,
 'ext.var': 16.75,
 'post.alpha': 181.95,
 'post.cov': 54.3,
 'post.mean': 232.95,
 'post.var': 57.8,
 'rand': 60.5,
 'spost.cov': 19.8,
 'spost.elbo': 2.25,
 'spost.mean': 166.95,
 'spost.var': 16.6,
 'vupd.cov': 13.0,
 'vupd.elbo': 2.8,
 'vupd.mean': 59.1,
 'vupd.var': 11.0}

# the tolerance each family's bound sits beside (tests/test_gpu_parity.py, test_gpu_extend.py, test_gpu_vfe_update.py,
# test_gpu_postfx.py), relative to the scale
OLD_TOLERANCE = {"post.alpha": 1e-9, "post.mean": 1e-9, "post.var": 1e-9, "post.cov": 1e-9,
                 "spost.mean": 1e-7, "spost.var": 1e-8, "spost.cov": 1e-8, "spost.elbo": 1e-9,
                 "rand": 1e-11,
                 "ext.alpha": 1e-9, "ext.mean": 1e-9, "ext.var": 1e-9, "ext.cov": 1e-9, "ext.logpdf_y": 1e-10,
                 "vupd.mean": 1e-7, "vupd.var": 1e-8, "vupd.cov": 1e-8, "vupd.elbo": 1e-9}


def _f(a, dt):
    return np.asarray(a, np.float64).astype(dt)


def _test_side(S_cross, S_prior, mean_s, dt, Ks=None, prior_var=None, Kss=None, cov=True):
    """(K*, k**, K**, m*) in dtype dt: from the specs, or from the matrices handed over (float64 values, taken as they are)"""
    Ks = T.dense(S_cross, dt) if Ks is None else _f(Ks, dt)
    if prior_var is None:
        prior_var = T.diag_of(S_prior, dt)
    else:
        prior_var = _f(prior_var, dt)
    if not cov:
        Kss = None
    elif Kss is None:
        Kss = PT._sym(T.dense(S_prior, dt))
    else:
        Kss = _f(Kss, dt)
    return Ks, prior_var, Kss, _f(mean_s, dt)


def posterior(S_train, noise_kind, noise, mean, y, S_cross, S_prior, mean_s, dt, cholesky=None, Ks=None, prior_var=None,
              Kss=None, cov=True):
    """the post.* families in dtype dt (for an extended posterior: S_train, noise, mean and y of the stacked data)"""
    c = PT.exact_core(S_train, noise_kind, noise, mean, y, dt, cholesky)
    n, Li, z = c["n"], c["Li"], c["z"]
    Ks, pv, Kss, ms = _test_side(S_cross, S_prior, mean_s, dt, Ks, prior_var, Kss, cov)
    half, two = dt(1) / dt(2), dt(2)
    out = dict(n=n, L=c["L"], alpha=c["alpha"], S_alpha=np.abs(Li).T @ (np.abs(Li) @ np.abs(c["delta"])))
    out["mean"], out["S_mean"] = ms + Ks @ c["alpha"], np.abs(ms) + np.abs(Ks) @ np.abs(c["alpha"])
    V = Li @ Ks.T
    sq = (V * V).sum(0)
    out["var"], out["S_var"] = pv - sq, np.abs(pv) + sq
    if cov:
        out["cov"], out["S_cov"] = Kss - V.T @ V, np.abs(Kss) + np.abs(V).T @ np.abs(V)
    logs = np.log(np.diag(c["L"]))
    log2pi = np.log(two * T._pi(dt))
    out["logpdf_y"] = -half * (dt(n) * log2pi + two * logs.sum() + z @ z)
    out["S_logpdf_y"] = half * (dt(n) * log2pi + two * np.abs(logs).sum() + z @ z)
    return out


def sparse_posterior(S_zz, z_noise_kind, z_noise, S_xz, noise_kind, noise, mean, y, S_xx, S_cross, S_prior, mean_s, dt,
                     cholesky=None, cov=True):
    """the spost.* families in dtype dt (after an update: S_xz, S_xx, noise, mean and y of the stacked data); the form is
    predgrad_truth.sparse_predict_grad's (Lz, Le), extended to the covariance and the ELBO (grad_truth.elbo_grad's value)"""
    c = PT.sparse_core(S_zz, z_noise_kind, z_noise, S_xz, noise_kind, noise, mean, y, dt, cholesky)
    n, m, sy, A, delta, u = c["n"], c["m"], c["sy"], c["A"], c["delta"], c["u"]
    Ks, pv, Kss, ms = _test_side(S_cross, S_prior, mean_s, dt, cov=cov)
    half, two = dt(1) / dt(2), dt(2)
    out = dict(n=n, m=m, alpha=c["alpha"])
    out["mean"], out["S_mean"] = ms + Ks @ c["alpha"], np.abs(ms) + np.abs(Ks) @ np.abs(c["alpha"])
    Bp = Ks @ c["Lzi"].T
    Cp = Bp @ c["Lei"].T
    sb, sc = (Bp * Bp).sum(1), (Cp * Cp).sum(1)
    out["var"], out["S_var"] = pv - sb + sc, np.abs(pv) + sb + sc
    if cov:
        out["cov"] = Kss - Bp @ Bp.T + Cp @ Cp.T
        out["S_cov"] = np.abs(Kss) + np.abs(Bp) @ np.abs(Bp).T + np.abs(Cp) @ np.abs(Cp).T
    var_x = T.diag_of(S_xx, dt)
    logs_e = np.log(np.diag(c["Le"]))
    log2pi = np.log(two * T._pi(dt))
    parts = [dt(n) * log2pi, np.log(sy).sum(), two * logs_e.sum(), delta @ delta, -(u @ u), (var_x / sy).sum(), -(A * A).sum()]
    out["elbo"] = -half * sum(parts)
    out["S_elbo"] = half * (dt(n) * log2pi + np.abs(np.log(sy)).sum() + two * np.abs(logs_e).sum() + delta @ delta + u @ u
                            + (np.abs(var_x) / sy).sum() + (A * A).sum())
    return out


def rand(S, noise_kind, noise, mean, Z, dt, cholesky=None):
    """sgp_rand: m + L Z, L the lower Cholesky factor of K + Sigma_y; Z is N x S"""
    cholesky = cholesky or T.cholesky
    n = int(sum(S["row_len"]))
    Lm = cholesky(PT._sym(T.dense(S, dt)) + T.noise_matrix(noise_kind, noise, n, dt))
    m, Zd = _f(mean, dt), _f(Z, dt).reshape(n, -1)
    return dict(n=n, rand=m[:, None] + Lm @ Zd, S_rand=np.abs(m)[:, None] + np.abs(Lm) @ np.abs(Zd))


# ---- units -------------------------------------------------------------------------------------------------------------
def posterior_units(prefix, out, R):
    """largest error of each family of `out` (alpha, mean, var, cov, logpdf_y: those present) against the truth R, in units"""
    n, u = R["n"], {}
    for key in ("alpha", "mean", "var", "cov"):
        if out.get(key) is not None:
            assert np.shape(out[key]) == R[key].shape, key
            u[f"{prefix}.{key}"] = units(out[key], R[key], scale_entries(R[key], R["S_" + key] / n))
    if out.get("logpdf_y") is not None:
        u[prefix + ".logpdf_y"] = units(out["logpdf_y"], R["logpdf_y"], scale_scalar(R["logpdf_y"], R["S_logpdf_y"], n))
    return u


def sparse_units(prefix, out, R):
    """mean, var, cov against the truth with the number of inducing points as the column count, elbo with the data's"""
    u = {}
    for key in ("mean", "var", "cov"):
        if out.get(key) is not None:
            assert np.shape(out[key]) == R[key].shape, key
            u[f"{prefix}.{key}"] = units(out[key], R[key], scale_entries(R[key], R["S_" + key] / R["m"]))
    if out.get("elbo") is not None:
        u[prefix + ".elbo"] = units(out["elbo"], R["elbo"], scale_scalar(R["elbo"], R["S_elbo"], R["n"]))
    return u


def rand_units(out, R):
    assert np.shape(out) == R["rand"].shape
    return {"rand": units(out, R["rand"], R["S_rand"])}


def reference_outputs(R):
    return {k: R.get(k) for k in ("alpha", "mean", "var", "cov", "logpdf_y", "elbo")}
