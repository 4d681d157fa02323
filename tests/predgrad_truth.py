"""Extended-precision truth for the prediction gradients (include/sthenomi_predgrad.h: sgp_posterior_predict_grad_x,
sgp_sparse_posterior_predict_grad_x).

TEST INFRASTRUCTURE ONLY.  A dtype-generic restatement of the header's formulas on top of tests/grad_truth.py (its kernels,
distances, Cholesky recurrences and units): run in np.longdouble it is the truth, run in np.float64 -- once with the column
recurrence, once with the factor taken in LAPACK's blocked order -- it is the yardstick that says what honest double
arithmetic delivers on the same problem.  No LAPACK solve and no numpy.linalg beyond that second factor.

  exact  : C = K + Sigma_y = L L', alpha = C^-1 (y - m), B = K* C^-1
  sparse : Lz Lz' = Kzz + Sigma_z, A = Lz^-1 Kzx Lambda, Le Le' = A A' + I, u = Le^-1 A delta (delta = Lambda (y - m),
           Lambda = diag(sy)^-1/2), alpha = Lz^-T Le^-T u, B' = K*z Lz^-T, C' = B' Le^-T, B = B' Lz^-1 - C' Le^-1 Lz^-1
  mean_i = m*_i + sum_j K*_ij alpha_j,  var_i = k**_ii - sum_j K*_ij B_ij
  gm[k][:, i] = sum over the cross terms with row input k, sum_j alpha_j coef rs_i cs_j kappa'(d2_ij) 2 (xr_i - xc_j)
  gv[k][:, i] = the same with alpha_j -> -2 B_ij
  gp[k]       = grad_truth.diag_grad(prior_ss, w = 1): the k**_ii part
Q with B = K* Q (C^-1, or Lz^-T (I - Le^-T Le^-1) Lz^-1) rides along for the tests that bound third derivatives.
exact_core / sparse_core hold the factorisations, alpha and u: the one computation tests/forward_truth.py shares.

Every sum comes with the sum of the absolute values of its addends (Sn_* = that sum / the number of columns, entry by
entry, as grad_truth.contract); the error unit is eps = 2^-53 times grad_truth.scale_entries of both.

Bounds, by the method of grad_truth.py: device <= MARGIN * max(e_float64 of the case, the family's floor), e_float64 the
larger figure of the two float64 runs, the floor the median of e_float64 over the final case list
(tests/test_gpu_predgrad.py's cases; `python tests/test_predgrad_truth_on_numpy.py` prints them)."""
import numpy as np

import grad_truth as T
from grad_truth import (cholesky, cholesky_blocked_order, kappa, read_spec, scale_entries, sqdist, tri_inverse,  # noqa: F401
                        units)

MARGIN, SELF_MARGIN, EPS = T.MARGIN, T.SELF_MARGIN, T.EPS

# sorted float64 figures of the final case list, family by family, and their medians (the floors)
MEASURED_FLOAT64 = {'pred.mean_x': [18.9, 19.4, 28.8, 51.5, 55.1, 64.8, 109.4, 187.5, 328.0, 546.1],
 'pred.var_x': [7.8, 29.2, 71.0, 158.4, 546.2, 715.7, 756.0, 1571.5, 1820.6, 96248.1],
 'spred.mean_x': [84.9, 117.7, 164.7, 198.8],
 'spred.var_x': [7.2, 38.5, 52.2, 74.7]}
FLOORS = {'pred.mean_x': 59.95,
 'pred.var_x': 630.95,
 'spred.mean_x': 141.2,
 'spred.var_x': 45.35}


def _sym(K):
    return np.tril(K) + np.tril(K, -1).T


def _contract_rows(S, alpha, Bm, dt):
    """gm, gv and their Sn over the terms of the cross spec S; alpha: (n_cols,), Bm: (n_rows, n_cols)"""
    terms, X_in = T._cast(S, dt)
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    coff = np.concatenate([[0], np.cumsum(S["col_len"])]).astype(int)
    gm, Sm = [np.zeros(a.shape, dt) for a in X_in], [np.zeros(a.shape, dt) for a in X_in]
    gv, Sv = [np.zeros(a.shape, dt) for a in X_in], [np.zeros(a.shape, dt) for a in X_in]
    row_read = [False] * len(X_in)
    two = dt(2)
    for (I, J, kind, ri, ci, coef, param, rs, cs) in terms:
        X, Y = X_in[ri], X_in[ci]
        row_read[ri] = True
        nc = max(Y.shape[1], 1)
        kp = kappa(kind, sqdist(X, Y), param, dt)[1]
        core = two * coef * kp
        if rs is not None:
            core = rs[:, None] * core
        if cs is not None:
            core = core * cs[None, :]
        a = alpha[coff[J]:coff[J + 1]]
        b = Bm[roff[I]:roff[I + 1], coff[J]:coff[J + 1]]
        cm, cv = core * a[None, :], -two * core * b
        for d in range(X.shape[0]):
            df = X[d][:, None] - Y[d][None, :]
            gm[ri][d] += (cm * df).sum(1)
            Sm[ri][d] += np.abs(cm * df).sum(1) / nc
            gv[ri][d] += (cv * df).sum(1)
            Sv[ri][d] += np.abs(cv * df).sum(1) / nc
    return dict(gm=gm, Sn_gm=Sm, gv=gv, Sn_gv=Sv, row_read=row_read)


def _finish(out, S_cross, S_prior, mean_s, alpha, Bm, Ks, dt):
    ms = np.asarray(mean_s, np.float64).astype(dt)
    prior = T.diag_of(S_prior, dt)
    out.update(_contract_rows(S_cross, alpha, Bm, dt))
    out["mean"], out["S_mean"] = ms + Ks @ alpha, np.abs(ms) + np.abs(Ks) @ np.abs(alpha)
    out["var"], out["S_var"] = prior - (Ks * Bm).sum(1), np.abs(prior) + np.abs(Ks * Bm).sum(1)
    dg = T.diag_grad(S_prior, np.ones(len(prior)), dt)
    out["gp"], out["S_gp"] = dg["gx"], dg["S_gx"]
    out["alpha"], out["B"] = alpha, Bm
    return out


def exact_core(S_train, noise_kind, noise, mean, y, dt, cholesky=None):
    """C = K + Sigma_y = L L', L^-1, delta = y - m and alpha = L^-T L^-1 delta in dtype dt: the one computation behind
    predict_grad and tests/forward_truth.py"""
    cholesky = cholesky or T.cholesky
    n = int(sum(S_train["row_len"]))
    C = _sym(T.dense(S_train, dt)) + T.noise_matrix(noise_kind, noise, n, dt)
    Lm = cholesky(C)
    Li = tri_inverse(Lm)
    delta = np.asarray(y, np.float64).astype(dt) - np.asarray(mean, np.float64).astype(dt)
    z = Li @ delta
    return dict(n=n, L=Lm, Li=Li, delta=delta, z=z, alpha=Li.T @ z)


def sparse_core(S_zz, z_noise_kind, z_noise, S_xz, noise_kind, noise, mean, y, dt, cholesky=None):
    """Lz^-1, A, Le, Le^-1, delta, u and alpha of the header's sparse statement in dtype dt (noise: scalar or diagonal)"""
    cholesky = cholesky or T.cholesky
    n, m = int(sum(S_xz["row_len"])), int(sum(S_xz["col_len"]))
    Kzz = _sym(T.dense(S_zz, dt)) + T.noise_matrix(z_noise_kind, z_noise, m, dt)
    Kxz = T.dense(S_xz, dt)
    sy = np.full(n, dt(noise)) if noise_kind == T.NOISE_SCALAR else np.asarray(noise, np.float64).astype(dt)
    rsig = dt(1) / np.sqrt(sy)
    Lzi = tri_inverse(cholesky(Kzz))
    A = (Lzi @ Kxz.T) * rsig[None, :]
    Le = cholesky(A @ A.T + np.eye(m, dtype=dt))
    Lei = tri_inverse(Le)
    delta = (np.asarray(y, np.float64).astype(dt) - np.asarray(mean, np.float64).astype(dt)) * rsig
    u = Lei @ (A @ delta)
    return dict(n=n, m=m, sy=sy, Lzi=Lzi, A=A, Le=Le, Lei=Lei, delta=delta, u=u, alpha=Lzi.T @ (Lei.T @ u))


def predict_grad(S_train, noise_kind, noise, mean, y, S_cross, S_prior, mean_s, dt, cholesky=None):
    """sgp_posterior_predict_grad_x as documented, in dtype dt"""
    c = exact_core(S_train, noise_kind, noise, mean, y, dt, cholesky)
    Ci = c["Li"].T @ c["Li"]
    Ks = T.dense(S_cross, dt)
    return _finish(dict(n=c["n"], Q=Ci), S_cross, S_prior, mean_s, c["alpha"], Ks @ Ci, Ks, dt)


def sparse_predict_grad(S_zz, z_noise_kind, z_noise, S_xz, noise_kind, noise, mean, y, S_cross, S_prior, mean_s, dt,
                        cholesky=None):
    """sgp_sparse_posterior_predict_grad_x as documented, in dtype dt (noise: scalar or diagonal)"""
    c = sparse_core(S_zz, z_noise_kind, z_noise, S_xz, noise_kind, noise, mean, y, dt, cholesky)
    Lzi, Lei = c["Lzi"], c["Lei"]
    Ks = T.dense(S_cross, dt)
    Bp = Ks @ Lzi.T
    Cp = Bp @ Lei.T
    Bm = Bp @ Lzi - (Cp @ Lei) @ Lzi
    Q = Lzi.T @ Lzi - (Lzi.T @ Lei.T) @ (Lei @ Lzi)            # B = K* Q
    return _finish(dict(n=c["m"], Q=Q), S_cross, S_prior, mean_s, c["alpha"], Bm, Ks, dt)


def family_units(prefix, out, R):
    """largest error of the two gradient families of `out` (dict with gm, gv: lists aligned with the cross spec's inputs)
    against the truth R, in units; inputs no term reads on its row side are exact zeros on both sides"""
    u = {prefix + ".mean_x": 0.0, prefix + ".var_x": 0.0}
    for key, fam in (("gm", ".mean_x"), ("gv", ".var_x")):
        assert len(out[key]) == len(R[key])
        for k, (a, e, s) in enumerate(zip(out[key], R[key], R["Sn_" + key])):
            assert np.shape(a) == e.shape, (key, k)
            if not R["row_read"][k]:
                assert not np.any(np.asarray(a)), (key, k)
                continue
            u[prefix + fam] = max(u[prefix + fam], units(a, e, scale_entries(e, s)))
    return u


def reference_outputs(R):
    return dict(gm=R["gm"], gv=R["gv"])
