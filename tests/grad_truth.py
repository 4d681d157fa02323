"""Extended-precision truth for the gradient entry points (include/sthenomi.h: sgp_logpdf_grad*, sgp_elbo_grad*,
sgp_kernelmatrix_diag_grad*).

TEST INFRASTRUCTURE ONLY.  A dtype-generic restatement of the documented results, driven by a flattened spec read back
with `read_spec` (np_terms.spec_terms): run in np.longdouble (64-bit mantissa) it is the truth, run in np.float64 it is the
yardstick that says what honest double arithmetic delivers on the same problem.  Nothing here calls the product, LAPACK
or numpy.linalg: kernels and their derivatives are written out analytically, distances are the direct sum of squared
differences (as on the device), the Cholesky factor and the triangular inverse are column / row recurrences in the working
dtype.

Every sum is returned with the sum of the absolute values of its addends, S; the error unit of the tests is
eps = 2^-53 times a scale built from both (`scale_scalar`, `scale_entries`).
"""
import numpy as np

EPS = 2.0 ** -53
SE, MATERN12, MATERN32, MATERN52, WHITE, CONST = range(6)       # == stheno_jl_amd.lib's kinds (asserted in read_spec)
NOISE_SCALAR, NOISE_DIAG, NOISE_DENSE = 0, 1, 2                 # tags of this file only

MARGIN = 8.0              # device <= MARGIN * max(e_float64 of the case, floor); the CPU file holds the float64 runs to 2
SELF_MARGIN = 2.0

# e_float64 of a case is the larger figure of two float64 runs of this reference: its own column recurrence and the same
# run with the factor taken in LAPACK's blocked order (`cholesky_blocked_order`) -- two orders of the same operations; the
# device's tiled factorisation is a third (docs/04_oracle_and_parity.md has the evidence that made the second run necessary).
# Floors F_family, in units: the median of e_float64 over the final case list (tests/test_gpu_grad_truth.py's cases;
# printed by `python tests/test_grad_truth_on_numpy.py`), so that a lucky float64 draw does not make a bound vanish.
# First the sorted measured lists, then their medians.
MEASURED_FLOAT64 = {'elbo.d_coef': [54.0, 57.9, 120.2, 147.1, 243.5, 1561.7, 36486.6, 58653.6],
 'elbo.d_inscale': [67.0, 86.3, 142.1, 256.5, 258.0, 607.8, 38143.2, 45682.8],
 'elbo.inputs': [67.9, 102.3, 118.5, 147.6, 201.4, 258.9, 14333.6, 27287.4],
 'elbo.noise': [0.8, 1.2, 1.4, 4.7, 6.8, 7.5, 9.4, 67.3],
 'elbo.value': [0.5, 0.9, 1.3, 1.5, 1.8, 1.9, 2.2, 5.0],
 'elbo.y': [2.1, 9.8, 10.4, 10.7, 16.9, 19.2, 48.1, 84.3],
 'elbo.z_noise': [2.7, 3.0, 4.3, 6.0, 7.2, 64.3, 171.1, 503.8],
 'lp.d_coef': [2.0, 3.0, 10.1, 13.7, 18.9, 20.5, 20.5, 21.2, 22.9, 24.2, 26.1, 33.0, 42.8, 50.8, 64.0, 67.6, 73.9, 80.0,
               82.8, 86.1, 90.8, 95.6, 109.0, 125.5, 126.8, 155.3, 155.4, 182.5, 192.1, 202.5, 210.9, 215.7, 282.7,
               294.8, 317.3, 321.8, 348.6, 432.7, 498.2, 517.3, 522.0, 587.1, 623.1, 1088.0, 1151.1, 1193.0, 1235.3,
               1379.1, 1502.2, 1697.7, 18967.6, 29754.6],
 'lp.d_inscale': [0.0, 11.3, 12.0, 13.0, 15.3, 17.3, 22.8, 29.6, 29.7, 30.0, 34.9, 39.7, 42.3, 43.1, 43.2, 44.5, 45.3,
                  54.8, 59.4, 60.1, 63.7, 72.5, 72.8, 92.4, 92.9, 115.3, 146.6, 180.5, 190.8, 199.3, 214.4, 263.1,
                  265.2, 285.6, 299.1, 340.4, 348.1, 351.7, 358.0, 403.3, 436.5, 495.1, 508.4, 894.2, 930.8, 950.4,
                  1088.6, 1504.8, 1706.3, 2968.6, 3617.7, 10853.3],
 'lp.inputs': [0.0, 13.4, 16.7, 17.7, 19.1, 20.8, 21.3, 22.1, 24.0, 24.4, 25.0, 26.4, 27.9, 29.0, 30.3, 30.4, 32.4,
               33.3, 33.5, 34.6, 36.3, 37.5, 39.6, 42.3, 50.1, 52.5, 54.3, 55.4, 57.9, 71.0, 71.7, 77.6, 79.9, 94.3,
               94.9, 108.7, 126.7, 138.7, 141.5, 166.2, 166.5, 168.0, 196.8, 244.4, 255.3, 302.3, 372.7, 500.1, 617.6,
               761.1, 1703.1, 10549.2],
 'lp.noise': [0.7, 3.8, 4.0, 4.8, 5.3, 5.7, 5.9, 6.1, 6.6, 6.8, 7.9, 8.2, 8.3, 9.6, 9.9, 10.1, 11.1, 12.1, 12.3, 12.5,
              12.6, 13.8, 14.2, 15.6, 16.1, 16.1, 16.3, 16.4, 17.3, 17.8, 19.2, 19.6, 22.3, 22.8, 24.5, 24.7, 27.8,
              28.4, 33.1, 33.4, 33.8, 34.3, 39.8, 43.1, 45.5, 49.3, 62.9, 84.5, 105.7, 128.7, 154.0, 557.6],
 'lp.scales': [82.6, 110.8, 317.1, 521.0, 621.6, 1152.5],
 'lp.value': [0.2, 0.2, 0.3, 0.4, 0.5, 0.5, 0.6, 0.6, 0.7, 0.7, 0.7, 0.8, 0.8, 0.8, 0.8, 0.8, 0.9, 0.9, 1.0, 1.0, 1.1,
              1.1, 1.2, 1.2, 1.3, 1.4, 1.5, 1.5, 1.5, 1.6, 1.7, 1.8, 2.1, 2.1, 2.3, 2.3, 2.4, 2.9, 4.1, 4.1, 5.6, 6.1,
              6.2, 6.7, 9.5, 12.4, 12.7, 13.4, 13.7, 14.0, 18.0, 19.8],
 'lp.y': [1.3, 6.2, 6.5, 6.5, 7.2, 7.2, 7.7, 9.1, 9.3, 9.4, 9.9, 10.4, 10.4, 10.9, 11.8, 12.4, 12.4, 13.5, 13.7, 13.7,
          14.9, 15.8, 18.0, 20.0, 21.1, 23.6, 26.9, 28.6, 28.9, 34.8, 38.3, 41.5, 46.9, 49.7, 56.7, 56.8, 58.9, 77.6,
          82.9, 85.3, 92.9, 95.9, 110.7, 124.3, 145.9, 146.9, 152.6, 179.2, 361.6, 402.2, 616.0, 765.7]}
FLOORS = {'elbo.d_coef': 195.3,
 'elbo.d_inscale': 257.25,
 'elbo.inputs': 174.5,
 'elbo.noise': 5.75,
 'elbo.value': 1.65,
 'elbo.y': 13.799999999999999,
 'elbo.z_noise': 6.6,
 'lp.d_coef': 155.35000000000002,
 'lp.d_inscale': 130.95,
 'lp.inputs': 53.4,
 'lp.noise': 16.200000000000003,
 'lp.scales': 419.05,
 'lp.value': 1.45,
 'lp.y': 25.25}

# the tolerance of the existing test that each family's bound must undercut by a factor 100 (relative to the scale)
OLD_TOLERANCE = {"lp": 1e-8, "elbo": 2e-5}


def require_extended():
    """The truth needs a long double with at least a 64-bit mantissa.  Raises (a skip would hide the whole file)."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("grad_truth: np.longdouble has a %d-bit mantissa here; the truth needs 63 or more"
                           % np.finfo(np.longdouble).nmant)
    return np.longdouble


# ---- reading a spec --------------------------------------------------------------------------------------------
def read_spec(spec):
    """dict(terms, inputs, row_len, col_len, symmetric) from a stheno_jl_amd.lib.Spec (the only product object read)."""
    import np_terms
    from stheno_jl_amd import lib as L
    assert (L.SE, L.MATERN12, L.MATERN32, L.MATERN52, L.WHITE, L.CONST) == (SE, MATERN12, MATERN32, MATERN52, WHITE, CONST)
    return dict(terms=np_terms.spec_terms(spec), inputs=[np.array(a, dtype=np.float64) for a in spec.inputs],
                row_len=[int(v) for v in spec.row_len], col_len=[int(v) for v in spec.col_len],
                symmetric=bool(spec.symmetric))


# ---- kernels ---------------------------------------------------------------------------------------------------
def kappa(kind, d2, param, dt):
    """(kappa, d kappa / d (d^2), d kappa(g x, g x') / dg at g = 1) of the squared distance, in dtype dt.
    dk/dg = 2 d2 kappa'.  Matern-1/2 at coincident points: the documented subgradient 0."""
    d2 = np.asarray(d2, dtype=dt)
    one, half = dt(1), dt(1) / dt(2)
    if kind == SE:
        k = np.exp(-half * d2)
        return k, -half * k, -d2 * k
    d = np.sqrt(d2)
    if kind == MATERN12:
        k = np.exp(-d)
        safe = np.where(d > 0, d, one)
        return k, np.where(d > 0, -half * k / safe, dt(0)), -d * k
    if kind == MATERN32:
        l = np.sqrt(dt(3)) * d
        e = np.exp(-l)
        return (one + l) * e, -(dt(3) / dt(2)) * e, -dt(3) * d2 * e
    if kind == MATERN52:
        l = np.sqrt(dt(5)) * d
        e = np.exp(-l)
        kp = -(dt(5) / dt(6)) * (one + l) * e
        return (one + l + dt(5) * d2 / dt(3)) * e, kp, dt(2) * d2 * kp
    if kind == WHITE:
        return (d2 == 0).astype(dt), np.zeros_like(d2), np.zeros_like(d2)
    if kind == CONST:
        return np.full_like(d2, dt(param)), np.zeros_like(d2), np.zeros_like(d2)
    raise ValueError(kind)


def sqdist(X, Y):
    """direct sum_d (a - b)^2, coordinate by coordinate, in the dtype of X"""
    d2 = np.zeros((X.shape[1], Y.shape[1]), dtype=X.dtype)
    for d in range(X.shape[0]):
        df = X[d][:, None] - Y[d][None, :]
        d2 += df * df
    return d2


# ---- linear algebra in the working dtype -----------------------------------------------------------------------------
def cholesky(C):
    """lower Cholesky factor, column by column"""
    n = C.shape[0]
    Lm = np.zeros_like(C)
    for j in range(n):
        col = C[j:, j] - Lm[j:, :j] @ Lm[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError("grad_truth.cholesky: not positive definite at column %d" % j)
        Lm[j:, j] = col / np.sqrt(col[0])
    return Lm


def cholesky_blocked_order(C):
    """The same factor in another order of the same float64 operations: LAPACK's blocked potrf (panel, triangular solve,
    rank-k update).  float64 only -- the second yardstick run, never the truth."""
    assert C.dtype == np.float64
    return np.linalg.cholesky(C)


def tri_inverse(Lm):
    """inverse of a lower triangular matrix, row by row"""
    n = Lm.shape[0]
    Li = np.zeros_like(Lm)
    for i in range(n):
        row = -(Lm[i, :i] @ Li[:i, :])
        row[i] += Lm.dtype.type(1)
        Li[i, :] = row / Lm[i, i]
    return Li


def _pi(dt):
    return dt(4) * np.arctan(dt(1))


# ---- the covariance of a spec and the contraction of a cotangent with its terms ----------------------------------------------
def _cast(S, dt):
    terms = []
    for (I, J, kind, ri, ci, coef, param, rs, cs) in S["terms"]:
        terms.append((I, J, kind, ri, ci, dt(coef), param, None if rs is None else rs.astype(dt),
                      None if cs is None else cs.astype(dt)))
    return terms, [a.astype(dt) for a in S["inputs"]]


def dense(S, dt):
    terms, inputs = _cast(S, dt)
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    coff = np.concatenate([[0], np.cumsum(S["col_len"])]).astype(int)
    K = np.zeros((roff[-1], coff[-1]), dtype=dt)
    for (I, J, kind, ri, ci, coef, param, rs, cs) in terms:
        blk = coef * kappa(kind, sqdist(inputs[ri], inputs[ci]), param, dt)[0]
        if rs is not None:
            blk = rs[:, None] * blk
        if cs is not None:
            blk = blk * cs[None, :]
        K[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += blk
    return K


def diag_of(S, dt):
    """var = sgp_kernelmatrix_diag(spec): sum over the terms of the diagonal block pairs of coef rs_i cs_i k(x_i, x'_i)"""
    terms, inputs = _cast(S, dt)
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    v = np.zeros(roff[-1], dtype=dt)
    for (I, J, kind, ri, ci, coef, param, rs, cs) in terms:
        if I != J:
            continue
        X, Y = inputs[ri], inputs[ci]
        k = coef * kappa(kind, ((X - Y) ** 2).sum(0) if X.shape[0] else np.zeros(X.shape[1], dt), param, dt)[0]
        v[roff[I]:roff[I + 1]] += k * (1 if rs is None else rs) * (1 if cs is None else cs)
    return v


def contract(S, G, dt, inputs=False, scales=False):
    """sum_ij G_ij d K_ij / d theta for every term of spec S (sgp_logpdf_grad's documented results), each with the sum of
    the absolute values of its addends:
      d_coef[t], d_inscale[t]             (S_coef, S_inscale; n_rows[t] for the scale)
      gx[k][d, i]                         (Sn_gx[k] = sum over terms of S_{d,i} / n_cols of that term)
      rowscale[t][i], colscale[t][j]      (Sn_* likewise); the column side only for a cross spec
    Symmetric spec: the row side carries the factor 2 of the mirror block (input and row-scale gradients)."""
    terms, X_in = _cast(S, dt)
    sym = S["symmetric"]
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    coff = np.concatenate([[0], np.cumsum(S["col_len"])]).astype(int)
    nt = len(terms)
    out = dict(d_coef=np.zeros(nt, dt), S_coef=np.zeros(nt, dt), d_inscale=np.zeros(nt, dt), S_inscale=np.zeros(nt, dt),
               n_rows=np.ones(nt, dt))
    if inputs:
        out["gx"] = [np.zeros(a.shape, dt) for a in X_in]
        out["Sn_gx"] = [np.zeros(a.shape, dt) for a in X_in]
    if scales:
        out["rowscale"], out["Sn_rowscale"] = [None] * nt, [None] * nt
        out["colscale"], out["Sn_colscale"] = [None] * nt, [None] * nt
    two = dt(2)
    side = two if sym else dt(1)
    for t, (I, J, kind, ri, ci, coef, param, rs, cs) in enumerate(terms):
        X, Y = X_in[ri], X_in[ci]
        nr, nc = X.shape[1], Y.shape[1]
        d2 = sqdist(X, Y)
        k, kp, dk = kappa(kind, d2, param, dt)
        g = G[roff[I]:roff[I + 1], coff[J]:coff[J + 1]]
        w = g
        if rs is not None:
            w = w * rs[:, None]
        if cs is not None:
            w = w * cs[None, :]
        a = w * k
        out["d_coef"][t], out["S_coef"][t] = a.sum(), np.abs(a).sum()
        a = w * dk
        out["d_inscale"][t], out["S_inscale"][t] = coef * a.sum(), abs(coef) * np.abs(a).sum()
        out["n_rows"][t] = max(nr, 1)
        if inputs:
            core = side * two * coef * (w * kp)            # d K_ij / d x_i = coef rs cs kappa' 2 (x_i - x'_j)
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
            base = coef * g * k
            if rs is not None:
                wc = base if cs is None else base * cs[None, :]
                out["rowscale"][t] = side * wc.sum(1)
                out["Sn_rowscale"][t] = side * np.abs(wc).sum(1) / max(nc, 1)
            if cs is not None and not sym:
                wr = base if rs is None else base * rs[:, None]
                out["colscale"][t] = wr.sum(0)
                out["Sn_colscale"][t] = np.abs(wr).sum(0) / max(nr, 1)
    return out


# ---- logpdf and its gradient -----------------------------------------------------------------------------------------
def noise_matrix(kind, noise, n, dt):
    if kind == NOISE_SCALAR:
        return dt(noise) * np.eye(n, dtype=dt)
    if kind == NOISE_DIAG:
        return np.diag(np.asarray(noise, dtype=np.float64).astype(dt))
    return np.asarray(noise, dtype=np.float64).astype(dt)


def logpdf_grad(S, noise_kind, noise, mean, y, dt, inputs=False, scales=False, cholesky=None, ops=None):
    """sgp_logpdf_grad_xs as documented, in dtype dt: alpha = C^-1 (y - m), G = (alpha alpha' - C^-1) / 2.
    `cholesky`: the factorisation to use (default: the column recurrence above).  `ops`: a module whose `dense` and
    `contract` read another kind of spec (tests/kprod_grad_truth.py: product chains); default: this one."""
    cholesky = cholesky or globals()["cholesky"]
    dense, contract = (globals()["dense"], globals()["contract"]) if ops is None else (ops.dense, ops.contract)
    n = int(sum(S["row_len"]))
    K = dense(S, dt)
    K = np.tril(K) + np.tril(K, -1).T                   # the lower triangle is the matrix (exactly symmetric)
    C = K + noise_matrix(noise_kind, noise, n, dt)
    Lm = cholesky(C)
    Li = tri_inverse(Lm)
    delta = np.asarray(y, np.float64).astype(dt) - np.asarray(mean, np.float64).astype(dt)
    z = Li @ delta
    Ci = Li.T @ Li
    alpha = Li.T @ z
    S_alpha = np.abs(Ci) @ np.abs(delta)
    half = dt(1) / dt(2)
    G = half * (np.outer(alpha, alpha) - Ci)
    S_G = half * (np.abs(np.outer(alpha, alpha)) + np.abs(Ci))
    logs = np.log(np.diag(Lm))
    lp = -half * (dt(n) * np.log(dt(2) * _pi(dt)) + dt(2) * logs.sum() + z @ z)
    S_lp = half * (dt(n) * np.log(dt(2) * _pi(dt)) + dt(2) * np.abs(logs).sum() + z @ z)
    out = contract(S, G, dt, inputs=inputs, scales=scales)
    out.update(n=n, value=lp, S_value=S_lp, alpha=alpha, S_alpha=S_alpha, G=G, S_G=S_G)
    if noise_kind == NOISE_SCALAR:
        out["noise"], out["S_noise"] = np.trace(G), np.trace(S_G)
    elif noise_kind == NOISE_DIAG:
        out["noise"], out["S_noise"] = np.diag(G).copy(), np.diag(S_G).copy()
    else:
        out["noise"], out["S_noise"] = G, S_G
    return out


# ---- elbo and its gradient (oracle/abstractgps.py: elbo_gradient_wrt_cov, restated from its docstring) -----------------------
def elbo_grad(Szz, Sxz, Sxx, noise_kind, noise, z_noise_kind, z_noise, mean, y, dt, inputs=False, cholesky=None, ops=None):
    """With Lambda = diag(sy)^-1/2, A = Lz^-1 Kzx Lambda, B = A A' + I, delta = Lambda (y - m), u = B^-1 A delta,
    J = Lz^-T:  dA = (I - B^-1 - u u') A + u delta';  dKxz = Lambda dA' Lz^-1;  dKzz = -1/2 J (B + B^-1 - 2 I + u u') J';
    ddelta = -delta + A' u;  dy = Lambda ddelta;  dvar = -1 / (2 sy);
    dsy = -1/(2 sy) + var/(2 sy^2) - (ddelta delta + diag(A' dA)) / (2 sy).
    `ops`: as for logpdf_grad, with `diag_of`."""
    cholesky = cholesky or globals()["cholesky"]
    dense, diag_of, contract = ((globals()["dense"], globals()["diag_of"], globals()["contract"]) if ops is None else
                                (ops.dense, ops.diag_of, ops.contract))
    n, m = int(sum(Sxz["row_len"])), int(sum(Sxz["col_len"]))
    half, one, two = dt(1) / dt(2), dt(1), dt(2)
    Kzz = dense(Szz, dt)
    Kzz = np.tril(Kzz) + np.tril(Kzz, -1).T + noise_matrix(z_noise_kind, z_noise, m, dt)
    Kxz = dense(Sxz, dt)
    var = diag_of(Sxx, dt)
    sy = np.full(n, dt(noise)) if noise_kind == NOISE_SCALAR else np.asarray(noise, np.float64).astype(dt)
    rsig = one / np.sqrt(sy)
    Lz = cholesky(Kzz)
    Lzi = tri_inverse(Lz)
    A = (Lzi @ Kxz.T) * rsig[None, :]
    I = np.eye(m, dtype=dt)
    B = A @ A.T + I
    Le = cholesky(B)
    Lei = tri_inverse(Le)
    Binv = Lei.T @ Lei
    delta = (np.asarray(y, np.float64).astype(dt) - np.asarray(mean, np.float64).astype(dt)) * rsig
    c = A @ delta
    b = Lei @ c
    u = Lei.T @ b
    uu = np.outer(u, u)
    Z = I - Binv - uu
    Sm = B + Binv - two * I + uu
    J = Lzi.T
    dA_T = A.T @ Z + np.outer(delta, u)
    dKxz = rsig[:, None] * (dA_T @ J.T)
    dKzz = -half * (J @ Sm @ J.T)
    ddelta = -delta + A.T @ u
    dy = ddelta * rsig
    diagdot = (A.T * dA_T).sum(1)
    dsy = -half / sy + half * var / sy ** 2 - half * (ddelta * delta + diagdot) / sy
    S_dsy = half / sy + half * np.abs(var) / sy ** 2 + half * (np.abs(ddelta * delta) + (np.abs(A.T) * np.abs(dA_T)).sum(1)) / sy
    logs_e = np.log(np.diag(Le))
    log2pi = np.log(two * _pi(dt))
    parts = [dt(n) * log2pi, np.log(sy).sum(), two * logs_e.sum(), delta @ delta, -(b @ b), (var / sy).sum(), -(A * A).sum()]
    value = -half * sum(parts)
    S_value = half * (dt(n) * log2pi + np.abs(np.log(sy)).sum() + two * np.abs(logs_e).sum() + delta @ delta + b @ b
                      + (np.abs(var) / sy).sum() + (A * A).sum())
    out = dict(n=n, m=m, value=value, S_value=S_value, y=dy, S_y=np.abs(delta * rsig) + (np.abs(A.T) @ np.abs(u)) * rsig,
               var=-half / sy, dKzz=dKzz, dKxz=dKxz)
    if noise_kind == NOISE_SCALAR:
        out["noise"], out["S_noise"] = dsy.sum(), S_dsy.sum()
    else:
        out["noise"], out["S_noise"] = dsy, S_dsy
    if z_noise_kind == NOISE_SCALAR:
        out["z_noise"], out["S_z_noise"] = np.trace(dKzz), np.abs(np.diag(dKzz)).sum()
    elif z_noise_kind == NOISE_DIAG:
        out["z_noise"], out["S_z_noise"] = np.diag(dKzz).copy(), np.abs(np.diag(dKzz))
    else:
        out["z_noise"], out["S_z_noise"] = dKzz, np.abs(dKzz)
    out["zz"] = contract(Szz, dKzz, dt, inputs=inputs)
    out["xz"] = contract(Sxz, dKxz, dt, inputs=inputs)
    return out


# ---- sgp_kernelmatrix_diag_grad / _grad_x with the caller's w ------------------------------------------------------------
def diag_grad(S, w, dt):
    """per term of the diagonal block pairs: d_coef = sum_i w_i rs_i cs_i k(x_i, x'_i), d_inscale = coef sum_i ... dk/dg,
    gx[ri] += 2 coef w rs cs kappa' (x - x'), gx[ci] -= the same; terms of other block pairs: exact zeros."""
    terms, X_in = _cast(S, dt)
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    w = np.asarray(w, np.float64).astype(dt)
    nt = len(terms)
    out = dict(d_coef=np.zeros(nt, dt), S_coef=np.zeros(nt, dt), d_inscale=np.zeros(nt, dt), S_inscale=np.zeros(nt, dt),
               gx=[np.zeros(a.shape, dt) for a in X_in], S_gx=[np.zeros(a.shape, dt) for a in X_in],
               diagonal=np.zeros(nt, bool))
    for t, (I, J, kind, ri, ci, coef, param, rs, cs) in enumerate(terms):
        if I != J:
            continue
        out["diagonal"][t] = True
        X, Y = X_in[ri], X_in[ci]
        df = X - Y
        d2 = np.zeros(X.shape[1], dt)
        for d in range(X.shape[0]):
            d2 += df[d] * df[d]
        k, kp, dk = kappa(kind, d2, param, dt)
        ww = w[roff[I]:roff[I + 1]] * (1 if rs is None else rs) * (1 if cs is None else cs)
        out["d_coef"][t], out["S_coef"][t] = (ww * k).sum(), np.abs(ww * k).sum()
        out["d_inscale"][t], out["S_inscale"][t] = coef * (ww * dk).sum(), abs(coef) * np.abs(ww * dk).sum()
        core = dt(2) * coef * (ww * kp)[None, :] * df
        out["gx"][ri] += core
        out["gx"][ci] -= core
        out["S_gx"][ri] += np.abs(core)
        out["S_gx"][ci] += np.abs(core)
    return out


# ---- units -----------------------------------------------------------------------------------------------------------
def scale_scalar(q, S, n_rows):
    """scale of a scalar sum q whose addends have absolute sum S: max(|q|, S / n_rows)"""
    return np.maximum(np.abs(q), S / n_rows)


def scale_entries(v, Sn):
    """scale of the entries of an array of sums: max(max |v|, S_entry / n_cols), Sn = S / n_cols entry by entry"""
    v = np.asarray(v)
    top = np.abs(v).max() if v.size else v.dtype.type(0)
    return np.maximum(top, Sn)


def units(got, truth, scale):
    """largest |got - truth| / (eps scale) over the entries, as a float; 0 for empty arrays.  NaN in `got` gives inf."""
    got, truth, scale = np.asarray(got), np.asarray(truth), np.asarray(scale)
    if truth.size == 0:
        return 0.0
    err = np.abs(got.astype(truth.dtype) - truth)
    if not np.all(np.isfinite(got)):
        return float("inf")
    safe = np.where(scale > 0, scale, 1)
    u = np.where(scale > 0, err / safe, np.where(err > 0, np.inf, 0))
    return float(u.max() / EPS)
