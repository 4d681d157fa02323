"""NumPy (float64) evaluator of the gradients of a spec with product chains with respect to the points its factors read and
to the row / column scale vectors of its heads, for a given cotangent G of the spec's matrix, and of the same gradients of the
spec's diagonal (include/sthenomi_kprod_grad.h).  On top of tests/kprod_np.py.  TEST INFRASTRUCTURE ONLY:
tests/test_kprod_grad_on_numpy.py checks it against central differences of its own sum(G * np_spec_matrix(spec)) and
sum(w * diag); tests/test_gpu_kprod_grad.py holds the library to it."""
import numpy as np

import kprod_np as kn
from stheno_jl_amd import lib as L

SQ3, SQ5 = kn.SQ3, kn.SQ5


def kappa_prime(kind, d2, param):
    """d k / d (d^2) of a distance kind (0 for CONST / WHITE; Matern-1/2 at coincident points: 0, as on the plain path)"""
    kind = int(kind) & L.KIND_MASK
    z = np.zeros_like(d2)
    if kind in (L.CONST, L.WHITE):
        return z
    if kind == L.RQ:
        l, _ = kn.rq_log1p_u(d2, param)
        return -0.5 * np.exp(-(param + 1.0) * l)
    if kind == L.SE:
        return -0.5 * np.exp(-0.5 * d2)
    d = np.sqrt(d2)
    if kind == L.MATERN12:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(d > 0.0, -0.5 * np.exp(-d) / np.where(d > 0.0, d, 1.0), 0.0)
    if kind == L.MATERN32:
        return -1.5 * np.exp(-SQ3 * d)
    if kind == L.MATERN52:
        return -(5.0 / 6.0) * (1.0 + SQ5 * d) * np.exp(-SQ5 * d)
    raise ValueError(kind)


def _offsets(spec):
    return np.concatenate([[0], np.cumsum(spec.row_len)]), np.concatenate([[0], np.cumsum(spec.col_len)])


def np_input_grads(spec, G, pairs=None):
    """For the cotangent G (spec.N x spec.M) of the spec's matrix K: the gradient of sum(G * K) split by side,
        row[k] / col[k]: (dim, n) per spec input -- what reaches input k through the terms that read it as their row / column
                         input (the total gradient is row[k] + col[k]);
        rs[t] / cs[t]:   per term (heads only; None elsewhere), d / d (row scale vector) and d / d (column scale vector).
    pairs: only these block pairs (I, J)."""
    roff, coff = _offsets(spec)
    row = [np.zeros(np.asarray(a).shape) for a in spec.inputs]
    col = [np.zeros(np.asarray(a).shape) for a in spec.inputs]
    rs, cs = [None] * spec.n_terms, [None] * spec.n_terms
    for I, J, ts in kn.chains(spec):
        if pairs is not None and (I, J) not in pairs:
            continue
        Gb = G[roff[I]:roff[I + 1], coff[J]:coff[J + 1]]
        T = [spec._terms[t] for t in ts]
        X = [(np.asarray(spec.inputs[t.row_input], dtype=float), np.asarray(spec.inputs[t.col_input], dtype=float)) for t in T]
        ks = [kn.factor(t.kind, xr, xc, t.param)[0] for t, (xr, xc) in zip(T, X)]
        coef, rsv, csv = kn._weights(spec, ts[0])
        full = 1.0
        for k in ks:
            full = full * k
        if spec.term_row_scale[ts[0]] is not None:
            rs[ts[0]] = np.sum(Gb * coef * csv * full, axis=1)
        if spec.term_col_scale[ts[0]] is not None:
            cs[ts[0]] = np.sum(Gb * coef * rsv * full, axis=0)
        W = coef * Gb * rsv * csv
        for a, t in enumerate(T):
            others = 1.0
            for b, k in enumerate(ks):
                if b != a:
                    others = others * k
            A = W * others
            xr, xc = X[a]
            if (int(t.kind) & L.KIND_MASK) == L.LINEAR:
                row[t.row_input] += xc @ A.T
                col[t.col_input] += xr @ A
                continue
            d2 = ((xr[:, :, None] - xc[:, None, :]) ** 2).sum(0)
            Cm = 2.0 * A * kappa_prime(t.kind, d2, t.param)
            # (direct differences, coordinate by coordinate, as the library forms them: x_i sum_j C_ij - sum_j C_ij x'_j cancels
            # where close pairs carry a large kappa' -- general-nu Matern below nu = 1, points on a line)
            for d in range(xr.shape[0]):
                E = Cm * (xr[d][:, None] - xc[d][None, :])
                row[t.row_input][d] += E.sum(1)
                col[t.col_input][d] -= E.sum(0)
    return dict(row=row, col=col, rs=rs, cs=cs)


def np_diag(spec):
    """the diagonal of the spec's matrix: var_i = sum over the chains of the pairs (I, I)"""
    return np.diag(kn.np_spec_matrix(spec)).copy()


def np_diag_grads(spec, w):
    """The gradients of sum(w * np_diag(spec)): (gc, gs, gp) per term (the conventions of kprod_np.np_contract), gx per spec
    input (row and column side added), rs / cs per term (heads with a scale vector; None elsewhere)."""
    roff, _ = _offsets(spec)
    n = spec.n_terms
    gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(n)
    gx = [np.zeros(np.asarray(a).shape) for a in spec.inputs]
    rs, cs = [None] * n, [None] * n
    for I, J, ts in kn.chains(spec):
        if I != J:
            continue
        wb = w[roff[I]:roff[I + 1]]
        T = [spec._terms[t] for t in ts]
        X = [(np.asarray(spec.inputs[t.row_input], dtype=float), np.asarray(spec.inputs[t.col_input], dtype=float)) for t in T]
        fs = []
        for t, (xr, xc) in zip(T, X):
            kind = int(t.kind) & L.KIND_MASK
            if kind == L.LINEAR:
                s = np.sum(xr * xc, axis=0)
                fs.append((s + t.param, 2.0 * s, np.ones_like(s)))
                continue
            d2 = np.sum((xr - xc) ** 2, axis=0)
            # kprod_np.factor between the 1-D points sqrt(d2_i) and 0: the same formulas at (a rounding of) d2_i
            fs.append(tuple(v[:, 0] for v in kn.factor(t.kind, np.sqrt(d2)[None, :], np.zeros((1, 1)), t.param)))
        head = ts[0]
        rv = spec.term_row_scale[head]
        cv = spec.term_col_scale[head]
        rsv = 1.0 if rv is None else np.asarray(rv)
        csv = 1.0 if cv is None else np.asarray(cv)
        coef = spec._terms[head].coef
        full = 1.0
        for f in fs:
            full = full * f[0]
        gc[head] = np.sum(wb * rsv * csv * full)
        if rv is not None:
            rs[head] = wb * coef * csv * full
        if cv is not None:
            cs[head] = wb * coef * rsv * full
        for a, t in enumerate(T):
            others = 1.0
            for b, f in enumerate(fs):
                if b != a:
                    others = others * f[0]
            A = wb * rsv * csv * coef * others
            gs[ts[a]] = np.sum(A * fs[a][1])
            gp[ts[a]] = np.sum(A * fs[a][2])
            xr, xc = X[a]
            if (int(t.kind) & L.KIND_MASK) == L.LINEAR:
                gx[t.row_input] += A[None, :] * xc
                gx[t.col_input] += A[None, :] * xr
                continue
            d2 = np.sum((xr - xc) ** 2, axis=0)
            c2 = 2.0 * A * kappa_prime(t.kind, d2, t.param)
            gx[t.row_input] += c2[None, :] * (xr - xc)
            gx[t.col_input] -= c2[None, :] * (xr - xc)
    return dict(gc=gc, gs=gs, gp=gp, gx=gx, rs=rs, cs=cs)
