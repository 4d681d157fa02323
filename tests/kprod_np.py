"""NumPy (float64) evaluator of specs with product chains (include/sthenomi_kprod.h): the matrix, and the contraction of a
cotangent G with the derivatives of every term.  TEST INFRASTRUCTURE ONLY (tests/test_kprod_on_numpy.py checks it against
explicit products of closed-form matrices; tests/test_gpu_kprod.py holds the library to it)."""
import numpy as np

from stheno_jl_amd import lib as L

SQ3, SQ5 = np.sqrt(3.0), np.sqrt(5.0)


def rq_log1p_u(d2, alpha):
    """(log1p(u), u), u = d2 / (2 alpha), as the library forms them: a finite d2 whose u overflows takes
    log(d2) - log(2 alpha)"""
    d2 = np.asarray(d2, dtype=np.float64)
    with np.errstate(over="ignore", divide="ignore"):
        u = d2 / (2.0 * alpha)
        l = np.log1p(u)
        return np.where((u > 1.7e308) & np.isfinite(d2), np.log(d2) - np.log(2.0 * alpha), l), u


def rq(d2, alpha):
    """(1 + d2 / (2 alpha))^-alpha by the library's formula, exp(-alpha log1p(d2 / (2 alpha)))"""
    return np.exp(-alpha * rq_log1p_u(d2, alpha)[0])


def rq_dscale(d2, alpha):
    """d k(g x, g y) / dg at g = 1 = -d2 (1 + u)^(-alpha - 1), u = d2 / (2 alpha); 0 where d2 overflowed"""
    l, u = rq_log1p_u(d2, alpha)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.where(u < 1e300, u / (1.0 + u), 1.0)
        return -(2.0 * alpha) * r * np.exp(-alpha * l)


def rq_dparam(d2, alpha):
    """d k / d alpha = k (u / (1 + u) - log1p(u)); 0 where k is"""
    l, u = rq_log1p_u(d2, alpha)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.where(u < 1e300, u / (1.0 + u), 1.0)
        k = np.exp(-alpha * l)
        return np.where(k == 0.0, 0.0, k * (r - l))


def factor(kind, Xr, Xc, param):
    """(k, d k / d inscale, d k / d param) of one factor between the columns of Xr (D x n) and Xc (D x m)"""
    kind = int(kind) & L.KIND_MASK
    if kind == L.LINEAR:
        s = Xr.T @ Xc
        return s + param, 2.0 * s, np.ones_like(s)
    d2 = ((Xr[:, :, None] - Xc[:, None, :]) ** 2).sum(0)
    z = np.zeros_like(d2)
    if kind == L.RQ:
        return rq(d2, param), rq_dscale(d2, param), rq_dparam(d2, param)
    if kind == L.CONST:
        return z + param, z, z + 1.0
    if kind == L.WHITE:
        return (d2 == 0.0).astype(np.float64), z, z
    if kind == L.SE:
        k = np.exp(-0.5 * d2)
        return k, -d2 * k, z
    d = np.sqrt(d2)
    if kind == L.MATERN12:
        k = np.exp(-d)
        return k, -d * k, z
    if kind == L.MATERN32:
        e = np.exp(-SQ3 * d)
        return (1.0 + SQ3 * d) * e, -3.0 * d2 * e, z
    if kind == L.MATERN52:
        e = np.exp(-SQ5 * d)
        return (1.0 + SQ5 * d + 5.0 * d2 / 3.0) * e, -(5.0 * d2 / 3.0) * (1.0 + SQ5 * d) * e, z
    raise ValueError(kind)


def chains(spec):
    """[(I, J, [term indices of one chain])] over every block pair of the spec; a plain term is a chain of one"""
    out = []
    tp, nb = spec._term_ptr, len(spec.col_len)
    for I in range(len(spec.row_len)):
        for J in range(nb):
            p = I * nb + J
            t = int(tp[p])
            while t < int(tp[p + 1]):
                e = t + 1
                while e < int(tp[p + 1]) and (spec._terms[e].kind & L.KIND_TIMES_PREV):
                    e += 1
                out.append((I, J, list(range(t, e))))
                t = e
    return out


def _weights(spec, t):
    """coef rs_i cs_j of the chain whose head is term t, as (coef, rs column | 1, cs row | 1)"""
    rs, cs = spec.term_row_scale[t], spec.term_col_scale[t]
    return (spec._terms[t].coef, 1.0 if rs is None else np.asarray(rs)[:, None], 1.0 if cs is None else np.asarray(cs)[None, :])


def np_spec_matrix(spec):
    """K of a lib.Spec whose terms are plain or chained (no patch / stencil sides)"""
    assert not spec.has_patch and not spec.has_stencil
    K = np.zeros((spec.N, spec.M))
    roff = np.concatenate([[0], np.cumsum(spec.row_len)])
    coff = np.concatenate([[0], np.cumsum(spec.col_len)])
    for I, J, ts in chains(spec):
        prod = 1.0
        for t in ts:
            T = spec._terms[t]
            prod = prod * factor(T.kind, spec.inputs[T.row_input], spec.inputs[T.col_input], T.param)[0]
        coef, rs, cs = _weights(spec, ts[0])
        K[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += coef * rs * prod * cs
    return K


def np_contract(spec, G):
    """(grad_coef, grad_inscale, grad_param), one entry per term of the spec, for the cotangent G of the spec's matrix:
    what sgp_logpdf_grad_param returns (include/sthenomi_kprod.h)"""
    n = spec.n_terms
    gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(n)
    roff = np.concatenate([[0], np.cumsum(spec.row_len)])
    coff = np.concatenate([[0], np.cumsum(spec.col_len)])
    for I, J, ts in chains(spec):
        Gb = G[roff[I]:roff[I + 1], coff[J]:coff[J + 1]]
        fs = [factor(spec._terms[t].kind, spec.inputs[spec._terms[t].row_input], spec.inputs[spec._terms[t].col_input],
                     spec._terms[t].param) for t in ts]
        coef, rs, cs = _weights(spec, ts[0])
        W = Gb * rs * cs
        full = 1.0
        for f in fs:
            full = full * f[0]
        gc[ts[0]] = np.sum(W * full)
        for a, t in enumerate(ts):
            others = 1.0
            for b, f in enumerate(fs):
                if b != a:
                    others = others * f[0]
            gs[t] = coef * np.sum(W * others * fs[a][1])
            gp[t] = coef * np.sum(W * others * fs[a][2])
    return gc, gs, gp
