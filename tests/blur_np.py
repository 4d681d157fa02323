"""The blur kind (csrc/blur_eval.h) restated in NumPy, dtype-generic: the formula, grad_truth's `ops` for specs that hold it
(`dense` / `contract`; tests/grad_truth.py: logpdf_grad(..., ops=blur_np)), and the NumPy double of the C boundary
(tests/np_capi.py) taught to evaluate it.  TEST INFRASTRUCTURE ONLY.

A term reads points of dimension 2 D: the locations, then the variances.  With u = mu - mu' and q = 1 + (s + s'):
k = prod_d q_d^(-1/2) exp(-1/2 sum_d u_d^2 / q_d).  An SE term is the same formula on zero variances."""
import numpy as np

import grad_truth as T
import np_capi
from stheno_jl_amd import lib as L


def is_blur(kind):
    return (int(kind) & L.KIND_MASK) == L.BLUR_SE


def pair(X, Y, dt=np.float64):
    """(u (D x n x m), w = 1 / q, S = s + s', k) of points (location rows, then variance rows) in dtype dt"""
    X, Y = np.asarray(X, dtype=dt), np.asarray(Y, dtype=dt)
    D = X.shape[0] // 2
    u, S = X[:D, :, None] - Y[:D, None, :], X[D:, :, None] + Y[D:, None, :]
    w = 1 / (1 + S)
    return u, w, S, np.sqrt(w.prod(0)) * np.exp(-(u * u * w).sum(0) / 2)


def _points(kind, X):
    assert is_blur(kind) or kind == L.SE
    return X if is_blur(kind) else np.vstack([X, 0 * X])


def dense(S, dt):
    terms, inputs = T._cast(S, dt)
    roff, coff = np.concatenate([[0], np.cumsum(S["row_len"])]), np.concatenate([[0], np.cumsum(S["col_len"])])
    K = np.zeros((roff[-1], coff[-1]), dtype=dt)
    for (I, J, kind, ri, ci, coef, param, rs, cs) in terms:
        blk = coef * pair(_points(kind, inputs[ri]), _points(kind, inputs[ci]), dt)[3]
        blk = blk * (1 if rs is None else rs[:, None]) * (1 if cs is None else cs[None, :])
        K[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += blk
    return K


def contract(S, G, dt, inputs=False, scales=False):
    """grad_truth.contract's d_coef, d_inscale and gx (variance rows included) with their absolute sums, for a symmetric spec
    of SE and blur terms (scale gradients are refused through blur terms: not stated here)"""
    assert S["symmetric"] and not scales
    terms, X_in = T._cast(S, dt)
    off = np.concatenate([[0], np.cumsum(S["row_len"])])
    nt = len(terms)
    out = dict(d_coef=np.zeros(nt, dt), S_coef=np.zeros(nt, dt), d_inscale=np.zeros(nt, dt), S_inscale=np.zeros(nt, dt),
               n_rows=np.ones(nt, dt), gx=[np.zeros(a.shape, dt) for a in X_in], Sn_gx=[np.zeros(a.shape, dt) for a in X_in])
    for t, (I, J, kind, ri, ci, coef, param, rs, cs) in enumerate(terms):
        u, w, Ss, k = pair(_points(kind, X_in[ri]), _points(kind, X_in[ci]), dt)
        g = G[off[I]:off[I + 1], off[J]:off[J + 1]] * (1 if rs is None else rs[:, None]) * (1 if cs is None else cs[None, :])
        a, h = g * k, (Ss * w + (u * w) ** 2).sum(0)
        out["d_coef"][t], out["S_coef"][t] = a.sum(), np.abs(a).sum()
        out["d_inscale"][t], out["S_inscale"][t] = -coef * (a * h).sum(), abs(coef) * (np.abs(a) * h).sum()
        out["n_rows"][t] = max(u.shape[1], 1)
        rows = X_in[ri].shape[0]                  # an SE term has no variance rows
        core = 2 * coef * a                       # symmetric: the row side carries the mirror block
        both = core * np.concatenate([-u * w, ((u * w) ** 2 - w) / 2])
        mag = np.abs(core) * np.concatenate([np.abs(u * w), ((u * w) ** 2 + w) / 2])
        out["gx"][ri] += both[:rows].sum(2)
        out["Sn_gx"][ri] += mag[:rows].sum(2) / max(u.shape[2], 1)
    return out


def _dense(before):
    def np_dense(self):
        if not any(is_blur(t[2]) for t in self.terms):
            return before(self)
        K = dense(dict(terms=self.terms, inputs=self.inputs, row_len=self.row_len, col_len=self.col_len), np.float64)
        return np.tril(K) + np.tril(K, -1).T if self.symmetric else K
    return np_dense


def install(monkeypatch):
    """the NumPy double of the C boundary with the blur kind: returns np_capi's context"""
    ctx = np_capi.install(monkeypatch)
    monkeypatch.setattr(np_capi._Spec, "dense", _dense(np_capi._Spec.dense))
    return ctx
