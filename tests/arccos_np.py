"""The arc-cosine kinds (include/sthenomi.h: SGP_NNGP, SGP_NTK) restated in NumPy from their DEFINITION -- acos, no angle tricks
-- dtype-generic: the formula, grad_truth's `ops` for specs that hold them (`dense` / `contract`; tests/grad_truth.py:
logpdf_grad(..., ops=arccos_np)), and the NumPy double of the C boundary (tests/np_capi.py) taught to evaluate them.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import grad_truth as T
import np_capi
from stheno_jl_amd import lib as L


def is_arccos(kind):
    return (int(kind) & L.KIND_MASK) in (L.NNGP, L.NTK)


def pair(X, Y, depth, dt=np.float64):
    """per pair of the D x n and D x m points: (nn = n_x n_y, c_0, c_L, t_L, c'_L, t'_L, xh, yh), ' = d / dc_0 with the 1 / sin
    term counted 0 where sin theta_l = 0.  A bit-equal pair has c_0 = 1 and an exactly opposite one c_0 = -1, whatever the
    rounding of the dot product says"""
    X, Y = np.asarray(X, dtype=dt), np.asarray(Y, dtype=dt)
    pi = T._pi(dt)
    nx, ny = np.sqrt((X * X).sum(0)), np.sqrt((Y * Y).sum(0))
    xh, yh = X / np.where(nx > 0, nx, 1), Y / np.where(ny > 0, ny, 1)
    c = np.clip(xh.T @ yh, -1, 1)
    live = (nx > 0)[:, None] & (ny > 0)[None, :]
    c[np.all(xh[:, :, None] == yh[:, None, :], axis=0) & live] = 1
    c[np.all(xh[:, :, None] == -yh[:, None, :], axis=0) & live] = -1
    c0, t, cp, tp = c, c, np.ones_like(c), np.ones_like(c)
    for _ in range(int(depth)):
        th, sn = np.arccos(c), np.sqrt((1 - c) * (1 + c))
        k0, k1 = 1 - th / pi, (sn + (pi - th) * c) / pi
        inv = np.where(sn > 0, 1 / (pi * np.where(sn > 0, sn, 1)), 0)
        tp = k0 * cp + tp * k0 + t * cp * inv
        cp, t, c = k0 * cp, k1 + t * k0, k1
    return nx[:, None] * ny[None, :], c0, c, t, cp, tp, xh, yh


def value(kind, X, Y, depth, dt=np.float64):
    """n_x n_y T: the kernel without coef and scale vectors"""
    nn, _, c, t, _, _, _, _ = pair(X, Y, depth, dt)
    return nn * (t if (int(kind) & L.KIND_MASK) == L.NTK else c)


def dense(S, dt):
    terms, inputs = T._cast(S, dt)
    roff, coff = np.concatenate([[0], np.cumsum(S["row_len"])]), np.concatenate([[0], np.cumsum(S["col_len"])])
    K = np.zeros((roff[-1], coff[-1]), dtype=dt)
    for (I, J, kind, ri, ci, coef, param, rs, cs) in terms:
        k = (value(kind, inputs[ri], inputs[ci], param, dt) if is_arccos(kind) else
             T.kappa(kind, T.sqdist(inputs[ri], inputs[ci]), param, dt)[0])
        blk = coef * k * (1 if rs is None else rs[:, None]) * (1 if cs is None else cs[None, :])
        K[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += blk
    return K


def contract(S, G, dt, inputs=False, scales=False):
    """grad_truth.contract's d_coef, d_inscale and gx with their absolute sums, for a symmetric spec of arc-cosine terms (scale
    gradients are refused through them: not stated here)"""
    assert S["symmetric"] and not scales
    terms, X_in = T._cast(S, dt)
    off = np.concatenate([[0], np.cumsum(S["row_len"])])
    nt = len(terms)
    out = dict(d_coef=np.zeros(nt, dt), S_coef=np.zeros(nt, dt), d_inscale=np.zeros(nt, dt), S_inscale=np.zeros(nt, dt),
               n_rows=np.ones(nt, dt), gx=[np.zeros(a.shape, dt) for a in X_in], Sn_gx=[np.zeros(a.shape, dt) for a in X_in])
    for t, (I, J, kind, ri, ci, coef, param, rs, cs) in enumerate(terms):
        assert is_arccos(kind)
        nn, c0, c, tl, cp, tp, xh, yh = pair(X_in[ri], X_in[ci], param, dt)
        ntk = (int(kind) & L.KIND_MASK) == L.NTK
        Tv, Tp = (tl, tp) if ntk else (c, cp)
        g = G[off[I]:off[I + 1], off[J]:off[J + 1]] * (1 if rs is None else rs[:, None]) * (1 if cs is None else cs[None, :])
        a = g * nn * Tv
        out["d_coef"][t], out["S_coef"][t] = a.sum(), np.abs(a).sum()
        out["d_inscale"][t], out["S_inscale"][t] = 2 * coef * a.sum(), 2 * abs(coef) * np.abs(a).sum()
        out["n_rows"][t] = max(nn.shape[0], 1)
        ny = np.sqrt((X_in[ci] * X_in[ci]).sum(0))
        core = 2 * coef * g * ny[None, :]          # symmetric: the row side carries the mirror block
        radial, tang = core * (Tv - c0 * Tp), core * Tp
        for d in range(X_in[ri].shape[0]):
            add = radial * xh[d][:, None] + tang * yh[d][None, :]
            out["gx"][ri][d] += add.sum(1)
            out["Sn_gx"][ri][d] += (np.abs(radial * xh[d][:, None]) + np.abs(tang * yh[d][None, :])).sum(1) / max(nn.shape[1], 1)
    return out


def _dense(before):
    def np_dense(self):
        if not any(is_arccos(t[2]) for t in self.terms):
            return before(self)
        K = dense(dict(terms=self.terms, inputs=self.inputs, row_len=self.row_len, col_len=self.col_len), np.float64)
        return np.tril(K) + np.tril(K, -1).T if self.symmetric else K
    return np_dense


def install(monkeypatch):
    """the NumPy double of the C boundary with the arc-cosine kinds: returns np_capi's context"""
    ctx = np_capi.install(monkeypatch)
    monkeypatch.setattr(np_capi._Spec, "dense", _dense(np_capi._Spec.dense))
    return ctx
