"""NumPy (float64) formulas of the Gibbs kind (csrc/gibbs_eval.h) in the library's own formulation, and the NumPy double of
the C boundary (tests/np_capi.py) taught to evaluate and contract it.  TEST INFRASTRUCTURE ONLY (tests/test_gibbs_on_numpy.py
holds the formulas and the host mirror to a long-double reference; tests/test_gpu_gibbs.py holds the library to one).

A term reads points of dimension D + 1: the location, then the lengthscale.  With s = |x - y|^2 over the location,
q = lx^2 + ly^2, c = 2 lx ly / q and p = param:  k = c^(p/2) exp(-s / q), exactly 0 where the exponential underflowed.

install(monkeypatch) makes np_capi's spec evaluator and term contraction know the kind, for the duration of a test."""
import numpy as np

import np_capi
from stheno_jl_amd import lib as L


def is_gibbs(kind):
    return (int(kind) & L.KIND_MASK) == L.GIBBS


def pair(X, Y):
    """dict(u (D x n x m), s, t = s / q, rq = 1 / q, h = sqrt(c), E, dead, lx (n x 1), ly (1 x m)) of gibbs_eval.h: gibbs_pair"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    u = X[:-1, :, None] - Y[:-1, None, :]
    s = np.zeros(u.shape[1:])
    for d in range(u.shape[0]):
        s = u[d] * u[d] + s
    lx, ly = X[-1][:, None], Y[-1][None, :]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        rq = 1.0 / (lx * lx + ly * ly)
        t = s * rq
        c = np.minimum(((2.0 * lx) * ly) * rq, 1.0)
        E = np.exp(np.maximum(-t, -800.0))
        E = np.where(np.isnan(t), 0.0, E)
    return dict(u=u, s=s, t=t, rq=rq, h=np.sqrt(c), E=E, dead=E == 0.0, lx=lx, ly=ly)


def value(P, p):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.where(P["dead"], 0.0, P["h"] ** int(p) * P["E"])


def term(param, X, Y):
    """(value, input-scale derivative -2 t k) of one term per pair of points, without coef and scales"""
    P = pair(X, Y)
    k = value(P, param)
    with np.errstate(invalid="ignore"):
        return k, np.where(P["dead"], 0.0, -2.0 * P["t"] * k)


def point_grads(param, X, Y):
    """(d k / d location of x (D x n x m), d k / d lx (n x m))"""
    P = pair(X, Y)
    k, l = value(P, param), P["lx"]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        dx = np.where(P["dead"], 0.0, k * (-2.0 * P["rq"]) * P["u"])
        dl = np.where(P["dead"], 0.0, k * (0.5 * param * (1.0 / l - 2.0 * l * P["rq"]) + 2.0 * P["t"] * l * P["rq"]))
    return dx, dl


def _scaled(blk, rs, cs):
    if rs is not None:
        blk = rs[:, None] * blk
    if cs is not None:
        blk = blk * cs[None, :]
    return blk


def _dense(before):
    def dense(self):
        if not any(is_gibbs(t[2]) for t in self.terms):
            return before(self)
        K = np.zeros((self.N, self.M))
        for t, (I, J, kind, ri, ci, coef, param, rs, cs) in enumerate(self.terms):
            r, c = self.block(t)
            blk = term(param, self.inputs[ri], self.inputs[ci])[0] if is_gibbs(kind) else np_capi._kern(kind, self.d2(t), param)
            K[r, c] += _scaled(coef * blk, rs, cs)
        if self.symmetric:
            K = np.tril(K) + np.tril(K, -1).T
        return K
    return dense


def _term_grads(before):
    def term_grads(self, s, G, grad_coef, grad_inscale, grad_inputs, grad_rowscale, grad_colscale=None):
        gb = [t for t, T in enumerate(s.terms) if is_gibbs(T[2])]
        if not gb:
            return before(self, s, G, grad_coef, grad_inscale, grad_inputs, grad_rowscale, grad_colscale)
        if grad_rowscale or grad_colscale:
            return self._fail("scale gradients through Gibbs terms are not supported")
        kept = list(s.terms)
        for t in gb:       # the plain terms go through the double's own contraction, the Gibbs terms stand aside as zeros
            I, J, _, ri, ci, _, _, rs, cs = kept[t]
            s.terms[t] = (I, J, L.CONST, ri, ci, 0.0, 0.0, rs, cs)
        rc = before(self, s, G, grad_coef, grad_inscale, grad_inputs, None, None)
        s.terms[:] = kept
        for t in gb:
            (I, J, kind, ri, ci, coef, param, rs, cs) = s.terms[t]
            r, c = s.block(t)
            X, Y = s.inputs[ri], s.inputs[ci]
            k, dk = term(param, X, Y)
            w = _scaled(G[r, c].copy(), rs, cs)
            if grad_coef is not None:
                grad_coef[t] = (w * k).sum()
            if grad_inscale is not None:
                grad_inscale[t] = coef * (w * dk).sum()
            if grad_inputs and grad_inputs[ri]:      # a symmetric cotangent, as the library asks: the row side, doubled
                dx, dlx = point_grads(param, X, Y)
                g = 2.0 * coef * np.vstack([(w[None] * dx).sum(2), (w * dlx).sum(1)[None]])
                np_capi._mat(grad_inputs[ri], g.shape[0], g.shape[1], g.shape[0])[:, :] += g
        return rc
    return term_grads


def install(monkeypatch):
    """the NumPy double of the C boundary with the Gibbs kind: returns np_capi's context"""
    ctx = np_capi.install(monkeypatch)
    monkeypatch.setattr(np_capi._Spec, "dense", _dense(np_capi._Spec.dense))
    monkeypatch.setattr(np_capi.FakeLib, "_term_grads", _term_grads(np_capi.FakeLib._term_grads))
    return ctx
