"""NumPy (float64) formulas of the derivative kinds (csrc/deriv_eval.h) in the library's own formulation and operation order,
and the NumPy double of the C boundary (tests/np_capi.py) taught to evaluate and contract them.  TEST INFRASTRUCTURE ONLY
(tests/test_deriv_truth_on_numpy.py holds the formulas to the 80-digit table; tests/test_gpu_deriv.py holds the library to
them).

A term of kind 32 + base with param = 17 a + b is, with u = x - y, s = |u|^2 and the pair's coefficients (A, B) -- and
(GA, GB, GC) for the input-scale derivative --
    (p+1, 0)  A u_p        (0, q+1)  -(A u_q)        (p+1, q+1)  (B u_p) u_q - A delta_pq
exactly 0 where the exponential underflowed (`dead`).

install(monkeypatch) makes np_capi's spec evaluator and term contraction know the three kinds, for the duration of a test."""
import numpy as np

import np_capi
from stheno_jl_amd import lib as L

DERIV_KINDS = tuple(L.DERIV_OF.values())
TINY_S, UP, DOWN = 1e-290, 2.0 ** 480, 2.0 ** -480
SQRT3, SQRT5, Q3 = 1.7320508075688772, 2.23606797749979, 5.196152422706632


def is_deriv(kind):
    return (int(kind) & L.KIND_MASK) in DERIV_KINDS


def sides(param):
    return divmod(int(param), L.DERIV_PARAM_BASE)


def differences(X, Y):
    """u (D x n x m) and s = sum_d u_d^2, d ascending"""
    u = X[:, :, None] - Y[:, None, :]
    s = np.zeros(u.shape[1:])
    for d in range(u.shape[0]):
        s = u[d] * u[d] + s
    return u, s


def pair_coefficients(base, u, s):
    """dict(A, B, GA, GB, GC, dead) of deriv_eval.h: deriv_pair"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if base == L.SE:
            E = np.exp(np.maximum(-0.5 * s, -800.0))
            out = dict(A=-E, B=-E, GA=E * (s - 1.0), GB=E * (s - 2.0), GC=-(E * s))
        elif base == L.MATERN32:
            up = s < TINY_S
            sr = np.where(up, ((u * UP) ** 2).sum(0) if up.any() else s, s)
            a = np.minimum(np.maximum(sr, 1e-300), 1e300)
            r = np.sqrt(a)
            rinv = 1.0 / r
            r, rinv = np.where(up, r * DOWN, r), np.where(up, rinv * UP, rinv)
            zero = sr == 0.0
            r, rinv = np.where(zero, 0.0, r), np.where(zero, 0.0, rinv)
            l = SQRT3 * r
            E = np.exp(np.maximum(-l, -800.0))
            E3, Eq = 3.0 * E, Q3 * E
            out = dict(A=-E3, B=-(Eq * rinv), GA=E3 * (l - 1.0), GB=(Eq * (l - 1.0)) * rinv, GC=-(Eq * r))
        elif base == L.MATERN52:
            l = SQRT5 * np.sqrt(np.minimum(np.maximum(s, 1e-300), 1e300))
            E = np.exp(np.maximum(-l, -800.0))
            E53, E253 = 1.6666666666666667 * E, 8.333333333333334 * E
            out = dict(A=-((1.0 + l) * E53), B=-E253, GA=E53 * ((5.0 * s - 1.0) - l), GB=E253 * (l - 2.0), GC=-(E253 * s))
        else:
            raise ValueError(base)
    out["dead"] = E == 0.0
    return out


def _entry(a, b, ca, cb, cd, u, dead):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if b == 0:
            v = ca * u[a - 1]
        elif a == 0:
            v = -(ca * u[b - 1])
        else:
            v = (cb * u[a - 1]) * u[b - 1] + (cd if a == b else 0.0)
    return np.where(dead, 0.0, v)


def term(kind, param, X, Y):
    """(value, input-scale derivative) of one term per pair of points, without coef and scales"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    a, b = sides(param)
    u, s = differences(X, Y)
    c = pair_coefficients((int(kind) & L.KIND_MASK) - L.DERIV_SE, u, s)
    return (_entry(a, b, c["A"], c["B"], -c["A"], u, c["dead"]), _entry(a, b, c["GA"], c["GB"], c["GC"], u, c["dead"]))


def dense_from_spec(spec):
    """np_terms.dense_from_spec for a lib.Spec that may hold derivative terms (no mirroring: every pair as its terms say)"""
    import np_terms
    roff = np.concatenate([[0], np.cumsum(spec.row_len)])
    coff = np.concatenate([[0], np.cumsum(spec.col_len)])
    K = np.zeros((spec.N, spec.M))
    for (I, J, kind, ri, ci, coef, param, rs, cs) in np_terms.spec_terms(spec):
        X, Y = spec.inputs[ri], spec.inputs[ci]
        if is_deriv(kind):
            blk = coef * term(kind, param, X, Y)[0]
        else:
            blk = coef * np_terms._kern(kind, differences(X, Y)[1], param)
        if rs is not None:
            blk = rs[:, None] * blk
        if cs is not None:
            blk = blk * cs[None, :]
        K[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += blk
    return K


def _dense(before):
    def dense(self):
        if not any(is_deriv(t[2]) for t in self.terms):
            return before(self)
        K = np.zeros((self.N, self.M))
        for t, (I, J, kind, ri, ci, coef, param, rs, cs) in enumerate(self.terms):
            r, c = self.block(t)
            if is_deriv(kind):
                blk = coef * term(kind, param, self.inputs[ri], self.inputs[ci])[0]
            else:
                blk = coef * np_capi._kern(kind, self.d2(t), param)
            if rs is not None:
                blk = rs[:, None] * blk
            if cs is not None:
                blk = blk * cs[None, :]
            K[r, c] += blk
        if self.symmetric:
            K = np.tril(K) + np.tril(K, -1).T
        return K
    return dense


def _term_grads(before):
    def term_grads(self, s, G, grad_coef, grad_inscale, grad_inputs, grad_rowscale, grad_colscale=None):
        dv = [t for t, T in enumerate(s.terms) if is_deriv(T[2])]
        if not dv:
            return before(self, s, G, grad_coef, grad_inscale, grad_inputs, grad_rowscale, grad_colscale)
        if grad_inputs or grad_rowscale or grad_colscale:
            return self._fail("input-point and scale gradients through derivative terms are not supported")
        kept = list(s.terms)
        for t in dv:       # the plain terms go through the double's own contraction, the derivative terms stand aside as zeros
            I, J, _, ri, ci, _, _, rs, cs = kept[t]
            s.terms[t] = (I, J, L.CONST, ri, ci, 0.0, 0.0, rs, cs)
        rc = before(self, s, G, grad_coef, grad_inscale, None, None, None)
        s.terms[:] = kept
        for t in dv:
            (I, J, kind, ri, ci, coef, param, rs, cs) = s.terms[t]
            r, c = s.block(t)
            k, dk = term(kind, param, s.inputs[ri], s.inputs[ci])
            w = G[r, c].copy()
            if rs is not None:
                w = w * rs[:, None]
            if cs is not None:
                w = w * cs[None, :]
            if grad_coef is not None:
                grad_coef[t] = (w * k).sum()
            if grad_inscale is not None:
                grad_inscale[t] = coef * (w * dk).sum()
        return rc
    return term_grads


def install(monkeypatch):
    """the NumPy double of the C boundary with the derivative kinds: returns np_capi's context"""
    ctx = np_capi.install(monkeypatch)
    monkeypatch.setattr(np_capi._Spec, "dense", _dense(np_capi._Spec.dense))
    monkeypatch.setattr(np_capi.FakeLib, "_term_grads", _term_grads(np_capi.FakeLib._term_grads))
    return ctx
