"""The NumPy double's version of include/sthenomi_predgrad.h (TEST INFRASTRUCTURE ONLY): what tests/np_capi.py's FakeLib
learns from the words of that header, shared by tests/test_predgrad_on_numpy_double.py and
tests/test_predgrad_truth_on_numpy.py.

  mean_out, var_out : what the double's own predict entry point answers for the same cross / prior_ss / mean_s
  grad_mean_inputs[k][:, i] = sum over the terms with row input k, sum_j alpha_j coef rs_i cs_j kappa'(d2_ij) 2 (xr_i - xc_j)
  grad_var_inputs[k][:, i]  = the same with alpha_j -> -2 B_ij, B = K* C^-1 (sparse: B' Lz^-1 - C' Le^-1 Lz^-1)
  grad_var_prior_inputs     = sgp_kernelmatrix_diag_grad_x(prior_ss, w = 1)
written only for inputs some term reads on its row side; rc < 0 (the message names the entry point and the word): a sharded
posterior ("multi-GPU"), sizes that do not match, a "product" chain or a kind beyond the six plain ones, a term with
reserved != 0 ("patch" / "stencil")."""
import numpy as np
import scipy.linalg as sla

import np_capi
from stheno_jl_amd import lib as L


def _entry(predict, who, sparse):
    def fn(self, post, cross, prior_ss, mean_s, mean_out, var_out, gm, gv, gp):
        self.predgrad_calls.append({"fn": who, "mean_s": bool(mean_s), "var": bool(var_out), "gm": bool(gm), "gv": bool(gv),
                                    "gp": bool(gp)})
        if id(post) in self.sharded:
            return self._fail(who + ": a posterior of a multi-GPU context (sharded factor) has no prediction gradient on the device")
        for ref in (cross, prior_ss):
            if not ref:
                continue
            c = np_capi._struct(ref)
            for t in range(c.term_ptr[c.n_row_blocks * c.n_col_blocks]):
                if c.terms[t].reserved:
                    return self._fail(who + ": gradients through patch (convolutional) / stencil terms are not supported")
                if (int(c.terms[t].kind) & L.KIND_TIMES_PREV) or (int(c.terms[t].kind) & L.KIND_MASK) > L.CONST:
                    return self._fail(who + ": gradients through product chains are not supported")
        sc = np_capi._Spec(cross)
        sp = np_capi._Spec(prior_ss) if prior_ss else None
        fac = self.sposts[id(post)] if sparse else self.posts[id(post)]
        alpha = fac[-1]
        if sc.M != len(alpha) or (sp is not None and (sp.N != sc.N or sp.M != sc.N)):
            return self._fail(who + ": sizes do not match")
        if sp is None and (var_out or gv or gp):
            return self._fail(who + ": prior_ss is required for the variance and its gradients")
        rc = getattr(self, predict)(post, cross, prior_ss, mean_s, mean_out, var_out, None, max(sc.N, 1))
        if rc:
            return rc
        Ks = sc.dense()
        if sparse:
            Lz, Le, _ = fac
            Bp = sla.solve_triangular(Lz, Ks.T, lower=True, check_finite=False)            # B'^T
            Cp = sla.solve_triangular(Le, Bp, lower=True, check_finite=False)              # C'^T
            Bt = sla.solve_triangular(Lz, Bp - sla.solve_triangular(Le, Cp, lower=True, trans="T", check_finite=False),
                                      lower=True, trans="T", check_finite=False)
        else:
            Bt = sla.cho_solve((fac[0], True), Ks.T, check_finite=False)
        Bm = Bt.T
        om = [np.zeros(X.shape) for X in sc.inputs]
        ov = [np.zeros(X.shape) for X in sc.inputs]
        row_read = [False] * len(sc.inputs)
        for t, (I, J, kind, ri, ci, coef, param, rs, cs) in enumerate(sc.terms):
            r, c = sc.block(t)
            row_read[ri] = True
            core = 2.0 * coef * np_capi._dkern_dd2(kind, sc.d2(t))
            if rs is not None:
                core = rs[:, None] * core
            if cs is not None:
                core = core * cs[None, :]
            diff = sc.inputs[ri][:, :, None] - sc.inputs[ci][:, None, :]
            om[ri] += ((core * alpha[c][None, :])[None, :, :] * diff).sum(2)
            ov[ri] += ((-2.0 * core * Bm[r, c])[None, :, :] * diff).sum(2)
        for ptrs, arrs in ((gm, om), (gv, ov)):
            for k, g in enumerate(arrs):
                if ptrs and ptrs[k] and row_read[k] and g.size:
                    np_capi._mat(ptrs[k], g.shape[0], g.shape[1], g.shape[0])[:, :] = g
        if gp:
            w = np.ones(max(sp.N, 1))
            return self.sgp_kernelmatrix_diag_grad_xs(None, prior_ss, L.dptr(w), None, None, gp, None, None)
        return 0
    return fn


ENTRY = {
    "sgp_posterior_predict_grad_x": _entry("sgp_posterior_predict", "sgp_posterior_predict_grad_x", False),
    "sgp_sparse_posterior_predict_grad_x": _entry("sgp_sparse_posterior_predict", "sgp_sparse_posterior_predict_grad_x", True),
}


def install(monkeypatch):
    """np_capi.install plus the two entry points; Context.predgrad is the double itself (it serves every library)"""
    ctx = np_capi.install(monkeypatch)
    assert sorted(ENTRY) == L.predgrad_symbols()
    for name, fn in ENTRY.items():
        monkeypatch.setattr(np_capi.FakeLib, name, fn, raising=False)
    ctx.lib.predgrad_calls, ctx.lib.sharded = [], set()
    ctx.predgrad = ctx.lib
    return ctx
