"""NumPy double of include/sthenomi_stencil_wo.h, for the CPU suite.

TEST DOUBLE ONLY, on top of tests/stencil_grad_np.py: the shared outputs come from that double's three entry points (a spec
with stencil terms expanded into the plain spec with the same matrix), the cotangent those calls contract is kept as they
pass it to their term sums, and the tables are the direct float64 contraction of the header's four sums against it
(tests/stencil_wo_truth.py).  `install()` routes the host mirror through it.  It says nothing about the HIP kernels."""
import ctypes as C

import numpy as np

import np_capi
import stencil_grad_np
import stencil_wo_truth as WT
from stheno_jl_amd import lib as L


class FakeLib(stencil_grad_np.FakeLib):
    def _term_grads(self, s, G, *args, **kw):
        self._cotangents = getattr(self, "_cotangents", []) + [np.array(G)]     # the call's own G, in the order contracted
        return super()._term_grads(s, G, *args, **kw)

    def _read(self, ref):
        c, s = np_capi._struct(ref), np_capi._Spec(ref)
        return dict(terms=s.terms, inputs=s.inputs, row_len=s.row_len, col_len=s.col_len, symmetric=s.symmetric,
                    stencils=[self._stencils_of(int(c.terms[t].reserved)) for t in range(len(s.terms))])

    def _check(self, who, S, gw, go):
        for t, sts in enumerate(S["stencils"]):
            for side in (0, 1):
                if sts[side] is None and ((gw and gw[2 * t + side]) or (go and go[2 * t + side])):
                    return self._fail(f"{who}: plain side: a grad_weights / grad_offsets entry of a side without a stencil must "
                                      "be NULL")
        return 0

    def _write(self, S, R, gw, go):
        for t, term in enumerate(R):
            for side in (0, 1):
                r = None if term is None else term["sides"][side]
                if r is None:
                    continue
                D, Q = r["o"].shape
                if gw and gw[2 * t + side]:
                    np_capi._vec(gw[2 * t + side], Q)[:] = r["w"]
                if go and go[2 * t + side]:
                    np_capi._vec(go[2 * t + side], D * Q)[:] = r["o"].T.ravel()       # offset q at [q * dim ...]

    def sgp_logpdf_grad_stencil_wo(self, ctx, spec, mean, kind, noise, y, lp_out, gy, gm, gn, gc, gs, gin, gw, go):
        S = self._read(spec)
        if self._check("sgp_logpdf_grad_stencil_wo", S, gw, go):
            return -1
        self._cotangents = []
        rc = self.sgp_logpdf_grad_stencil(ctx, spec, mean, kind, noise, y, lp_out, gy, gm, gn, gc, gs, gin)
        if rc:
            return rc
        self._write(S, WT.contract(S, self._cotangents[0], np.float64), gw, go)
        return 0

    def sgp_kernelmatrix_diag_grad_stencil_wo(self, ctx, spec, w, gc, gs, gin, gw, go):
        S = self._read(spec)
        if self._check("sgp_kernelmatrix_diag_grad_stencil_wo", S, gw, go):
            return -1
        rc = self.sgp_kernelmatrix_diag_grad_stencil(ctx, spec, w, gc, gs, gin)
        if rc:
            return rc
        self._write(S, WT.contract_diag(S, np_capi._vec(w, int(sum(S["row_len"]))), np.float64), gw, go)
        return 0

    def sgp_elbo_grad_stencil_wo(self, ctx, zz, xz, var_x, mean_x, nk, noise_x, zk, z_noise, y, elbo_out, gy, gm, gn, gv, gzn,
                                 gc_zz, gs_zz, gc_xz, gs_xz, gin_zz, gin_xz, gw_zz, go_zz, gw_xz, go_xz):
        Sz, Sx = self._read(zz), self._read(xz)
        if self._check("sgp_elbo_grad_stencil_wo", Sz, gw_zz, go_zz) or self._check("sgp_elbo_grad_stencil_wo", Sx, gw_xz, go_xz):
            return -1
        self._cotangents = []
        rc = self.sgp_elbo_grad_stencil(ctx, zz, xz, var_x, mean_x, nk, noise_x, zk, z_noise, y, elbo_out, gy, gm, gn, gv, gzn,
                                        gc_zz, gs_zz, gc_xz, gs_xz, gin_zz, gin_xz)
        if rc:
            return rc
        dKzz, dKxz = self._cotangents      # (np_capi contracts zz first, then xz)
        self._write(Sz, WT.contract(Sz, dKzz, np.float64), gw_zz, go_zz)
        self._write(Sx, WT.contract(Sx, dKxz, np.float64), gw_xz, go_xz)
        return 0


class FakeContext(stencil_grad_np.FakeContext):
    def __init__(self):
        self.lib, self.handle, self.device, self.is_multi = FakeLib(), C.c_void_p(1), 0, False

    stencil_wo = property(lambda self: self.lib)


def install(monkeypatch):
    """Route the host mirror's calls, the stencil registration and the entry points of sthenomi_stencil_grad.h and
    sthenomi_stencil_wo.h through the double for the duration of one test."""
    ctx = FakeContext()
    monkeypatch.setattr(L, "_default_ctx", ctx)
    monkeypatch.setattr(L, "load", lambda: ctx.lib)
    monkeypatch.setattr(L, "stencil_lib", lambda: ctx.lib)
    monkeypatch.setattr(L, "stencil_grad_lib", lambda: ctx.lib)
    monkeypatch.setattr(L, "stencil_wo_lib", lambda: ctx.lib)
    return ctx
