"""NumPy double of include/sthenomi_stencil_grad.h (and of sgp_stencil_register, include/sthenomi_stencil.h), for the CPU
suite.

TEST DOUBLE ONLY, on top of tests/np_capi.py: a spec with stencil terms is expanded into the plain spec with the same matrix
(tests/stencil_grad_truth.py: a stencil term is the sum of Q_r Q_c plain terms on shifted inputs, the weights in their
coefficients), the plain double computes on it, and the per-term and per-input results are added back onto the owning term
(d_coef weighted by w_p v_q, d_inscale as it is) and input (the sum over its shifted views).  The operators the host mirror
calls around the three gradient entry points (sgp_kernelmatrix, sgp_kernelmatrix_diag, sgp_logpdf, sgp_elbo) expand
likewise.  `install()` routes the host mirror through it, as np_capi.install does.  Patch (convolutional) sides are not
carried here: tests/conv_grad_np.py has them.  It says nothing about the HIP kernels."""
import ctypes as C

import numpy as np

import np_capi
import stencil_grad_truth as ST
from stheno_jl_amd import lib as L


class _Expanded:
    """the plain lib.Spec behind a spec with stencil terms, and how its terms / inputs map back"""

    def __init__(self, ref, stencils_of):
        c = np_capi._struct(ref)
        s = np_capi._Spec(ref)
        nt = len(s.terms)
        S = dict(terms=s.terms, inputs=s.inputs, row_len=s.row_len, col_len=s.col_len, symmetric=s.symmetric,
                 stencils=[stencils_of(int(c.terms[t].reserved)) for t in range(nt)])
        Sx, self.owner, weight, self.in_map = ST.expand(S)
        self.weight = weight.astype(np.float64)
        pairs = {}
        for (I, J, kind, ri, ci, coef, param, rs, cs) in Sx["terms"]:
            pairs.setdefault((I, J), []).append((kind, ri, ci, float(coef), param, rs, cs))
        self.spec = L.Spec(s.row_len, s.col_len, Sx["inputs"], pairs, s.symmetric)
        # (L.Spec lays the terms out pair by pair, each pair's in the order given: the order of Sx["terms"], which follows
        # the caller's terms pair by pair)
        self.ref = C.byref(self.spec.c)
        self.nt, self.ntx, self.inputs = nt, len(Sx["terms"]), s.inputs

    def fold(self, vx, out, weighted):
        """out[t] = the (weighted) sum of the expanded terms' entries of term t"""
        if out:
            v = np.zeros(self.nt)
            np.add.at(v, self.owner, vx[:self.ntx] * (self.weight if weighted else 1.0))
            np_capi._vec(out, self.nt)[:] = v

    def buffers(self):
        gx = [np.zeros(np.asarray(a).shape, order="F") for a in self.spec.inputs]
        return gx, (C.POINTER(C.c_double) * max(1, len(gx)))(*[L.dptr(a) for a in gx])

    def fold_inputs(self, gx, want):
        """want[k] (where asked for) = the sum of the gradients of the shifted views of input k"""
        for k, X in enumerate(self.inputs):
            if not want or not want[k]:
                continue
            tot = np.zeros(X.shape)
            for (kk, _), idx in self.in_map.items():
                if kk == k:
                    for e in idx:
                        tot += gx[e]
            np_capi._mat(want[k], X.shape[0], X.shape[1], X.shape[0])[:, :] = tot


class FakeLib(np_capi.FakeLib):
    def __init__(self):
        super().__init__()
        self.stencils = []          # id k >= 1 is stencils[k - 1]: (offsets D x Q, weights Q)

    # -- include/sthenomi_stencil.h
    def sgp_stencil_register(self, ctx, desc, id_out):
        st = np_capi._struct(desc)
        D, Q = int(st.dim), int(st.npoints)
        if not (1 <= D <= L.STENCIL_MAX_DIM and 1 <= Q <= L.STENCIL_MAX_POINTS):
            return self._fail("sgp_stencil_register: beyond the limits of include/sthenomi_stencil.h")
        A = np_capi._vec(st.offsets, D * Q).reshape(Q, D).T.copy()
        w = np_capi._vec(st.weights, Q).copy()
        for k, (B, v) in enumerate(self.stencils):
            if B.shape == A.shape and np.array_equal(A, B) and np.array_equal(w, v):
                np_capi._struct(id_out).value = k + 1
                return 0
        self.stencils.append((A, w))
        np_capi._struct(id_out).value = len(self.stencils)
        return 0

    def _stencils_of(self, code):
        r, c = code & 0xffff, (code >> 16) & 0xffff
        return (self.stencils[r - 1] if r else None, self.stencils[c - 1] if c else None)

    def _has_stencil(self, ref):
        c = np_capi._struct(ref)
        return any(c.terms[t].reserved for t in range(c.term_ptr[c.n_row_blocks * c.n_col_blocks]))

    def _plain(self, ref):
        """the spec itself when it has no stencil terms, else the reference of its expansion (kept alive on self)"""
        if not self._has_stencil(ref):
            return ref
        self._last = getattr(self, "_last", [])[-7:] + [_Expanded(ref, self._stencils_of)]
        return self._last[-1].ref

    # -- the operators of include/sthenomi.h that run on stencil terms and that the host mirror calls around the gradients
    def sgp_kernelmatrix(self, ctx, spec, K, ldk):
        return super().sgp_kernelmatrix(ctx, self._plain(spec), K, ldk)

    def sgp_kernelmatrix_diag(self, ctx, spec, out):
        return super().sgp_kernelmatrix_diag(ctx, self._plain(spec), out)

    def sgp_logpdf(self, ctx, spec, *args):
        return super().sgp_logpdf(ctx, self._plain(spec), *args)

    def sgp_elbo(self, ctx, zz, xz, *args):
        return super().sgp_elbo(ctx, self._plain(zz), self._plain(xz), *args)

    # -- the gradient entry points of the other headers refuse stencil terms, as the library does
    def _refuse(self, who, *specs):
        if any(self._has_stencil(sp) for sp in specs):
            return self._fail(f"{who}: gradients through stencil terms are not supported")
        return 0

    def sgp_logpdf_grad_xs(self, ctx, spec, *args):
        return self._refuse("sgp_logpdf_grad", spec) or super().sgp_logpdf_grad_xs(ctx, spec, *args)

    def sgp_kernelmatrix_diag_grad_xs(self, ctx, spec, *args):
        return self._refuse("sgp_kernelmatrix_diag_grad", spec) or super().sgp_kernelmatrix_diag_grad_xs(ctx, spec, *args)

    def sgp_elbo_grad_xs(self, ctx, zz, xz, *args):
        return self._refuse("sgp_elbo_grad", zz, xz) or super().sgp_elbo_grad_xs(ctx, zz, xz, *args)

    # -- include/sthenomi_stencil_grad.h
    def _multi(self, ctx, who):
        if getattr(self, "multi_handles", None) and ctx.value in self.multi_handles:
            return self._fail(f"{who}: not supported on a multi-GPU context")
        return 0

    def sgp_logpdf_grad_stencil(self, ctx, spec, mean, kind, noise, y, lp_out, gy, gm, gn, gc, gs, gin):
        if self._multi(ctx, "sgp_logpdf_grad_stencil"):
            return -1
        e = _Expanded(spec, self._stencils_of)
        gcx, gsx = np.zeros(max(1, e.ntx)), np.zeros(max(1, e.ntx))
        gx, ptrs = e.buffers()
        rc = super().sgp_logpdf_grad_xs(ctx, e.ref, mean, kind, noise, y, lp_out, gy, gm, gn, L.dptr(gcx), L.dptr(gsx),
                                        ptrs if gin else None, None)
        if rc:
            return rc
        e.fold(gcx, gc, True)
        e.fold(gsx, gs, False)
        e.fold_inputs(gx, gin)
        return 0

    def sgp_kernelmatrix_diag_grad_stencil(self, ctx, spec, w, gc, gs, gin):
        if self._multi(ctx, "sgp_kernelmatrix_diag_grad_stencil"):
            return -1
        e = _Expanded(spec, self._stencils_of)
        gcx, gsx = np.zeros(max(1, e.ntx)), np.zeros(max(1, e.ntx))
        gx, ptrs = e.buffers()
        rc = super().sgp_kernelmatrix_diag_grad_xs(ctx, e.ref, w, L.dptr(gcx), L.dptr(gsx), ptrs if gin else None, None, None)
        if rc:
            return rc
        e.fold(gcx, gc, True)
        e.fold(gsx, gs, False)
        e.fold_inputs(gx, gin)
        return 0

    def sgp_elbo_grad_stencil(self, ctx, zz, xz, var_x, mean_x, nk, noise_x, zk, z_noise, y, elbo_out, gy, gm, gn, gv, gzn,
                              gc_zz, gs_zz, gc_xz, gs_xz, gin_zz, gin_xz):
        if self._multi(ctx, "sgp_elbo_grad_stencil"):
            return -1
        ez, ex = _Expanded(zz, self._stencils_of), _Expanded(xz, self._stencils_of)
        bufs = [[np.zeros(max(1, e.ntx)) for _ in range(2)] for e in (ez, ex)]
        (gxz, pz), (gxx, px) = ez.buffers(), ex.buffers()
        rc = super().sgp_elbo_grad_xs(ctx, ez.ref, ex.ref, var_x, mean_x, nk, noise_x, zk, z_noise, y, elbo_out, gy, gm, gn, gv,
                                      gzn, L.dptr(bufs[0][0]), L.dptr(bufs[0][1]), L.dptr(bufs[1][0]), L.dptr(bufs[1][1]),
                                      pz if gin_zz else None, px if gin_xz else None, None, None, None)
        if rc:
            return rc
        for e, (bc, bs), gc, gs, gx, gin in ((ez, bufs[0], gc_zz, gs_zz, gxz, gin_zz), (ex, bufs[1], gc_xz, gs_xz, gxx, gin_xz)):
            e.fold(bc, gc, True)
            e.fold(bs, gs, False)
            e.fold_inputs(gx, gin)
        return 0


class FakeContext(np_capi.FakeContext):
    def __init__(self):
        self.lib, self.handle, self.device, self.is_multi = FakeLib(), C.c_void_p(1), 0, False

    stencil_grad = property(lambda self: self.lib)


def install(monkeypatch):
    """Route the host mirror's calls, the stencil registration and the entry points of sthenomi_stencil_grad.h through the
    double for the duration of one test."""
    ctx = FakeContext()
    monkeypatch.setattr(L, "_default_ctx", ctx)
    monkeypatch.setattr(L, "load", lambda: ctx.lib)
    monkeypatch.setattr(L, "stencil_lib", lambda: ctx.lib)
    monkeypatch.setattr(L, "stencil_grad_lib", lambda: ctx.lib)
    return ctx
