"""NumPy double of include/sthenomi_conv_grad.h (and of sgp_conv_geom, include/sthenomi_conv.h), for the CPU suite.

TEST DOUBLE ONLY, on top of tests/np_capi.py: a spec with patch terms is expanded into the plain spec with the same matrix
(tests/conv_grad_truth.py: a patch term is the sum over patch positions of plain terms on patch-extracted inputs), the plain
double computes on it, and the per-term results are added back onto the owning term.  The operators the host mirror calls
around the three gradient entry points (sgp_kernelmatrix, sgp_kernelmatrix_diag, sgp_logpdf, sgp_elbo) expand likewise.
`install()` routes the host mirror through it, as np_capi.install does.  It says nothing about the HIP kernels."""
import ctypes as C

import numpy as np

import conv_grad_truth as CT
import np_capi
from stheno_jl_amd import lib as L


class _Expanded:
    """the plain lib.Spec behind a spec with patch terms, and how its terms / inputs map back"""

    def __init__(self, ref, geoms_of):
        c = np_capi._struct(ref)
        s = np_capi._Spec(ref)
        nt = len(s.terms)
        S = dict(terms=s.terms, inputs=s.inputs, row_len=s.row_len, col_len=s.col_len, symmetric=s.symmetric,
                 geoms=[geoms_of(int(c.terms[t].reserved)) for t in range(nt)])
        Sx, self.owner, self.in_map = CT.expand(S)
        pairs = {}
        for (I, J, kind, ri, ci, coef, param, rs, cs) in Sx["terms"]:
            pairs.setdefault((I, J), []).append((kind, ri, ci, coef, param, rs, cs))
        self.spec = L.Spec(s.row_len, s.col_len, Sx["inputs"], pairs, s.symmetric)
        self.ref = C.byref(self.spec.c)
        self.nt, self.ntx, self.n_inputs = nt, len(Sx["terms"]), len(s.inputs)
        self.images = {k for (k, geom) in self.in_map if geom is not None}

    def fold(self, vx, out):
        """out[t] = the sum of the expanded terms' entries of term t"""
        if out:
            v = np.zeros(self.nt)
            np.add.at(v, self.owner, vx[:self.ntx])
            np_capi._vec(out, self.nt)[:] = v


class FakeLib(np_capi.FakeLib):
    def __init__(self):
        super().__init__()
        self.geoms = []          # id k >= 1 is geoms[k - 1]

    # -- include/sthenomi_conv.h
    def sgp_conv_geom(self, ctx, geom, id_out):
        g = np_capi._struct(geom)
        key = (int(g.height), int(g.width), int(g.patch_h), int(g.patch_w))
        if key not in self.geoms:
            self.geoms.append(key)
        np_capi._struct(id_out).value = self.geoms.index(key) + 1
        return 0

    def _geoms_of(self, code):
        r, c = code & 0xffff, (code >> 16) & 0xffff
        return (self.geoms[r - 1] if r else None, self.geoms[c - 1] if c else None)

    def _plain(self, ref):
        """the spec itself when it has no patch terms, else the reference of its expansion (kept alive on self)"""
        c = np_capi._struct(ref)
        nt = c.term_ptr[c.n_row_blocks * c.n_col_blocks]
        if not any(c.terms[t].reserved for t in range(nt)):
            return ref
        self._last = _Expanded(ref, self._geoms_of)
        return self._last.ref

    # -- the operators of include/sthenomi.h that run on patch terms and that the host mirror calls around the gradients
    def sgp_kernelmatrix(self, ctx, spec, K, ldk):
        return super().sgp_kernelmatrix(ctx, self._plain(spec), K, ldk)

    def sgp_kernelmatrix_diag(self, ctx, spec, out):
        return super().sgp_kernelmatrix_diag(ctx, self._plain(spec), out)

    def sgp_logpdf(self, ctx, spec, *args):
        return super().sgp_logpdf(ctx, self._plain(spec), *args)

    def sgp_elbo(self, ctx, zz, xz, *args):
        return super().sgp_elbo(ctx, self._plain(zz), self._plain(xz), *args)

    # -- include/sthenomi_conv_grad.h
    def sgp_logpdf_grad_conv(self, ctx, spec, mean, kind, noise, y, lp_out, gy, gm, gn, gc, gs):
        e = _Expanded(spec, self._geoms_of)
        gcx, gsx = np.zeros(max(1, e.ntx)), np.zeros(max(1, e.ntx))
        rc = self.sgp_logpdf_grad(ctx, e.ref, mean, kind, noise, y, lp_out, gy, gm, gn, L.dptr(gcx), L.dptr(gsx))
        if rc:
            return rc
        e.fold(gcx, gc)
        e.fold(gsx, gs)
        return 0

    def sgp_kernelmatrix_diag_grad_conv(self, ctx, spec, w, gc, gs):
        e = _Expanded(spec, self._geoms_of)
        gcx, gsx = np.zeros(max(1, e.ntx)), np.zeros(max(1, e.ntx))
        rc = self.sgp_kernelmatrix_diag_grad(ctx, e.ref, w, L.dptr(gcx), L.dptr(gsx))
        if rc:
            return rc
        e.fold(gcx, gc)
        e.fold(gsx, gs)
        return 0

    def sgp_elbo_grad_conv(self, ctx, zz, xz, var_x, mean_x, nk, noise_x, zk, z_noise, y, elbo_out, gy, gm, gn, gv, gzn,
                           gc_zz, gs_zz, gc_xz, gs_xz, gin_zz, gin_xz):
        ez, ex = _Expanded(zz, self._geoms_of), _Expanded(xz, self._geoms_of)
        for e, gin in ((ez, gin_zz), (ex, gin_xz)):
            if gin and any(gin[k] for k in e.images):
                return self._fail("sgp_elbo_grad_conv: an input read by a patch (convolutional) side holds images, and "
                                  "gradients with respect to images are not supported: its grad_inputs entry must be NULL")
        bufs = [[np.zeros(max(1, e.ntx)) for _ in range(2)] for e in (ez, ex)]
        gxs = [[np.zeros(np.asarray(a).shape, order="F") for a in e.spec.inputs] for e in (ez, ex)]
        ptrs = [(C.POINTER(C.c_double) * max(1, len(g)))(*[L.dptr(a) for a in g]) for g in gxs]
        rc = self.sgp_elbo_grad_x(ctx, ez.ref, ex.ref, var_x, mean_x, nk, noise_x, zk, z_noise, y, elbo_out, gy, gm, gn, gv,
                                  gzn, L.dptr(bufs[0][0]), L.dptr(bufs[0][1]), L.dptr(bufs[1][0]), L.dptr(bufs[1][1]),
                                  ptrs[0] if gin_zz else None, ptrs[1] if gin_xz else None)
        if rc:
            return rc
        for e, (bc, bs), gc, gs, gx, gin in ((ez, bufs[0], gc_zz, gs_zz, gxs[0], gin_zz), (ex, bufs[1], gc_xz, gs_xz, gxs[1], gin_xz)):
            e.fold(bc, gc)
            e.fold(bs, gs)
            for (k, geom), idx in e.in_map.items():
                if gin and geom is None and gin[k]:
                    a = gx[idx[0]]
                    np_capi._mat(gin[k], a.shape[0], a.shape[1], a.shape[0])[:, :] = a
        return 0


class FakeContext(np_capi.FakeContext):
    def __init__(self):
        self.lib, self.handle, self.device, self.is_multi = FakeLib(), C.c_void_p(1), 0, False

    conv_grad = property(lambda self: self.lib)


def install(monkeypatch):
    """Route the host mirror's calls, the geometry registration and the entry points of sthenomi_conv_grad.h through the
    double for the duration of one test."""
    ctx = FakeContext()
    monkeypatch.setattr(L, "_default_ctx", ctx)
    monkeypatch.setattr(L, "load", lambda: ctx.lib)
    monkeypatch.setattr(L, "conv_lib", lambda: ctx.lib)
    monkeypatch.setattr(L, "conv_grad_lib", lambda: ctx.lib)
    return ctx
