"""Input-point, function-scale and ELBO gradients through product chains without a GPU: the NumPy evaluator
(tests/kprod_grad_np.py) against central differences of its own matrix, the extension header include/sthenomi_kprod_grad.h
(plain C, exactly what libsthenomi_kprod_grad.so exports and lib.py types), the host functions logpdf_and_gradient_param /
elbo_and_gradient_param over a NumPy double of the three entry points, and the refusals."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import kprod_grad_np as kg
import kprod_np as kn
import np_capi
import stheno_jl_amd as P
from np_capi import _mat, _vec
from stheno_jl_amd import lib as L
from test_capi_symbols import _c_exports, _symbols_of
from test_julia_shim_static import _ctypes_kind
from test_kprod_on_numpy import golden_kernel, np_logpdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.filterwarnings("error::DeprecationWarning")
SYMS = ["sgp_elbo_grad_param", "sgp_kernelmatrix_diag_grad_param", "sgp_logpdf_grad_param_xs"]


def _atom(kernel):
    return P.atomic(P.GP(kernel), P.GPC())


def _model(kernel):
    return P.gppp(lambda GP: {"f": GP(kernel)})


def every_kind():
    """a chain of eight with every kind but WHITE, over different views (with_lengthscale), and LINEAR beside them"""
    wl = P.with_lengthscale
    return 0.8 * (wl(P.SEKernel(), 2.0) * wl(P.Matern12Kernel(), 3.0) * wl(P.Matern32Kernel(), 2.5) * P.Matern52Kernel() *
                  P.RationalQuadraticKernel(1.3) * P.LinearKernel(1.0) * P.ConstantKernel(1.1) * wl(P.SEKernel(), 4.0))


def shared_input():
    """factors that read ONE spec input (no transform on any of them), a WHITE factor, and a plain term"""
    return (1.3 * P.SEKernel() * P.Matern32Kernel() * P.LinearKernel(0.5) + 0.6 * P.Matern52Kernel() * P.WhiteKernel() +
            0.4 * P.Matern12Kernel() + 0.2 * P.PolynomialKernel(2, 0.3))


# ---- 1. the evaluator against central differences of its own matrix -----------------------------------------------------
def _fd_inputs(spec, value, h=1e-6):
    out = []
    for X in spec.inputs:
        g = np.zeros(X.shape)
        for d in range(X.shape[0]):
            for i in range(X.shape[1]):
                x0 = X[d, i]
                X[d, i] = x0 + h
                fp = value()
                X[d, i] = x0 - h
                fn = value()
                X[d, i] = x0
                g[d, i] = (fp - fn) / (2 * h)
        out.append(g)
    return out


def _scale_vectors(spec):
    """{id: (vector, [(term, side)])} over the scale vectors of a spec"""
    vecs = {}
    for t in range(spec.n_terms):
        for side, v in (("row", spec.term_row_scale[t]), ("col", spec.term_col_scale[t])):
            if v is not None:
                vecs.setdefault(id(v), (v, []))[1].append((t, side))
    return vecs


def _fd_vector(v, value, h=1e-6):
    g = np.zeros(len(v))
    for i in range(len(v)):
        v0 = v[i]
        v[i] = v0 + h
        fp = value()
        v[i] = v0 - h
        fn = value()
        v[i] = v0
        g[i] = (fp - fn) / (2 * h)
    return g


FD_TOL = 2e-8   # central differences at h = 1e-6 of sums of O(1) smooth entries: h^2 f''' / 6 + eps |f| / h ~ 1e-9


def _near(a, e, tol=FD_TOL):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(e)))) <= tol * max(1.0, float(np.max(np.abs(e))))


@pytest.mark.parametrize("kernel,D", [(every_kind, 1), (every_kind, 3), (shared_input, 2), (golden_kernel, 1)])
@pytest.mark.parametrize("shape", ["symmetric", "rectangular"])
def test_evaluator_matches_central_differences_of_its_own_matrix(kernel, D, shape):
    rng = np.random.default_rng(3 + D)
    sigma = lambda v: 1.0 + 0.5 * float(np.sin(np.sum(v)))      # noqa: E731
    F = P.gppp(lambda GP: (lambda f: {"f": f, "g": sigma * f})(GP(kernel())))
    pts = lambda n: (rng.standard_normal(n) if D == 1 else P.ColVecs(np.asfortranarray(rng.standard_normal((D, n)))))      # noqa: E731
    x = P.BlockData([P.GPPPInput("g", pts(5)), P.GPPPInput("f", pts(4))])
    if shape == "symmetric":
        spec, _, _ = P.build_spec(F, x)
        G = rng.standard_normal((9, 9))
        G = G + G.T
    else:
        spec, _, _ = P.build_spec(F, x, None, P.BlockData([P.GPPPInput("f", pts(3)), P.GPPPInput("g", pts(4))]))
        G = rng.standard_normal((9, 7))
    assert spec.has_kprod
    value = lambda: float(np.sum(G * kn.np_spec_matrix(spec)))      # noqa: E731
    ev = kg.np_input_grads(spec, G)
    for k, fd in enumerate(_fd_inputs(spec, value)):
        assert _near(ev["row"][k] + ev["col"][k], fd), k
        if shape == "symmetric":      # the device's convention: the row side twice
            assert _near(2.0 * ev["row"][k], fd), k
    seen = 0
    for v, users in _scale_vectors(spec).values():
        want = sum(ev["rs" if side == "row" else "cs"][t] for t, side in users)
        assert _near(want, _fd_vector(v, value)), users
        seen += 1
    assert seen >= 1


def test_evaluator_of_the_diagonal_matches_central_differences():
    """var(f(a x) + f(b x)) with every kind (two views: the distance kinds do not cancel), and LINEAR / Polynomial with one
    array on both sides (both sides add); scale vectors on the diagonal"""
    rng = np.random.default_rng(8)
    sigma = lambda v: 1.0 + 0.5 * float(np.sin(np.sum(v)))      # noqa: E731
    for kernel, two_views in ((every_kind, True), (shared_input, True), (shared_input, False)):
        if two_views:
            F = P.gppp(lambda GP: (lambda f: {"f": f, "g": sigma * (P.stretch(f, 0.7) + P.stretch(f, 1.6))})(GP(kernel())))
        else:
            F = P.gppp(lambda GP: (lambda f: {"f": f, "g": sigma * f})(GP(kernel())))
        x = P.BlockData([P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((2, n))))) for n in (5, 4)])
        spec, _, _ = P.build_spec(F, x)
        w = rng.standard_normal(9)
        value = lambda: float(np.sum(w * kg.np_diag(spec)))      # noqa: E731
        ev = kg.np_diag_grads(spec, w)
        fds = _fd_inputs(spec, value)
        for k, fd in enumerate(fds):
            assert _near(ev["gx"][k], fd), (kernel.__name__, two_views, k)
        assert max(np.max(np.abs(fd)) for fd in fds) > 1e-3      # LINEAR alone moves the diagonal on one view
        for v, users in _scale_vectors(spec).values():
            want = sum(ev["rs" if side == "row" else "cs"][t] for t, side in users if ev["rs" if side == "row" else "cs"][t] is not None)
            assert _near(want, _fd_vector(v, value)), users
        # d / d coef, inscale and param: the contraction of kprod_np with the diagonal matrix of w
        ec, es, ep = kn.np_contract(spec, np.diag(w))
        assert _near(ev["gc"], ec, 1e-12) and _near(ev["gs"], es, 1e-12) and _near(ev["gp"], ep, 1e-12)


def test_times_constant_one_in_the_evaluator():
    """the bound tests/test_gpu_kprod_grad.py uses between `k * ConstantKernel(1)` and `k`: the evaluator's two forms differ
    by multiplications with 1.0 only -- its own need is 0; the device bound is derived there from the summation length"""
    rng = np.random.default_rng(5)
    X = P.ColVecs(np.asfortranarray(rng.standard_normal((3, 9))))
    G = rng.standard_normal((9, 9))
    for k in (P.SEKernel, P.Matern12Kernel, P.Matern32Kernel, P.Matern52Kernel):
        plain, _, _ = P.build_spec(_model(1.7 * P.with_lengthscale(k(), 0.6)), P.GPPPInput("f", X))
        chained, _, _ = P.build_spec(_model(1.7 * P.with_lengthscale(k(), 0.6) * P.ConstantKernel(1.0)), P.GPPPInput("f", X))
        a, b = kg.np_input_grads(plain, G), kg.np_input_grads(chained, G)
        tot = lambda e: sum(np.abs(r).sum() for r in e["row"])      # noqa: E731
        need = abs(tot(a) - tot(b)) / tot(a)
        print(f"{k.__name__}: evaluator's need {need:.2e}")
        assert need <= 1e-15


# ---- 2. the extension header ----------------------------------------------------------------------------------------------
def test_header_library_and_signature_tables_agree():
    syms = _symbols_of("sthenomi_kprod_grad.h")
    assert syms == SYMS == L.kprod_grad_symbols()
    assert _c_exports(L.KPROD_GRAD_LIB_PATH) == syms
    for other in (L.LIB_PATH, L.KPROD_LIB_PATH, L.BATCH_LIB_PATH, L.POOL_LIB_PATH):
        assert not set(syms) & set(_c_exports(other))
    assert not set(syms) & set(_symbols_of("sthenomi.h")) and not set(syms) & set(_symbols_of("sthenomi_kprod.h"))
    assert _c_exports(L.LIB_PATH) == _symbols_of("sthenomi.h")              # the product library exports what it did
    assert _c_exports(L.KPROD_LIB_PATH) == _symbols_of("sthenomi_kprod.h")
    lib = L.kprod_grad_lib()
    assert all(hasattr(lib, s) for s in syms) and isinstance(L.Context.kprod_grad, property)
    # argument by argument against the header's prototypes (the style of tests/test_extend_abi_static.py)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sthenomi_kprod_grad.h")).read(), flags=re.S)
    counts = {}
    for name in SYMS:
        proto = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
        kinds = []
        for arg in proto.split(","):
            arg = " ".join(arg.split())
            kinds.append("ptr" if "*" in arg else "i64" if arg.startswith("int64_t") else "i32" if arg.startswith("int ") else "?")
        res, args = L._SIGS_KPROD_GRAD[name]
        assert _ctypes_kind(res) == "i32"
        assert [_ctypes_kind(a) for a in args] == kinds, name
        counts[name] = len(kinds)
    assert counts == {"sgp_logpdf_grad_param_xs": 15, "sgp_kernelmatrix_diag_grad_param": 9, "sgp_elbo_grad_param": 27}


def test_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "kprod_grad_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_kprod_grad.h"
int main(int argc, char** argv) {
  typedef int (*lp_t)(sgp_ctx*, const sgp_cov_spec*, const double*, int, const double*, const double*, double*, double*,
                      double*, double*, double*, double*, double*, double* const*, double* const*);
  typedef int (*dg_t)(sgp_ctx*, const sgp_cov_spec*, const double*, double*, double*, double*, double* const*, double* const*,
                      double* const*);
  typedef int (*el_t)(sgp_ctx*, const sgp_cov_spec*, const sgp_cov_spec*, const double*, const double*, int, const double*, int,
                      const double*, const double*, double*, double*, double*, double*, double*, double*, double*, double*,
                      double*, double*, double*, double*, double* const*, double* const*, double* const*, double* const*,
                      double* const*);
  lp_t a = 0;
  dg_t b = 0;
  el_t c = 0;
  void* h;
  printf("fnptr %d %d %d\n", (int)sizeof(a = &sgp_logpdf_grad_param_xs), (int)sizeof(b = &sgp_kernelmatrix_diag_grad_param),
         (int)sizeof(c = &sgp_elbo_grad_param));
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  printf("%s\n", dlsym(h, "sgp_logpdf_grad_param_xs") && dlsym(h, "sgp_kernelmatrix_diag_grad_param") &&
                 dlsym(h, "sgp_elbo_grad_param") ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "kprod_grad_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, L.KPROD_GRAD_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "8", "8", "8", "resolved"], (out.stdout, out.stderr)


# ---- 3. the host functions over a NumPy double of the three entry points ------------------------------------------------------
class FakeKprodGrad:
    """include/sthenomi_kprod_grad.h in NumPy, on the lib.Spec objects themselves (found again through `specs`, which the
    patched Spec.ref fills): kprod_np for the matrix and the term contractions, kprod_grad_np for inputs and scales"""

    def __init__(self):
        self.specs = {}

    def _spec(self, ref):
        return self.specs[C.addressof(ref._obj)]

    @staticmethod
    def _put_terms(dst, src, n):
        if dst:
            _vec(dst, n)[:] = src

    @staticmethod
    def _put_inputs(dst, arrs):
        for k, g in enumerate(arrs):
            if dst and dst[k]:
                _mat(dst[k], g.shape[0], g.shape[1], g.shape[0])[:, :] = g

    @staticmethod
    def _put_scales(dst, arrs, factor=1.0):
        for t, g in enumerate(arrs):
            if dst and dst[t] and g is not None:
                _vec(dst[t], len(g))[:] = factor * g

    def sgp_kernelmatrix_diag(self, ctx, spec, out):
        s = self._spec(spec)
        _vec(out, s.N)[:] = kg.np_diag(s)
        return 0

    def sgp_logpdf_grad_param_xs(self, ctx, spec, mean, kind, noise, y, lp, gy, gm, gn, gc, gs, gp, gin, grs):
        s = self._spec(spec)
        n = s.N
        assert kind == L.NOISE_SCALAR
        Cm = kn.np_spec_matrix(s) + noise[0] * np.eye(n)
        delta = _vec(y, n) - (_vec(mean, n) if mean else 0.0)
        Li = sla.solve_triangular(np.linalg.cholesky(Cm), np.eye(n), lower=True)      # (the library's route: C^-1 = L^-T L^-1)
        Ci = Li.T @ Li
        al = Li.T @ (Li @ delta)
        G = 0.5 * (np.outer(al, al) - Ci)
        lp[0] = np_logpdf(Cm, delta)
        _vec(gy, n)[:] = -al
        _vec(gm, n)[:] = al
        gn[0] = np.trace(G)
        for dst, src in zip((gc, gs, gp), kn.np_contract(s, G)):
            self._put_terms(dst, src, s.n_terms)
        ev = kg.np_input_grads(s, G)
        self._put_inputs(gin, [2.0 * r for r in ev["row"]])
        self._put_scales(grs, ev["rs"], 2.0)
        return 0

    def sgp_kernelmatrix_diag_grad_param(self, ctx, spec, w, gc, gs, gp, gin, grs, gcs):
        s = self._spec(spec)
        ev = kg.np_diag_grads(s, _vec(w, s.N))
        for dst, key in ((gc, "gc"), (gs, "gs"), (gp, "gp")):
            self._put_terms(dst, ev[key], s.n_terms)
        self._put_inputs(gin, ev["gx"])
        self._put_scales(grs, ev["rs"])
        self._put_scales(gcs, ev["cs"])
        return 0

    def sgp_elbo_grad_param(self, ctx, zz, xz, var_x, mean_x, nk, noise_x, zk, z_noise, y, elbo_out, gy, gm, gn, gv, gzn,
                            gcz, gsz, gpz, gcx, gsx, gpx, gin_zz, gin_xz, grs_zz, grs_xz, gcs_xz):
        sz, sx = self._spec(zz), self._spec(xz)
        M, N = sz.N, sx.N
        assert nk == L.NOISE_SCALAR and zk == L.NOISE_SCALAR
        s2 = noise_x[0]
        v = _vec(var_x, N)
        resid = _vec(y, N) - (_vec(mean_x, N) if mean_x else 0.0)
        elbo_out[0], (dKzz, dKxz, dy, dsy) = titsias(kn.np_spec_matrix(sz) + z_noise[0] * np.eye(M), kn.np_spec_matrix(sx), v,
                                                    resid, s2, cotangents=True)
        _vec(gy, N)[:] = dy
        _vec(gm, N)[:] = -dy
        gn[0] = dsy
        _vec(gv, N)[:] = -0.5 / s2
        gzn[0] = np.trace(dKzz)
        for dsts, s, G in (((gcz, gsz, gpz), sz, dKzz), ((gcx, gsx, gpx), sx, dKxz)):
            for dst, src in zip(dsts, kn.np_contract(s, G)):
                self._put_terms(dst, src, s.n_terms)
        ez, ex = kg.np_input_grads(sz, dKzz), kg.np_input_grads(sx, dKxz)
        self._put_inputs(gin_zz, [2.0 * r for r in ez["row"]])
        self._put_inputs(gin_xz, [r + c for r, c in zip(ex["row"], ex["col"])])
        self._put_scales(grs_zz, ez["rs"], 2.0)
        self._put_scales(grs_xz, ex["rs"])
        self._put_scales(gcs_xz, ex["cs"])
        return 0


def titsias(Kzz, Kxz, var_x, y, s2, cotangents=False):
    """the Titsias bound from NumPy matrices (Kzz with its jitter), and its cotangents (oracle/abstractgps.py's derivation)"""
    M, N = Kzz.shape[0], Kxz.shape[0]
    Lz = np.linalg.cholesky(Kzz)
    Lzi = sla.solve_triangular(Lz, np.eye(M), lower=True)
    rsig = 1.0 / np.sqrt(s2)                                   # (Lambda = diag(s2)^-1/2, applied as a product)
    A = (Lzi @ Kxz.T) * rsig                                   # (through Lz^-1, the library's route)
    Bm = A @ A.T + np.eye(M)
    Le = np.linalg.cholesky(Bm)
    delta = y * rsig
    b = sla.solve_triangular(Le, A @ delta, lower=True)
    val = -0.5 * (N * np.log(2.0 * np.pi) + N * np.log(s2) + 2.0 * np.log(np.diag(Le)).sum() + delta @ delta - b @ b) \
        - 0.5 * (np.sum(var_x) / s2 - np.sum(A * A))
    if not cotangents:
        return float(val)
    Lei = sla.solve_triangular(Le, np.eye(M), lower=True)      # (B^-1 = Le^-T Le^-1, the library's route)
    u = Lei.T @ b
    Binv = Lei.T @ Lei
    Z = np.eye(M) - Binv - np.outer(u, u)
    S = Bm + Binv - 2.0 * np.eye(M) + np.outer(u, u)
    J = Lzi.T
    dA_T = A.T @ Z + np.outer(delta, u)
    ddelta = -delta + A.T @ u
    dsy = -0.5 / s2 + 0.5 * var_x / s2 ** 2 - 0.5 * (ddelta * delta + (A.T * dA_T).sum(1)) / s2
    return float(val), ((-0.5 * J @ S @ J.T), (dA_T @ J.T) * rsig, ddelta * rsig, float(dsy.sum()))


def install_fake(monkeypatch):
    ctx = np_capi.install(monkeypatch)
    fake = FakeKprodGrad()
    ctx.kprod_grad = fake
    ctx.lib.sgp_kernelmatrix_diag = fake.sgp_kernelmatrix_diag
    real_ref = L.Spec.ref

    def ref(self, c=None):
        r = real_ref(self, c)
        fake.specs[C.addressof(self.c)] = self
        return r

    monkeypatch.setattr(L.Spec, "ref", ref)
    return ctx


TH0 = dict(v1=4.0, l=1.5, r=0.6, v2=0.7, alpha=1.3, l2=0.8, v3=0.1, c=0.25)


def hyper_model(bump=None):
    """sigma * stretch(GP(SE(l) * (Periodic(r) o ScaleTransform) + RQ + Polynomial(2, c)), 0.8); bump: {x: eps} added to
    sigma at single points (central differences with respect to sigma(x_i))"""
    th = TH0
    k = (th["v1"] * P.with_lengthscale(P.SEKernel(), th["l"]) * (P.PeriodicKernel(th["r"]) @ P.ScaleTransform(1.0 / 0.9)) +
         th["v2"] * P.with_lengthscale(P.RationalQuadraticKernel(th["alpha"]), th["l2"]) +
         th["v3"] * P.PolynomialKernel(2, th["c"]))
    # piecewise constant in x: g["x"] is the gradient through the kernel's points, with sigma(x) held (its own derivative is
    # the caller's business, through `scales`), and a central difference in x must hold it too
    sigma = lambda v: 1.0 + 0.5 * float(np.sin(np.floor(4.0 * np.sum(v)))) + (bump or {}).get(float(np.sum(v)), 0.0)      # noqa: E731
    return P.gppp(lambda GP: {"f": sigma * P.stretch(GP(k), 0.8)})


def _case():
    rng = np.random.default_rng(17)
    xs = [np.sort(rng.uniform(-3.0, 3.0, n)) for n in (9, 7)]
    zs = [np.sort(rng.uniform(-3.0, 3.0, n)) for n in (4, 3)]
    y = np.sin(2.0 * np.concatenate(xs)) + 0.3 * rng.standard_normal(16)
    data = lambda vs: P.BlockData([P.GPPPInput("f", v) for v in vs])      # noqa: E731
    return xs, zs, y, data


def np_lp(F, x, y, noise=0.1):
    return np_logpdf(kn.np_spec_matrix(P.build_spec(F, x)[0]) + noise * np.eye(len(y)), y)


def np_bound(F, x, z, y, noise=0.1, znoise=1e-3):
    Kzz = kn.np_spec_matrix(P.build_spec(F, z)[0]) + znoise * np.eye(P.build_spec(F, z)[0].N)
    return titsias(Kzz, kn.np_spec_matrix(P.build_spec(F, x, None, z)[0]), kg.np_diag(P.build_spec(F, x)[0]), y, noise)


def test_host_functions_match_central_differences_of_numpy(monkeypatch):
    """x / z / scales of logpdf_and_gradient_param and elbo_and_gradient_param against central differences (h = 1e-6) of the
    NumPy logpdf and Titsias bound built from np_spec_matrix.  The evaluator's need is printed; the GPU test's bounds for the
    same checks (1e-5 logpdf points, 5e-5 ELBO points) hold with room"""
    install_fake(monkeypatch)
    xs, zs, y, data = _case()
    F = hyper_model()
    g = P.logpdf_and_gradient_param(F(data(xs), 0.1), y, inputs=True, scales=True)
    assert g["_spec"].has_kprod and abs(g["logpdf"] - np_lp(F, data(xs), y)) <= 1e-12 * abs(g["logpdf"])
    assert len(g["terms"]) == 15 and all("d_param" in r and "chain" in r and "factor" in r for r in g["terms"])
    h, need = 1e-6, 0.0
    for I in range(2):
        for i in range(len(xs[I])):
            vp, vn = [v.copy() for v in xs], [v.copy() for v in xs]
            vp[I][i] += h
            vn[I][i] -= h
            fd = (np_lp(F, data(vp), y) - np_lp(F, data(vn), y)) / (2 * h)
            a = np.asarray(g["x"][I]).ravel()[i]
            need = max(need, abs(a - fd) / max(1.0, abs(fd)))
    print(f"logpdf points: the evaluator needs {need:.2e}")
    assert need <= 1e-5 / 2
    # scales: d logpdf / d sigma(x_i)
    recs = g["scales"]
    assert len(recs) == 2 and sorted(len(r["d_values"]) for r in recs) == [7, 9]
    need = 0.0
    for r in recs:
        pts = np.asarray(r["x"].x if hasattr(r["x"], "x") else r["x"], dtype=float).ravel()
        for i in (0, len(pts) - 1):
            fd = (np_lp(hyper_model({float(pts[i]): h}), data(xs), y) - np_lp(hyper_model({float(pts[i]): -h}), data(xs), y)) / (2 * h)
            need = max(need, abs(r["d_values"][i] - fd) / max(1.0, abs(fd)))
    print(f"logpdf scales: the evaluator needs {need:.2e}")
    assert need <= 1e-5 / 2
    # the ELBO
    ge = P.elbo_and_gradient_param(P.VFE(F(data(zs), 1e-3)), F(data(xs), 0.1), y, inputs=True)
    assert abs(ge["elbo"] - np_bound(F, data(xs), data(zs), y)) <= 1e-12 * abs(ge["elbo"])
    assert len(ge["zz_terms"]) == 15 and len(ge["xz_terms"]) == 20 and len(ge["xx_terms"]) == 10
    assert all("d_param" in r for key in ("zz_terms", "xz_terms", "xx_terms") for r in ge[key])
    need = 0.0
    for which, vals in (("x", xs), ("z", zs)):
        for I in range(2):
            for i in range(len(vals[I])):
                vp, vn = [v.copy() for v in vals], [v.copy() for v in vals]
                vp[I][i] += h
                vn[I][i] -= h
                args = (lambda v: (data(v), data(zs))) if which == "x" else (lambda v: (data(xs), data(v)))      # noqa: E731
                fd = (np_bound(F, *args(vp), y) - np_bound(F, *args(vn), y)) / (2 * h)
                a = np.asarray(ge[which][I]).ravel()[i]
                need = max(need, abs(a - fd) / max(1.0, abs(fd)))
    print(f"ELBO points: the evaluator needs {need:.2e}")
    assert need <= 5e-5 / 2


# ---- 4. / 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_old_host_functions_still_refuse_product_models(monkeypatch):
    install_fake(monkeypatch)
    f = _atom(golden_kernel())
    x, y = np.linspace(0.0, 1.0, 4), np.zeros(4)
    for kw in (dict(inputs=True), dict(scales=True)):
        with pytest.raises(NotImplementedError, match="product.*logpdf_and_gradient_param"):
            P.logpdf_and_gradient(f(x, 0.1), y, **kw)
    with pytest.raises(NotImplementedError, match="product.*elbo_and_gradient_param"):
        P.elbo_and_gradient(P.VFE(f(np.zeros(2))), f(x, 0.1), y)


def test_new_host_functions_refuse_patch_stencil_and_multi_gpu(monkeypatch):
    from test_conv_on_numpy import images
    ctx = install_fake(monkeypatch)
    Fs = P.gppp(lambda GP: (lambda f: {"f": f, "s": P.stencil(f, np.zeros((1, 2)), [1.0, -1.0])})(GP(P.SEKernel())))
    xs = P.GPPPInput("s", np.linspace(0, 1, 4))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.logpdf_and_gradient_param(Fs(xs, 0.1), np.zeros(4))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.elbo_and_gradient_param(P.VFE(Fs(P.GPPPInput("s", np.zeros(2)))), Fs(xs, 0.1), np.zeros(4))
    Fc = P.gppp(lambda GP: (lambda g: {"g": g, "f": P.patch_convolve(g, patch_shape=(3, 3))})(GP(P.SEKernel())))
    with pytest.raises(NotImplementedError, match="patch"):
        P.logpdf_and_gradient_param(Fc(P.GPPPInput("f", images(2)), 0.1), np.zeros(2))
    ctx.is_multi = True
    f = _atom(golden_kernel())
    x, y = np.linspace(0.0, 1.0, 4), np.zeros(4)
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        P.logpdf_and_gradient_param(f(x, 0.1), y)
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        P.elbo_and_gradient_param(P.VFE(f(np.zeros(2))), f(x, 0.1), y)
