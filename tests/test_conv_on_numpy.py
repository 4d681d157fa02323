"""Convolutional GPs (patch_convolve) without a GPU: a NumPy evaluator of specs with patch terms, checked against the explicit
sum over extract_patches; the flattener's term selectors and geometries; the warp refusals; the extension header
include/sthenomi_conv.h (plain C, exactly what libsthenomi_conv.so exports)."""
import os
import subprocess

import numpy as np
import pytest

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the NumPy evaluator (also used by test_gpu_conv.py) ------------------------------------------------------------
def np_kernel(kind, d2, param):
    d = np.sqrt(d2)
    if kind == P.lib.SE:
        return np.exp(-0.5 * d2)
    if kind == P.lib.MATERN12:
        return np.exp(-d)
    if kind == P.lib.MATERN32:
        return (1.0 + np.sqrt(3.0) * d) * np.exp(-np.sqrt(3.0) * d)
    if kind == P.lib.MATERN52:
        return (1.0 + np.sqrt(5.0) * d + 5.0 * d2 / 3.0) * np.exp(-np.sqrt(5.0) * d)
    if kind == P.lib.WHITE:
        return (d2 == 0.0).astype(np.float64)
    return np.full(d2.shape, float(param))


def np_patches(X, geom):
    """(P, n, ph * pw): every patch of every image, column-major flattened"""
    H, W, ph, pw = geom
    imgs = np.asarray(X).reshape(H, W, -1, order="F")
    n = imgs.shape[2]
    return np.stack([imgs[pr:pr + ph, pc:pc + pw, :].reshape(ph * pw, n, order="F").T
                     for pc in range(W - pw + 1) for pr in range(H - ph + 1)])


def np_spec_matrix(spec):
    """K of a lib.Spec, patch terms included: sum over the patches of both sides of the kernel of every pair of points"""
    K = np.zeros((spec.N, spec.M))
    roff = np.concatenate([[0], np.cumsum(spec.row_len)])
    coff = np.concatenate([[0], np.cumsum(spec.col_len)])
    tp = spec._term_ptr
    nb = len(spec.col_len)
    for I in range(len(spec.row_len)):
        for J in range(nb):
            p = I * nb + J
            for t in range(int(tp[p]), int(tp[p + 1])):
                T = spec._terms[t]
                rg, cg = spec.term_geoms[t]
                Xr, Xc = spec.inputs[T.row_input], spec.inputs[T.col_input]
                R = np_patches(Xr, rg) if rg else Xr.T[None]
                Cc = np_patches(Xc, cg) if cg else Xc.T[None]
                d2 = ((R[:, :, None, None, :] - Cc[None, None, :, :, :]) ** 2).sum(-1)   # (Pr, nr, Pc, nc)
                k = np_kernel(T.kind, d2, T.param).sum(axis=(0, 2))
                rs = spec.term_row_scale[t]
                cs = spec.term_col_scale[t]
                k = T.coef * k
                if rs is not None:
                    k = np.asarray(rs)[:, None] * k
                if cs is not None:
                    k = k * np.asarray(cs)[None, :]
                K[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += k
    return K


def conv_model(kernel=None, warp=None):
    """@gppp let g = GP(kernel); f = patch_convolve(g) end (the reference example), optionally f = patch_convolve(warp(g))"""
    kernel = kernel if kernel is not None else 1.7 * P.with_lengthscale(P.SEKernel(), 1.3)

    def build(GP):
        g = GP(kernel)
        h = GP(0.5 * P.Matern32Kernel())
        inner = g if warp is None else warp(g)
        f = P.patch_convolve(inner)
        return {"g": g, "h": h, "f": f, "fh": f + h, "f2": 2.0 * f - 0.5 + f}
    return P.gppp(build)


def images(n, H=8, W=8, seed=0):
    return P.ImageVector(np.random.default_rng(seed).standard_normal((H, W, n)))


def explicit_cov(x, x2, var, ell, H=8, W=8):
    """sum_p sum_q var exp(-|x_p - x'_q|^2 / (2 ell^2)) over extract_patches (the reference example's cov)"""
    xs = P.extract_patches(x, (3, 3), (H, W))
    x2s = P.extract_patches(x2, (3, 3), (H, W)) if x2 is not None else None
    n = len(x)
    K = np.zeros((n, len(x2) if x2 is not None else n))
    for a in xs:
        for b in (x2s if x2s is not None else xs):
            d2 = ((a.X[:, :, None] - b.X[:, None, :]) ** 2).sum(0)
            K += var * np.exp(-0.5 * d2 / ell ** 2)
    return K


# ---- tests ----------------------------------------------------------------------------------------------------------
def test_evaluator_matches_the_explicit_patch_sum():
    f = conv_model()
    x = images(6)
    spec, _, _ = P.build_spec(f, P.GPPPInput("f", x))
    K = np_spec_matrix(spec)
    Ke = explicit_cov(x, None, 1.7, 1.3)
    assert np.max(np.abs(K - Ke)) <= 1e-12 * np.max(np.abs(Ke))
    # cross-covariance with pseudo-points placed in g: sum_p k(patch_p x_i, z_j)
    z = P.ColVecs(np.random.default_rng(3).standard_normal((9, 5)))
    spec, _, _ = P.build_spec(f, P.GPPPInput("f", x), None, P.GPPPInput("g", z))
    Kxz = np_spec_matrix(spec)
    ref = sum(1.7 * np.exp(-0.5 * ((a.X[:, :, None] - z.X[:, None, :]) ** 2).sum(0) / 1.3 ** 2)
              for a in P.extract_patches(x))
    assert np.max(np.abs(Kxz - ref)) <= 1e-12 * np.max(np.abs(ref))


def test_extract_patches_layout():
    X = np.arange(4 * 5 * 2, dtype=np.float64).reshape(4, 5, 2, order="F")
    ps = P.extract_patches(P.ImageVector(X), (2, 3))
    assert len(ps) == 3 * 3
    # p-major listing, each patch X[p:p+2, q:q+3, n] column-major
    assert np.array_equal(ps[1].X[:, 1], X[0:2, 1:4, 1].reshape(-1, order="F"))
    assert np.array_equal(ps[3].X[:, 0], X[1:3, 0:3, 0].reshape(-1, order="F"))
    # a ColVecs of flattened images reads the same
    cv = P.ColVecs(X.reshape(20, 2, order="F"))
    assert all(np.array_equal(a.X, b.X) for a, b in zip(ps, P.extract_patches(cv, (2, 3), (4, 5))))


def test_mean_is_the_sum_over_patches():
    def build(GP):
        g = GP(lambda v: float(np.sum(v) ** 2), P.SEKernel())
        return {"g": g, "f": P.patch_convolve(g) + 3.0}
    f = P.gppp(build)
    x = images(4)
    m = P.mean_vector(f, P.GPPPInput("f", x))
    ref = 3.0 + sum(np.sum(a.X, axis=0) ** 2 for a in P.extract_patches(x))
    assert np.allclose(m, ref, rtol=1e-14, atol=0)


def test_flattener_selectors_and_geometries():
    f = conv_model()
    x = images(5)
    z = P.ColVecs(np.random.default_rng(1).standard_normal((9, 3)))
    geo = (8, 8, 3, 3)
    # f alone: one term, both sides patched, the images (scaled by 1 / lengthscale) as the inputs
    spec, _, _ = P.build_spec(f, P.GPPPInput("f", x))
    assert spec.n_terms == 1 and spec.term_geoms == [(geo, geo)] and spec.has_patch
    assert spec.inputs[0].shape == (64, 5) and np.allclose(spec.inputs[0], x.X / 1.3)
    assert not spec.f32_supported()
    # f with g: the (f, g) pair patched on the rows only, (g, f) on the columns only, (g, g) plain
    spec, _, _ = P.build_spec(f, P.BlockData([P.GPPPInput("f", x), P.GPPPInput("g", z)]))
    assert list(spec._term_ptr) == [0, 1, 2, 3, 4]
    assert spec.term_geoms == [(geo, geo), (geo, None), (None, geo), (None, None)]
    # f + h: the conv term and h's plain term share the diagonal pair
    spec, _, _ = P.build_spec(f, P.GPPPInput("fh", x))
    assert sorted(spec.term_geoms, key=str) == sorted([(geo, geo), (None, None)], key=str)
    assert {spec.inputs[spec._terms[t].row_input].shape[0] for t in range(spec.n_terms)} == {64}
    # scalar scales and + known compose: 2 f - 0.5 + f has coefficient 3 on each side
    spec, _, _ = P.build_spec(f, P.GPPPInput("f2", x))
    assert spec.n_terms == 1 and spec._terms[0].coef == pytest.approx(9.0 * 1.7)
    # a plain spec is unchanged
    spec, _, _ = P.build_spec(f, P.GPPPInput("g", z))
    assert not spec.has_patch and spec.term_geoms == [(None, None)]


def test_scalar_stretch_commutes_and_other_warps_are_refused():
    x = images(3)
    f = conv_model(warp=lambda g: P.stretch(g, 0.5))
    spec, _, _ = P.build_spec(f, P.GPPPInput("f", x))
    assert np.allclose(spec.inputs[0], 0.5 * x.X / 1.3)
    for warp, name in [(lambda g: P.select(g, [0, 1, 2]), "Select"), (lambda g: P.shift(g, 1.0), "Shift"),
                       (lambda g: P.periodic(g, 1.0), "Periodic"), (lambda g: P.stretch(g, [1.0, 2.0]), "Stretch"),
                       (lambda g: P.compose(g, np.tanh), "tanh")]:
        with pytest.raises(NotImplementedError, match=name):
            P.build_spec(conv_model(warp=warp), P.GPPPInput("f", x))
    with pytest.raises(NotImplementedError, match="function scale"):
        P.build_spec(conv_model(warp=lambda g: (lambda v: 1.0) * g), P.GPPPInput("f", x))
    with pytest.raises(NotImplementedError, match="input transform"):
        P.build_spec(conv_model(kernel=P.TransformedKernel(P.SEKernel(), P.PeriodicTransform(1.0))), P.GPPPInput("f", x))


def test_conv_gradients_are_refused_on_the_host():
    f = conv_model()
    x = images(4)
    fx = f(P.GPPPInput("f", x), 0.1)
    with pytest.raises(NotImplementedError, match="patch_convolve"):
        P.logpdf_and_gradient(fx, np.zeros(4))
    with pytest.raises(NotImplementedError, match="patch_convolve"):
        P.logpdf_and_gradient_batch([fx], [np.zeros(4)])
    z = P.GPPPInput("g", P.ColVecs(np.zeros((9, 2))))
    with pytest.raises(NotImplementedError, match="patch_convolve"):
        P.elbo_and_gradient(P.VFE(f(z)), fx, np.zeros(4))


def test_conv_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "conv_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_conv.h"
int main(int argc, char** argv) {
  typedef int (*fn_t)(sgp_ctx*, const sgp_patch_geom*, int32_t*);
  fn_t probe = 0;
  sgp_patch_geom g = {28, 28, 3, 3};
  void* h;
  printf("fnptr %d geom %d\n", (int)sizeof(probe = &sgp_conv_geom), (int)sizeof(g));
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  printf("%s\n", dlsym(h, "sgp_conv_geom") ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "conv_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, P.lib.CONV_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "8", "geom", "16", "resolved"], (out.stdout, out.stderr)


def test_conv_library_exports_exactly_its_header():
    syms = _symbols_of("sthenomi_conv.h")
    assert syms == ["sgp_conv_geom"] == P.lib.conv_symbols()
    assert _c_exports(P.lib.CONV_LIB_PATH) == syms
    assert not set(syms) & set(_c_exports(P.lib.LIB_PATH))
    assert not set(syms) & set(_symbols_of("sthenomi.h"))
    assert hasattr(P.lib.conv_lib(), "sgp_conv_geom")
