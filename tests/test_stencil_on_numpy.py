"""Stencil GPs (stencil, quadrature_convolve) without a GPU: a NumPy evaluator of specs with stencil terms, checked against
the explicit double sum over shifted points; the flattener's one term per pair of paths, with the offsets mapped through
Shift / Stretch / Select / with_lengthscale and nested stencils folded; the stencil mean; the refusals; the extension
header include/sthenomi_stencil.h (plain C, exactly what libsthenomi_stencil.so exports)."""
import os
import subprocess

import numpy as np
import pytest

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_conv_on_numpy import images, np_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the NumPy evaluator (also used by test_gpu_stencil.py) ---------------------------------------------------------
def _shifted(X, st):
    """(Q, n, D) the points of X (D x n) minus every offset of the stencil; a plain side is the one-point stencil 0"""
    X = np.asarray(X)
    if st is None:
        return X.T[None], np.ones(1)
    A, w = st
    return np.stack([(X - A[:, q:q + 1]).T for q in range(A.shape[1])]), np.asarray(w)


def np_spec_matrix(spec):
    """K of a lib.Spec, stencil terms included: sum_p w_p sum_q v_q k(x_i - a_p, y_j - b_q) per term"""
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
                rst, cst = spec.term_stencils[t]
                R, wr = _shifted(spec.inputs[T.row_input], rst)
                Cc, wc = _shifted(spec.inputs[T.col_input], cst)
                d2 = ((R[:, :, None, None, :] - Cc[None, None, :, :, :]) ** 2).sum(-1)   # (Qr, nr, Qc, nc)
                k = np.einsum("p,piqj,q->ij", wr, np_kernel(T.kind, d2, T.param), wc)
                k = T.coef * k
                rs, cs = spec.term_row_scale[t], spec.term_col_scale[t]
                if rs is not None:
                    k = np.asarray(rs)[:, None] * k
                if cs is not None:
                    k = k * np.asarray(cs)[None, :]
                K[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += k
    return K


def se(x, y, ell=1.0):
    """exp(-|x - y|^2 / (2 ell^2)) of the columns of x (D x n) and y (D x m)"""
    return np.exp(-0.5 * ((x[:, :, None] - y[:, None, :]) ** 2).sum(0) / ell ** 2)


def stencil_model(A, w, kernel=None, warp=None, B=None, v=None):
    """f = GP(kernel); g = stencil(warp(f), A, w); h = stencil(f, B, v) (or g); plus sums and scales of g"""
    kernel = kernel if kernel is not None else 1.3 * P.SEKernel()

    def build(GP):
        f = GP(kernel)
        u = GP(0.4 * P.Matern32Kernel())
        inner = f if warp is None else warp(f)
        g = P.stencil(inner, A, w)
        h = P.stencil(f, B, v) if B is not None else g
        return {"f": f, "u": u, "g": g, "h": h, "gu": g + u, "g2": 2.0 * g - 0.5 + g}
    return P.gppp(build)


# ---- tests ----------------------------------------------------------------------------------------------------------
def test_evaluator_matches_the_explicit_double_sum():
    rng = np.random.default_rng(0)
    A, w = rng.standard_normal((2, 4)), rng.standard_normal(4)
    B, v = rng.standard_normal((2, 3)), rng.standard_normal(3)
    F = stencil_model(A, w, B=B, v=v)
    x, y = P.ColVecs(rng.standard_normal((2, 7))), P.ColVecs(rng.standard_normal((2, 5)))
    # cov(g, h): both sides carry (different) stencils
    spec, _, _ = P.build_spec(F, P.GPPPInput("g", x), None, P.GPPPInput("h", y))
    ref = sum(w[p] * v[q] * 1.3 * se(x.X - A[:, p:p + 1], y.X - B[:, q:q + 1]) for p in range(4) for q in range(3))
    assert np.max(np.abs(np_spec_matrix(spec) - ref)) <= 1e-13 * np.max(np.abs(ref))
    # cov(g, f): one-sided
    spec, _, _ = P.build_spec(F, P.GPPPInput("g", x), None, P.GPPPInput("f", y))
    ref = sum(w[p] * 1.3 * se(x.X - A[:, p:p + 1], y.X) for p in range(4))
    assert np.max(np.abs(np_spec_matrix(spec) - ref)) <= 1e-13 * np.max(np.abs(ref))
    spec, _, _ = P.build_spec(F, P.GPPPInput("f", y), None, P.GPPPInput("g", x))
    assert np.max(np.abs(np_spec_matrix(spec) - ref.T)) <= 1e-13 * np.max(np.abs(ref))


def test_one_term_per_pair_of_paths():
    t, wq = np.polynomial.hermite.hermgauss(15)

    def build(GP):
        f = GP(P.with_lengthscale(P.Matern52Kernel(), 0.5))
        return {"f": f, "g": P.quadrature_convolve(f)}
    F = P.gppp(build)
    x = np.linspace(-2.0, 2.0, 6)
    xb = P.BlockData([P.GPPPInput("f", x), P.GPPPInput("g", x)])
    spec, _, _ = P.build_spec(F, xb)
    assert spec.n_terms == 4 and spec.has_stencil and not spec.has_patch
    assert spec.term_geoms == [(None, None)] * 4
    # the offsets scaled by the kernel's 1 / lengthscale, like the points
    st = (2.0 * t.reshape(1, -1), wq)
    got = spec.term_stencils
    assert got[0] == (None, None)
    assert got[1][0] is None and np.array_equal(got[1][1][0], st[0]) and np.array_equal(got[1][1][1], wq)
    assert got[2][1] is None and np.array_equal(got[2][0][0], st[0])
    assert all(np.array_equal(a[0], st[0]) and np.array_equal(a[1], wq) for a in got[3])
    assert np.array_equal(spec.inputs[0], 2.0 * x.reshape(1, -1))
    assert not spec.f32_supported()
    # sums, scalar scales and + known: g + u keeps its stencil term next to u's plain term; 2 g - 0.5 + g has coef 9
    F = stencil_model(np.array([0.0, -3.0]), np.array([1.0, 1.0]))
    spec, _, _ = P.build_spec(F, P.GPPPInput("gu", x))
    assert spec.n_terms == 2 and sorted(str(s[0] is None) for s in spec.term_stencils) == ["False", "True"]
    spec, _, _ = P.build_spec(F, P.GPPPInput("g2", x))
    assert spec.n_terms == 1 and spec._terms[0].coef == pytest.approx(9.0 * 1.3)
    # a plain spec is unchanged
    spec, _, _ = P.build_spec(F, P.GPPPInput("f", x))
    assert not spec.has_stencil and spec.term_stencils == [(None, None)]


def test_offsets_map_through_shift_stretch_select_and_lengthscale():
    rng = np.random.default_rng(1)
    x = P.ColVecs(rng.standard_normal((3, 5)))
    w = rng.standard_normal(3)
    A3 = rng.standard_normal((3, 3))
    L = rng.standard_normal((2, 2))
    sh = np.array([0.5, -1.0])
    cases = [
        # (g, expected points, expected offsets): the stencil's offsets live in the coordinates of g's inputs
        # Select picks rows of the points and the offsets, then Shift moves the points, not the offsets
        (lambda f: P.stencil(P.select(P.shift(f, sh), [2, 0]), A3, w), x.X[[2, 0]] - sh[:, None], A3[[2, 0]]),
        # Select then a matrix Stretch: both map the points and the offsets alike
        (lambda f: P.stencil(P.select(P.stretch(f, L), [2, 0]), A3, w), L @ x.X[[2, 0]], L @ A3[[2, 0]]),
        # a stencil of 2-D points directly below a Shift of them
    ]
    for make, X_exp, A_exp in cases:
        def build(GP, make=make):
            f = GP(P.with_lengthscale(P.SEKernel(), 4.0))     # the kernel's ScaleTransform scales points and offsets
            return {"f": f, "g": make(f)}
        spec, _, _ = P.build_spec(P.gppp(build), P.GPPPInput("g", x))
        assert spec.n_terms == 1
        rst, cst = spec.term_stencils[0]
        assert np.allclose(spec.inputs[0], X_exp / 4.0, rtol=1e-14, atol=1e-15)
        assert np.allclose(rst[0], A_exp / 4.0, rtol=1e-14, atol=1e-15) and np.array_equal(rst[1], w)
        assert np.array_equal(cst[0], rst[0]) and np.array_equal(cst[1], w)
    # a scalar Stretch of 1-D points; an integer Select of 2-D points
    xs = rng.standard_normal(4)

    def build(GP):
        f = GP(P.SEKernel())
        return {"f": f, "g": P.stencil(P.stretch(f, 3.0), [1.0, -2.0], [0.5, 0.25]),
                "s": P.stencil(P.select(f, 1), np.array([[1.0, 5.0], [2.0, 6.0]]), [1.0, 1.0])}
    F = P.gppp(build)
    spec, _, _ = P.build_spec(F, P.GPPPInput("g", xs))
    assert np.array_equal(spec.term_stencils[0][0][0], np.array([[3.0, -6.0]]))
    assert np.array_equal(spec.inputs[0], 3.0 * xs.reshape(1, -1))
    spec, _, _ = P.build_spec(F, P.GPPPInput("s", P.ColVecs(rng.standard_normal((2, 4)))))
    assert np.array_equal(spec.term_stencils[0][0][0], np.array([[2.0, 6.0]]))
    assert spec.inputs[0].shape == (1, 4)


def test_nested_stencils_fold_into_one():
    rng = np.random.default_rng(2)
    a, w = np.array([0.5, -1.0]), np.array([2.0, 3.0])
    b, v = np.array([0.25, 0.0, -0.75]), np.array([1.0, -1.0, 0.5])

    def build(GP):
        f = GP(P.Matern12Kernel())
        return {"f": f, "g": P.stencil(P.stencil(f, b, v), a, w)}
    F = P.gppp(build)
    x = rng.standard_normal(6)
    spec, _, _ = P.build_spec(F, P.GPPPInput("g", x))
    assert spec.n_terms == 1
    A, W = spec.term_stencils[0][0]
    assert A.shape == (1, 6)
    assert np.array_equal(A[0], np.array([a[p] + b[q] for p in range(2) for q in range(3)]))
    assert np.array_equal(W, np.array([w[p] * v[q] for p in range(2) for q in range(3)]))
    # the same matrix as the explicit quadruple sum
    ref = sum(w[p] * v[q] * w[r] * v[s] * np.exp(-np.abs((x[:, None] - a[p] - b[q]) - (x[None, :] - a[r] - b[s])))
              for p in range(2) for q in range(3) for r in range(2) for s in range(3))
    assert np.max(np.abs(np_spec_matrix(spec) - ref)) <= 1e-13 * np.max(np.abs(ref))
    # beyond 64 folded points
    big = np.linspace(-1, 1, 9)

    def build2(GP):
        f = GP(P.SEKernel())
        return {"g": P.stencil(P.stencil(f, big, np.ones(9)), big, np.ones(9))}
    with pytest.raises(NotImplementedError, match="stencil"):
        P.build_spec(P.gppp(build2), P.GPPPInput("g", x))


def test_stencil_matches_the_composed_sum_of_shifts_on_the_evaluator():
    """the stencil spec and the composed sum of shift views are the same matrix (on the evaluators)"""
    import test_conv_on_numpy as conv_np
    a, w = np.array([-0.3, 0.0, 0.7]), np.array([0.5, 1.5, -2.0])

    def build(GP):
        f = GP(P.with_lengthscale(P.Matern32Kernel(), 0.8))
        fs = w[0] * P.shift(f, a[0])
        for k in range(1, 3):
            fs = fs + w[k] * P.shift(f, a[k])
        return {"f": f, "g": P.stencil(f, a, w), "fs": fs}
    F = P.gppp(build)
    x = np.linspace(-1.0, 1.0, 7)
    Kg = np_spec_matrix(P.build_spec(F, P.GPPPInput("g", x))[0])
    spec_s = P.build_spec(F, P.GPPPInput("fs", x))[0]
    assert spec_s.n_terms == 9
    Ks = conv_np.np_spec_matrix(spec_s)
    assert np.max(np.abs(Kg - Ks)) <= 1e-13 * np.max(np.abs(Ks))


def test_stencil_mean():
    def build(GP):
        f = GP(lambda v: float(v) ** 2, P.SEKernel())
        return {"f": f, "g": P.stencil(f, [1.0, -2.0], [0.5, 3.0]) + 1.0}
    F = P.gppp(build)
    x = np.array([0.0, 1.5, -2.0])
    m = P.mean_vector(F, P.GPPPInput("g", x))
    assert np.allclose(m, 1.0 + 0.5 * (x - 1.0) ** 2 + 3.0 * (x + 2.0) ** 2, rtol=1e-15, atol=0)

    def build2(GP):
        f = GP(lambda v: float(v[0] - 2.0 * v[1]), P.SEKernel())
        return {"g": P.stencil(f, np.array([[1.0, 0.0], [0.0, 1.0]]), [2.0, -1.0])}
    X = np.random.default_rng(3).standard_normal((2, 4))
    m = P.mean_vector(P.gppp(build2), P.GPPPInput("g", P.ColVecs(X)))
    ref = 2.0 * ((X[0] - 1.0) - 2.0 * X[1]) - (X[0] - 2.0 * (X[1] - 1.0))
    assert np.allclose(m, ref, rtol=1e-14, atol=1e-15)
    # quadrature_convolve's mean: the hermgauss sum of the mean
    t, wq = np.polynomial.hermite.hermgauss(15)

    def build3(GP):
        f = GP(lambda v: np.sin(v), P.SEKernel())
        return {"g": P.quadrature_convolve(f)}
    m = P.mean_vector(P.gppp(build3), P.GPPPInput("g", x))
    assert np.allclose(m, [np.sum(wq * np.sin(xi - t)) for xi in x], rtol=1e-13, atol=1e-15)


def test_constructor_checks():
    f = P.atomic(P.GP(P.SEKernel()), P.GPC())
    with pytest.raises(ValueError, match="stencil"):
        P.stencil(f, [0.0, 1.0], [1.0])
    with pytest.raises(ValueError, match="stencil"):
        P.stencil(f, [], [])
    with pytest.raises(ValueError, match="finite"):
        P.stencil(f, [0.0], [np.inf])
    g = P.stencil(f, np.zeros((2, 3)), np.ones(3))
    assert g.args[0] == "stencil" and g.args[2].shape == (2, 3)
    with pytest.raises(ValueError, match="dimension"):
        P.build_spec(g, np.zeros(4))


def test_refusals_name_the_construct():
    x = np.linspace(0.0, 1.0, 4)
    A, w = [0.0, 0.5], [1.0, 1.0]
    for warp, name in [(lambda f: (lambda v: 1.0) * f, "function scale"), (lambda f: P.periodic(f, 1.0), "Periodic"),
                       (lambda f: P.compose(f, np.tanh), "tanh")]:
        with pytest.raises(NotImplementedError, match=name):
            P.build_spec(stencil_model(A, w, warp=warp), P.GPPPInput("g", x))
    with pytest.raises(NotImplementedError, match="PeriodicTransform"):
        P.build_spec(stencil_model(A, w, kernel=P.TransformedKernel(P.SEKernel(), P.PeriodicTransform(1.0))),
                     P.GPPPInput("g", x))
    # a nested GPPP below a stencil
    nested = P.atomic(P.gppp(lambda GP: {"a": GP(P.SEKernel())}), P.GPC())
    with pytest.raises(NotImplementedError, match="stencil of a nested GPPP"):
        P.build_spec(P.stencil(nested, A, w), P.GPPPInput("a", x))
    # any mix with patch_convolve: by nesting, either way, and through a term with a patch side and a stencil side
    im = images(3)

    def mixed(GP):
        f = GP(P.SEKernel())
        return {"f": f, "pc": P.patch_convolve(P.stencil(f, np.zeros((9, 1)), [1.0])),
                "sp": P.stencil(P.patch_convolve(f), np.zeros((64, 1)), [1.0]),
                "c": P.patch_convolve(f), "s": P.stencil(f, np.zeros((9, 2)), [1.0, 2.0])}
    F = P.gppp(mixed)
    with pytest.raises(NotImplementedError, match="stencil"):
        P.build_spec(F, P.GPPPInput("pc", im))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.build_spec(F, P.GPPPInput("sp", im))
    with pytest.raises(NotImplementedError, match="patch_convolve.*stencil"):
        P.build_spec(F, P.GPPPInput("c", im), None, P.GPPPInput("s", P.ColVecs(np.zeros((9, 2)))))


def test_host_refuses_gradients_and_fp32():
    F = stencil_model([0.0, 0.5], [1.0, -1.0])
    x = P.GPPPInput("g", np.linspace(0.0, 1.0, 4))
    fx = F(x, 0.1)
    with pytest.raises(NotImplementedError, match="stencil"):
        P.logpdf_and_gradient(fx, np.zeros(4))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.logpdf_and_gradient_batch([fx], [np.zeros(4)])
    z = P.GPPPInput("f", np.zeros(2))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.elbo_and_gradient(P.VFE(F(z)), fx, np.zeros(4))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.logpdf_f32(F(P.GPPPInput("g", np.linspace(0.0, 1.0, 4).astype(np.float32)), 0.1), np.zeros(4, np.float32))


def test_stencil_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "stencil_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_stencil.h"
int main(int argc, char** argv) {
  typedef int (*fn_t)(sgp_ctx*, const sgp_stencil*, int32_t*);
  fn_t probe = 0;
  double a[2] = {-1.0, 1.0}, w[2] = {0.5, -0.5};
  sgp_stencil st = {1, 2, a, w};
  void* h;
  printf("fnptr %d stencil %d\n", (int)sizeof(probe = &sgp_stencil_register), (int)sizeof(st));
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  printf("%s\n", dlsym(h, "sgp_stencil_register") ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "stencil_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, P.lib.STENCIL_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "8", "stencil", "24", "resolved"], (out.stdout,
                                                                                                        out.stderr)


def test_stencil_library_exports_exactly_its_header():
    syms = _symbols_of("sthenomi_stencil.h")
    assert syms == ["sgp_stencil_register"] == P.lib.stencil_symbols()
    assert _c_exports(P.lib.STENCIL_LIB_PATH) == syms
    assert not set(syms) & set(_c_exports(P.lib.LIB_PATH))
    assert not set(syms) & set(_c_exports(P.lib.CONV_LIB_PATH))
    assert not set(syms) & set(_symbols_of("sthenomi.h"))
    assert hasattr(P.lib.stencil_lib(), "sgp_stencil_register")
