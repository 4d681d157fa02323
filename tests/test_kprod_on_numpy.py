"""Kernel products, RationalQuadratic, Linear, Polynomial and Periodic kernels without a GPU: the 60-digit table of the RQ
formula and its error model (tests/kprod_truth.py), the NumPy evaluator of specs with product chains (tests/kprod_np.py)
against explicit products of closed-form matrices, a scikit-learn golden with a locally periodic, a rational-quadratic and a
polynomial term, the flattener's chains, the refusals, and the extension header include/sthenomi_kprod.h (plain C, exactly
what libsthenomi_kprod.so exports)."""
import base64
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

import kprod_np as kn
import kprod_truth as kt
import oracle.kernelfunctions as okf
import oracle.stheno as ost
import stheno_jl_amd as P
from stheno_jl_amd import lib as L
from test_capi_symbols import _c_exports, _symbols_of
from test_conv_on_numpy import images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.filterwarnings("error::DeprecationWarning")


# ---- closed forms, written independently of the evaluator ------------------------------------------------------------
def _d2(X, Y):
    return ((X[:, :, None] - Y[:, None, :]) ** 2).sum(0)


def c_se(X, Y, ell=1.0):
    return np.exp(-0.5 * _d2(X, Y) / ell ** 2)


def c_m32(X, Y, ell=1.0):
    d = np.sqrt(3.0 * _d2(X, Y)) / ell
    return (1.0 + d) * np.exp(-d)


def c_rq(X, Y, alpha, ell=1.0):
    return (1.0 + _d2(X, Y) / (2.0 * alpha * ell ** 2)) ** -alpha


def c_lin(X, Y, c=0.0):
    return X.T @ Y + c


def c_per(X, Y, r, period=1.0):
    """KernelFunctions PeriodicKernel(r) o ScaleTransform(1 / period): exp(-sum_d sin^2(pi (x_d - y_d) / period) / r_d^2 / 2)"""
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (X.shape[0],))
    s = np.sin(np.pi * (X[:, :, None] - Y[:, None, :]) / period) / r[:, None, None]
    return np.exp(-0.5 * (s ** 2).sum(0))


def golden_kernel():
    """the scikit-learn golden's signal kernel in this package's terms"""
    return (4.0 * P.with_lengthscale(P.SEKernel(), 1.5) * (P.PeriodicKernel(0.6) @ P.ScaleTransform(1.0 / 0.9)) +
            0.7 * P.with_lengthscale(P.RationalQuadraticKernel(1.3), 0.8) + 0.1 * P.PolynomialKernel(2, 0.25))


def load_golden():
    """(x, y, the rows g["K_rows"] of scikit-learn's kernel matrix, the file)"""
    with open(os.path.join(ROOT, "tests", "golden", "sklearn_kprod.json")) as fh:
        g = json.load(fh)
    arr = lambda k: np.frombuffer(base64.b64decode(g[k]), dtype="<f8")      # noqa: E731
    return arr("x"), arr("y"), arr("K").reshape(len(g["K_rows"]), g["n"]), g


def np_logpdf(C, y):
    c = scipy.linalg.cholesky(C, lower=True)
    a = scipy.linalg.solve_triangular(c, y, lower=True)
    return -0.5 * float(a @ a) - float(np.sum(np.log(np.diag(c)))) - 0.5 * len(y) * np.log(2.0 * np.pi)


def _atom(kernel):
    return P.atomic(P.GP(kernel), P.GPC())


# ---- 1. the truth table and the error model ----------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", kt.ALPHAS)
def test_numpy_rq_formula_stays_within_half_the_models_bound(alpha):
    """the condition on the error model: the float64 NumPy evaluation of the formula the device uses stays within HALF of
    the bound on every grid point (otherwise the model is wrong), is exactly 1 at d2 = 0, exactly 0 where it must be"""
    g = kt.load()[alpha]
    assert len(g) >= 50 and g.d2[0] == 0.0 and np.isinf(g.d2).sum() == 1
    assert ((g.d2 > 0.99e300) & (g.d2 < 1.01e300)).sum() == 1 and ((g.d2 > 0.99e-300) & (g.d2 < 1.01e-300)).sum() >= 1
    assert ((g.d2 > 0) & (g.d2 < np.finfo(np.float64).tiny)).sum() >= 2         # subnormal squared distances
    got = kn.rq(g.d2, alpha)
    print(f"\nRQ alpha={alpha}: NumPy, largest error in ulps of the truth per band: {kt.band_maxima(g, got)}")
    bad = kt.violations(g, got, fraction=0.5)
    assert bad.size == 0, kt.describe(g, got, bad)
    assert got[0] == 1.0 and not np.any(np.isnan(got)) and got[np.isinf(g.d2)][0] == 0.0
    if alpha >= 1.0:
        assert g.must_zero.sum() >= 10 and (g.band == 2).sum() >= 5             # the underflow region is visited


@pytest.mark.parametrize("alpha", kt.ALPHAS)
def test_numpy_rq_derivatives_against_the_table(alpha):
    """the two derivatives the gradient contraction uses, as the evaluator (and the device) forms them"""
    g = kt.load()[alpha]
    dk, dp = kn.rq_dscale(g.d2, alpha), kn.rq_dparam(g.d2, alpha)
    assert not np.any(np.isnan(dk)) and not np.any(np.isnan(dp))
    assert np.all(np.abs(dk - g.dk) <= kt.dscale_tolerance(g)), np.flatnonzero(np.abs(dk - g.dk) > kt.dscale_tolerance(g))
    assert np.all(np.abs(dp - g.dp) <= kt.dparam_tolerance(g)), np.flatnonzero(np.abs(dp - g.dp) > kt.dparam_tolerance(g))
    assert dk[np.isinf(g.d2)][0] == 0.0 and dp[np.isinf(g.d2)][0] == 0.0 and dk[0] == 0.0 and dp[0] == 0.0


# ---- 2. the evaluator against explicit products ------------------------------------------------------------------------
def test_evaluator_matches_explicit_products_of_closed_forms():
    rng = np.random.default_rng(1)
    X, Y = rng.standard_normal((3, 7)), rng.standard_normal((3, 5))
    k = (1.7 * P.SEKernel() * P.with_lengthscale(P.Matern32Kernel(), 0.7) * P.RationalQuadraticKernel(0.9) +
         0.3 * P.PolynomialKernel(3, 0.5) + P.LinearKernel(0.2) * P.with_lengthscale(P.SEKernel(), 2.0))
    spec, _, _ = P.build_spec(_atom(k), P.ColVecs(X), None, P.ColVecs(Y))
    want = (1.7 * c_se(X, Y) * c_m32(X, Y, 0.7) * c_rq(X, Y, 0.9) + 0.3 * c_lin(X, Y, 0.5) ** 3 +
            c_lin(X, Y, 0.2) * c_se(X, Y, 2.0))
    got = kn.np_spec_matrix(spec)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert [len(ts) for _, _, ts in kn.chains(spec)] == [3, 3, 2] and spec.has_kprod and not spec.f32_supported()


def test_periodic_kernel_is_se_over_the_sincos_embedding():
    rng = np.random.default_rng(2)
    X, Y = rng.uniform(-2, 2, (2, 9)), rng.uniform(-2, 2, (2, 6))
    for r, k in (((0.6, 1.4), P.PeriodicKernel((0.6, 1.4))), (0.8, P.PeriodicKernel(0.8))):
        spec, _, _ = P.build_spec(_atom(k), P.ColVecs(X), None, P.ColVecs(Y))
        assert spec.n_terms == 1 and spec.inputs[0].shape == (4, 9) and not spec.has_kprod       # a plain SE term
        assert np.abs(kn.np_spec_matrix(spec) - c_per(X, Y, r)).max() <= 3e-15
    # the vjp of the embedding, by central differences of a linear functional
    chain = (("scale", 1.3), ("sincos", (0.6, 1.4)))
    W = rng.standard_normal((4, 9))
    g = P.kernels.chain_vjp(chain, X, W)
    h = 1e-6
    for (d, j) in ((0, 0), (1, 4), (0, 8)):
        E = np.zeros_like(X)
        E[d, j] = h
        fd = (np.sum(W * P.kernels.apply_chain(chain, X + E)) - np.sum(W * P.kernels.apply_chain(chain, X - E))) / (2 * h)
        assert abs(g[d, j] - fd) <= 1e-8 * max(1.0, abs(fd))


def test_evaluator_contraction_matches_central_differences_of_its_own_matrix():
    """np_contract is the reference of the GPU gradient test: its three outputs against finite differences of sum(G o K)"""
    rng = np.random.default_rng(3)
    x = rng.uniform(-2, 2, 11)
    G = rng.standard_normal((11, 11))

    def K(c=4.0, g_se=1.0, g_per=1.0, alpha=1.3, g_rq=1.0, c_lin=0.25, g_lin=1.0):
        k = (c * P.with_lengthscale(P.SEKernel(), 1.5 / g_se) * (P.PeriodicKernel(0.6 / g_per) @ P.ScaleTransform(1.0 / 0.9)) +
             0.7 * P.with_lengthscale(P.RationalQuadraticKernel(alpha), 0.8 / g_rq) +
             0.1 * P.with_lengthscale(P.LinearKernel(c_lin), 1.0 / g_lin) * P.LinearKernel(c_lin))
        return P.build_spec(_atom(k), x)[0]

    spec = K()
    gc, gs, gp = kn.np_contract(spec, G)
    f = lambda **kw: float(np.sum(G * kn.np_spec_matrix(K(**kw))))      # noqa: E731
    h = 1e-6
    fd = lambda name, v0: (f(**{name: v0 + h}) - f(**{name: v0 - h})) / (2 * h)      # noqa: E731
    # terms: 0 SE (head), 1 SE over sincos, 2 RQ, 3 LINEAR (head), 4 LINEAR
    assert [T.kind for T in spec._terms[:5]] == [L.SE, L.SE | L.KIND_TIMES_PREV, L.RQ, L.LINEAR, L.LINEAR | L.KIND_TIMES_PREV]
    for got, want in ((gc[0], fd("c", 4.0)), (gs[0], fd("g_se", 1.0)), (gs[1], fd("g_per", 1.0)), (gp[2], fd("alpha", 1.3)),
                      (gs[2], fd("g_rq", 1.0)), (gp[3] + gp[4], fd("c_lin", 0.25)), (gs[3], fd("g_lin", 1.0))):
        assert abs(got - want) <= 2e-7 * max(1.0, abs(want)), (got, want)
    assert gc[1] == 0.0 and gc[4] == 0.0 and gp[0] == 0.0 and gp[1] == 0.0


# ---- 3. scikit-learn golden ---------------------------------------------------------------------------------------------
def test_sklearn_golden_through_flattener_and_evaluator():
    x, y, Kg, g = load_golden()
    assert len(x) == 150 and x.min() >= -3 and x.max() <= 3 and 1e3 < g["cond"] < 1e4
    # the two statements of the model agree: closed forms in this package's parametrisation against scikit-learn's matrix
    X = x[None, :]
    closed = (4.0 * c_se(X, X, 1.5) * c_per(X, X, 0.6, 0.9) + 0.7 * c_rq(X, X, 1.3, 0.8) + 0.1 * c_lin(X, X, 0.25) ** 2)
    rows = g["K_rows"]
    assert len(rows) == 15 and np.abs(closed[rows] - Kg).max() <= 1e-14 * np.abs(Kg).max()
    spec, _, _ = P.build_spec(_atom(golden_kernel()), x)
    assert spec.n_terms == 5 and [len(ts) for _, _, ts in kn.chains(spec)] == [2, 1, 2]
    K = kn.np_spec_matrix(spec)
    assert np.abs(K[rows] - Kg).max() <= 1e-13 * np.abs(Kg).max()
    lml = np_logpdf(K + g["noise"] * np.eye(150), y)
    assert abs(lml - g["lml"]) <= 1e-10 * abs(g["lml"]), (lml, g["lml"])


# ---- 4. the flattener ----------------------------------------------------------------------------------------------------
def test_products_of_sums_are_distributed_with_the_right_coefficients():
    a, b, c = 1.5, -0.4, 3.0
    k = (a * P.SEKernel() + b * P.Matern12Kernel()) * (c * P.Matern32Kernel() + P.Matern52Kernel())
    lp = k.leaf_products()
    assert [(co, [f[0] for f in fs]) for co, fs in lp] == [(a * c, [L.SE, L.MATERN32]), (a, [L.SE, L.MATERN52]),
                                                           (b * c, [L.MATERN12, L.MATERN32]), (b, [L.MATERN12, L.MATERN52])]
    with pytest.raises(NotImplementedError, match="product"):
        k.leaf_terms()
    assert isinstance(P.SEKernel() * P.Matern32Kernel(), P.KernelProduct)
    assert isinstance(P.SEKernel() * 2.0, P.ScaledKernel) and isinstance(2 * P.SEKernel(), P.ScaledKernel)
    spec, _, _ = P.build_spec(_atom(k), np.linspace(0, 1, 4))
    T = spec._terms
    assert spec.n_terms == 8 and spec.inputs[0].shape == (1, 4) and len(spec.inputs) == 1
    assert [T[t].kind for t in range(8)] == [L.SE, L.MATERN32 | 0x100, L.SE, L.MATERN52 | 0x100, L.MATERN12,
                                             L.MATERN32 | 0x100, L.MATERN12, L.MATERN52 | 0x100]
    assert [T[t].coef for t in range(8)] == [a * c, 1.0, a, 1.0, b * c, 1.0, b, 1.0]
    # product-free kernels keep their leaf_terms 4-tuples and their specs
    k0 = 2.0 * P.with_lengthscale(P.SEKernel(), 0.5) + P.ConstantKernel(0.3)
    assert k0.leaf_terms() == [(L.SE, 2.0, 0.0, (("scale", 2.0),)), (L.CONST, 1.0, 0.3, ())]
    assert k0.leaf_products() == [(2.0, [(L.SE, 0.0, (("scale", 2.0),))]), (1.0, [(L.CONST, 0.3, ())])]
    assert not P.build_spec(_atom(k0), np.linspace(0, 1, 4))[0].has_kprod
    assert P.PolynomialKernel(3, 0.5).leaf_products() == [(1.0, [(L.LINEAR, 0.5, ())] * 3)]
    assert P.RationalQuadraticKernel().alpha == 2.0 and P.LinearKernel().c == 0.0 and P.PolynomialKernel().degree == 2


def test_transforms_above_a_product_reach_every_factor():
    inner = P.with_lengthscale(P.SEKernel(), 0.5) * P.RationalQuadraticKernel(0.7) * P.LinearKernel(0.1)
    k = P.with_lengthscale(inner, 2.0) @ P.PeriodicTransform(0.3)
    (coef, fs), = k.leaf_products()
    per, sc = ("periodic", 0.3), ("scale", 0.5)
    assert coef == 1.0 and [f[2] for f in fs] == [(per,), (per, sc), (per, sc)]      # (SE: 2.0 * 0.5 merged away)
    rng = np.random.default_rng(4)
    x, y = rng.uniform(-1, 1, 6), rng.uniform(-1, 1, 5)
    spec, _, _ = P.build_spec(_atom(k), x, None, y)
    emb = lambda v: np.vstack([np.sin(2 * np.pi * 0.3 * v), np.cos(2 * np.pi * 0.3 * v)])     # noqa: E731
    X, Y = emb(x), emb(y)
    want = c_se(X, Y, 1.0) * c_rq(0.5 * X, 0.5 * Y, 0.7) * c_lin(0.5 * X, 0.5 * Y, 0.1)
    assert np.abs(kn.np_spec_matrix(spec) - want).max() <= 1e-14 * np.abs(want).max()


class _OProd(okf.Kernel):
    """an entrywise product for the oracle's recursion (closed forms; the oracle itself has no product kernel)"""

    def __init__(self, *fs):
        self.fs = fs

    def matrix(self, X, Y=None, faithful=True):
        Y = X if Y is None else Y
        out = 1.0
        for f in self.fs:
            out = out * f(X, Y)
        return out


def test_product_inside_a_gppp_with_sums_scales_and_stretch_matches_the_recursion():
    """the reference's recursion (oracle/stheno.py), given closed-form product kernels, against the evaluator on the
    flattened spec: cov over three processes in BlockData, and a rectangular cross"""
    def build(api, k1, k2):
        gpc = api.GPC()
        f1, f2 = api.atomic(api.GP(k1), gpc), api.atomic(api.GP(k2), gpc)
        f3 = 2.0 * api.stretch(f1, 0.7) + f2
        return {"f1": f1, "f2": f2, "f3": f3, "f4": f3 - 0.5 * f1}, gpc

    import models
    k1p = 1.3 * P.SEKernel() * P.with_lengthscale(P.RationalQuadraticKernel(0.8), 1.2) + 0.2 * P.Matern32Kernel()
    k2p = P.PolynomialKernel(2, 0.3) * P.with_lengthscale(P.Matern12Kernel(), 0.9)
    k1o = okf.KernelSum([_OProd(lambda X, Y: 1.3 * c_se(X, Y), lambda X, Y: c_rq(X, Y, 0.8, 1.2)), 0.2 * okf.Matern32Kernel()])
    k2o = _OProd(lambda X, Y: c_lin(X, Y, 0.3) ** 2, lambda X, Y: np.exp(-np.sqrt(_d2(X, Y)) / 0.9))
    fo, go = build(models.oracle_api(), k1o, k2o)
    fp, gp = build(models.product_api(), k1p, k2p)
    rng = np.random.default_rng(5)
    names = ["f1", "f3", "f4", "f2"]
    xs = [rng.standard_normal(n) for n in (4, 5, 3, 6)]
    xo = ost.BlockData([ost.GPPPInput(k, x) for k, x in zip(names, xs)])
    xp = P.BlockData([P.GPPPInput(k, x) for k, x in zip(names, xs)])
    Ko = ost.GPPP(fo, go).cov(xo)
    spec, _, _ = P.build_spec(P.GPPP(fp, gp), xp)
    assert spec.has_kprod
    np.testing.assert_allclose(kn.np_spec_matrix(spec), Ko, rtol=1e-12, atol=1e-13)
    ys = rng.standard_normal(7)
    Kx = ost.GPPP(fo, go).cov(xo, ost.GPPPInput("f4", ys))
    specx, _, _ = P.build_spec(P.GPPP(fp, gp), xp, None, P.GPPPInput("f4", ys))
    np.testing.assert_allclose(kn.np_spec_matrix(specx), Kx, rtol=1e-12, atol=1e-13)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_products_below_patch_convolve_or_a_stencil_are_refused_by_name():
    k = P.SEKernel() * P.Matern32Kernel()
    F = P.gppp(lambda GP: (lambda f: {"f": f, "s": P.stencil(f, np.zeros((1, 2)), [1.0, -1.0])})(GP(k)))
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(F, P.GPPPInput("s", np.linspace(0, 1, 4)))
    Fc = P.gppp(lambda GP: (lambda g: {"g": g, "f": P.patch_convolve(g, patch_shape=(3, 3))})(GP(P.RationalQuadraticKernel(1.0))))
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(Fc, P.GPPPInput("f", images(2)))
    nine = P.SEKernel()
    for _ in range(8):
        nine = nine * P.SEKernel()
    with pytest.raises(NotImplementedError, match="product.*limit"):
        P.build_spec(_atom(nine), np.linspace(0, 1, 4))


def test_host_refuses_what_the_library_does_not_carry_before_any_call():
    """each raises NotImplementedError naming "product" on the host, before the library is reached (no GPU here)"""
    x = np.linspace(0.0, 1.0, 4)
    f = _atom(golden_kernel())
    fx = f(x, 0.1)
    y = np.zeros(4)
    for kw in (dict(inputs=True), dict(scales=True)):
        with pytest.raises(NotImplementedError, match="product"):
            P.logpdf_and_gradient(fx, y, **kw)
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_and_gradient_batch([fx], [y])
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_and_gradient_pool([fx], [y])
    with pytest.raises(NotImplementedError, match="product"):
        P.elbo_and_gradient(P.VFE(f(np.zeros(2))), fx, y)
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_f32(f(x.astype(np.float32), 0.1), y.astype(np.float32))
    for bad in (lambda: P.RationalQuadraticKernel(0.0), lambda: P.LinearKernel(-1.0), lambda: P.PolynomialKernel(0),
                lambda: P.PolynomialKernel(2.5), lambda: P.PeriodicKernel(0.0)):
        with pytest.raises(ValueError):
            bad()


# ---- 6. the extension header ------------------------------------------------------------------------------------------------
def test_kprod_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "kprod_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_kprod.h"
int main(int argc, char** argv) {
  typedef int (*fn_t)(sgp_ctx*, const sgp_cov_spec*, const double*, int, const double*, const double*, double*, double*,
                      double*, double*, double*, double*, double*);
  fn_t probe = 0;
  sgp_term t;
  void* h;
  t.kind = SGP_LINEAR | SGP_KIND_TIMES_PREV;
  printf("fnptr %d kind %d rq %d factors %d dim %d\n", (int)sizeof(probe = &sgp_logpdf_grad_param), (int)t.kind, (int)SGP_RQ,
         SGP_KPROD_MAX_FACTORS, SGP_KPROD_MAX_DIM);
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  printf("%s\n", dlsym(h, "sgp_logpdf_grad_param") ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "kprod_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, L.KPROD_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "8", "kind", "263", "rq", "6", "factors", "8", "dim", "16",
                                                          "resolved"], (out.stdout, out.stderr)
    assert (L.RQ, L.LINEAR, L.KIND_TIMES_PREV, L.KPROD_MAX_FACTORS, L.KPROD_MAX_DIM) == (6, 7, 0x100, 8, 16)


def test_kprod_library_exports_exactly_its_header():
    syms = _symbols_of("sthenomi_kprod.h")
    assert syms == ["sgp_logpdf_grad_param"] == L.kprod_symbols()
    assert _c_exports(L.KPROD_LIB_PATH) == syms
    for other in (L.LIB_PATH, L.CONV_LIB_PATH, L.STENCIL_LIB_PATH, L.BATCH_LIB_PATH, L.POOL_LIB_PATH):
        assert not set(syms) & set(_c_exports(other))
    assert not set(syms) & set(_symbols_of("sthenomi.h"))
    assert hasattr(L.kprod_lib(), "sgp_logpdf_grad_param")
