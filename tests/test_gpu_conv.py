"""Convolutional GPs on the device: patch terms assembled by conv.hip against the NumPy evaluator, the composed sum-of-select
model, the plain term (patch == image), and the operators built on the assembly (logpdf, rand, posterior, ELBO); the paths
without a patch kernel refuse patch terms."""
import ctypes as C

import numpy as np
import pytest

import stheno_jl_amd as P
from test_conv_on_numpy import conv_model, images, np_spec_matrix

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300)


KERNELS = {"se": lambda: 1.7 * P.with_lengthscale(P.SEKernel(), 2.5),
           "m52": lambda: 0.8 * P.with_lengthscale(P.Matern52Kernel(), 3.0)}


def setup(kernel="se", n=20, m=7, seed=0):
    f = conv_model(KERNELS[kernel]())
    x = P.GPPPInput("f", images(n, seed=seed))
    z = P.GPPPInput("g", P.ColVecs(np.random.default_rng(seed + 1).standard_normal((9, m))))
    return f, x, z


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_cov_var_cross_match_the_numpy_evaluator(kernel):
    f, x, z = setup(kernel)
    for args in [(x,), (x, z), (z, x)]:
        spec, _, _ = P.build_spec(f, args[0], None, args[1] if len(args) > 1 else None)
        K = P.cov(f(args[0])) if len(args) == 1 else P.cov(f(args[0]), f(args[1]))
        assert rel(K, np_spec_matrix(spec)) <= 1e-13
    spec, _, _ = P.build_spec(f, x)
    assert rel(P.var(f(x)), np.diag(np_spec_matrix(spec))) <= 1e-13
    # joint blocks (f, g, f + h): every mix of patched and plain sides in one symmetric spec, lower triangle + mirror
    xb = P.BlockData([x, z, P.GPPPInput("fh", x.x)])
    spec, _, _ = P.build_spec(f, xb)
    K = P.cov(f(xb))
    assert rel(K, np_spec_matrix(spec)) <= 1e-13
    assert np.array_equal(K, K.T)


def test_matches_the_composed_sum_of_selects():
    """the same matrix through the existing assembly: f = sum_p select(g, idx_p) over the 36 patches of 8 x 8 images"""
    H = W = 8
    idx = [[(pr + a) + (pc + b) * H for b in range(3) for a in range(3)] for pc in range(W - 2) for pr in range(H - 2)]

    def build(GP):
        g = GP(KERNELS["se"]())
        fs = P.select(g, idx[0])
        for ix in idx[1:]:
            fs = fs + P.select(g, ix)
        return {"g": g, "f": P.patch_convolve(g), "fs": fs}
    f = P.gppp(build)
    im = images(12)
    Kc = P.cov(f(P.GPPPInput("f", im)))
    Ks = P.cov(f(P.GPPPInput("fs", P.ColVecs(im.X))))
    assert rel(Kc, Ks) <= 1e-12


def test_whole_image_patch_is_bit_identical_to_the_plain_term():
    """P = 1 (patch == image): the patch kernels reproduce the plain assembly bit for bit"""
    def build(GP):
        g = GP(KERNELS["m52"]())
        return {"g": g, "f": P.patch_convolve(g, patch_shape=(3, 3))}
    f = P.gppp(build)
    X = np.random.default_rng(5).standard_normal((3, 3, 150))
    xi, xc = P.GPPPInput("f", P.ImageVector(X)), P.GPPPInput("g", P.ColVecs(X.reshape(9, -1, order="F")))
    z = P.GPPPInput("g", P.ColVecs(np.random.default_rng(6).standard_normal((9, 40))))
    assert np.array_equal(P.cov(f(xi)), P.cov(f(xc)))
    assert np.array_equal(P.cov(f(xi), f(z)), P.cov(f(xc), f(z)))
    assert np.array_equal(P.cov(f(z), f(xi)), P.cov(f(z), f(xc)))
    assert np.array_equal(P.var(f(xi)), P.var(f(xc)))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_var_is_diag_of_cov_bit_for_bit(kernel):
    f, x, _ = setup(kernel, n=150)
    assert np.array_equal(P.var(f(x)), np.diag(P.cov(f(x))))
    xh = P.GPPPInput("fh", x.x)      # a conv term and a plain term in one pair
    assert np.array_equal(P.var(f(xh)), np.diag(P.cov(f(xh))))


def np_logpdf(K, m, y):
    L = np.linalg.cholesky(K)
    a = np.linalg.solve(L, y - m)
    return -0.5 * a @ a - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2 * np.pi)


def test_logpdf_rand_posterior_match_numpy_cholesky():
    f, x, z = setup("se", n=40)
    spec, _, _ = P.build_spec(f, x)
    K = np_spec_matrix(spec) + 0.1 * np.eye(40)
    rng = np.random.default_rng(11)
    y = rng.standard_normal(40)
    fx = f(x, 0.1)
    assert abs(P.logpdf(fx, y) - np_logpdf(K, 0.0, y)) <= 1e-10 * abs(np_logpdf(K, 0.0, y))
    Z = rng.standard_normal((40, 3))
    s = P.rand(rng, fx, 3, Z=Z)
    assert rel(s, np.linalg.cholesky(K) @ Z) <= 1e-10
    post = P.posterior(fx, y)
    xs = P.GPPPInput("f", images(9, seed=4))
    ks, _, _ = P.build_spec(f, xs, None, x)
    kss, _, _ = P.build_spec(f, xs)
    Ksx, Kss = np_spec_matrix(ks), np_spec_matrix(kss)
    m, v = P.mean_and_var(post(xs))
    assert rel(m, Ksx @ np.linalg.solve(K, y)) <= 1e-10
    assert rel(v, np.diag(Kss - Ksx @ np.linalg.solve(K, Ksx.T))) <= 1e-10
    # predictions at the pseudo-point process g
    kz, _, _ = P.build_spec(f, z, None, x)
    assert rel(P.mean(post(z)), np_spec_matrix(kz) @ np.linalg.solve(K, y)) <= 1e-10


def np_titsias(Kff_diag, Kfz, Kzz, y, s2):
    n = len(y)
    Lz = np.linalg.cholesky(Kzz)
    A = np.linalg.solve(Lz, Kfz.T)
    Q = A.T @ A
    return np_logpdf(Q + s2 * np.eye(n), 0.0, y) - 0.5 * (np.sum(Kff_diag) - np.trace(Q)) / s2


def test_elbo_matches_the_titsias_bound():
    f, x, z = setup("m52", n=60, m=10)
    y = np.random.default_rng(2).standard_normal(60)
    val = P.elbo(P.VFE(f(z)), f(x, 0.1), y)
    sxx, _, _ = P.build_spec(f, x)
    sxz, _, _ = P.build_spec(f, x, None, z)
    szz, _, _ = P.build_spec(f, z)
    ref = np_titsias(np.diag(np_spec_matrix(sxx)), np_spec_matrix(sxz), np_spec_matrix(szz) + 1e-18 * np.eye(10), y, 0.1)
    assert abs(val - ref) <= 1e-10 * abs(ref)


def test_the_reference_example_sequence_on_28x28_images():
    """examples/convolutional_gp/script.jl on synthetic 28 x 28 images (no MNIST here)"""
    def build(GP):
        g = GP(1.0 * P.with_lengthscale(P.SEKernel(), 1.0))
        return {"g": g, "f": P.patch_convolve(g)}
    f = P.gppp(build)
    rng = np.random.default_rng(28)
    x = P.ImageVector(rng.uniform(0.0, 1.0, (28, 28, 10)).astype(np.float32))
    fx = P.GPPPInput("f", x)
    assert np.all(P.mean(f(fx)) == 0)
    c1 = P.cov(f(fx), f(P.GPPPInput("g", P.extract_patches(x)[0])))
    assert c1.shape == (10, 10)
    K = P.cov(f(fx))
    v = P.var(f(fx))
    assert np.array_equal(v, np.diag(K))
    x64 = P.GPPPInput("f", P.ImageVector(x.X.reshape(28, 28, 10, order="F")))
    spec, _, _ = P.build_spec(f, x64)
    assert rel(P.cov(f(x64)), np_spec_matrix(spec)) <= 1e-13
    z = P.GPPPInput("g", P.ColVecs(rng.standard_normal((9, 100))))
    x = P.GPPPInput("f", P.ImageVector(rng.uniform(0.0, 1.0, (28, 28, 15))))
    y = P.rand(rng, f(x, 0.1))
    assert y.shape == (15,)
    assert P.cov(f(x), f(z)).shape == (15, 100)
    val = P.elbo(P.VFE(f(z)), f(x, 0.1), y)
    assert np.isfinite(val) and val <= P.logpdf(f(x, 0.1), y) + 1e-8


def _bound_call(spec, fn, *args):
    ctx = P.lib.default_context()
    return fn(ctx.handle, spec.ref(ctx), *args)


def test_gradient_and_fp32_entry_points_refuse_patch_terms():
    f, x, _ = setup("se", n=16)
    spec, _, _ = P.build_spec(f, x)
    lib = P.lib.load()
    n = 16
    m, y, nz = np.zeros(n), np.ones(n), np.array([0.1])
    lp, gy, gm, gn, gc, gs = np.zeros(1), np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(1), np.zeros(1)
    d = P.lib.dptr
    rc = _bound_call(spec, lib.sgp_logpdf_grad, d(m), P.lib.NOISE_SCALAR, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc),
                     d(gs))
    assert rc < 0 and "patch" in P.lib.last_error()
    rc = _bound_call(spec, lib.sgp_kernelmatrix_diag_grad, d(y), d(gc), d(gs))
    assert rc < 0 and "patch" in P.lib.last_error()
    K32 = np.zeros((n, n), dtype=np.float32)
    rc = _bound_call(spec, lib.sgp_kernelmatrix_f32, K32.ctypes.data_as(C.POINTER(C.c_float)), n)
    assert rc < 0 and "fp32" in P.lib.last_error()
    rc = _bound_call(spec, lib.sgp_logpdf_f32, d(m), P.lib.NOISE_SCALAR, d(nz), d(y), d(lp))
    assert rc < 0 and "fp32" in P.lib.last_error()
    # and the plain kernel matrix of the same spec still runs
    K = np.zeros((n, n), order="F")
    assert _bound_call(spec, lib.sgp_kernelmatrix, d(K), n) == 0
    assert rel(K, np_spec_matrix(spec)) <= 1e-13


def test_a_float32_model_runs_on_the_fp64_path():
    f, x, _ = setup("se", n=12)
    x32 = P.GPPPInput("f", P.ImageVector(x.x.X.reshape(8, 8, 12, order="F").astype(np.float32)))
    K32 = P.cov(f(x32))
    assert K32.dtype == np.float32
    spec, _, _ = P.build_spec(f, x32)
    assert not spec.f32_supported()
    assert np.array_equal(K32, P.cov(f(P.GPPPInput("f", P.ImageVector(x32.x.X.reshape(8, 8, 12, order="F"))))).astype(np.float32))


def test_multi_gpu_context_refuses_patch_terms():
    f, x, _ = setup("se", n=16)
    spec, _, _ = P.build_spec(f, x)
    mctx = P.lib.Context(devices=[0, 0])
    try:
        with pytest.raises(P.SthenoMIError, match="multi-GPU"):
            spec.ref(mctx)
        # ids registered on a single-GPU context mean nothing on the multi-GPU one
        spec.ref(P.lib.default_context())
        K = np.zeros((16, 16), order="F")
        rc = mctx.lib.sgp_kernelmatrix(mctx.handle, C.byref(spec.c), P.lib.dptr(K), 16)
        assert rc < 0 and "geometry" in P.lib.last_error()
    finally:
        mctx.close()
