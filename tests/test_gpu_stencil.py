"""Stencil GPs on the device: stencil terms assembled by stencil.hip against the NumPy evaluator and the composed sum of
shift views, the plain term (one point, zero offset, unit weight), and the operators built on the assembly (logpdf, rand,
posterior, ELBO); the reference's quadrature-convolution, custom-affine-transformation and differentiation examples; the
paths without a stencil kernel refuse stencil terms."""
import ctypes as C

import numpy as np
import pytest

import stheno_jl_amd as P
from test_conv_on_numpy import conv_model, images
from test_stencil_on_numpy import np_spec_matrix

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300)


KERNELS = {"se": lambda: 1.7 * P.with_lengthscale(P.SEKernel(), 0.9),
           "m12": lambda: 0.8 * P.with_lengthscale(P.Matern12Kernel(), 1.4),
           "m32": lambda: 1.2 * P.Matern32Kernel(),
           "m52": lambda: 0.6 * P.with_lengthscale(P.Matern52Kernel(), 0.5)}


def model(kernel, D, seed=0):
    """f; g = stencil(f, A, w); h = stencil(f, B, v) with a different stencil; u an independent plain process"""
    rng = np.random.default_rng(seed)
    A, w = 0.5 * rng.standard_normal((D, 5)), rng.standard_normal(5)
    B, v = 0.5 * rng.standard_normal((D, 3)), rng.standard_normal(3)

    def build(GP):
        f = GP(KERNELS[kernel]())
        u = GP(0.3 * P.SEKernel())
        g = P.stencil(f, A, w)
        return {"f": f, "u": u, "g": g, "h": P.stencil(f, B, v), "gu": 0.7 * g + u + f}
    return P.gppp(build)


def pts(D, n, seed):
    X = np.random.default_rng(seed).uniform(-2.0, 2.0, (D, n))
    return X[0] if D == 1 else P.ColVecs(X)


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_cov_var_cross_match_the_numpy_evaluator(kernel, D):
    F = model(kernel, D)
    x, y = pts(D, 150, 1), pts(D, 70, 2)
    g, h, f = P.GPPPInput("g", x), P.GPPPInput("h", y), P.GPPPInput("f", y)
    # two-sided (the same and different stencils per side), one-sided either way round
    for a, b in [(g, None), (g, h), (g, f), (f, g), (h, P.GPPPInput("gu", x))]:
        spec, _, _ = P.build_spec(F, a, None, b)
        K = P.cov(F(a)) if b is None else P.cov(F(a), F(b))
        assert rel(K, np_spec_matrix(spec)) <= 1e-12
    spec, _, _ = P.build_spec(F, g)
    assert rel(P.var(F(g)), np.diag(np_spec_matrix(spec))) <= 1e-12
    # joint blocks: plain, one-sided and two-sided pairs in one symmetric spec at odd tile offsets, lower tiles + mirror
    xb = P.BlockData([P.GPPPInput("f", pts(D, 61, 3)), g, P.GPPPInput("gu", pts(D, 90, 4)), h])
    spec, _, _ = P.build_spec(F, xb)
    K = P.cov(F(xb))
    assert rel(K, np_spec_matrix(spec)) <= 1e-12
    assert np.array_equal(K, K.T)
    assert rel(P.var(F(xb)), np.diag(np_spec_matrix(spec))) <= 1e-12


@pytest.mark.parametrize("kernel", ["se", "m52"])
def test_matches_the_composed_sum_of_shifts(kernel):
    rng = np.random.default_rng(7)
    A, w = rng.standard_normal((2, 6)), rng.standard_normal(6)

    def build(GP):
        f = GP(KERNELS[kernel]())
        fs = w[0] * P.shift(f, A[:, 0])
        for q in range(1, 6):
            fs = fs + w[q] * P.shift(f, A[:, q])
        return {"f": f, "g": P.stencil(f, A, w), "fs": fs}
    F = P.gppp(build)
    x = P.ColVecs(rng.standard_normal((2, 200)))
    z = P.ColVecs(rng.standard_normal((2, 33)))
    assert rel(P.cov(F(P.GPPPInput("g", x))), P.cov(F(P.GPPPInput("fs", x)))) <= 1e-12
    assert rel(P.cov(F(P.GPPPInput("g", x)), F(P.GPPPInput("f", z))),
               P.cov(F(P.GPPPInput("fs", x)), F(P.GPPPInput("f", z)))) <= 1e-12
    assert rel(P.var(F(P.GPPPInput("g", x))), P.var(F(P.GPPPInput("fs", x)))) <= 1e-12


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_unit_stencil_is_bit_identical_to_the_plain_term(kernel):
    """one point, zero offset, unit weight: x - 0 == x and the weights multiply by 1 exactly"""
    def build(GP):
        f = GP(KERNELS[kernel]())
        return {"f": f, "g": P.stencil(f, np.zeros((3, 1)), [1.0])}
    F = P.gppp(build)
    x, z = pts(3, 300, 5), pts(3, 41, 6)
    xf, xg, zf, zg = (P.GPPPInput(k, v) for k, v in [("f", x), ("g", x), ("f", z), ("g", z)])
    assert np.array_equal(P.cov(F(xg)), P.cov(F(xf)))
    assert np.array_equal(P.cov(F(xg), F(zf)), P.cov(F(xf), F(zf)))
    assert np.array_equal(P.cov(F(zf), F(xg)), P.cov(F(zf), F(xf)))
    assert np.array_equal(P.cov(F(xg), F(zg)), P.cov(F(xf), F(zf)))
    assert np.array_equal(P.var(F(xg)), P.var(F(xf)))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_var_is_diag_of_cov_bit_for_bit(kernel):
    F = model(kernel, 3)
    for k in ["g", "gu", "h"]:
        x = P.GPPPInput(k, pts(3, 260, 8))
        assert np.array_equal(P.var(F(x)), np.diag(P.cov(F(x))))


def np_logpdf(K, m, y):
    L = np.linalg.cholesky(K)
    a = np.linalg.solve(L, y - m)
    return -0.5 * a @ a - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2 * np.pi)


def test_logpdf_rand_posterior_match_numpy_cholesky():
    F = model("m52", 1)
    x = P.GPPPInput("gu", pts(1, 60, 9))
    spec, _, _ = P.build_spec(F, x)
    K = np_spec_matrix(spec) + 0.1 * np.eye(60)
    rng = np.random.default_rng(11)
    y = rng.standard_normal(60)
    fx = F(x, 0.1)
    assert abs(P.logpdf(fx, y) - np_logpdf(K, 0.0, y)) <= 1e-10 * abs(np_logpdf(K, 0.0, y))
    Z = rng.standard_normal((60, 3))
    assert rel(P.rand(rng, fx, 3, Z=Z), np.linalg.cholesky(K) @ Z) <= 1e-10
    post = P.posterior(fx, y)
    for k in ["g", "h", "f"]:
        xs = P.GPPPInput(k, pts(1, 25, 12))
        Ksx = np_spec_matrix(P.build_spec(F, xs, None, x)[0])
        Kss = np_spec_matrix(P.build_spec(F, xs)[0])
        m, v = P.mean_and_var(post(xs))
        assert rel(m, Ksx @ np.linalg.solve(K, y)) <= 1e-10
        assert rel(v, np.diag(Kss - Ksx @ np.linalg.solve(K, Ksx.T))) <= 1e-9


def test_elbo_matches_the_titsias_bound():
    """pseudo-points in f, data on g (a well-conditioned K(z, z): the bound's reference is a plain NumPy solve)"""
    F = model("m52", 1)
    x, z = P.GPPPInput("g", pts(1, 80, 13)), P.GPPPInput("f", np.linspace(-2.0, 2.0, 8))
    y = np.random.default_rng(2).standard_normal(80)
    val = P.elbo(P.VFE(F(z)), F(x, 0.1), y)
    Kxx = np_spec_matrix(P.build_spec(F, x)[0])
    Kxz = np_spec_matrix(P.build_spec(F, x, None, z)[0])
    Kzz = np_spec_matrix(P.build_spec(F, z)[0]) + 1e-18 * np.eye(8)
    A = np.linalg.solve(np.linalg.cholesky(Kzz), Kxz.T)
    Q = A.T @ A
    ref = np_logpdf(Q + 0.1 * np.eye(80), 0.0, y) - 0.5 * (np.trace(Kxx) - np.trace(Q)) / 0.1
    assert abs(val - ref) <= 1e-10 * abs(ref)


def test_the_quadrature_convolution_example():
    """examples/quadrature-convolution/script.jl: observe f and g = convolve(f) at 2 points each, posterior marginals of
    both on 100 points, against the example's explicit quadrature formulas"""
    def build(GP):
        f = GP(P.with_lengthscale(P.Matern52Kernel(), 0.5))
        return {"f": f, "g": P.quadrature_convolve(f)}
    F = P.gppp(build)
    rng = np.random.default_rng(123)
    xf, xg = rng.uniform(0.0, 1.0, 2) + 1.0, -rng.uniform(0.0, 1.0, 2) - 1.0
    x_obs = P.vcat(P.GPPPInput("f", xf), P.GPPPInput("g", xg))
    y = P.rand(rng, F(x_obs, 1e-3))
    post = P.posterior(F(x_obs, 1e-3), y)
    x_plot = np.linspace(-5.0, 5.0, 100)
    t, w = np.polynomial.hermite.hermgauss(15)

    def k(a, b):
        r = np.sqrt(5.0) * np.abs(a[:, None] - b[None, :]) / 0.5
        return (1.0 + r + r * r / 3.0) * np.exp(-r)

    def k_gf(a, b):      # cov(g, f, a, b) = sum_p w_p k(a - t_p, b)
        return sum(w[p] * k(a - t[p], b) for p in range(15))

    def k_gg(a, b):      # cov(g, g, a, b) = sum_p sum_q w_p w_q k(a - t_p, b - t_q)
        return sum(w[p] * w[q] * k(a - t[p], b - t[q]) for p in range(15) for q in range(15))
    Koo = np.block([[k(xf, xf), k_gf(xg, xf).T], [k_gf(xg, xf), k_gg(xg, xg)]]) + 1e-3 * np.eye(4)
    for key, Kpo, kpp in [("f", np.hstack([k(x_plot, xf), k_gf(xg, x_plot).T]), np.diag(k(x_plot, x_plot))),
                          ("g", np.hstack([k_gf(x_plot, xf), k_gg(x_plot, xg)]), np.diag(k_gg(x_plot, x_plot)))]:
        ms = P.marginals(post(P.GPPPInput(key, x_plot), 1e-6))
        m_ref = Kpo @ np.linalg.solve(Koo, y)
        v_ref = kpp - np.sum(Kpo * np.linalg.solve(Koo, Kpo.T).T, axis=1) + 1e-6
        assert rel([d.mu for d in ms], m_ref) <= 1e-9
        assert rel([d.sigma for d in ms], np.sqrt(v_ref)) <= 1e-8


def test_the_custom_affine_transformation_identities():
    """examples/custom_affine_transformations/script.jl: (A f)(x) = f(x) + f(x + 3) - 2 as stencil(f, [0, -3], [1, 1]) - 2"""
    def build(GP):
        f = GP(P.SEKernel())
        return {"f": f, "Af": P.stencil(f, [0.0, -3.0], [1.0, 1.0]) - 2.0}
    F = P.gppp(build)
    rng = np.random.default_rng(4)
    x_f, x_Af, z_Af = (P.GPPPInput(k, rng.standard_normal(n)) for k, n in [("f", 11), ("Af", 13), ("Af", 9)])
    assert np.allclose(P.mean(F(x_Af)), -2.0 * np.ones(13), rtol=0, atol=0)
    K = P.cov(F(x_Af))
    assert np.allclose(P.cov(F(x_Af), F(x_Af)), K, rtol=1e-14, atol=0)
    assert np.allclose(P.var(F(x_Af)), np.diag(K), rtol=1e-14, atol=0)
    assert np.allclose(P.cov(F(x_f), F(x_Af)), P.cov(F(x_Af), F(x_f)).T, rtol=1e-14, atol=0)
    # and the example's own formula for cov(Af, Af, x, y)
    a, b = x_Af.x, z_Af.x

    def k(u, v):
        return np.exp(-0.5 * (u[:, None] - v[None, :]) ** 2)
    ref = k(a, b) + k(a, b + 3) + k(a + 3, b) + k(a + 3, b + 3)
    assert rel(P.cov(F(x_Af), F(z_Af)), ref) <= 1e-13
    assert rel(P.cov(F(x_Af), F(x_f)), k(a, x_f.x) + k(a + 3, x_f.x)) <= 1e-13


def test_the_differentiation_known_answer_through_a_stencil():
    """examples/differentiation/script.jl:120-134 with the derivative as stencil(f, [-h, h], [1/2h, -1/2h])"""
    h = 1e-3

    def build(GP):
        f = GP(P.SEKernel())
        return {"f": f, "df": P.stencil(f, [-h, h], [1.0 / (2.0 * h), -1.0 / (2.0 * h)])}
    F = P.gppp(build)
    x_obs, x_pred = np.linspace(-3.0, 3.0, 25), np.linspace(-2.5, 2.5, 25)
    for fn, dfn in ((np.sin, np.cos), (np.cos, lambda t: -np.sin(t))):
        post = P.posterior(F(P.GPPPInput("f", x_obs), 1e-12), fn(x_obs))
        m = post.mean(P.GPPPInput("df", x_pred))
        assert np.linalg.norm(m - dfn(x_pred)) <= 1e-5 * np.linalg.norm(dfn(x_pred))
        assert np.max(post.var(P.GPPPInput("df", x_pred))) < 1e-3


# ---- refusals and the registration ABI ------------------------------------------------------------------------------
def _bound_call(spec, fn, *args):
    ctx = P.lib.default_context()
    return fn(ctx.handle, spec.ref(ctx), *args)


def test_gradient_and_fp32_entry_points_refuse_stencil_terms():
    F = model("se", 1)
    n = 16
    spec, _, _ = P.build_spec(F, P.GPPPInput("g", pts(1, n, 15)))
    lib = P.lib.load()
    m, y, nz = np.zeros(n), np.ones(n), np.array([0.1])
    lp, gy, gm, gn, gc, gs = np.zeros(1), np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(1), np.zeros(1)
    d = P.lib.dptr
    rc = _bound_call(spec, lib.sgp_logpdf_grad, d(m), P.lib.NOISE_SCALAR, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc),
                     d(gs))
    assert rc < 0 and "stencil" in P.lib.last_error()
    rc = _bound_call(spec, lib.sgp_kernelmatrix_diag_grad, d(y), d(gc), d(gs))
    assert rc < 0 and "stencil" in P.lib.last_error()
    ctx = P.lib.default_context()
    PD = C.POINTER(C.c_double)
    one = lambda a: (PD * 1)(d(a))          # noqa: E731
    rc = P.lib.batch_lib().sgp_logpdf_grad_batch(
        ctx.handle, 1, (C.POINTER(P.lib.sgp_cov_spec) * 1)(C.pointer(spec.bind(ctx).c)), one(m), P.lib.NOISE_SCALAR,
        one(nz), one(y), d(lp), one(gy), one(gm), one(gn), one(gc), one(gs), (C.c_int * 1)())
    assert rc < 0 and "stencil" in P.lib.last_error()
    K32 = np.zeros((n, n), dtype=np.float32)
    rc = _bound_call(spec, lib.sgp_kernelmatrix_f32, K32.ctypes.data_as(C.POINTER(C.c_float)), n)
    assert rc < 0 and "stencil" in P.lib.last_error() and "fp32" in P.lib.last_error()
    rc = _bound_call(spec, lib.sgp_logpdf_f32, d(m), P.lib.NOISE_SCALAR, d(nz), d(y), d(lp))
    assert rc < 0 and "stencil" in P.lib.last_error()
    # the patch refusals keep their messages
    cspec, _, _ = P.build_spec(conv_model(), P.GPPPInput("f", images(4)))
    rc = _bound_call(cspec, lib.sgp_kernelmatrix_diag_grad, d(np.ones(4)), d(gc), d(gs))
    assert rc < 0 and "patch" in P.lib.last_error()
    # and the fp64 kernel matrix of the stencil spec still runs
    K = np.zeros((n, n), order="F")
    assert _bound_call(spec, lib.sgp_kernelmatrix, d(K), n) == 0
    assert rel(K, np_spec_matrix(spec)) <= 1e-12


def test_a_float32_model_runs_on_the_fp64_path():
    F = model("m32", 1)
    x32 = pts(1, 20, 16).astype(np.float32)
    K32 = P.cov(F(P.GPPPInput("g", x32)))
    assert K32.dtype == np.float32
    assert np.array_equal(K32, P.cov(F(P.GPPPInput("g", x32.astype(np.float64)))).astype(np.float32))


def _register(ctx, A, w):
    A = np.ascontiguousarray(np.asarray(A, dtype=np.float64).reshape(-1, len(w)).T)    # column-major D x Q
    w = np.ascontiguousarray(w, dtype=np.float64)
    st = P.lib.sgp_stencil(A.shape[1], len(w), P.lib.dptr(A), P.lib.dptr(w))
    sid = C.c_int32(-1)
    rc = P.lib.stencil_lib().sgp_stencil_register(ctx.handle, C.byref(st), C.byref(sid))
    return rc, sid.value


def test_registration_ids_and_limits():
    ctx = P.lib.Context(0)
    try:
        rc1, a = _register(ctx, [[0.5, -0.5]], [1.0, 2.0])
        rc2, b = _register(ctx, [[0.5, -0.5]], [1.0, 2.0])
        rc3, c = _register(ctx, [[0.5, -0.5]], [1.0, 2.0 + 2e-16 * 2])
        assert rc1 == rc2 == rc3 == 0 and a == b >= 1 and c != a
        # ids share the patch geometries' table
        gid = C.c_int32()
        assert P.lib.conv_lib().sgp_conv_geom(ctx.handle, C.byref(P.lib.sgp_patch_geom(8, 8, 3, 3)), C.byref(gid)) == 0
        assert gid.value not in (a, c)
        assert _register(ctx, np.zeros((16, 64)), np.ones(64))[0] == 0
        for A, w in [(np.zeros((1, 65)), np.ones(65)), (np.zeros((17, 2)), np.ones(2)), ([[0.0]], [np.inf]),
                     ([[np.nan]], [1.0])]:
            rc, _ = _register(ctx, A, w)
            assert rc < 0 and "stencil" in P.lib.last_error()
    finally:
        ctx.close()


def test_spec_checks_of_stencil_ids():
    ctx = P.lib.default_context()
    lib = P.lib.load()
    F = model("se", 1)
    n = 8
    spec, _, _ = P.build_spec(F, P.GPPPInput("g", pts(1, n, 17)))
    spec.bind(ctx)
    K = np.zeros((n, n), order="F")
    call = lambda: lib.sgp_kernelmatrix(ctx.handle, C.byref(spec.c), P.lib.dptr(K), n)   # noqa: E731
    good = spec._terms[0].reserved
    # an unknown id: the message names both tables' registrations
    spec._terms[0].reserved = 0xfff0 | (0xfff0 << 16)
    assert call() < 0 and "stencil" in P.lib.last_error() and "geometry" in P.lib.last_error()
    # a stencil of another dimension than its side
    _, sid2 = _register(ctx, np.zeros((2, 1)), [1.0])
    spec._terms[0].reserved = sid2
    assert call() < 0 and "stencil" in P.lib.last_error()
    # a patch side paired with a stencil side
    gid = C.c_int32()
    assert P.lib.conv_lib().sgp_conv_geom(ctx.handle, C.byref(P.lib.sgp_patch_geom(1, 1, 1, 1)), C.byref(gid)) == 0
    spec._terms[0].reserved = gid.value | ((good & 0xffff) << 16)
    assert call() < 0 and "stencil" in P.lib.last_error() and "patch" in P.lib.last_error()
    spec._terms[0].reserved = good
    assert call() == 0 and rel(K, np_spec_matrix(spec)) <= 1e-12


def test_multi_gpu_context_refuses_stencil_terms():
    F = model("se", 1)
    n = 16
    spec, _, _ = P.build_spec(F, P.GPPPInput("g", pts(1, n, 18)))
    mctx = P.lib.Context(devices=[0, 0])
    try:
        rc, _ = _register(mctx, [[0.0]], [1.0])
        assert rc < 0 and "stencil" in P.lib.last_error() and "multi-GPU" in P.lib.last_error()
        with pytest.raises(NotImplementedError, match="stencil"):
            spec.ref(mctx)
        # ids registered on a single-GPU context mean nothing on the multi-GPU one
        spec.ref(P.lib.default_context())
        K = np.zeros((n, n), order="F")
        rc = mctx.lib.sgp_kernelmatrix(mctx.handle, C.byref(spec.c), P.lib.dptr(K), n)
        assert rc < 0 and "stencil" in P.lib.last_error()
    finally:
        mctx.close()
