"""The Gibbs kind on the device (csrc/gibbs.hip; include/sthenomi.h: SGP_GIBBS) against the formula written directly in long
double.  Bounds, in units of 2^-53 (docs/03_kernels.md, 3.2g; x = s / q): an entry is right to U = x (D + 6) + 5 p + 8 units of
itself (+ 2^-1070 where it is subnormal); a gradient sum to U + 10 units of the sum of its absolute addends, with 2 units of
|a_i a_j| + |C^-1_ij| for the cotangent the device forms.  Every case has N <= 300."""
import ctypes as C

import numpy as np
import pytest

import stheno_jl_amd as P
from stheno_jl_amd import lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]
LD, EPS, TINY = np.longdouble, 2.0 ** -53, 2.0 ** -1070
PD = C.POINTER(C.c_double)


def pair_ld(X, Y):
    """(s / q, q, c, location differences) of points (location rows, then the lengthscale row) in long double"""
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD)
    u = X[:-1, :, None] - Y[:-1, None, :]
    lx, ly = X[-1][:, None], Y[-1][None, :]
    q = lx * lx + ly * ly
    return (u * u).sum(0) / q, q, 2 * lx * ly / q, u


def gibbs_ld(X, Y, p):
    x, _, c, _ = pair_ld(X, Y)
    return c ** (LD(p) / 2) * np.exp(-x)


def units(X, Y, p):
    return pair_ld(X, Y)[0].astype(np.float64) * (X.shape[0] + 5) + 5 * p + 8


def points(dim, n, seed):
    """n points of dimension dim: from 8 points on, a coincident pair, lengthscale ratios 10^+-3 and a far point"""
    rng = np.random.default_rng(seed)
    Z = np.asfortranarray(np.vstack([rng.uniform(-1.0, 1.0, (dim - 1, n)), rng.uniform(0.2, 1.5, (1, n))]))
    if n >= 8:
        Z[:, 1] = Z[:, 0]
        Z[-1, 2], Z[-1, 3] = 1e3 * Z[-1, 0], 1e-3 * Z[-1, 0]
        Z[:-1, 4] = 300.0
        Z[:, n - 1] = Z[:, n // 2]              # coincident across a tile edge
    return Z


def call(fn, spec, *args):
    ctx = L.default_context()
    return fn(ctx.handle, spec.ref(ctx), *args)


def matrix(spec):
    K = np.zeros((spec.N, spec.M), order="F")
    assert call(L.load().sgp_kernelmatrix, spec, L.dptr(K), spec.N) == 0, L.last_error()
    return K


def check_values(K, Zr, Zc, p, coef, rs, cs):
    w = (coef * rs)[:, None] * cs[None, :]
    x = pair_ld(Zr, Zc)[0]
    ref = w.astype(LD) * gibbs_ld(Zr, Zc, p)
    frac = np.abs(K - ref).astype(np.float64) / (units(Zr, Zc, p) * EPS * np.abs(ref).astype(np.float64) + TINY * np.abs(w))
    assert np.all(frac <= 1.0), (float(frac.max()), np.unravel_index(frac.argmax(), frac.shape))
    assert np.all(K[x > 800] == 0.0)
    same = np.all(Zr[:, :, None] == Zc[:, None, :], axis=0)
    assert np.array_equal(K[same], w[same])
    return float(frac.max()), int((x > 800).sum()), int(same.sum())


@pytest.mark.parametrize("p", [1, "D", 16])
@pytest.mark.parametrize("dim", [2, 3, 5, 16])
def test_values_exact_cases_and_diagonal(dim, p):
    p = dim - 1 if p == "D" else p
    worst = 0.0
    for n in (1, 127, 128, 129, 257):
        Z, r = points(dim, n, 10 * dim + n), np.linspace(0.5, 1.5, n)
        spec = L.Spec([n], [n], [Z], {(0, 0): [(L.GIBBS, 0, 0, -0.75, float(p), r, r)]}, True)
        K = matrix(spec)
        frac, dead, same = check_values(K, Z, Z, p, -0.75, r, r)
        assert n < 8 or (dead >= 2 * (n - 2) and same >= n + 4)
        diag = np.zeros(n)
        assert call(L.load().sgp_kernelmatrix_diag, spec, L.dptr(diag)) == 0, L.last_error()
        assert np.array_equal(diag, np.diag(K)) and np.array_equal(K, K.T)
        worst = max(worst, frac)
    A, B = points(dim, 129, 7), points(dim, 65, 8)
    B[:, 9] = A[:, 128]
    ra, cb = np.linspace(0.5, 1.5, 129), np.linspace(2.0, 1.0, 65)
    K = matrix(L.Spec([129], [65], [A, B], {(0, 0): [(L.GIBBS, 0, 1, 1.25, float(p), ra, cb)]}, False))
    worst = max(worst, check_values(K, A, B, p, 1.25, ra, cb)[0])
    print(f"dim {dim} p {p}: largest value error / bound = {worst:.3g}")


def test_group_of_two_powers_between_an_se_term_and_an_rq_chain():
    Z = points(4, 130, 3)
    X = np.asfortranarray(Z[:-1])
    terms = [(L.RQ, 1, 1, 0.5, 2.0, None, None), (L.GIBBS, 0, 0, 0.7, 1.0, None, None), (L.SE, 1, 1, 0.3, 0.0, None, None),
             (L.GIBBS, 0, 0, 0.2, 3.0, None, None)]
    K = matrix(L.Spec([130], [130], [Z, X], {(0, 0): terms}, True))
    d2 = ((X[:, :, None] - X[:, None, :]).astype(LD) ** 2).sum(0)
    parts = [LD(0.5) * (1 + d2 / 4) ** -2, LD(0.7) * gibbs_ld(Z, Z, 1), LD(0.3) * np.exp(-d2 / 2), LD(0.2) * gibbs_ld(Z, Z, 3)]
    bound = (units(Z, Z, 3) + 16) * EPS * sum(np.abs(q) for q in parts).astype(np.float64) + TINY
    assert np.all(np.abs(K - sum(parts)) <= bound)


def grad_x(spec, y, dense_noise=None):
    """sgp_logpdf_grad_x outputs; dense_noise: Sigma_y as a matrix, whose gradient is the cotangent G itself"""
    n, nt, d = spec.N, spec.n_terms, L.dptr
    out = dict(lp=np.zeros(1), gy=np.zeros(n), gm=np.zeros(n), gn=np.zeros((n, n) if dense_noise is not None else 1, order="F"),
               gc=np.zeros(nt), gs=np.zeros(nt), gx=[np.zeros(a.shape, order="F") for a in spec.inputs])
    noise = np.asfortranarray(dense_noise) if dense_noise is not None else np.array([0.1])
    ptrs = (PD * len(out["gx"]))(*[d(a) for a in out["gx"]])
    rc = call(L.load().sgp_logpdf_grad_x, spec, d(np.zeros(n)), 2 if dense_noise is not None else 0, d(noise), d(y), d(out["lp"]),
              d(out["gy"]), d(out["gm"]), d(out["gn"]), d(out["gc"]), d(out["gs"]), ptrs)
    assert rc == 0, L.last_error()
    return out


@pytest.mark.parametrize("two_inputs", [False, True])
@pytest.mark.parametrize("dim,n", [(2, 129), (5, 257), (16, 129)])
def test_gradients_against_the_long_double_contraction(dim, n, two_inputs):
    p, coef = dim - 1, 0.8
    na = 70 if two_inputs else n
    Zs = [points(dim, na, dim), points(dim, n - na, dim + 1)] if two_inputs else [points(dim, n, dim)]
    lens = [Z.shape[1] for Z in Zs]
    pairs = {(I, J): [(L.GIBBS, I, J, coef, float(p), None, None), (L.GIBBS, I, J, 0.1, 16.0, None, None)]
             for I in range(len(Zs)) for J in range(len(Zs))}
    spec = L.Spec(lens, lens, Zs, pairs, True)
    y = np.cos(np.arange(n) * 0.37)
    out = grad_x(spec, y, dense_noise=0.1 * np.eye(n))
    again = grad_x(spec, y, dense_noise=0.1 * np.eye(n))
    for k in ("gc", "gs", "gn"):
        assert np.array_equal(out[k], again[k])
    assert all(np.array_equal(a, b) for a, b in zip(out["gx"], again["gx"]))
    Z, off = np.hstack(Zs), np.concatenate([[0], np.cumsum(lens)])
    G, aa = out["gn"].astype(LD), np.abs(np.outer(out["gy"], out["gy"]))
    rel = 2 * EPS * 0.5 * (aa + np.abs(aa - 2 * out["gn"])) / np.where(G == 0, 1, np.abs(G))      # of the cotangent the kernels form
    x, q, _, u = pair_ld(Z, Z)
    lx = Z[-1].astype(LD)[:, None]
    ref, err = np.zeros(Z.shape, dtype=LD), np.zeros(Z.shape, dtype=LD)
    for ti, (c, pw) in enumerate(((coef, p), (0.1, 16))):      # p >= D: positive definite
        k, tol = gibbs_ld(Z, Z, pw), (units(Z, Z, pw) + 10) * EPS + rel
        for I, J in ((I, J) for I in range(len(Zs)) for J in range(I + 1)):
            blk, t = np.s_[off[I]:off[I + 1], off[J]:off[J + 1]], 2 * (I * len(Zs) + J) + ti      # the lower pairs, per term
            for got, add in ((out["gc"][t], G * k), (out["gs"][t], c * G * (-2 * x) * k)):
                e = float((np.abs(add) * tol)[blk].sum()) + TINY
                assert abs(got - add[blk].sum()) <= e, (I, J, pw, got, float(add[blk].sum()), e)
        loc = c * G * k * (-2 * u / q)
        dl = c * G * k * (LD(pw) / 2 * (1 / lx - 2 * lx / q) + 2 * x * lx / q)
        dl_abs = np.abs(c * G * k) * (LD(pw) / 2 * (1 / lx + 2 * lx / q) + 2 * x * lx / q)
        ref += np.vstack([loc.sum(-1), dl.sum(-1)[None]])
        err += np.vstack([(np.abs(loc) * tol).sum(-1), (dl_abs * tol).sum(-1)[None]])
    # symmetric spec and cotangent: the row side of every pair, mirror pairs included, covers both roles
    frac = (np.abs(np.hstack(out["gx"]) - 2 * ref) / (2 * err + TINY)).astype(np.float64)
    worst = float(frac.max())
    assert np.all(frac <= 1.0), (worst, np.unravel_index(frac.argmax(), frac.shape))
    print(f"dim {dim} n {n}: largest input-gradient error / bound = {worst:.3g}")


def test_end_to_end_model_and_pool_member():
    n = 300
    x = np.linspace(-1.5, 1.5, n)
    ell = lambda X: 0.3 + 0.2 * X[0] ** 2         # noqa: E731
    f = P.atomic(P.GP(P.GibbsKernel(ell)), P.GPC())
    y = np.sin(3 * x) + 0.1 * np.cos(17 * x)
    Z = np.vstack([x, ell(x[None])])
    Kl = gibbs_ld(Z, Z, 1)
    Kn = Kl.astype(np.float64) + 0.1 * np.eye(n)
    Lc = np.linalg.cholesky(Kn)
    a = np.linalg.solve(Lc.T, np.linalg.solve(Lc, y))
    ref = -0.5 * (y @ a + 2 * np.log(np.diag(Lc)).sum() + n * np.log(2 * np.pi))
    fx = f(x, 0.1)
    assert abs(P.logpdf(fx, y) - ref) <= 1e-10 * abs(ref)
    xs = np.linspace(-1.4, 1.4, 33)
    Zs = np.vstack([xs, ell(xs[None])])
    Ks = gibbs_ld(Zs, Z, 1).astype(np.float64)
    mean, var = P.mean_and_var(P.posterior(fx, y)(xs))
    V = np.linalg.solve(Lc, Ks.T)
    assert np.max(np.abs(mean - Ks @ a)) <= 1e-9 and np.max(np.abs(var - (1.0 - (V * V).sum(0)))) <= 1e-9
    z, jz = x[7::30], 1e-6      # 10 inducing points, a proper subset: the rectangular block K(x, z) matters
    Zz = np.vstack([z, ell(z[None])])
    Lz = np.linalg.cholesky(gibbs_ld(Zz, Zz, 1).astype(np.float64) + jz * np.eye(len(z)))
    A = np.linalg.solve(Lz, gibbs_ld(Zz, Z, 1).astype(np.float64)) / np.sqrt(0.1)
    Lb = np.linalg.cholesky(np.eye(len(z)) + A @ A.T)
    c = np.linalg.solve(Lb, A @ y) / np.sqrt(0.1)
    ref = -0.5 * (n * np.log(2 * np.pi * 0.1) + 2 * np.log(np.diag(Lb)).sum() + y @ y / 0.1 - c @ c) - 0.5 * (n / 0.1 - (A * A).sum())
    assert abs(P.elbo(P.VFE(f(z, jz)), fx, y) - ref) <= 1e-10 * abs(ref)
    g = P.atomic(P.GP(P.SEKernel()), P.GPC())
    members = [(fx, y), (g(x[:200], 0.2), y[:200])]
    own = [P.logpdf_and_gradient(m, v) for m, v in members]
    pooled = P.logpdf_and_gradient_pool([m[0] for m in members], [m[1] for m in members])
    for o, q in zip(own, pooled):
        assert o["logpdf"] == q["logpdf"] and all(np.array_equal(u, v) for u, v in zip(o["_raw"], q["_raw"]))


def test_refusals_name_gibbs():
    n = 16
    Z = {d: points(d, n, d) for d in (1, 2, 17)}
    lib, d, ctx, TP = L.load(), L.dptr, L.default_context(), L.KIND_TIMES_PREV

    def spec_of(terms, dim=2, reserved=0, symmetric=True):
        sp = L.Spec([n], [n], [Z[dim]], {(0, 0): [(k, 0, 0, c, p, None, None) for (k, c, p) in terms]}, symmetric)
        sp._terms[0].reserved = reserved
        return sp

    def refused(rc, what):
        assert rc < 0 and "Gibbs" in L.last_error(), (what, rc, L.last_error())

    K = np.zeros((n, n), order="F")
    km = lambda sp: call(lib.sgp_kernelmatrix, sp, d(K), n)      # noqa: E731
    for param in (0.0, 1.5, float("nan"), -1.0, 17.0, 1e30):
        refused(km(spec_of([(L.GIBBS, 1.0, param)])), param)
    for dim in (1, 17):
        refused(km(spec_of([(L.GIBBS, 1.0, 1.0)], dim=dim)), dim)
    refused(km(spec_of([(L.SE, 1.0, 0.0), (L.GIBBS | TP, 1.0, 1.0)])), "a Gibbs continuation")
    refused(km(spec_of([(L.GIBBS, 1.0, 1.0), (L.SE | TP, 1.0, 0.0)])), "a continuation of a Gibbs term")
    refused(km(spec_of([(L.GIBBS, 1.0, 1.0)], reserved=1)), "reserved != 0")
    spec = spec_of([(L.GIBBS, 1.0, 1.0)])
    assert km(spec) == 0
    m, y, nz, lp, w = np.zeros(n), np.ones(n), np.array([0.1]), np.zeros(1), np.ones(n)
    gy, gm, gn, gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1)
    gx, rsc = np.zeros((2, n), order="F"), np.zeros(n)
    ptrs, scl, nulls = (PD * 1)(d(gx)), (PD * 1)(d(rsc)), (PD * 2)()
    head = (d(m), 0, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc), d(gs))
    assert call(lib.sgp_logpdf_grad_xs, spec, *head, ptrs, None) == 0, L.last_error()
    refused(call(lib.sgp_logpdf_grad_xs, spec, *head, ptrs, scl), "sgp_logpdf_grad_xs with scale outputs")
    refused(call(ctx.kprod.sgp_logpdf_grad_param, spec, *head, d(gp)), "sgp_logpdf_grad_param")
    refused(call(ctx.kprod_grad.sgp_logpdf_grad_param_xs, spec, *head, d(gp), ptrs, nulls), "sgp_logpdf_grad_param_xs")
    refused(call(ctx.conv_grad.sgp_logpdf_grad_conv, spec, *head), "sgp_logpdf_grad_conv")
    refused(call(ctx.stencil_grad.sgp_logpdf_grad_stencil, spec, *head, ptrs), "sgp_logpdf_grad_stencil")
    refused(call(ctx.stencil_wo.sgp_logpdf_grad_stencil_wo, spec, *head, ptrs, nulls, nulls), "sgp_logpdf_grad_stencil_wo")
    refused(call(lib.sgp_kernelmatrix_diag_grad, spec, d(w), d(gc), d(gs)), "sgp_kernelmatrix_diag_grad")
    refused(call(lib.sgp_kernelmatrix_diag_grad_x, spec, d(w), d(gc), d(gs), ptrs), "sgp_kernelmatrix_diag_grad_x")
    K32, f32 = np.zeros((n, n), dtype=np.float32, order="F"), lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    refused(call(lib.sgp_kernelmatrix_f32, spec, f32(K32), n), "sgp_kernelmatrix_f32")
    refused(call(lib.sgp_logpdf_f32, spec, d(m), 0, d(nz), d(y), d(lp)), "sgp_logpdf_f32")
    Zr, o32 = np.zeros((n, 1), order="F"), np.zeros((n, 1), dtype=np.float32, order="F")
    refused(call(lib.sgp_rand_f32, spec, d(m), 0, d(nz), d(Zr), n, 1, f32(o32), n), "sgp_rand_f32")
    cross = spec_of([(L.GIBBS, 1.0, 1.0)], symmetric=False)
    refused(call(lib.sgp_posterior_mean_var_f32, spec, d(m), 0, d(nz), d(y), cross.ref(ctx), spec.ref(ctx), d(m), f32(o32), f32(o32)),
            "sgp_posterior_mean_var_f32")
    refused(call(lib.sgp_elbo_grad, spec, cross.ref(ctx), d(w), d(m), 0, d(nz), 0, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(rsc),
                 d(gp), d(gc), d(gs), d(gc), d(gs)), "sgp_elbo_grad")
    # the prediction gradients against kept factors of the host's making; then the host's own refusals
    gk = P.GibbsKernel(lambda X: 0.5 + 0.0 * X[0])
    f = P.atomic(P.GP(gk), P.GPC())
    xh = np.linspace(-1.0, 1.0, n)
    fx = f(xh, 0.1)
    for post in (P.posterior(fx, y), P.posterior(P.VFE(f(xh[::2], 1e-6)), fx, y)):
        fn = getattr(ctx.predgrad, post._stem + "_predict_grad_x")
        refused(fn(post._ensure(), cross.ref(ctx), spec.ref(ctx), d(m), d(gy), d(gm), None, None, None), post._stem)
    mixed = P.atomic(P.GP(gk + P.RationalQuadraticKernel()), P.GPC())(xh, 0.1)
    for fn in (lambda: P.elbo_and_gradient(P.VFE(f(xh[::2], 1e-6)), fx, y), lambda: P.logpdf_and_gradient(fx, y, scales=True),
               lambda: P.logpdf_and_gradient(mixed, y),
               lambda: P.mean_and_var_and_gradient(P.posterior(fx, y)(xh[:3])), lambda: P.posterior_mean_and_var_f32(fx, y, xh[:3])):
        with pytest.raises(NotImplementedError, match="Gibbs"):
            fn()
