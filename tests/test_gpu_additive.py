"""The additive kinds on the device (csrc/additive.hip; include/sthenomi.h: SGP_ADDITIVE_*) against the formula written directly
in long double (tests/additive_ref.py, which states the bounds of docs/03_kernels.md 3.2h).  Measured on one MI355X, largest
error as a fraction of the bound: see the docstrings.  Every case has N <= 300."""
import ctypes as C
from math import comb

import numpy as np
import pytest

import additive_ref as R
import stheno_jl_amd as P
from stheno_jl_amd import lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]
LD, EPS, TINY = R.LD, R.EPS, R.TINY
PD = C.POINTER(C.c_double)
BASES = [L.SE, L.MATERN12, L.MATERN32, L.MATERN52]


def call(fn, spec, *args):
    ctx = L.default_context()
    return fn(ctx.handle, spec.ref(ctx), *args)


def matrix(spec):
    K = np.zeros((spec.N, spec.M), order="F")
    assert call(L.load().sgp_kernelmatrix, spec, L.dptr(K), spec.N) == 0, L.last_error()
    return K


def check_values(K, base, Zr, Zc, r, coef, rs, cs):
    D = Zr.shape[0]
    z, _, _, x = R.coords(base, Zr, Zc)
    e = R.esp_brute(z, r) if D <= 5 else R.esp(z, r)[r]
    if D == 5:      # the long-double recurrence, which stands in at D = 16, against the brute-force sum
        assert np.all(np.abs(R.esp(z, r)[r] - e) <= 16 * 2.0 ** -64 * e)
    w = (coef * rs)[:, None] * cs[None, :]
    ref = w.astype(LD) * e
    bound = R.units(base, x, r) * EPS * np.abs(ref).astype(np.float64) + TINY * np.abs(w) * comb(D, r)
    frac = np.abs(K - ref).astype(np.float64) / bound
    assert np.all(frac <= 1.0), (float(frac.max()), np.unravel_index(frac.argmax(), frac.shape))
    dead = (x > 800).sum(0)
    assert np.all(K[D - dead < r] == 0.0)
    same = np.all(Zr[:, :, None] == Zc[:, None, :], axis=0)
    assert np.array_equal(K[same], (comb(D, r) * w)[same])
    return float(frac.max()), int((D - dead < r).sum()), int(same.sum())


@pytest.mark.parametrize("D,r", [(1, 1), (3, 1), (3, 2), (3, 3), (5, 1), (5, 2), (5, 5), (16, 1), (16, 2), (16, 8)])
@pytest.mark.parametrize("base", BASES)
def test_values_exact_cases_and_diagonal(base, D, r):
    """MI355X: at most 0.375 of the bound (SE, D = 1, r = 1); 0.37, 0.23 and 0.18 for the Matern bases"""
    kind, worst = L.ADDITIVE_OF[base], 0.0
    for n in (1, 127, 128, 129, 257):
        Z, s = R.points(D, n, 10 * D + n), np.linspace(0.5, 1.5, n)
        spec = L.Spec([n], [n], [Z], {(0, 0): [(kind, 0, 0, -0.75, float(r), s, s)]}, True)
        K = matrix(spec)
        frac, zeros, same = check_values(K, base, Z, Z, r, -0.75, s, s)
        assert n < 8 or (zeros >= 2 * (n - 2) and same >= n + 4)
        diag = np.zeros(n)
        assert call(L.load().sgp_kernelmatrix_diag, spec, L.dptr(diag)) == 0, L.last_error()
        assert np.array_equal(diag, np.diag(K)) and np.array_equal(K, K.T)
        worst = max(worst, frac)
    A, B = R.points(D, 129, 7), R.points(D, 65, 8)
    B[:, 9] = A[:, 128]
    ra, cb = np.linspace(0.5, 1.5, 129), np.linspace(2.0, 1.0, 65)
    K = matrix(L.Spec([129], [65], [A, B], {(0, 0): [(kind, 0, 1, 1.25, float(r), ra, cb)]}, False))
    worst = max(worst, check_values(K, base, A, B, r, 1.25, ra, cb)[0])
    print(f"base {base} D {D} r {r}: largest value error / bound = {worst:.3g}")


def group_coefs(D, Rmax):
    """orders 1 .. Rmax with mixed signs, each scaled to its binomial coefficient so that no order drowns the others"""
    return [(-0.1 if k % 2 == 0 else 1.0 / k) / comb(D, k) for k in range(1, Rmax + 1)]


@pytest.mark.parametrize("Rmax", [2, 4, 8])
def test_group_equals_the_sum_of_its_single_term_matrices(Rmax):
    """one launch group (one recurrence for all orders) against Rmax single-term specs: the group's Rmax fmas, the Rmax
    roundings of the single matrices and the Rmax - 1 of their NumPy sum, in units of the sum of the absolute addends"""
    D, n, base = 9, 130, L.MATERN32
    Z, kind = R.points(D, n, Rmax), L.ADDITIVE_OF[base]
    cf = group_coefs(D, Rmax)
    one = [matrix(L.Spec([n], [n], [Z], {(0, 0): [(kind, 0, 0, c, float(k + 1), None, None)]}, True)) for k, c in enumerate(cf)]
    K = matrix(L.Spec([n], [n], [Z], {(0, 0): [(kind, 0, 0, c, float(k + 1), None, None) for k, c in enumerate(cf)]}, True))
    assert np.all(np.abs(K - sum(one)) <= (3 * Rmax) * EPS * sum(np.abs(m) for m in one))


def grad_x(spec, y, dense_noise):
    """sgp_logpdf_grad_x outputs; Sigma_y as a matrix, whose gradient is the cotangent G itself"""
    n, nt, d = spec.N, spec.n_terms, L.dptr
    out = dict(lp=np.zeros(1), gy=np.zeros(n), gm=np.zeros(n), gn=np.zeros((n, n), order="F"), gc=np.zeros(nt), gs=np.zeros(nt),
               gx=[np.zeros(a.shape, order="F") for a in spec.inputs])
    ptrs = (PD * len(out["gx"]))(*[d(a) for a in out["gx"]])
    rc = call(L.load().sgp_logpdf_grad_x, spec, d(np.zeros(n)), 2, d(np.asfortranarray(dense_noise)), d(y), d(out["lp"]),
              d(out["gy"]), d(out["gm"]), d(out["gn"]), d(out["gc"]), d(out["gs"]), ptrs)
    assert rc == 0, L.last_error()
    return out


@pytest.mark.parametrize("D,Rmax", [(1, 1), (3, 2), (5, 4), (16, 8)])
@pytest.mark.parametrize("base", BASES)
def test_gradients_against_the_long_double_contraction(base, D, Rmax):
    """two blocks of 170 and 130 points: a mirror pair and a tile edge are crossed.  MI355X: at most 0.027 of the bound
    (Matern-1/2, D = 1), which the cotangent's allowance dominates"""
    lens, kind, cf = [170, 130], L.ADDITIVE_OF[base], group_coefs(D, Rmax)
    Zs = [R.points(D, lens[0], D), R.points(D, lens[1], D + 1)]
    n = sum(lens)
    pairs = {(I, J): [(kind, I, J, c, float(k + 1), None, None) for k, c in enumerate(cf)] for I in range(2) for J in range(2)}
    spec = L.Spec(lens, lens, Zs, pairs, True)
    y = np.cos(np.arange(n) * 0.37)
    out, again = grad_x(spec, y, np.eye(n)), grad_x(spec, y, np.eye(n))
    for k in ("gc", "gs", "gn"):
        assert np.array_equal(out[k], again[k])
    assert all(np.array_equal(a, b) for a, b in zip(out["gx"], again["gx"]))
    Z, off = np.hstack(Zs), np.concatenate([[0], np.cumsum(lens)])
    G, aa = out["gn"].astype(LD), np.abs(np.outer(out["gy"], out["gy"]))
    rel = 2 * EPS * 0.5 * (aa + np.abs(aa - 2 * out["gn"])) / np.where(G == 0, 1, np.abs(G))      # of the cotangent the kernels form
    z, kx, u, x = R.coords(base, Z, Z)
    tol = (R.units(base, x, Rmax) + 2 * D + 12) * EPS + rel
    e = R.esp(z, Rmax)
    skip = [R.esp(z, Rmax - 1, skip=d) for d in range(D)]
    worst = 0.0
    for k, c in enumerate(cf):      # grad_coef and grad_inscale, per lower pair and term
        ds = c * G * sum(2 * u[d] * u[d] * kx[d] * skip[d][k] for d in range(D))
        for I, J in ((0, 0), (1, 0), (1, 1)):
            blk, t = np.s_[off[I]:off[I + 1], off[J]:off[J + 1]], Rmax * (2 * I + J) + k
            for got, add in ((out["gc"][t], G * e[k + 1]), (out["gs"][t], ds)):
                err = float((np.abs(add) * tol)[blk].sum()) + TINY
                assert abs(got - add[blk].sum()) <= err, (I, J, k + 1, got, float(add[blk].sum()), err)
                worst = max(worst, float(abs(got - add[blk].sum())) / err)
    # the input points; symmetric spec and cotangent: the row side of every pair, mirror pairs included, covers both roles
    ref, err = np.zeros(Z.shape, dtype=LD), np.zeros(Z.shape, dtype=LD)
    for d in range(D):
        A = sum(c * skip[d][k] for k, c in enumerate(cf))
        A_abs = sum(abs(c) * skip[d][k] for k, c in enumerate(cf))
        ref[d] = (G * A * 2 * kx[d] * u[d]).sum(-1)
        err[d] = (np.abs(G * 2 * kx[d] * u[d]) * A_abs * tol).sum(-1)
    frac = (np.abs(np.hstack(out["gx"]) - 2 * ref) / (2 * err + TINY)).astype(np.float64)
    assert np.all(frac <= 1.0), (float(frac.max()), np.unravel_index(frac.argmax(), frac.shape))
    print(f"base {base} D {D} R {Rmax}: largest gradient error / bound = {max(worst, float(frac.max())):.3g}")


def test_host_level_logpdf_elbo_additive_gp_batch_and_d_transform():
    n, D, v = 300, 3, [0.7, 0.4, 0.2]
    rng = np.random.default_rng(5)
    X, ell = np.asfortranarray(rng.uniform(-1.5, 1.5, (D, n))), np.array([0.6, 0.9, 1.4])
    y = np.sin(3 * X[0]) + 0.3 * X[1] * X[2] + 0.1 * np.cos(17 * X[0])
    k = P.additive_kernel(P.Matern52Kernel(), v) @ P.ARDTransform(1.0 / ell)
    f = P.atomic(P.GP(k), P.GPC())

    def dense(A, B):
        e = R.esp(R.coords(L.MATERN52, A / ell[:, None], B / ell[:, None])[0], 3)
        return sum(c * e[r + 1] for r, c in enumerate(v)).astype(np.float64)

    Lc = np.linalg.cholesky(dense(X, X) + 0.1 * np.eye(n))
    a = np.linalg.solve(Lc.T, np.linalg.solve(Lc, y))
    ref = -0.5 * (y @ a + 2 * np.log(np.diag(Lc)).sum() + n * np.log(2 * np.pi))
    fx = f(P.ColVecs(X), 0.1)
    assert abs(P.logpdf(fx, y) - ref) <= 1e-10 * abs(ref)
    Xz, jz = np.asfortranarray(X[:, 7::30]), 1e-6      # 10 inducing points, a proper subset: the rectangular block matters
    Lz = np.linalg.cholesky(dense(Xz, Xz) + jz * np.eye(10))
    A = np.linalg.solve(Lz, dense(Xz, X)) / np.sqrt(0.1)
    Lb = np.linalg.cholesky(np.eye(10) + A @ A.T)
    c = np.linalg.solve(Lb, A @ y) / np.sqrt(0.1)
    kxx = np.diag(dense(X, X))
    want = -0.5 * (n * np.log(2 * np.pi * 0.1) + 2 * np.log(np.diag(Lb)).sum() + y @ y / 0.1 - c @ c) - 0.5 * (kxx.sum() / 0.1 - (A * A).sum())
    assert abs(P.elbo(P.VFE(f(P.ColVecs(Xz), jz)), fx, y) - want) <= 1e-10 * abs(want)
    # order 1 with SE is the additive_gp model of D select views
    gpc = P.GPC()
    parts = [P.atomic(P.GP(0.8 * P.SEKernel()), gpc) for _ in range(D)]
    g, h = P.additive_gp(parts), P.atomic(P.GP(P.additive_kernel(P.SEKernel(), [0.8])), P.GPC())
    assert np.max(np.abs(P.prior_cov(g, P.ColVecs(X)) - P.prior_cov(h, P.ColVecs(X)))) <= 1e-10
    # d_transform of the ARDTransform against the long-double contraction: d K / d a_d = sum_t c_t e_{r_t - 1}(z without d)
    # 2 kappa' u_d (x_d - y_d) with u the scaled difference; G from logpdf's own gradient with respect to dense noise
    rec = P.logpdf_and_gradient(fx, y, inputs=True)
    Kinv = np.linalg.inv((dense(X, X) + 0.1 * np.eye(n)).astype(LD).astype(np.float64))
    G = 0.5 * (np.outer(a, a) - Kinv)
    z, kx, u, _ = R.coords(L.MATERN52, X / ell[:, None], X / ell[:, None])
    dX = X[:, :, None] - X[:, None, :]
    want = np.array([float((G * sum(c * R.esp(z, 2, skip=d)[r] for r, c in enumerate(v)) * 2 * kx[d] * u[d] * dX[d]).sum())
                     for d in range(D)])
    got = rec["terms"][0]["d_transform"]
    assert np.max(np.abs(got - want)) <= 1e-8 * np.max(np.abs(want))
    own = [P.logpdf_and_gradient(fx, y), P.logpdf_and_gradient(h(P.ColVecs(X), 0.2), y)]
    both = P.logpdf_and_gradient_batch([fx, h(P.ColVecs(X), 0.2)], [y, y])
    for o, q in zip(own, both):
        assert o["logpdf"] == q["logpdf"] and all(np.array_equal(s, t) for s, t in zip(o["_raw"], q["_raw"]))


def test_refusals_name_additive():
    n, TP = 16, L.KIND_TIMES_PREV
    Z = {d: R.points(d, n, d) for d in (2, 9, 17)}
    lib, d, ctx, AD = L.load(), L.dptr, L.default_context(), L.ADDITIVE_SE

    def spec_of(terms, dim=2, reserved=0, symmetric=True):
        sp = L.Spec([n], [n], [Z[dim]], {(0, 0): [(k, 0, 0, c, p, None, None) for (k, c, p) in terms]}, symmetric)
        sp._terms[0].reserved = reserved
        return sp

    def refused(rc, what):
        assert rc < 0 and "additive" in L.last_error(), (what, rc, L.last_error())

    K = np.zeros((n, n), order="F")
    km = lambda sp: call(lib.sgp_kernelmatrix, sp, d(K), n)      # noqa: E731
    for param in (0.0, 1.5, float("nan"), -1.0, 3.0, 1e30):
        refused(km(spec_of([(AD, 1.0, param)])), param)
    refused(km(spec_of([(AD, 1.0, 9.0)], dim=9)), "order 9")
    refused(km(spec_of([(AD, 1.0, 1.0)], dim=17)), "dimension 17")
    refused(km(spec_of([(L.SE, 1.0, 0.0), (AD | TP, 1.0, 1.0)])), "an additive continuation")
    refused(km(spec_of([(AD, 1.0, 1.0), (L.SE | TP, 1.0, 0.0)])), "a continuation of an additive term")
    refused(km(spec_of([(AD, 1.0, 1.0)], reserved=1)), "reserved != 0")
    for code in range(41, 48):
        assert km(spec_of([(code, 1.0, 1.0)])) < 0 and "unknown kernel kind" in L.last_error()
    spec = spec_of([(AD, 1.0, 2.0)])
    assert km(spec) == 0
    m, y, nz, lp, w = np.zeros(n), np.ones(n), np.array([0.1]), np.zeros(1), np.ones(n)
    gy, gm, gn, gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1)
    gx, rsc = np.zeros((2, n), order="F"), np.zeros(n)
    ptrs, scl, nulls = (PD * 1)(d(gx)), (PD * 1)(d(rsc)), (PD * 2)()
    head = (d(m), 0, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc), d(gs))
    assert call(lib.sgp_logpdf_grad_xs, spec, *head, ptrs, None) == 0, L.last_error()
    K32, f32 = np.zeros((n, n), dtype=np.float32, order="F"), lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    Zr, o32 = np.zeros((n, 1), order="F"), np.zeros((n, 1), dtype=np.float32, order="F")
    cross = spec_of([(AD, 1.0, 2.0)], symmetric=False)
    for what, rc in (
            ("sgp_logpdf_grad_xs with scale outputs", lambda: call(lib.sgp_logpdf_grad_xs, spec, *head, ptrs, scl)),
            ("sgp_logpdf_grad_param", lambda: call(ctx.kprod.sgp_logpdf_grad_param, spec, *head, d(gp))),
            ("sgp_logpdf_grad_param_xs", lambda: call(ctx.kprod_grad.sgp_logpdf_grad_param_xs, spec, *head, d(gp), ptrs, nulls)),
            ("sgp_logpdf_grad_conv", lambda: call(ctx.conv_grad.sgp_logpdf_grad_conv, spec, *head)),
            ("sgp_logpdf_grad_stencil", lambda: call(ctx.stencil_grad.sgp_logpdf_grad_stencil, spec, *head, ptrs)),
            ("sgp_logpdf_grad_stencil_wo", lambda: call(ctx.stencil_wo.sgp_logpdf_grad_stencil_wo, spec, *head, ptrs, nulls, nulls)),
            ("sgp_kernelmatrix_diag_grad", lambda: call(lib.sgp_kernelmatrix_diag_grad, spec, d(w), d(gc), d(gs))),
            ("sgp_kernelmatrix_diag_grad_x", lambda: call(lib.sgp_kernelmatrix_diag_grad_x, spec, d(w), d(gc), d(gs), ptrs)),
            ("sgp_kernelmatrix_f32", lambda: call(lib.sgp_kernelmatrix_f32, spec, f32(K32), n)),
            ("sgp_logpdf_f32", lambda: call(lib.sgp_logpdf_f32, spec, d(m), 0, d(nz), d(y), d(lp))),
            ("sgp_rand_f32", lambda: call(lib.sgp_rand_f32, spec, d(m), 0, d(nz), d(Zr), n, 1, f32(o32), n)),
            ("sgp_posterior_mean_var_f32", lambda: call(lib.sgp_posterior_mean_var_f32, spec, d(m), 0, d(nz), d(y), cross.ref(ctx),
                                                        spec.ref(ctx), d(m), f32(o32), f32(o32))),
            ("sgp_elbo_grad", lambda: call(lib.sgp_elbo_grad, spec, cross.ref(ctx), d(w), d(m), 0, d(nz), 0, d(nz), d(y), d(lp), d(gy),
                                           d(gm), d(gn), d(rsc), d(gp), d(gc), d(gs), d(gc), d(gs)))):
        refused(rc(), what)
    # the prediction gradients against kept factors of the host's making; then the host's own refusals
    ak = P.AdditiveKernel(P.SEKernel(), 2)
    f = P.atomic(P.GP(ak), P.GPC())
    xh = P.ColVecs(Z[2])
    fx = f(xh, 0.1)
    for post in (P.posterior(fx, y), P.posterior(P.VFE(f(P.ColVecs(Z[2][:, ::2]), 1e-6)), fx, y)):
        fn = getattr(ctx.predgrad, post._stem + "_predict_grad_x")
        refused(fn(post._ensure(), cross.ref(ctx), spec.ref(ctx), d(m), d(gy), d(gm), None, None, None), post._stem)
    mixed = P.atomic(P.GP(ak + P.RationalQuadraticKernel()), P.GPC())(xh, 0.1)
    for fn in (lambda: P.elbo_and_gradient(P.VFE(f(P.ColVecs(Z[2][:, ::2]), 1e-6)), fx, y),
               lambda: P.logpdf_and_gradient(fx, y, scales=True), lambda: P.logpdf_and_gradient(mixed, y),
               lambda: P.mean_and_var_and_gradient(P.posterior(fx, y)(P.ColVecs(Z[2][:, :3]))),
               lambda: P.posterior_mean_and_var_f32(fx, y, P.ColVecs(Z[2][:, :3]))):
        with pytest.raises(NotImplementedError, match="additive"):
            fn()
