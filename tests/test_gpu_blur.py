"""The blur kind on the device (csrc/blur.hip; include/sthenomi.h: SGP_BLUR_SE).  Values against the formula in 60 digits
(mpmath, on a sub-grid of the matrix) and in long double (every entry; its own error, about D 2^-64, is far below the bound):
an entry is right to U = x (D + 3) + D + 8 units of 2^-53 of itself (docs/03_kernels.md, 3.2i; x = 1/2 sum_d u_d^2 / q_d).
Gradients of the host's logpdf_and_gradient against tests/grad_truth.py in long double (ops: tests/blur_np.py), inside its
margin: MARGIN x max(the float64 runs' figure, the family's floor).  The model: f at 70 points, blur(f, s) at 130 -- the SE
path, the one-sided and the two-sided mode, two tile rows of which one is clipped."""
import ctypes as C
import functools

import mpmath
import numpy as np
import pytest

import blur_np
import grad_truth as T
import stheno_jl_amd as P
import test_gpu_grad_truth as GT
from stheno_jl_amd import lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]
LD, EPS, TINY = np.longdouble, 2.0 ** -53, 2.0 ** -1070
PD = C.POINTER(C.c_double)
DIMS = [1, 3, 8]


@functools.lru_cache(maxsize=None)
def points(D):
    """Z: the 2 D x 200 points of the two blocks as the terms read them (zero variances for the 70 of f)"""
    rng = np.random.default_rng(D)
    X1, X2 = rng.uniform(-1.0, 1.0, (D, 70)), rng.uniform(-1.0, 1.0, (D, 130))
    S2 = rng.uniform(0.05, 2.0, (D, 130))
    X2[:, 0], S2[:, 0] = X1[:, 0], 0.0                     # coincident with a point of f, no footprint: exactly the weight
    X2[:, 1], S2[:, 1] = X2[:, 129], S2[:, 129]            # coincident across a tile edge
    X1[:, 5], X2[:, 7] = 300.0, -300.0                     # far points: the exponential underflows
    S2[:, 9] = 0.0
    return np.asfortranarray(np.hstack([np.vstack([X1, 0 * X1]), np.vstack([X2, S2])]))


def call(fn, spec, *args):
    ctx = L.default_context()
    return fn(ctx.handle, spec.ref(ctx), *args)


def matrix(spec):
    K = np.zeros((spec.N, spec.M), order="F")
    assert call(L.load().sgp_kernelmatrix, spec, L.dptr(K), spec.N) == 0, L.last_error()
    return K


def one_pair(kind, Zr, Zc=None, coef=0.7):
    pairs = {(0, 0): [(kind, 0, 0 if Zc is None else 1, coef, 0.0, None, None)]}
    return L.Spec([Zr.shape[1]], [(Zr if Zc is None else Zc).shape[1]], [Zr] if Zc is None else [Zr, Zc], pairs, Zc is None)


@pytest.mark.parametrize("D", DIMS)
def test_values_and_exact_cases(D):
    Z = points(D)
    f = P.atomic(P.GP(0.7 * P.SEKernel()), P.GPC())
    x1, x2 = (P.ColVecs(np.asfortranarray(Z[:D, sl])) for sl in (slice(0, 70), slice(70, 200)))
    spec, _, _ = P.build_spec(P.cross([f, P.blur(f, lambda X: Z[D:, 70:])]), P.BlockData([x1, x2]))
    assert [int(spec._terms[spec._term_ptr[p]].kind) for p in range(4)] == [L.SE, L.BLUR_SE, L.BLUR_SE, L.BLUR_SE]
    K = matrix(spec)
    u, w, _, k = blur_np.pair(Z, Z, LD)
    x = ((u * u * w).sum(0) / 2).astype(np.float64)
    U = x * (D + 3) + D + 8
    frac = np.abs(K - LD(0.7) * k).astype(np.float64) / (U * EPS * 0.7 * np.abs(k).astype(np.float64) + TINY)
    assert np.all(frac <= 1.0), (float(frac.max()), np.unravel_index(frac.argmax(), frac.shape))
    mpmath.mp.dps = 60
    for i in range(0, 200, 7):                              # 60 digits on a sub-grid that meets every block pair
        for j in range(0, 200, 5):
            q = [1 + mpmath.mpf(Z[D + d, i]) + mpmath.mpf(Z[D + d, j]) for d in range(D)]
            t = sum((mpmath.mpf(Z[d, i]) - mpmath.mpf(Z[d, j])) ** 2 / q[d] for d in range(D))
            ref = mpmath.mpf(0.7) * mpmath.exp(-t / 2) / mpmath.sqrt(mpmath.fprod(q))
            assert abs(mpmath.mpf(K[i, j]) - ref) <= float(U[i, j]) * EPS * abs(ref) + TINY, (i, j)
    assert np.all(K[x > 800] == 0.0) and (x > 800).sum() >= 2 * 198
    same = np.all(Z[:, :, None] == Z[:, None, :], axis=0) & np.all(Z[D:] == 0, axis=0)[:, None]
    assert same.sum() >= 70 + 4 and np.all(K[same] == 0.7)
    diag = np.zeros(200)
    assert call(L.load().sgp_kernelmatrix_diag, spec, L.dptr(diag)) == 0, L.last_error()
    assert np.array_equal(diag, np.diag(K)) and np.array_equal(K, K.T)
    # zero variances on both sides: the bits of the SE kind on the location rows
    Z1 = np.asfortranarray(Z[:, :70])
    assert np.array_equal(matrix(one_pair(L.BLUR_SE, Z1)), matrix(one_pair(L.SE, np.asfortranarray(Z1[:D]))))
    # the one-sided mode against the two-sided one: a single column with a footprint changes that column alone
    Z2, Z1b = np.asfortranarray(Z[:, 70:]), Z1.copy(order="F")
    Z1b[D:, 33] = 0.25
    one, two = matrix(one_pair(L.BLUR_SE, Z2, Z1)), matrix(one_pair(L.BLUR_SE, Z2, Z1b))
    keep = np.arange(70) != 33
    assert np.array_equal(one[:, keep], two[:, keep]) and not np.array_equal(one[:, 33], two[:, 33])
    assert np.array_equal(one, K[70:, :70]) and np.array_equal(matrix(one_pair(L.BLUR_SE, Z1, Z2)), one.T)
    print(f"D {D}: largest value error / bound = {float(frac.max()):.3g}")


def test_the_reference_integral_figures():
    m = P.gppp(lambda GP: (lambda f: dict(f=f, v=P.blur(f, 1.0)))(GP(P.SEKernel())))
    K = P.prior_cov(m, P.BlockData([P.GPPPInput("v", np.zeros(1)), P.GPPPInput("f", np.zeros(1))]))
    assert abs(K[0, 0] - 1 / np.sqrt(3)) <= 4 * EPS and abs(K[0, 1] - 1 / np.sqrt(2)) <= 4 * EPS
    post = P.posterior(m(P.GPPPInput("v", np.zeros(1)), 1e-9), np.ones(1))
    t, w = np.polynomial.hermite.hermgauss(40)
    assert abs((w / np.sqrt(np.pi)) @ P.mean(post(P.GPPPInput("f", np.sqrt(2.0) * t))) - 1.0) <= 1e-6


@pytest.mark.parametrize("D", DIMS)
def test_logpdf_elbo_and_host_gradients_against_grad_truth(D):
    """f = SE o Select(perm) o Stretch(diag a) under the node: the kernel reads (a x)[perm] and (a^2 s)[perm], so the host's
    chain back to the user's points and to the node's variances carries a, a^2 and the scatter of perm"""
    Z = np.delete(points(D), [5, 77], axis=1)                            # without the far points: 69 + 129
    X, s, n = Z[:D], Z[D:, 69:], 198
    a, perm = np.linspace(0.8, 1.3, D), np.roll(np.arange(D), 1)
    var = lambda Xn: s if Xn.shape[1] == 129 else s[:, ::13]             # noqa: E731
    fg = P.gppp(lambda GP: (lambda h: dict(f=h, g=P.blur(h, var)))(
        P.compose(P.compose(GP(0.7 * P.SEKernel()), P.Select(perm)), P.Stretch(np.diag(a)))))
    xs = [P.ColVecs(np.asfortranarray(X[:, :69])), P.ColVecs(np.asfortranarray(X[:, 69:]))]
    fx = fg(P.BlockData([P.GPPPInput("f", xs[0]), P.GPPPInput("g", xs[1])]), 0.1)
    y = np.cos(np.arange(n) * 0.37)
    g = P.logpdf_and_gradient(fx, y, inputs=True)
    S = T.read_spec(g["_spec"])
    R, *R64 = (T.logpdf_grad(S, T.NOISE_SCALAR, 0.1, P.mean(fx), y, dt, inputs=True, cholesky=ch, ops=blur_np)
               for dt, ch in ((T.require_extended(), None), (np.float64, None), (np.float64, T.cholesky_blocked_order)))
    assert abs(P.logpdf(fx, y) - R["value"]) <= 1e-10 * abs(R["value"])
    # the ELBO with 10 blurred inducing points, from the same long-double matrix
    K = blur_np.dense(S, LD)
    K, zi, I, yl = np.tril(K) + np.tril(K, -1).T, np.arange(69, n, 13), np.eye(10, dtype=LD), y.astype(LD)
    A = T.tri_inverse(T.cholesky(K[np.ix_(zi, zi)] + LD(1e-6) * I)) @ K[zi] / np.sqrt(LD(0.1))
    Lb = T.cholesky(I + A @ A.T)
    c = T.tri_inverse(Lb) @ (A @ yl) / np.sqrt(LD(0.1))
    ref = -(n * np.log(2 * np.pi * LD(0.1)) + 2 * np.log(np.diag(Lb)).sum() + yl @ yl / LD(0.1) - c @ c
            + np.diag(K).sum() / LD(0.1) - (A * A).sum()) / 2
    fz = fg(P.GPPPInput("g", P.ColVecs(np.asfortranarray(X[:, 69::13]))), 1e-6)
    assert abs(P.elbo(P.VFE(fz), fx, y) - ref) <= 1e-10 * abs(ref)
    # every output family of the library inside grad_truth's margin
    dev = GT.logpdf_units(GT._logpdf_outputs(g), R)
    e64 = [GT.logpdf_units(GT._reference_outputs(r), R) for r in R64]
    bound = {fam: T.MARGIN * max(max(e[fam] for e in e64), T.FLOORS[fam]) for fam in dev}
    print(f"D {D}:", {fam: (round(dev[fam], 1), round(bound[fam], 1)) for fam in dev})
    assert all(dev[fam] <= bound[fam] for fam in dev)

    def back(rows, fac):                                                 # kernel coordinates -> the user's / the node's
        out = np.zeros(rows.shape, dtype=rows.dtype)
        out[perm] = fac[perm][:, None] * rows
        return out
    origin = g["_spec"].input_origin
    for b in range(2):                                                   # `x`: the location rows of every view of block b
        views = [k for k in range(len(origin)) if origin[k][1] == b]
        want, Sn = (sum(back(R[key][k][:D], a) for k in views) for key in ("gx", "Sn_gx"))
        assert T.units(g["x"][b], want, T.scale_entries(want, Sn)) <= bound["lp.inputs"]
    blurred = [r for r in g["terms"] if r["kind"] == L.BLUR_SE]
    assert [(r["I"], r["J"], r["d_variance"][1] is None) for r in blurred] == [(1, 0, True), (1, 1, False)]      # the lower pairs
    for r in blurred:
        for side, k in zip(r["d_variance"], (r["row_input"], r["col_input"])):
            if side is not None:
                want, Sn = back(R["gx"][k][D:], a * a), back(R["Sn_gx"][k][D:], a * a)
                assert side.shape == (D, 129) and T.units(side, want, T.scale_entries(want, Sn)) <= bound["lp.inputs"]


def test_refusals_name_blur_and_codes_52_to_55_are_unknown():
    n, lib, d, ctx, TP = 16, L.load(), L.dptr, L.default_context(), L.KIND_TIMES_PREV
    Z = {dim: np.asfortranarray(np.random.default_rng(dim).uniform(0.1, 1.0, (dim, n))) for dim in (2, 3, 18)}
    K = np.zeros((n, n), order="F")

    def spec_of(terms, dim=2, reserved=0, symmetric=True, Zin=None):
        sp = L.Spec([n], [n], [Z[dim] if Zin is None else Zin], {(0, 0): [(k, 0, 0, 1.0, 0.0, None, None) for k in terms]}, symmetric)
        sp._terms[0].reserved = reserved
        return sp

    def refused(rc, what, word="blur"):
        assert rc < 0 and word in L.last_error(), (what, rc, L.last_error())

    km = lambda sp: call(lib.sgp_kernelmatrix, sp, d(K), n)      # noqa: E731
    for code in (52, 53, 54, 55):
        refused(km(spec_of([code])), code, "unknown kernel kind")
    bad = [Z[2].copy(order="F") for _ in range(3)]
    for Zb, v in zip(bad, (-1e-300, float("nan"), float("inf"))):
        Zb[1, 11] = v
    for sp in ([spec_of([L.BLUR_SE], dim=3), spec_of([L.BLUR_SE], dim=18), spec_of([L.SE, L.BLUR_SE | TP]),
                spec_of([L.BLUR_SE, L.SE | TP]), spec_of([L.BLUR_SE], reserved=1)] + [spec_of([L.BLUR_SE], Zin=Zb) for Zb in bad]):
        refused(km(sp), sp)
    spec, cross = spec_of([L.BLUR_SE]), spec_of([L.BLUR_SE], symmetric=False)
    assert km(spec) == 0
    m, y, nz, lp, w = np.zeros(n), np.ones(n), np.array([0.1]), np.zeros(1), np.ones(n)
    gy, gm, gn, gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1)
    gx, rsc = np.zeros((2, n), order="F"), np.zeros(n)
    ptrs, scl, nulls = (PD * 1)(d(gx)), (PD * 1)(d(rsc)), (PD * 2)()
    head = (d(m), 0, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc), d(gs))
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    K32, o32, Zr = np.zeros((n, n), dtype=np.float32, order="F"), np.zeros((n, 1), dtype=np.float32, order="F"), np.zeros((n, 1), order="F")
    assert call(lib.sgp_logpdf_grad_xs, spec, *head, ptrs, None) == 0, L.last_error()
    for where, name, args in [
            (lib, "sgp_logpdf_grad_xs", head + (ptrs, scl)), (ctx.kprod, "sgp_logpdf_grad_param", head + (d(gp),)),
            (ctx.kprod_grad, "sgp_logpdf_grad_param_xs", head + (d(gp), ptrs, nulls)), (ctx.conv_grad, "sgp_logpdf_grad_conv", head),
            (ctx.stencil_grad, "sgp_logpdf_grad_stencil", head + (ptrs,)),
            (ctx.stencil_wo, "sgp_logpdf_grad_stencil_wo", head + (ptrs, nulls, nulls)),
            (lib, "sgp_kernelmatrix_diag_grad", (d(w), d(gc), d(gs))), (lib, "sgp_kernelmatrix_diag_grad_x", (d(w), d(gc), d(gs), ptrs)),
            (lib, "sgp_kernelmatrix_f32", (f32(K32), n)), (lib, "sgp_logpdf_f32", (d(m), 0, d(nz), d(y), d(lp))),
            (lib, "sgp_rand_f32", (d(m), 0, d(nz), d(Zr), n, 1, f32(o32), n)),
            (lib, "sgp_posterior_mean_var_f32", (d(m), 0, d(nz), d(y), cross.ref(ctx), spec.ref(ctx), d(m), f32(o32), f32(o32))),
            (lib, "sgp_elbo_grad", (cross.ref(ctx), d(w), d(m), 0, d(nz), 0, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(rsc), d(gp),
                                    d(gc), d(gs), d(gc), d(gs)))]:
        refused(call(getattr(where, name), spec, *args), name)
    g = P.blur(P.atomic(P.GP(P.SEKernel()), P.GPC()), 0.3)      # the prediction gradients against kept factors of the host's making
    xh = np.linspace(-1.0, 1.0, n)
    fx = g(xh, 0.1)
    for post in (P.posterior(fx, y), P.posterior(P.VFE(g(xh[::2], 1e-6)), fx, y)):
        fn = getattr(ctx.predgrad, post._stem + "_predict_grad_x")
        refused(fn(post._ensure(), cross.ref(ctx), spec.ref(ctx), d(m), d(gy), d(gm), None, None, None), post._stem)
