"""The derivative kinds on the device (csrc/deriv.hip; include/sthenomi.h: SGP_DERIV_*): values against the 80-digit table
(tests/deriv_truth.py) within its first-order bounds, the exact coincident and overflow values, var == diag(cov) and
cov(f, df) == cov(df, f)' bit for bit across tile edges and with coincident pairs off the diagonal, positive definiteness of
the joint matrix, the reference example's own known-answer check with its own tolerances, an antiderivative model against
the long-double truth of the same model, gradients inside MARGIN x max(e_float64, floor) of the extended-precision truth
(tests/deriv_grad_truth.py) with bit-reproducibility, the input-scale coefficients against the table on the device, pool members, and every refusal of the boundary by name.  Every case has N <= 300."""
import ctypes as C

import numpy as np
import pytest

import deriv_grad_truth as GT
import deriv_np as dn
import deriv_truth as dt
import stheno_jl_amd as P
from stheno_jl_amd import lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]

BASES = {"se": (L.DERIV_SE, P.SEKernel), "m32": (L.DERIV_MATERN32, P.Matern32Kernel), "m52": (L.DERIV_MATERN52, P.Matern52Kernel)}
EPS = 2.0 ** -53
PD = C.POINTER(C.c_double)


def _call(fn, spec, *args):
    ctx = L.default_context()
    return fn(ctx.handle, spec.ref(ctx), *args)


def _cross_spec(terms, X, Y):
    """one block pair between the columns of X and of Y; terms: (kind, coef, param)"""
    return L.Spec([X.shape[1]], [Y.shape[1]], [np.asfortranarray(X), np.asfortranarray(Y)],
                  {(0, 0): [(k, 0, 1, c, p, None, None) for (k, c, p) in terms]}, False)


def _matrix(spec):
    K = np.zeros((spec.N, spec.M), order="F")
    assert _call(L.load().sgp_kernelmatrix, spec, L.dptr(K), spec.N) == 0, L.last_error()
    return K


# ---- 1. values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", sorted(BASES))
def test_values_match_the_table_within_its_bounds(base):
    kind = BASES[base][0]
    worst = 0.0
    for D, G in dt.load()[base].items():
        for ab, rec in G["terms"].items():
            a, b = ab
            K = _matrix(_cross_spec([(kind, 1.0, float(17 * a + b))], G["X"], G["Y"]))
            got = np.diag(K)
            err, bound = np.abs(got - rec["value"]), dt.value_bound(base, D, G, rec)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (base, D, ab, got, rec["value"], bound)
            assert np.all(got[rec["must_zero"]] == 0.0), (base, D, ab, "exact zeros at coincident / far / overflowed pairs")
            ex = rec["exact"]
            assert np.all(got[ex[:, 0].astype(int)] == ex[:, 1]), (base, D, ab, "the exact coincident values")
    print(f"{base}: largest value error / bound = {worst:.3g}")


def _gradient_observation_blocks(D=3, sizes=(37, 29, 64), seed=3):
    """(f: 37, d0 f: 29, d2 f: 64) with points shared between blocks (coincident pairs off the diagonal) and inside one"""
    rng = np.random.default_rng(seed)
    Xs = [np.asfortranarray(rng.standard_normal((D, n)) * 0.7) for n in sizes]
    Xs[1][:, :9] = Xs[0][:, 4:13]
    Xs[2][:, 5:25] = Xs[1][:, 3:23]
    Xs[2][:, 40] = Xs[2][:, 41]
    return Xs


def _joint_model(kernel, dims):
    gpc = P.GPC()
    f = P.atomic(P.GP(kernel), gpc)
    return P.cross([f] + [P.derivative(f, d) for d in dims])


@pytest.mark.parametrize("base", sorted(BASES))
def test_var_is_diag_cov_and_cross_blocks_transpose_bit_for_bit(base):
    Xs = _gradient_observation_blocks()
    F = _joint_model(P.with_lengthscale(BASES[base][1](), 1.5), (0, 2))
    x = P.BlockData([P.ColVecs(X) for X in Xs])
    K = P.cov(F(x))
    assert np.array_equal(P.var(F(x)), np.diag(K))
    assert np.array_equal(K, K.T)
    spec, _, _ = P.build_spec(F, x)
    ref = dn.dense_from_spec(spec)
    assert np.max(np.abs(K - ref)) <= 64 * EPS * np.max(np.abs(ref))
    # coincident pairs off the diagonal: cov(f(x), d0 f(x)) is exactly 0, cov(d0 f(x), d2 f(x)) is exactly 0 (p != q)
    assert np.all(np.diag(K[37:37 + 9, 4:13]) == 0.0)
    assert np.all(np.diag(K[37 + 29 + 5:37 + 29 + 25, 37 + 3:37 + 23]) == 0.0)
    # ... and not across a tile edge only by luck: rows 130, columns 70 of a rectangular cross-covariance, both orders
    rng = np.random.default_rng(5)
    A, B = np.asfortranarray(rng.standard_normal((3, 130))), np.asfortranarray(rng.standard_normal((3, 70)))
    B[:, 7] = A[:, 129]
    gpc = P.GPC()
    f = P.atomic(P.GP(BASES[base][1]()), gpc)
    df = P.derivative(f, 1)
    K_fd = P.cov(f(P.ColVecs(A)), df(P.ColVecs(B)))
    K_df = P.cov(df(P.ColVecs(B)), f(P.ColVecs(A)))
    assert K_fd.shape == (130, 70) and np.array_equal(K_fd, K_df.T)
    assert K_fd[129, 7] == 0.0
    K_dd = P.cov(df(P.ColVecs(A)), df(P.ColVecs(B)))
    assert K_dd[129, 7] == {"se": 1.0, "m32": 3.0, "m52": 5.0 / 3.0}[base]
    sp, _, _ = P.build_spec(df, P.ColVecs(A), df, P.ColVecs(B))
    ref = dn.dense_from_spec(sp)
    assert np.max(np.abs(K_dd - ref)) <= 64 * EPS * np.max(np.abs(ref))


# ---- 2. positive definiteness ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", sorted(BASES))
def test_joint_matrix_of_f_and_its_gradient_is_positive_definite(base):
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(10.0), np.arange(6.0), indexing="ij")).reshape(2, -1)      # 60 well-separated points
    X = np.asfortranarray(g * 0.9 + rng.uniform(-0.1, 0.1, g.shape))
    F = _joint_model(BASES[base][1](), (0, 1))
    x = P.BlockData([P.ColVecs(X)] * 3)
    spec, _, _ = P.build_spec(F, x)
    # first, on the CPU: the evaluator's matrix factors in long double with every pivot well above rounding
    Kl = dn.dense_from_spec(spec).astype(np.longdouble) + np.longdouble(0.1) * np.eye(180, dtype=np.longdouble)
    piv = dt.cholesky_ld(Kl)
    assert piv is not None and np.min(np.diag(piv)) ** 2 > 0.05
    y = np.sin(np.arange(180.0))
    lp = P.logpdf(F(x, 0.1), y)          # raises PosDefException on info != 0
    z = dt.solve_lower_ld(piv, y.astype(np.longdouble))
    ref = float(-0.5 * (180 * np.log(2 * np.longdouble(np.pi)) + 2 * np.sum(np.log(np.diag(piv))) + z @ z))
    assert abs(lp - ref) <= 1e-10 * abs(ref)


# ---- 3. the reference example's own check (examples/differentiation/script.jl:120-134), its own tolerances ------------------
def _approx(a, b, rtol):
    """Julia's isapprox for vectors: norm(a - b) <= rtol max(norm(a), norm(b))"""
    return np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(a), np.linalg.norm(b))


@pytest.mark.parametrize("fn, dfn", [(np.sin, np.cos), (np.cos, lambda t: -np.sin(t))], ids=["sin", "cos"])
def test_posterior_derivative_of_trigonometric_observations(fn, dfn):
    model = P.gppp(lambda GP: (lambda f: dict(f=f, df=P.derivative(f)))(GP(P.SEKernel())))
    x_obs, x_pred = np.linspace(-3.0, 3.0, 25), np.linspace(-2.5, 2.5, 25)
    post = P.posterior(model(P.GPPPInput("f", x_obs), 1e-12), fn(x_obs))
    xd = P.GPPPInput("df", x_pred)
    assert _approx(dfn(x_pred), P.mean(post(xd)), 1e-5)
    assert _approx(dfn(x_pred), np.ravel(P.rand(np.random.default_rng(123456), post(xd, 1e-8))), 1e-3)


# ---- 4. antiderivative model ------------------------------------------------------------------------------------------------
def test_antiderivative_model_matches_its_long_double_truth():
    model = P.gppp(lambda GP: (lambda F: dict(F=F, f=P.derivative(F)))(GP(P.SEKernel())))
    xs = np.linspace(-5.0, 5.0, 20)
    x_obs = P.BlockData([P.GPPPInput("F", np.array([-5.1])), P.GPPPInput("f", xs)])
    y = np.r_[0.0, np.sin(xs)]
    noise = 1e-6
    xt = P.GPPPInput("F", np.linspace(-4.5, 4.5, 33))
    got = P.mean(P.posterior(model(x_obs, noise), y)(xt))
    # the same model in long double: the evaluator's own matrices (exact inputs), a long-double Cholesky
    spec, _, _ = P.build_spec(model, x_obs)
    cross, _, _ = P.build_spec(model, xt, model, x_obs)
    Kl = dn.dense_from_spec(spec).astype(np.longdouble) + np.longdouble(noise) * np.eye(21, dtype=np.longdouble)
    Lc = dt.cholesky_ld(Kl)
    alpha = dt.solve_upper_ld(Lc.T, dt.solve_lower_ld(Lc, y.astype(np.longdouble)))
    ref = (dn.dense_from_spec(cross).astype(np.longdouble) @ alpha).astype(np.float64)
    # conditioning: the float64 matrix entries carry ~8 eps; through the solve they grow by at most cond(K + noise I)
    cond = float(np.linalg.cond(Kl.astype(np.float64)))
    tol = 64 * EPS * cond * np.max(np.abs(ref))
    assert np.max(np.abs(got - ref)) <= tol, (float(np.max(np.abs(got - ref))), tol)
    assert np.max(np.abs(ref - (np.cos(-5.1) - np.cos(xt.x)))) < 0.05      # (and it is the antiderivative: a sanity line)


# ---- 5. gradients -----------------------------------------------------------------------------------------------------------
def _outputs(g):
    gc, gs = g["_raw"]
    nt = g["_spec"].n_terms
    return dict(value=g["logpdf"], y=g["y"], mean=g["mean"], noise=g["noise"], d_coef=gc[:nt], d_inscale=gs[:nt])


@pytest.mark.parametrize("name", GT.CASES)
def test_gradient_against_the_extended_precision_truth_and_repeats_bit_for_bit(name):
    """every output family of sgp_logpdf_grad inside MARGIN x max(e_float64 of the case, floor) of the long-double truth
    (tests/deriv_grad_truth.py: the project's method, on top of tests/grad_truth.py); two calls give the same bits"""
    fx, y = GT.build_case(name, P)
    g1 = P.logpdf_and_gradient(fx, y)
    g2 = P.logpdf_and_gradient(fx, y)
    for a, b in zip(g1["_raw"], g2["_raw"]):
        assert np.array_equal(a, b)
    assert g1["logpdf"] == g2["logpdf"]
    assert g1["_spec"].has_deriv and any("deriv" in r for r in g1["terms"])
    _, (R, *R64) = GT.case_truth(name, P)
    dev, e64 = GT.units(_outputs(g1), R), GT.yardstick(R, R64)
    for fam in sorted(dev):
        print(f"{name:8s} {fam:10s} device {dev[fam]:9.1f}  float64 {e64[fam]:9.1f}  floor {GT.FLOORS[fam]:8.1f}")
    bad = {fam: (dev[fam], e64[fam]) for fam in dev if not dev[fam] <= GT.bound(fam, e64[fam])}
    assert not bad, (name, bad)


@pytest.mark.parametrize("base", sorted(BASES))
def test_input_scale_coefficients_match_the_table_on_the_device(base):
    """GA, GB, GC of csrc/deriv_eval.h (the Matern-3/2 rescaled path included) held to the 80-digit table ON THE DEVICE, pair by
    pair: a two-point model -- block 0 the pair's column point, block 1 its row point, an SE term of variance 1 on each
    diagonal block, the derivative term alone in pair (1, 0) (its mirror image in (0, 1)), noise 8 -- whose sgp_logpdf_grad
    returns grad_inscale[t] = G_10 (u . grad_u T) and grad_coef[t] = G_10 T for that term.  C = [[9, v], [v, 9]] with v the
    table's value, so G_10 = (alpha_1 alpha_0 - C^-1_10) / 2 is known in long double, and well conditioned (|v| <= 3).
    Bound: the table's own bound of the entry times |G_10|, the table's value bound times |d G_10 / dv| |entry| for the device's
    own v, and 32 units of the product for the 2 x 2 factorisation and the contraction."""
    kind = BASES[base][0]
    LD = np.longdouble
    lib, d = L.load(), L.dptr
    yv = np.array([0.75, -1.25])
    worst = 0.0
    for D, G in dt.load()[base].items():
        for (a, b), rec in G["terms"].items():
            vb, gb = dt.value_bound(base, D, G, rec), dt.inscale_bound(base, D, G, rec)
            for i in range(G["X"].shape[1]):
                x, yc = np.asfortranarray(G["X"][:, i:i + 1]), np.asfortranarray(G["Y"][:, i:i + 1])
                pairs = {(0, 0): [(L.SE, 0, 0, 1.0, 0.0, None, None)], (1, 1): [(L.SE, 1, 1, 1.0, 0.0, None, None)],
                         (1, 0): [(kind, 1, 0, 1.0, float(17 * a + b), None, None)],
                         (0, 1): [(kind, 0, 1, 1.0, float(17 * b + a), None, None)]}
                sp = L.Spec([1, 1], [1, 1], [yc, x], pairs, True)
                t10 = int(sp._term_ptr[2])
                m, nz, lp = np.zeros(2), np.array([8.0]), np.zeros(1)
                gy, gm, gn, gc, gs = np.zeros(2), np.zeros(2), np.zeros(1), np.zeros(4), np.zeros(4)
                rc = _call(lib.sgp_logpdf_grad, sp, d(m), 0, d(nz), d(yv), d(lp), d(gy), d(gm), d(gn), d(gc), d(gs))
                assert rc == 0, L.last_error()
                v, dv = LD(rec["value"][i]), LD(rec["inscale"][i])
                det = LD(81) - v * v
                Ci = np.array([[9, -v], [-v, 9]], dtype=LD) / det
                al = Ci @ yv.astype(LD)
                G10 = (al[1] * al[0] - Ci[1, 0]) / 2
                dG = (abs(al[0] * al[0]) + abs(al[1] * al[1]) + 1) / det            # a bound of |d G_10 / dv| (|C^-1| <= 1 / 8)
                for got, want, own in ((gs[t10], G10 * dv, gb[i]), (gc[t10], G10 * v, vb[i])):
                    bound = float(abs(G10)) * own + float(dG * abs(want / G10)) * vb[i] + 32 * EPS * float(abs(want)) + dt.FLOOR
                    err = abs(got - float(want))
                    worst = max(worst, err / bound)
                    assert err <= bound, (base, D, (a, b), i, got, float(want), bound)
    print(f"{base}: largest input-scale / value error through the gradient, as a fraction of the bound = {worst:.3g}")


def test_pool_members_return_their_own_bits():
    members = [GT.build_case("se_d3", P), GT.build_case("m52_d1", P)]
    own = [P.logpdf_and_gradient(fx, y) for fx, y in members]
    pooled = P.logpdf_and_gradient_pool([m[0] for m in members], [m[1] for m in members])
    for o, p in zip(own, pooled):
        assert o["logpdf"] == p["logpdf"]
        for a, b in zip(o["_raw"], p["_raw"]):
            assert np.array_equal(a, b)


# ---- 6. refusals through the C boundary -------------------------------------------------------------------------------------
def _refused(rc, what):
    msg = L.last_error()
    assert rc < 0 and "derivative" in msg, (what, rc, msg)


def test_malformed_derivative_terms_are_refused_by_name():
    n = 8
    rng = np.random.default_rng(12)
    X = {D: np.asfortranarray(rng.standard_normal((D, n))) for D in (1, 2, 16, 17)}

    def rc_of(terms, D=2, reserved=0):
        sp = L.Spec([n], [n], [X[D]], {(0, 0): [(k, 0, 0, c, p, None, None) for (k, c, p) in terms]}, True)
        sp._terms[0].reserved = reserved
        K = np.zeros((n, n), order="F")
        return _call(L.load().sgp_kernelmatrix, sp, L.dptr(K), n)

    for param in (0.0, 1.5, float("nan"), -1.0, 289.0, 1e30):
        assert rc_of([(L.DERIV_SE, 1.0, param)]) < 0 and "SGP_DERIV: param" in L.last_error(), param
    assert rc_of([(L.DERIV_SE, 1.0, 17.0 * 3)]) < 0 and "SGP_DERIV: a differentiated coordinate" in L.last_error()
    assert rc_of([(L.DERIV_MATERN52, 1.0, 3.0)]) < 0 and "SGP_DERIV: a differentiated coordinate" in L.last_error()
    assert rc_of([(L.DERIV_MATERN32, 1.0, 18.0)], D=17) < 0 and "SGP_DERIV: the input dimension" in L.last_error()
    assert rc_of([(L.DERIV_SE, 1.0, 18.0)], D=16) == 0
    assert rc_of([(L.DERIV_SE + 1, 1.0, 18.0)]) < 0 and "unknown kernel kind" in L.last_error()       # Matern-1/2: no code
    assert rc_of([(36, 1.0, 18.0)]) < 0 and "unknown kernel kind" in L.last_error()
    TP = L.KIND_TIMES_PREV
    _refused(rc_of([(L.SE, 1.0, 0.0), (L.DERIV_SE | TP, 1.0, 18.0)]), "a derivative continuation")
    _refused(rc_of([(L.DERIV_SE, 1.0, 18.0), (L.SE | TP, 1.0, 0.0)]), "a continuation of a derivative term")
    _refused(rc_of([(L.DERIV_SE, 1.0, 18.0)], reserved=1), "reserved != 0")


def test_entry_points_without_a_derivative_kernel_refuse_by_name():
    n = 16
    gpc = P.GPC()
    f = P.atomic(P.GP(P.SEKernel()), gpc)
    F = P.cross([f, P.derivative(f)])
    xh = np.linspace(-1.0, 1.0, n // 2)
    spec, _, _ = P.build_spec(F, P.BlockData([xh, xh + 0.05]))
    nt = spec.n_terms
    lib, d = L.load(), L.dptr
    ctx = L.default_context()
    m, y, nz, lp = np.zeros(n), np.ones(n), np.array([0.1]), np.zeros(1)
    gy, gm, gn, gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(nt), np.zeros(nt), np.zeros(nt)
    gx = [np.zeros(a.shape, order="F") for a in spec.inputs]
    ptrs = (PD * len(gx))(*[d(a) for a in gx])
    nulls = (PD * max(1, nt))()
    nulls2 = (PD * max(1, 2 * nt))()
    head = (d(m), 0, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc), d(gs))
    assert _call(lib.sgp_logpdf_grad, spec, *head) == 0, L.last_error()
    _refused(_call(lib.sgp_logpdf_grad_x, spec, *head, ptrs), "sgp_logpdf_grad_x")
    _refused(_call(lib.sgp_logpdf_grad_xs, spec, *head, ptrs, nulls), "sgp_logpdf_grad_xs")
    _refused(_call(ctx.kprod.sgp_logpdf_grad_param, spec, *head, d(gp)), "sgp_logpdf_grad_param")
    _refused(_call(ctx.kprod_grad.sgp_logpdf_grad_param_xs, spec, *head, d(gp), ptrs, nulls), "sgp_logpdf_grad_param_xs")
    _refused(_call(ctx.conv_grad.sgp_logpdf_grad_conv, spec, *head), "sgp_logpdf_grad_conv")
    _refused(_call(ctx.stencil_grad.sgp_logpdf_grad_stencil, spec, *head, ptrs), "sgp_logpdf_grad_stencil")
    _refused(_call(ctx.stencil_wo.sgp_logpdf_grad_stencil_wo, spec, *head, ptrs, nulls2, nulls2), "sgp_logpdf_grad_stencil_wo")
    w = np.ones(n)
    _refused(_call(lib.sgp_kernelmatrix_diag_grad, spec, d(w), d(gc), d(gs)), "sgp_kernelmatrix_diag_grad")
    _refused(_call(lib.sgp_kernelmatrix_diag_grad_x, spec, d(w), d(gc), d(gs), ptrs), "sgp_kernelmatrix_diag_grad_x")
    _refused(_call(ctx.kprod_grad.sgp_kernelmatrix_diag_grad_param, spec, d(w), d(gc), d(gs), d(gp), ptrs, nulls, nulls),
             "sgp_kernelmatrix_diag_grad_param")
    _refused(_call(ctx.stencil_grad.sgp_kernelmatrix_diag_grad_stencil, spec, d(w), d(gc), d(gs), ptrs),
             "sgp_kernelmatrix_diag_grad_stencil")
    _refused(_call(ctx.conv_grad.sgp_kernelmatrix_diag_grad_conv, spec, d(w), d(gc), d(gs)), "sgp_kernelmatrix_diag_grad_conv")
    K32 = np.zeros((n, n), dtype=np.float32, order="F")
    _refused(_call(lib.sgp_kernelmatrix_f32, spec, K32.ctypes.data_as(C.POINTER(C.c_float)), n), "sgp_kernelmatrix_f32")
    _refused(_call(lib.sgp_logpdf_f32, spec, d(m), 0, d(nz), d(y), d(lp)), "sgp_logpdf_f32")
    fx = F(P.BlockData([xh, xh + 0.05]), 0.1)
    # the ELBO family: zz and xz both carry derivative terms (F at inducing and at data points)
    xz_x, xz_z = P.BlockData([xh, xh + 0.05]), P.BlockData([xh[::2], xh[::2] + 0.05])
    zz = P.build_spec(F, xz_z)[0]
    xz = P.build_spec(F, xz_x, F, xz_z)[0]
    mz = zz.N
    ntz, ntx = max(1, zz.n_terms), max(1, xz.n_terms)
    var_x, znz, eo, gv, gzn = np.ones(n), np.array([1e-6]), np.zeros(1), np.zeros(n), np.zeros(1)
    gcz, gsz, gcx, gsx = np.zeros(ntz), np.zeros(ntz), np.zeros(ntx), np.zeros(ntx)
    ehead = (ctx.handle, zz.ref(ctx), xz.ref(ctx), d(var_x), d(m), 0, d(nz), 0, d(znz), d(y), d(eo), d(gy), d(gm), d(gn), d(gv),
             d(gzn), d(gcz), d(gsz), d(gcx), d(gsx))
    pz = (PD * max(1, len(zz.inputs)))()
    px = (PD * max(1, len(xz.inputs)))()
    assert mz == 8
    _refused(lib.sgp_elbo_grad(*ehead), "sgp_elbo_grad")
    _refused(lib.sgp_elbo_grad_x(*ehead, pz, px), "sgp_elbo_grad_x")
    _refused(ctx.conv_grad.sgp_elbo_grad_conv(*ehead, pz, px), "sgp_elbo_grad_conv")
    _refused(ctx.stencil_grad.sgp_elbo_grad_stencil(*ehead, pz, px), "sgp_elbo_grad_stencil")
    # prediction gradients: a kept exact posterior and a kept sparse posterior of the same model, derivative terms in the
    # test-side specs
    xs = P.BlockData([xh[:3], xh[:2] + 0.01])
    for post in (P.posterior(fx, y), P.posterior(P.VFE(F(xz_z, 1e-6)), fx, y)):
        sparse = not isinstance(post, P.PosteriorGP)
        cross = P.build_spec(F, xs, F, xz_z if sparse else xz_x)[0]
        pss = P.build_spec(F, xs)[0]
        ms, mo, vo = np.zeros(5), np.zeros(5), np.zeros(5)
        pc, pp = (PD * max(1, len(cross.inputs)))(), (PD * max(1, len(pss.inputs)))()
        fn = ctx.predgrad.sgp_sparse_posterior_predict_grad_x if sparse else ctx.predgrad.sgp_posterior_predict_grad_x
        _refused(fn(post._ensure(), cross.ref(ctx), pss.ref(ctx), d(ms), d(mo), d(vo), pc, pc, pp), fn.__name__)
    # the two remaining fp32 entry points
    Z = np.zeros((n, 1), order="F")
    o32 = np.zeros((n, 1), dtype=np.float32, order="F")
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    _refused(_call(lib.sgp_rand_f32, spec, d(m), 0, d(nz), d(Z), n, 1, f32(o32), n), "sgp_rand_f32")
    plain = P.build_spec(f, xh)[0]
    crs = P.build_spec(F, xs, f, xh)[0]
    pss = P.build_spec(F, xs)[0]
    mo32, vo32 = np.zeros(5, dtype=np.float32), np.zeros(5, dtype=np.float32)
    _refused(lib.sgp_posterior_mean_var_f32(ctx.handle, plain.ref(ctx), d(m), 0, d(nz), d(y), crs.ref(ctx), pss.ref(ctx),
                                            d(np.zeros(5)), f32(mo32), f32(vo32)), "sgp_posterior_mean_var_f32")
    # the host functions that must refuse, through the real library's specs
    for call in (lambda: P.logpdf_and_gradient(fx, y, inputs=True), lambda: P.logpdf_and_gradient_param(fx, y),
                 lambda: P.elbo_and_gradient(P.VFE(F(P.BlockData([xh[::2], xh[::2] + 0.05]), 1e-6)), fx, y),
                 lambda: P.mean_and_var_and_gradient(P.posterior(fx, y)(P.BlockData([xh[:3], xh[:2]])))):
        with pytest.raises(NotImplementedError, match="derivative"):
            call()
