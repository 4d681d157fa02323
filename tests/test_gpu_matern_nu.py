"""General-nu Matern (SGP_MATERN_NU = 20, GeneralMaternKernel; csrc/kprod.hip: matern_nu_derivs) on the device: the formula
against the 60-digit table under the bound (A + 4 x + C n) 2^-53 of tests/matern_nu_truth.py, the closed forms at
nu = 1/2, 3/2, 5/2, the bit identities, the gradient families against the contractions of the table-backed restatement
(tests/matern_nu_np.py), every operator downstream of assembly against the NumPy evaluator plus a SciPy Cholesky, and the
refusals.  Every case has N <= 257."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import kernel_truth as kt0
import kprod_grad_np as kg
import kprod_np as kn
import matern_nu_np as mn
import matern_nu_truth as mt
import stheno_jl_amd as P
from stheno_jl_amd import lib as L
from test_gpu_kernel_formulas import _pair_at_offsets
from test_gpu_kprod import _G, _atom, _call, _kernelmatrix_rc, _model, _two_blocks, analytic_inscale, rel
from test_gpu_kprod_grad import _check_against_evaluator, _close
from test_gpu_parity import REL
from test_kprod_grad_on_numpy import titsias
from test_kprod_on_numpy import np_logpdf

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]

wl = P.with_lengthscale
GM = P.GeneralMaternKernel


@pytest.fixture(autouse=True)
def _evaluator_knows_kind_20(monkeypatch):
    mn.install(monkeypatch)


# ---- 1. the formula against the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,coord", [(1, 0), (16, 11)])
@pytest.mark.parametrize("nu", mt.NUS)
def test_values_against_the_table(nu, D, coord):
    """cov(f, [0], t) of a bare atomic GP(GeneralMaternKernel(nu)): a chain of one, no coefficient -- the entry IS the
    device's formula at d2 = fl(t t).  Bound: (A + 4 x + C n) 2^-53 relative to the truth, A = 128, C = 3.
    MI355X maxima (units of 2^-53; the largest over the two D) are recorded in docs/03_kernels.md section 3.2e"""
    g = mt.load()[nu]
    x0, xt = _pair_at_offsets(D, coord, g.t)
    K = P.prior_cov(_atom(GM(nu)), x0, xt)
    assert K.shape == (1, len(g))
    e = mt.err_units(g, K)
    live = g.k > np.finfo(np.float64).tiny
    worst = int(np.argmax(np.where(live, e / mt.bound_units(nu, g.x), 0.0)))
    print(f"\nMatern nu={nu} D={D}: largest error {e[live].max():.1f} x 2^-53 of the truth; largest fraction of the bound "
          f"{e[worst] / mt.bound_units(nu, g.x[worst]):.3f} at x = {g.x[worst]:.4g}")
    bad = mt.violations(g, K, fraction=1.0)
    assert bad.size == 0, mt.describe(g, K, bad)
    assert K[0, 0] == 1.0 and not np.any(np.isnan(K))
    assert K[0, -1] == 0.0 and K[0, -2] == 0.0 and np.all(K.ravel()[g.must_zero] == 0.0)      # overflowed, underflowed


@pytest.mark.parametrize("nu", [0.3, 1.0, 3.7, 32.0])
def test_matrix_over_the_tables_offsets_is_symmetric_and_its_diagonal_is_var(nu):
    """the table's offsets as 1-D points (0 first): K is exactly symmetric, var == diag(cov) bit for bit, exactly 1 on the
    diagonal and at the repeated point, exactly 0 and never NaN against the point 1e160 away; row 0 is the table again"""
    g = mt.load()[nu]
    pts = np.concatenate([[0.0], g.t])                # (g.t[0] is 0 too: a coincident pair off the diagonal)
    f = _atom(GM(nu))
    K = P.prior_cov(f, pts)
    assert K.shape == (20, 20) and np.array_equal(K, K.T) and not np.any(np.isnan(K))
    assert np.array_equal(P.prior_var(f, pts), np.diag(K)) and np.all(np.diag(K) == 1.0) and K[0, 1] == 1.0
    assert np.all(K[-1, :-1] == 0.0)
    assert mt.violations(g, K[0, 1:], fraction=1.0).size == 0


# ---- 2. the closed forms ------------------------------------------------------------------------------------------------------
def _raw_spec(terms, X):
    """one block pair over one input; terms: (kind, coef, param)"""
    n = X.shape[1]
    return L.Spec([n], [n], [X], {(0, 0): [(k, 0, 0, c, p, None, None) for (k, c, p) in terms]}, True)


def _kernelmatrix(spec):
    ctx = L.default_context()
    K = np.zeros((spec.N, spec.N), order="F")
    rc = ctx.lib.sgp_kernelmatrix(ctx.handle, spec.ref(ctx), L.dptr(K), spec.N)
    assert rc == 0, L.last_error()
    return K


@pytest.mark.parametrize("nu,name", [(0.5, "matern12"), (1.5, "matern32"), (2.5, "matern52")])
def test_kind_20_at_a_half_integer_order_agrees_with_the_closed_form_kind(nu, name):
    """raw specs (GeneralMaternKernel is not what MaternKernel(1/2) builds): both kinds see the same d2 and are within their
    own bounds of one truth: (6 + 4 l) ulp (tests/kernel_truth.py) plus (A + 4 x + C n) 2^-53 relative, x = l.  The points
    spread over four decades so that l runs from 1e-3 to 60"""
    rng = np.random.default_rng(3)
    X = np.asfortranarray(rng.standard_normal((3, 150)) * 10.0 ** rng.uniform(-3, 1.3, 150))
    Kg, Kc = _kernelmatrix(_raw_spec([(L.MATERN_NU, 1.0, nu)], X)), _kernelmatrix(_raw_spec([(kt0.KIND[name], 1.0, 0.0)], X))
    l = kt0.C_OF[name] * np.sqrt(mn._sq_dists(X, X))
    tol = kt0.bound_ulps(name, (l / kt0.C_OF[name]) ** 2, np.spacing(Kc)) * np.spacing(Kc) + mt.bound_units(nu, l) * mt.EPS * Kc + mt.TINY
    err = np.abs(Kg - Kc)
    print(f"\nnu={nu}: max |kind 20 - {name}| / tolerance = {np.max(err / tol):.3f}; l up to {l.max():.1f}")
    assert np.all(err <= tol) and l.max() > 30.0 and np.sum((l > 0) & (l < 0.01)) > 10
    assert np.all(np.diag(Kg) == 1.0) and np.array_equal(Kg, Kg.T)


# ---- 3. bit identities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [0.3, 1.25, 25.0])
def test_times_constant_one_is_bit_identical(nu):
    k = 1.7 * wl(GM(nu), 0.6)
    x, ins = _two_blocks(3, seed=5, n=(130, 70))
    plain, chained = _model(k), _model(k * P.ConstantKernel(1.0))
    assert P.build_spec(chained, x)[0].n_terms == 2 * P.build_spec(plain, x)[0].n_terms
    assert np.array_equal(P.prior_cov(chained, x), P.prior_cov(plain, x))
    assert np.array_equal(P.prior_var(chained, x), P.prior_var(plain, x))
    assert np.array_equal(P.prior_cov(chained, ins[1], ins[0]), P.prior_cov(plain, ins[1], ins[0]))


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------
def _grad_kernel(nu, chained):
    k = 1.3 * wl(GM(nu), 0.8)
    return k * (wl(P.SEKernel(), 1.5) @ P.SelectTransform([0, 2])) + 0.3 * P.Matern52Kernel() if chained else k


def _grad_case(nu, chained):
    rng = np.random.default_rng(int(10 * nu) + chained)
    X = np.asfortranarray(rng.standard_normal((3, 150)) / np.sqrt(3.0))
    X[:, 7] = X[:, 3]                                   # a coincident pair: the subgradient / the limit at d2 = 0
    Z = np.asfortranarray(1.2 * rng.standard_normal((3, 40)) / np.sqrt(3.0))
    return (_model(_grad_kernel(nu, chained)), P.GPPPInput("f", P.ColVecs(X)), P.GPPPInput("f", P.ColVecs(Z)),
            rng.standard_normal(150))


@pytest.mark.parametrize("chained", [False, True], ids=["alone", "chain_with_se_on_a_select_view"])
@pytest.mark.parametrize("nu", [0.3, 1.25, 3.7])
def test_logpdf_gradients_match_the_contractions_of_the_restatement(nu, chained):
    """logpdf_and_gradient_param, N = 150, D = 3: coefficient, input-scale and parameter outputs against kprod_np.np_contract
    (1e-8; the input scale against the analytic dk / dg of tests/kprod_grad_truth.py, at 1e-8 too), the point gradients against kprod_grad_np.np_input_grads (the rule of
    tests/test_gpu_kprod_grad.py: _check_against_evaluator); grad_param of the kind is exactly 0"""
    F, x, _, y = _grad_case(nu, chained)
    g = P.logpdf_and_gradient_param(F(x, 0.1), y, inputs=True)
    spec = g["_spec"]
    G, Cm = _G(spec, 0.1, y)
    assert abs(g["logpdf"] - np_logpdf(Cm, y)) <= REL * abs(g["logpdf"])
    gc, gs, gp = g["_raw"]
    ec, _, ep = kn.np_contract(spec, G)
    es = analytic_inscale(spec, G)
    for t in range(spec.n_terms):
        assert abs(gc[t] - ec[t]) <= 1e-8 * max(1.0, abs(ec[t])), (t, gc[t], ec[t])
        assert abs(gp[t] - ep[t]) <= 1e-8 * max(1.0, abs(ep[t])), (t, gp[t], ep[t])
        assert abs(gs[t] - es[t]) <= 1e-8 * max(1.0, abs(es[t])), (t, gs[t], es[t])
    kinds = np.array([spec._terms[t].kind & L.KIND_MASK for t in range(spec.n_terms)])
    assert np.sum(kinds == L.MATERN_NU) == 1 and np.all(gp[:spec.n_terms][kinds == L.MATERN_NU] == 0.0)
    assert all(r["d_param"] == 0.0 for r in g["terms"] if r["kind"] == L.MATERN_NU)
    assert abs(gs[0]) > 1e-3 and (len(kinds) == 3) == chained
    o, ev, _ = _check_against_evaluator(spec, 0.1, y)
    assert max(np.max(np.abs(e)) for e in ev["row"]) > 1e-3


@pytest.mark.parametrize("chained", [False, True], ids=["alone", "chain_with_se_on_a_select_view"])
@pytest.mark.parametrize("nu", [0.3, 1.25, 3.7])
def test_elbo_gradients_match_the_contractions_of_the_restatement(nu, chained):
    """elbo_and_gradient_param, N = 150, M = 40: the value against the dense Titsias bound, the term outputs and the point
    gradients of K(z, z) and K(x, z) against the evaluator contracting NumPy's cotangents (2e-5 of the largest entry:
    tests/test_gpu_kprod_grad.py's bound for these contractions)"""
    F, x, z, y = _grad_case(nu, chained)
    g = P.elbo_and_gradient_param(P.VFE(F(z, 1e-3)), F(x, 0.1), y, inputs=True)
    assert g["elbo"] == P.elbo(P.VFE(F(z, 1e-3)), F(x, 0.1), y)
    zz, xz, xx = (g["_specs"][k] for k in ("zz", "xz", "xx"))
    ref, (dKzz, dKxz, _, _) = titsias(kn.np_spec_matrix(zz) + 1e-3 * np.eye(40), kn.np_spec_matrix(xz), kg.np_diag(xx), y, 0.1,
                                      cotangents=True)
    assert abs(g["elbo"] - ref) <= 1e-10 * abs(ref)
    ez, ex = kg.np_input_grads(zz, dKzz), kg.np_input_grads(xz, dKxz)
    for k, a in enumerate(g["zz_inputs"]):
        assert _close(a, 2.0 * ez["row"][k], 2e-5), ("zz", k)
    for k, a in enumerate(g["xz_inputs"]):
        assert _close(a, ex["row"][k] + ex["col"][k], 2e-5), ("xz", k)
    for key, sp, Gc in (("zz", zz, dKzz), ("xz", xz, dKxz)):
        for got, want in zip(g["_raw"][key], kn.np_contract(sp, Gc)):
            assert _close(got[:sp.n_terms], want, 2e-5), key
    for key in ("zz_terms", "xz_terms", "xx_terms"):
        assert all(r["d_param"] == 0.0 for r in g[key] if r["kind"] == L.MATERN_NU)


# ---- 5. operators ---------------------------------------------------------------------------------------------------------------
def _op_kernel():
    """a chain of four factors (the limit at D = 9 .. 16) with two orders of the kind on both branches of the routine, a
    chain of one, and a plain term"""
    return (1.2 * wl(GM(1.25), 1.5) * wl(P.SEKernel(), 3.0) * wl(GM(0.3), 0.5) * P.ConstantKernel(1.1) + 0.4 * wl(GM(7.5), 2.0) +
            0.3 * P.Matern52Kernel())


@pytest.mark.parametrize("D", [1, 8, 9, 16])
@pytest.mark.parametrize("N", [128, 150, 257])
def test_operators_match_scipy_on_the_evaluators_matrix(N, D):
    """logpdf, rand with a given Z, posterior mean / var / cov, update_posterior, elbo, the VFE posterior,
    logpdf(post(x*, S*), y*), logpdf_batch and logpdf_pool: against the NumPy evaluator plus a SciPy Cholesky, at the
    tolerances of the matching tests of tests/test_gpu_kinds.py and tests/test_gpu_kprod.py (REL = 1e-10; 1e-9 between the
    extended and the stacked posterior; batch and pool members bit-equal to their own calls).  The VFE posterior has no
    test there: its reference solves with K(z, z) + 1e-4 I, condition number below 1e6, so 1e-9 is held"""
    F = _model(_op_kernel())
    x, ins = _two_blocks(D, seed=7 * N + D, n=(N - 50, 50))
    rng = np.random.default_rng(N + D)
    y = rng.standard_normal(N)
    spec, _, _ = P.build_spec(F, x)
    assert spec.has_kprod and max(len(ts) for _, _, ts in kn.chains(spec)) == 4
    Cm = kn.np_spec_matrix(spec) + 0.1 * np.eye(N)
    fx = F(x, 0.1)
    ref = np_logpdf(Cm, y)
    assert abs(P.logpdf(fx, y) - ref) <= REL * abs(ref)
    Z = np.asfortranarray(rng.standard_normal((N, 2)))
    assert rel(P.rand(None, fx, 2, Z=Z), scipy.linalg.cholesky(Cm, lower=True) @ Z) <= REL
    Xs = np.asfortranarray(rng.standard_normal((D, 20)) / np.sqrt(D))
    xs = P.GPPPInput("f", Xs[0].copy() if D == 1 else P.ColVecs(Xs))
    Ksx, Kss = kn.np_spec_matrix(P.build_spec(F, xs, None, x)[0]), kn.np_spec_matrix(P.build_spec(F, xs)[0])
    post = P.posterior(fx, y)
    m, v = P.mean_and_var(post(xs))
    m_ref, c_ref = Ksx @ np.linalg.solve(Cm, y), Kss - Ksx @ np.linalg.solve(Cm, Ksx.T)
    assert rel(m, m_ref) <= REL and rel(v, np.diag(c_ref)) <= REL and rel(post.cov(xs), c_ref) <= REL
    # logpdf of new observations under the posterior
    ys = rng.standard_normal(20)
    lp_ref = np_logpdf(c_ref + 0.2 * np.eye(20), ys - m_ref)
    assert abs(P.logpdf(post(xs, 0.2), ys) - lp_ref) <= REL * abs(lp_ref)
    # the posterior extended by the second block against the stacked one
    p_ext = P.update_posterior(P.posterior(F(ins[0], 0.1), y[:N - 50]), F(ins[1], 0.1), y[N - 50:])
    assert rel(p_ext.alpha, post.alpha) < 1e-9
    me, ve = p_ext.mean_and_var(xs)
    assert np.max(np.abs(me - m_ref)) < 1e-9 and np.max(np.abs(ve - np.diag(c_ref))) < 1e-9
    # the sparse side
    Zs = np.asfortranarray(1.2 * rng.standard_normal((D, 24)) / np.sqrt(D))
    z = P.GPPPInput("f", Zs[0].copy() if D == 1 else P.ColVecs(Zs))
    Kzz = kn.np_spec_matrix(P.build_spec(F, z)[0]) + 1e-4 * np.eye(24)
    Kxz = kn.np_spec_matrix(P.build_spec(F, x, None, z)[0])
    val = P.elbo(P.VFE(F(z, 1e-4)), fx, y)
    ref = titsias(Kzz, Kxz, kg.np_diag(spec), y, 0.1)
    assert abs(val - ref) <= 1e-10 * abs(ref)
    vp = P.posterior(P.VFE(F(z, 1e-4)), fx, y)
    Ksz = kn.np_spec_matrix(P.build_spec(F, xs, None, z)[0])
    S = Kzz + Kxz.T @ Kxz / 0.1
    mv_ref = Ksz @ np.linalg.solve(S, Kxz.T @ y) / 0.1
    cv_ref = Kss - Ksz @ np.linalg.solve(Kzz, Ksz.T) + Ksz @ np.linalg.solve(S, Ksz.T)
    mv, vv = vp.mean_and_var(xs)
    assert rel(mv, mv_ref) <= 1e-9 and rel(vv, np.diag(cv_ref)) <= 1e-9
    # batch and pool members: bit-equal to their own calls
    k2, k3 = 0.7 * wl(GM(2.0), 1.3) * P.LinearKernel(0.3) + 0.5 * GM(0.75), wl(GM(12.0), 0.9)
    mem = [(fx, y)] + [(_atom(k)(np.sort(rng.uniform(-3, 3, n)), 0.15), rng.standard_normal(n))
                       for k, n in ((k2, N), (k2, N - 13), (k3, N - 27))]
    own = np.array([P.logpdf(f, v) for f, v in mem])
    assert np.all(np.isfinite(own))
    assert np.array_equal(P.logpdf_batch([mem[0][0], mem[1][0]], [mem[0][1], mem[1][1]]), own[:2])
    got, report = P.logpdf_pool([mem[i][0] for i in (0, 2, 3)], [mem[i][1] for i in (0, 2, 3)], return_report=True)
    assert np.array_equal(got, own[[0, 2, 3]]) and report["pooled_members"] == 3


def test_an_underflowed_se_times_the_kind_is_an_exact_zero():
    """two clusters 1e160 apart: the squared distance overflows, SE underflows, the kind is an exact 0 there with exact-zero
    derivatives: nothing is NaN, in the matrix or in any gradient output"""
    F = _model(1.5 * P.SEKernel() * GM(1.25) + 0.5 * GM(0.3))
    x, _ = _two_blocks(3, seed=9, n=(130, 70), shift=1e160)
    y = np.random.default_rng(10).standard_normal(200)
    K = P.prior_cov(F, x)
    assert np.all(np.isfinite(K)) and np.all(K[:130, 130:] == 0.0) and np.array_equal(K, K.T)
    assert np.array_equal(P.prior_var(F, x), np.diag(K))
    g = P.logpdf_and_gradient_param(F(x, 0.1), y, inputs=True)
    assert np.isfinite(g["logpdf"]) and all(np.all(np.isfinite(a)) for a in g["_raw"])
    assert all(np.all(np.isfinite(np.asarray(a))) for a in g["inputs"])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def _small_raw(terms, D=1, n=8):
    return _raw_spec(terms, np.asfortranarray(np.random.default_rng(12).standard_normal((D, n))))


def test_orders_outside_the_range_and_the_neighbouring_codes_are_refused_by_name():
    TP = L.KIND_TIMES_PREV
    assert _kernelmatrix_rc(_small_raw([(L.MATERN_NU, 2.0, 0.75), (L.MATERN_NU | TP, 1.0, 32.0), (L.MATERN_NU, 1.0, 1e-3)])) == 0
    assert _kernelmatrix_rc(_small_raw([(L.SE, 1.0, 0.0), (L.MATERN_NU | TP, 1.0, 2.5)], D=16)) == 0
    for nu in (0.0, -1.0, float("nan"), float("inf"), 32.5):
        for terms in ([(L.MATERN_NU, 1.0, nu)], [(L.SE, 1.0, 0.0), (L.MATERN_NU | TP, 1.0, nu)]):
            rc = _kernelmatrix_rc(_small_raw(terms))
            assert rc < 0 and "nu" in L.last_error() and "SGP_MATERN_NU" in L.last_error(), (nu, rc, L.last_error())
    for kind in (18, 19, 19 | TP, 21):
        assert _kernelmatrix_rc(_small_raw([(L.SE, 1.0, 0.0), (kind, 1.0, 1.0)])) < 0, kind
        assert "unknown kernel kind" in L.last_error(), (kind, L.last_error())
    rc = _kernelmatrix_rc(_small_raw([(L.MATERN_NU, 1.0, 1.0)], D=17))
    assert rc < 0 and "product" in L.last_error()


def test_entry_points_without_a_product_instantiation_refuse_the_kind():
    """fp32, the gradient batch and the gradient pool, naming "product"; a multi-GPU context too"""
    n = 16
    x = np.linspace(-1.0, 1.0, n)
    spec, _, _ = P.build_spec(_atom(GM(1.25)), x)
    assert spec.n_terms == 1 and spec.has_kprod
    lib, d = L.load(), L.dptr
    PD = C.POINTER(C.c_double)
    m, y, nz, lp = np.zeros(n), np.ones(n), np.array([0.1]), np.zeros(1)
    gy, gm, gn, gc, gs = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(1), np.zeros(1)
    refused = lambda rc: rc < 0 and "product" in L.last_error()      # noqa: E731
    ctx = L.default_context()
    one = lambda a: (PD * 1)(d(a))          # noqa: E731
    specs = (C.POINTER(L.sgp_cov_spec) * 1)(C.pointer(spec.c))
    spec.ref(ctx)
    rc = L.batch_lib().sgp_logpdf_grad_batch(ctx.handle, 1, specs, one(m), L.NOISE_SCALAR, one(nz), one(y), d(lp), one(gy),
                                             one(gm), one(gn), one(gc), one(gs), (C.c_int * 1)())
    assert refused(rc)
    rc = L.pool_lib().sgp_logpdf_grad_pool(ctx.handle, 1, specs, one(m), (C.c_int * 1)(L.NOISE_SCALAR), one(nz), one(y), d(lp),
                                           one(gy), one(gm), one(gn), one(gc), one(gs), (C.c_int * 1)(), None)
    assert refused(rc)
    assert refused(_call(lib.sgp_logpdf_f32, spec, d(m), L.NOISE_SCALAR, d(nz), d(y), d(lp)))
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_f32(_atom(GM(1.25))(x.astype(np.float32), 0.1), y.astype(np.float32))
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_and_gradient_batch([_atom(GM(1.25))(x, 0.1)], [y])
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_and_gradient_pool([_atom(GM(1.25))(x, 0.1)], [y])
