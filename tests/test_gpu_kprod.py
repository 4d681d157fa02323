"""Product chains, RationalQuadratic and Linear kernels on the device (csrc/kprod.hip; include/sthenomi_kprod.h): the RQ
formula against the 60-digit table (tests/kprod_truth.py), matrices against the NumPy evaluator (tests/kprod_np.py), the bit
identities that pin the shared formulas, every operator downstream of assembly, the gradient with its parameter output, zero
factors, and the refusals.  Every case has N <= 512."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import kprod_np as kn
import kprod_truth as kt
import stheno_jl_amd as P
from stheno_jl_amd import lib as L
from test_gpu_kernel_formulas import _pair_at_offsets
from test_gpu_parity import REL
from test_kprod_on_numpy import golden_kernel, load_golden, np_logpdf

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]


def analytic_inscale(spec, G):
    """d / d input scale of every term for the cotangent G, from the analytic dk / dg of tests/kprod_grad_truth.py run in float64:
    held to the 1e-8 of d_coef (the step _oracle_term_grads took for the plain kinds, tests/test_gpu_kernel_formulas.py)"""
    import kprod_grad_truth as KT
    return KT.contract(KT.read_spec(spec), G, np.float64)["d_inscale"]


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _atom(kernel):
    return P.atomic(P.GP(kernel), P.GPC())


def _model(kernel):
    return P.gppp(lambda GP: {"f": GP(kernel)})


def _two_blocks(D, seed, n=(170, 130), shift=None):
    """N = 300 in two blocks of one process: straddles a tile; -> (BlockData, [inputs of each block])"""
    rng = np.random.default_rng(seed)
    Xs = [np.asfortranarray(rng.standard_normal((D, m)) / np.sqrt(D)) for m in n]
    if shift is not None:
        Xs[1][0] += shift
    ins = [P.GPPPInput("f", X[0].copy() if D == 1 else P.ColVecs(X)) for X in Xs]
    return P.BlockData(ins), ins


def _golden_on_two_blocks(kernel=None):
    rng = np.random.default_rng(11)
    xs = [np.sort(rng.uniform(-3.0, 3.0, m)) for m in (170, 130)]
    ins = [P.GPPPInput("f", x) for x in xs]
    y = np.sin(2.0 * np.concatenate(xs)) + 0.3 * rng.standard_normal(300)
    return _model(kernel if kernel is not None else golden_kernel()), P.BlockData(ins), ins, y


# ---- 1. values against the table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,coord", [(1, 0), (16, 11)])
@pytest.mark.parametrize("alpha", kt.ALPHAS)
def test_rq_values_against_the_table(alpha, D, coord):
    """cov(f, [0], t) of a bare atomic GP(RationalQuadraticKernel(alpha)): a chain of one, no coefficient -- the entry IS
    the device's formula at d2 = fl(t t)"""
    g = kt.load()[alpha]
    x0, xt = _pair_at_offsets(D, coord, g.t)
    K = P.prior_cov(_atom(P.RationalQuadraticKernel(alpha)), x0, xt)
    assert K.shape == (1, len(g))
    print(f"\nRQ alpha={alpha} D={D}: largest error in ulps of the truth per band: {kt.band_maxima(g, K)}")
    bad = kt.violations(g, K)
    assert bad.size == 0, kt.describe(g, K, bad)
    assert K[0, 0] == 1.0 and not np.any(np.isnan(K)) and K[0, np.isinf(g.d2)][0] == 0.0
    assert np.all(K.ravel()[g.must_zero] == 0.0)


# ---- 2. matrices ------------------------------------------------------------------------------------------------------------
def _chain_kernel(nf):
    wl = P.with_lengthscale
    if nf == 2:     # a chain, a plain term and a chain of one: three classes of launch in one pair
        return 1.3 * wl(P.SEKernel(), 1.3) * P.Matern32Kernel() + 0.4 * P.Matern52Kernel() + 0.2 * P.RationalQuadraticKernel(0.7)
    if nf == 3:     # two chains of three: at D = 16 they do not fit one launch (6 x 16 > 64)
        return (0.9 * wl(P.Matern52Kernel(), 0.8) * P.RationalQuadraticKernel(0.7) * P.LinearKernel(0.5) +
                1.1 * P.LinearKernel(0.2) * wl(P.SEKernel(), 2.0) * wl(P.Matern12Kernel(), 1.5))
    return 0.8 * (wl(P.SEKernel(), 2.0) * wl(P.Matern12Kernel(), 3.0) * wl(P.Matern32Kernel(), 2.5) * P.Matern52Kernel() *
                  P.RationalQuadraticKernel(1.3) * P.LinearKernel(1.0) * P.ConstantKernel(1.1) * wl(P.SEKernel(), 4.0))


@pytest.mark.parametrize("nf,D", [(2, 1), (2, 3), (2, 16), (3, 1), (3, 3), (3, 16), (8, 1), (8, 3)])
def test_cov_var_and_cross_match_the_evaluator(nf, D):
    F = _model(_chain_kernel(nf))
    x, ins = _two_blocks(D, seed=10 * nf + D)
    spec, _, _ = P.build_spec(F, x)
    assert max(len(ts) for _, _, ts in kn.chains(spec)) == nf
    K = P.prior_cov(F, x)
    Kn = kn.np_spec_matrix(spec)
    assert K.shape == (300, 300) and rel(K, Kn) <= 1e-13
    assert np.array_equal(K, K.T)
    assert np.array_equal(P.prior_var(F, x), np.diag(K))
    Kc = P.prior_cov(F, ins[0], ins[1])                         # the rectangular assembly
    assert np.array_equal(Kc, K[:170, 170:])
    assert rel(Kc, kn.np_spec_matrix(P.build_spec(F, ins[0], None, ins[1])[0])) <= 1e-13


# ---- 3. bit identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "matern12", "matern32", "matern52"])
def test_times_constant_one_reproduces_the_plain_kernel(name):
    """k * ConstantKernel(1.0) runs through kprod.hip, k through kernelmatrix.hip: the multiplication by 1.0 is exact, so equal
    bits mean the two paths share the formulas and the distance"""
    k = {"se": P.SEKernel, "matern12": P.Matern12Kernel, "matern32": P.Matern32Kernel, "matern52": P.Matern52Kernel}[name]
    x, ins = _two_blocks(3, seed=5)
    plain, chained = _model(1.7 * P.with_lengthscale(k(), 0.6)), _model(1.7 * P.with_lengthscale(k(), 0.6) * P.ConstantKernel(1.0))
    assert P.build_spec(chained, x)[0].has_kprod and not P.build_spec(plain, x)[0].has_kprod
    assert np.array_equal(P.prior_cov(chained, x), P.prior_cov(plain, x))
    assert np.array_equal(P.prior_var(chained, x), P.prior_var(plain, x))
    assert np.array_equal(P.prior_cov(chained, ins[1], ins[0]), P.prior_cov(plain, ins[1], ins[0]))


def test_products_commute_and_a_chain_of_one_equals_itself_in_a_longer_list():
    x, _ = _two_blocks(3, seed=6)
    a, b = P.with_lengthscale(P.Matern32Kernel(), 0.7), P.RationalQuadraticKernel(0.9)
    assert np.array_equal(P.prior_cov(_model(a * b), x), P.prior_cov(_model(b * a), x))
    rq = 0.6 * P.with_lengthscale(P.RationalQuadraticKernel(1.3), 0.8)
    longer = 0.0 * P.SEKernel() * P.Matern32Kernel() + rq          # a chain that contributes exact zeros, then the RQ
    spec, _, _ = P.build_spec(_model(longer), x)
    assert spec.n_terms == 4 * 3 and [len(ts) for _, _, ts in kn.chains(spec)][:2] == [2, 1]
    assert np.array_equal(P.prior_cov(_model(longer), x), P.prior_cov(_model(rq), x))


# ---- 4. composed check ------------------------------------------------------------------------------------------------------
def test_product_entries_against_the_entrywise_product_of_two_plain_calls():
    x, _ = _two_blocks(3, seed=7)
    k1, k2 = P.with_lengthscale(P.SEKernel(), 0.9), P.with_lengthscale(P.Matern52Kernel(), 1.4)
    K = P.prior_cov(_model(k1 * k2), x)
    ref = P.prior_cov(_model(k1), x) * P.prior_cov(_model(k2), x)
    assert np.all(np.abs(K - ref) <= 2.0 * np.spacing(ref))


# ---- 5. operators -----------------------------------------------------------------------------------------------------------
def test_logpdf_rand_and_posterior_match_scipy_on_the_evaluators_matrix():
    F, x, ins, y = _golden_on_two_blocks()
    spec, _, _ = P.build_spec(F, x)
    Cm = kn.np_spec_matrix(spec) + 0.1 * np.eye(300)
    ref = np_logpdf(Cm, y)
    fx = F(x, 0.1)
    assert abs(P.logpdf(fx, y) - ref) <= REL * abs(ref)
    Z = np.asfortranarray(np.random.default_rng(1).standard_normal((300, 3)))
    assert rel(P.rand(None, fx, 3, Z=Z), scipy.linalg.cholesky(Cm, lower=True) @ Z) <= REL
    xs = P.GPPPInput("f", np.linspace(-3.5, 3.5, 40))
    Ksx = kn.np_spec_matrix(P.build_spec(F, xs, None, x)[0])
    Kss = kn.np_spec_matrix(P.build_spec(F, xs)[0])
    m, v = P.mean_and_var(P.posterior(fx, y)(xs))
    assert rel(m, Ksx @ np.linalg.solve(Cm, y)) <= REL
    assert rel(v, np.diag(Kss - Ksx @ np.linalg.solve(Cm, Ksx.T))) <= REL


def test_sklearn_log_marginal_likelihood():
    x, y, Kg, g = load_golden()
    f = _atom(golden_kernel())
    assert rel(P.prior_cov(f, x)[g["K_rows"]], Kg) <= 1e-13
    lp = P.logpdf(f(x, g["noise"]), y)
    assert abs(lp - g["lml"]) <= 1e-10 * abs(g["lml"]), (lp, g["lml"])


def test_elbo_matches_the_titsias_bound():
    F, _, ins, y = _golden_on_two_blocks()
    x, z = ins[0], P.GPPPInput("f", np.linspace(-2.8, 2.8, 8))
    y = y[:170]
    val = P.elbo(P.VFE(F(z)), F(x, 0.1), y)
    Kxx = kn.np_spec_matrix(P.build_spec(F, x)[0])
    Kxz = kn.np_spec_matrix(P.build_spec(F, x, None, z)[0])
    Kzz = kn.np_spec_matrix(P.build_spec(F, z)[0]) + 1e-18 * np.eye(8)
    A = np.linalg.solve(np.linalg.cholesky(Kzz), Kxz.T)
    Q = A.T @ A
    ref = np_logpdf(Q + 0.1 * np.eye(170), y) - 0.5 * (np.trace(Kxx) - np.trace(Q)) / 0.1
    assert abs(val - ref) <= 1e-10 * abs(ref)


# ---- 6. batch, pool and extend -----------------------------------------------------------------------------------------------
def test_batch_and_pool_members_are_bit_equal_to_their_own_calls():
    rng = np.random.default_rng(8)
    kernels = [golden_kernel(), 2.0 * P.SEKernel() * P.LinearKernel(0.3) + 0.5 * P.Matern32Kernel(),
               P.with_lengthscale(P.RationalQuadraticKernel(0.6), 0.7) * P.PeriodicKernel(0.9)]
    same = [(_atom(k)(np.sort(rng.uniform(-3, 3, 150)), 0.1 + 0.05 * i), rng.standard_normal(150)) for i, k in enumerate(kernels)]
    own = np.array([P.logpdf(fx, y) for fx, y in same])
    assert np.array_equal(P.logpdf_batch([s[0] for s in same], [s[1] for s in same]), own)
    ragged = [(_atom(k)(np.sort(rng.uniform(-3, 3, n)), 0.2), rng.standard_normal(n)) for k, n in zip(kernels, (100, 300, 129))]
    own = np.array([P.logpdf(fx, y) for fx, y in ragged])
    got, report = P.logpdf_pool([s[0] for s in ragged], [s[1] for s in ragged], return_report=True)
    assert np.array_equal(got, own) and report["pooled_members"] == 3


def test_update_posterior_on_a_product_model_agrees_with_the_stacked_posterior():
    F, _, ins, y = _golden_on_two_blocks()
    p_ext = P.update_posterior(P.posterior(F(ins[0], 0.1), y[:170]), F(ins[1], 0.1), y[170:])
    p_one = P.posterior(F(P.BlockData(ins), 0.1), y)
    assert rel(p_ext.alpha, p_one.alpha) < 1e-9
    xs = P.GPPPInput("f", np.linspace(-3.5, 3.5, 25))
    (me, ve), (m1, v1) = p_ext.mean_and_var(xs), p_one.mean_and_var(xs)
    assert np.max(np.abs(me - m1)) < 1e-9 and np.max(np.abs(ve - v1)) < 1e-9
    assert np.max(np.abs(p_ext.cov(xs) - p_one.cov(xs))) < 1e-9


# ---- 7. gradient ------------------------------------------------------------------------------------------------------------
def _G(spec, noise, y):
    Cm = kn.np_spec_matrix(spec) + noise * np.eye(len(y))
    Ci = np.linalg.inv(Cm)
    al = Ci @ y
    return 0.5 * (np.outer(al, al) - Ci), Cm


def test_gradient_outputs_match_the_numpy_contraction_and_the_existing_entry_point():
    F, x, _, y = _golden_on_two_blocks()
    g = P.logpdf_and_gradient(F(x, 0.1), y)
    spec = g["_spec"]
    gc, gs, gp = g["_raw"]
    assert spec.n_terms == 20 and spec.has_kprod
    G, Cm = _G(spec, 0.1, y)
    assert abs(g["logpdf"] - np_logpdf(Cm, y)) <= REL * abs(g["logpdf"])
    ec, _, ep = kn.np_contract(spec, G)
    es = analytic_inscale(spec, G)
    for t in range(spec.n_terms):
        assert abs(gc[t] - ec[t]) <= 1e-8 * max(1.0, abs(ec[t])), (t, gc[t], ec[t])
        assert abs(gp[t] - ep[t]) <= 1e-8 * max(1.0, abs(ep[t])), (t, gp[t], ep[t])
        assert abs(gs[t] - es[t]) <= 1e-8 * max(1.0, abs(es[t])), (t, gs[t], es[t])
    cont = [t for t in range(20) if spec._terms[t].kind & L.KIND_TIMES_PREV]
    assert len(cont) == 8 and np.all(gc[cont] == 0.0)
    assert np.abs(g["noise"] - np.trace(G)) <= 1e-8 * max(1.0, abs(np.trace(G)))
    # the existing entry point takes the spec and returns the same coef / inscale bits
    ctx = L.default_context()
    d = L.dptr
    m, nz, lp = np.zeros(300), np.array([0.1]), np.zeros(1)
    gy, gm, gn, gc2, gs2 = np.zeros(300), np.zeros(300), np.zeros(1), np.zeros(20), np.zeros(20)
    rc = ctx.lib.sgp_logpdf_grad(ctx.handle, spec.ref(ctx), d(m), L.NOISE_SCALAR, d(nz), d(np.ascontiguousarray(y)), d(lp),
                                 d(gy), d(gm), d(gn), d(gc2), d(gs2))
    assert rc == 0, L.last_error()
    assert np.array_equal(gc2, gc) and np.array_equal(gs2, gs) and lp[0] == g["logpdf"] and np.array_equal(gy, g["y"])


def _check_contraction(F, x, y, noise=0.1):
    """matrix, logpdf and the three gradient outputs of F at x against the evaluator; -> (the gradient dict, K)"""
    g = P.logpdf_and_gradient(F(x, noise), y)
    spec = g["_spec"]
    K = P.prior_cov(F, x)
    assert rel(K, kn.np_spec_matrix(spec)) <= 1e-13 and np.array_equal(K, K.T)
    assert np.array_equal(P.prior_var(F, x), np.diag(K))
    G, Cm = _G(spec, noise, y)
    assert abs(g["logpdf"] - np_logpdf(Cm, y)) <= REL * abs(g["logpdf"])
    gc, gs, gp = g["_raw"]
    ec, _, ep = kn.np_contract(spec, G)
    es = analytic_inscale(spec, G)
    for t in range(spec.n_terms):
        assert abs(gc[t] - ec[t]) <= 1e-8 * max(1.0, abs(ec[t])), (t, gc[t], ec[t])
        assert abs(gp[t] - ep[t]) <= 1e-8 * max(1.0, abs(ep[t])), (t, gp[t], ep[t])
        assert abs(gs[t] - es[t]) <= 1e-8 * max(1.0, abs(es[t])), (t, gs[t], es[t])
    return g, K


@pytest.mark.parametrize("nf,D", [(4, 16), (8, 8)])
def test_gradient_at_the_limits_of_a_chain(nf, D):
    """the DMAX = 16 and DMAX = 8 instantiations of the contraction at their largest chains (4 x 16 = 8 x 8 = 64: all of the
    65 KiB of dynamic LDS, every register array full)"""
    wl = P.with_lengthscale
    k = _chain_kernel(8) if nf == 8 else 0.9 * wl(P.SEKernel(), 2.0) * P.RationalQuadraticKernel(0.7) * P.LinearKernel(0.5) * \
        wl(P.Matern32Kernel(), 1.5)
    x, _ = _two_blocks(D, seed=100 + D)
    g, _ = _check_contraction(_model(k), x, np.random.default_rng(D).standard_normal(300))
    assert max(len(ts) for _, _, ts in kn.chains(g["_spec"])) == nf and g["_spec"].inputs[0].shape[0] == D


def test_function_scaled_process_with_a_product_kernel():
    """g = sigma(x) * f with f ~ GP(product): the head of every chain carries a row scale, a column scale or both, on the
    assembly, the diagonal and the contraction"""
    k = 1.4 * P.SEKernel() * P.with_lengthscale(P.RationalQuadraticKernel(0.9), 1.2) + 0.3 * P.LinearKernel(0.4) * P.Matern32Kernel()
    sigma = lambda v: 1.0 + 0.5 * float(np.sin(np.sum(v)))      # noqa: E731
    F = P.gppp(lambda GP: (lambda f: {"f": f, "g": sigma * f})(GP(k)))
    rng = np.random.default_rng(21)
    Xs = [np.asfortranarray(rng.standard_normal((3, m)) / np.sqrt(3.0)) for m in (170, 130)]
    x = P.BlockData([P.GPPPInput("g", P.ColVecs(Xs[0])), P.GPPPInput("f", P.ColVecs(Xs[1]))])
    g, K = _check_contraction(F, x, rng.standard_normal(300))
    spec = g["_spec"]
    heads = [ts[0] for _, _, ts in kn.chains(spec)]
    scaled = [(spec.term_row_scale[t] is not None, spec.term_col_scale[t] is not None) for t in heads]
    assert scaled == [(True, True)] * 2 + [(True, False)] * 2 + [(False, True)] * 2 + [(False, False)] * 2
    s0 = np.array([sigma(Xs[0][:, i]) for i in range(170)])
    Kf = P.prior_cov(F, P.BlockData([P.GPPPInput("f", P.ColVecs(X)) for X in Xs]))
    assert rel(K[:170, :170], s0[:, None] * Kf[:170, :170] * s0[None, :]) <= 1e-14
    assert rel(K[:170, 170:], s0[:, None] * Kf[:170, 170:]) <= 1e-14
    Kc = P.prior_cov(F, x.X[0], x.X[1])
    assert np.array_equal(Kc, K[:170, 170:])


def test_gradient_records_match_central_differences_of_the_hyperparameters():
    """lengthscale l, periodic r, alpha, the RQ lengthscale, c and the three variances; step and tolerance of
    test_logpdf_gradient_* in tests/test_gpu_parity.py"""
    th0 = dict(v1=4.0, l=1.5, r=0.6, v2=0.7, alpha=1.3, l2=0.8, v3=0.1, c=0.25)

    def kernel(th):
        return (th["v1"] * P.with_lengthscale(P.SEKernel(), th["l"]) * (P.PeriodicKernel(th["r"]) @ P.ScaleTransform(1.0 / 0.9)) +
                th["v2"] * P.with_lengthscale(P.RationalQuadraticKernel(th["alpha"]), th["l2"]) +
                th["v3"] * P.PolynomialKernel(2, th["c"]))

    _, x, _, y = _golden_on_two_blocks()
    lp = lambda th: P.logpdf(_model(kernel(th))(x, 0.1), y)      # noqa: E731
    g = P.logpdf_and_gradient(_model(kernel(th0))(x, 0.1), y)
    recs = g["terms"]
    assert len(recs) == 15 and [r["factor"] for r in recs[:5]] == [0, 1, 0, 0, 1] and recs[1]["chain"] == 0
    pos = lambda k, key: sum(r[key] for i, r in enumerate(recs) if i % 5 == k)      # noqa: E731
    got = dict(v1=pos(0, "d_coef"), l=-pos(0, "d_inscale") / th0["l"], r=-pos(1, "d_inscale") / th0["r"],
               v2=pos(2, "d_coef"), alpha=pos(2, "d_param"), l2=-pos(2, "d_inscale") / th0["l2"], v3=pos(3, "d_coef"),
               c=pos(3, "d_param") + pos(4, "d_param"))
    h = 1e-5
    for name, v0 in th0.items():
        fd = (lp({**th0, name: v0 + h}) - lp({**th0, name: v0 - h})) / (2 * h)
        assert abs(got[name] - fd) <= 1e-6 * max(1.0, abs(fd)), (name, got[name], fd)


# ---- 8. zero factors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["white_factor", "far_clusters"])
def test_zero_factors_give_exact_zeros_and_finite_values(case):
    if case == "white_factor":
        k = 1.5 * P.SEKernel() * P.WhiteKernel() * P.RationalQuadraticKernel(0.8) + 0.5 * P.Matern32Kernel()
        x, _ = _two_blocks(3, seed=9)
    else:
        k = 1.5 * P.SEKernel() * P.RationalQuadraticKernel(0.8) * P.LinearKernel(0.3) + 0.5 * P.Matern32Kernel()
        x, _ = _two_blocks(3, seed=9, shift=1e3)
    F = _model(k)
    y = np.random.default_rng(10).standard_normal(300)
    g = P.logpdf_and_gradient(F(x, 0.1), y)
    spec = g["_spec"]
    assert np.isfinite(g["logpdf"]) and all(np.all(np.isfinite(a)) for a in g["_raw"]) and np.all(np.isfinite(g["y"]))
    K = P.prior_cov(F, x)
    assert not np.any(np.isnan(K)) and rel(K, kn.np_spec_matrix(spec)) <= 1e-13
    if case == "far_clusters":
        assert np.all(K[:170, 170:] == 0.0)
    # pairs (0, 1) and (1, 0): terms 4 .. 11; the chain is the first three of each pair's four
    cross = [t for p in (1, 2) for t in range(4 * p, 4 * p + 3)]
    assert all(spec._terms[t].kind in (L.SE, (L.WHITE if case == "white_factor" else L.RQ) | 0x100,
                                       (L.RQ if case == "white_factor" else L.LINEAR) | 0x100) for t in cross)
    for a in g["_raw"]:
        assert np.all(a[cross] == 0.0)
    G, _ = _G(spec, 0.1, y)
    ec, _, ep = kn.np_contract(spec, G)
    assert rel(g["_raw"][0], ec) <= 1e-8 and rel(g["_raw"][1], analytic_inscale(spec, G)) <= 1e-8 and rel(g["_raw"][2], ep) <= 1e-8


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def _call(fn, spec, *args):
    ctx = L.default_context()
    return fn(ctx.handle, spec.ref(ctx), *args)


def test_entry_points_without_a_product_instantiation_refuse_by_name():
    n = 16
    f = _atom(golden_kernel())
    x = np.linspace(-1.0, 1.0, n)
    spec, _, _ = P.build_spec(f, x)
    lib, d = L.load(), L.dptr
    PD = C.POINTER(C.c_double)
    m, y, nz, lp = np.zeros(n), np.ones(n), np.array([0.1]), np.zeros(1)
    gy, gm, gn, gc, gs = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(5), np.zeros(5)
    gx = [np.zeros(a.shape, order="F") for a in spec.inputs]
    ptrs = (PD * len(gx))(*[d(a) for a in gx])
    base = (d(m), L.NOISE_SCALAR, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc), d(gs))
    refused = lambda rc: rc < 0 and "product" in L.last_error()      # noqa: E731
    assert refused(_call(lib.sgp_logpdf_grad_x, spec, *base, ptrs))
    assert refused(_call(lib.sgp_logpdf_grad_xs, spec, *base, None, (PD * 5)()))
    assert refused(_call(lib.sgp_kernelmatrix_diag_grad, spec, d(y), d(gc), d(gs)))
    assert refused(_call(lib.sgp_kernelmatrix_diag_grad_x, spec, d(y), d(gc), d(gs), ptrs))
    ctx = L.default_context()
    one = lambda a: (PD * 1)(d(a))          # noqa: E731
    specs = (C.POINTER(L.sgp_cov_spec) * 1)(C.pointer(spec.c))
    rc = L.batch_lib().sgp_logpdf_grad_batch(ctx.handle, 1, specs, one(m), L.NOISE_SCALAR, one(nz), one(y), d(lp), one(gy),
                                             one(gm), one(gn), one(gc), one(gs), (C.c_int * 1)())
    assert refused(rc)
    rc = L.pool_lib().sgp_logpdf_grad_pool(ctx.handle, 1, specs, one(m), (C.c_int * 1)(L.NOISE_SCALAR), one(nz), one(y), d(lp),
                                           one(gy), one(gm), one(gn), one(gc), one(gs), (C.c_int * 1)(), None)
    assert refused(rc)
    # the ELBO gradient: products in K(z, z) and K(x, z)
    z = np.linspace(-1.0, 1.0, 4)
    zz, xz = P.build_spec(f, z)[0], P.build_spec(f, x, None, z)[0]
    gz, gzs, gxz, gxs = np.zeros(5), np.zeros(5), np.zeros(5), np.zeros(5)
    rc = lib.sgp_elbo_grad(ctx.handle, zz.ref(ctx), xz.ref(ctx), d(np.ones(n)), d(m), L.NOISE_SCALAR, d(nz), L.NOISE_SCALAR,
                           d(np.array([1e-6])), d(y), d(lp), d(gy), d(gm), d(gn), d(np.zeros(n)), d(np.zeros(1)), d(gz), d(gzs),
                           d(gxz), d(gxs))
    assert refused(rc)
    # fp32 entry points refuse; a Float32 model returns Float32 through the fp64 path
    K32 = np.zeros((n, n), dtype=np.float32)
    assert refused(_call(lib.sgp_kernelmatrix_f32, spec, K32.ctypes.data_as(C.POINTER(C.c_float)), n))
    assert "fp32" in L.last_error()
    assert refused(_call(lib.sgp_logpdf_f32, spec, d(m), L.NOISE_SCALAR, d(nz), d(y), d(lp)))
    x32, y32 = x.astype(np.float32), np.sin(x).astype(np.float32)
    K = P.prior_cov(f, x32)
    assert K.dtype == np.float32 and np.array_equal(K, P.prior_cov(f, x32.astype(np.float64)).astype(np.float32))
    lp32 = P.logpdf(f(x32, 0.1), y32)
    assert isinstance(lp32, np.float32) and lp32 == np.float32(P.logpdf(f(x32.astype(np.float64), 0.1), y32.astype(np.float64)))
    # the host raises before the call
    for kw in (dict(inputs=True), dict(scales=True)):
        with pytest.raises(NotImplementedError, match="product"):
            P.logpdf_and_gradient(f(x, 0.1), y, **kw)


def test_multi_gpu_context_refuses_product_specs():
    f = _atom(P.SEKernel() * P.Matern32Kernel())
    spec, _, _ = P.build_spec(f, np.linspace(0.0, 1.0, 16))
    mctx = L.Context(devices=[0, 0])
    try:
        K = np.zeros((16, 16), order="F")
        rc = mctx.lib.sgp_kernelmatrix(mctx.handle, spec.ref(mctx), L.dptr(K), 16)
        assert rc < 0 and "product" in L.last_error() and "multi-GPU" in L.last_error()
        out = np.zeros(1)
        rc = mctx.lib.sgp_logpdf(mctx.handle, spec.ref(mctx), None, L.NOISE_SCALAR, L.dptr(np.array([0.1])),
                                 L.dptr(np.ones(16)), 16, 1, L.dptr(out))
        assert rc < 0 and "product" in L.last_error()
    finally:
        mctx.close()


def _kernelmatrix_rc(spec):
    K = np.zeros((spec.N, spec.M), order="F")
    return _call(L.load().sgp_kernelmatrix, spec, L.dptr(K), spec.N)


def test_malformed_chains_and_the_limits_are_refused_by_name():
    n = 8
    rng = np.random.default_rng(12)
    X = {D: np.asfortranarray(rng.standard_normal((D, n))) for D in (1, 2, 16, 17)}
    TP = L.KIND_TIMES_PREV

    def spec_of(terms, D=1, reserved=None):
        """one block pair over one input of dimension D; terms: (kind, coef, param[, row_scale])"""
        full = [(k, 0, 0, c, p, (rs[0] if rs else None), None) for (k, c, p, *rs) in terms]
        sp = L.Spec([n], [n], [X[D]], {(0, 0): full}, True)
        for t, code in (reserved or {}).items():
            sp._terms[t].reserved = code
        return sp

    ok = spec_of([(L.SE, 2.0, 0.0), (L.LINEAR | TP, 1.0, 0.5), (L.RQ, 1.0, 1.3)])
    assert _kernelmatrix_rc(ok) == 0
    bad = {
        "continuation first": spec_of([(L.SE | TP, 1.0, 0.0), (L.SE, 1.0, 0.0)]),
        "continuation coef": spec_of([(L.SE, 1.0, 0.0), (L.SE | TP, 2.0, 0.0)]),
        "continuation scale": spec_of([(L.SE, 1.0, 0.0), (L.SE | TP, 1.0, 0.0, np.ones(n))]),
        "continuation reserved": spec_of([(L.SE, 1.0, 0.0), (L.SE | TP, 1.0, 0.0)], reserved={1: 1}),
        "head reserved": spec_of([(L.SE, 1.0, 0.0), (L.SE | TP, 1.0, 0.0)], reserved={0: 1}),
        "new kind reserved": spec_of([(L.RQ, 1.0, 1.0)], reserved={0: 1 << 16}),
        "rq alpha": spec_of([(L.RQ, 1.0, 0.0)]),
        "linear c": spec_of([(L.LINEAR, 1.0, -0.5)]),
        "nine factors": spec_of([(L.SE, 1.0, 0.0)] + [(L.SE | TP, 1.0, 0.0)] * 8),
        "five factors at D = 16": spec_of([(L.SE, 1.0, 0.0)] + [(L.SE | TP, 1.0, 0.0)] * 4, D=16),
        "dimension 17": spec_of([(L.SE, 1.0, 0.0), (L.SE | TP, 1.0, 0.0)], D=17),
        "rq dimension 17": spec_of([(L.RQ, 1.0, 1.0)], D=17),
    }
    for what, sp in bad.items():
        rc = _kernelmatrix_rc(sp)
        assert rc < 0 and "product" in L.last_error(), (what, rc, L.last_error())
    # at the limits: 8 factors at D = 2, 4 at D = 16
    assert _kernelmatrix_rc(spec_of([(L.SE, 1.0, 0.0)] + [(L.MATERN32 | TP, 1.0, 0.0)] * 7, D=2)) == 0
    assert _kernelmatrix_rc(spec_of([(L.SE, 1.0, 0.0)] + [(L.SE | TP, 1.0, 0.0)] * 3, D=16)) == 0
    unknown = spec_of([(8, 1.0, 0.0)])
    assert _kernelmatrix_rc(unknown) < 0 and "unknown kernel kind" in L.last_error()
