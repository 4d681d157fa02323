"""The Cosine and GammaExponential kinds on the device (csrc/kprod.hip: cosine_eval / gexp_eval and their derivative
routines; include/sthenomi_kprod.h): the formulas against the 60-digit table (tests/kinds_truth.py), matrices against the NumPy
evaluator (tests/kinds_np.py on top of tests/kprod_np.py) under the summed error models, the bit identities, the anchors of
the GammaExponential convention, every operator downstream of assembly on a spectral-mixture GP, the gradient families, exact
zeros and overflow, batch / pool members, and the refusals.  Every case has N <= 330."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import kinds_np as kd
import kinds_truth as kt
import kprod_grad_np as kg
import kprod_np as kn
import stheno_jl_amd as P
from stheno_jl_amd import lib as L
from test_gpu_kernel_formulas import _pair_at_offsets
from test_gpu_kprod import _G, _atom, _call, _kernelmatrix_rc, _model, _two_blocks, analytic_inscale, rel
from test_gpu_kprod_grad import _check_against_evaluator, _check_diag, _close, _lp_param_xs, _without_pairs
from test_gpu_parity import REL
from test_kprod_grad_on_numpy import titsias
from test_kprod_on_numpy import np_logpdf

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]

N2 = (130, 70)          # two blocks, N = 200: block 0 fills tile 0 and starts tile 1; the pair (1, 0) is off the diagonal
wl = P.with_lengthscale


# ---- 1. values against the table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,coord", [(1, 0), (16, 11)])
def test_cosine_values_against_the_table(D, coord):
    """cov(f, [0], t) of a bare atomic GP(CosineKernel()): a chain of one, no coefficient -- the entry IS the device's
    formula at d2 = fl(t t).  Bound: c0 + pi d |sin pi d| + (pi d)^2 eps / 2 units of 2^-53 (tests/kinds_truth.py)"""
    g = kt.load()["cosine"]
    x0, xt = _pair_at_offsets(D, coord, g.t)
    K = P.prior_cov(_atom(P.CosineKernel()), x0, xt)
    assert K.shape == (1, len(g))
    print(f"\nCosine D={D}: largest error per band (units of 2^-53, fraction of the bound): {kt.cosine_band_maxima(g, K)}")
    bad = kt.cosine_violations(g, K, fraction=1.0)
    assert bad.size == 0, kt.describe(g, K, bad)
    assert K[0, 0] == 1.0 and not np.any(np.isnan(K)) and np.all(K[0, np.isinf(g.d2)] == 1.0)


@pytest.mark.parametrize("D,coord", [(1, 0), (16, 11)])
@pytest.mark.parametrize("gamma", kt.GAMMAS)
def test_gammaexp_values_against_the_table(gamma, D, coord):
    """the same for GammaExponentialKernel(gamma).  Bound: 2 + 32 a ulps of the truth, a = d2^(gamma / 2)"""
    g = kt.load()[gamma]
    x0, xt = _pair_at_offsets(D, coord, g.t)
    K = P.prior_cov(_atom(P.GammaExponentialKernel(gamma)), x0, xt)
    assert K.shape == (1, len(g))
    print(f"\nGammaExp gamma={gamma} D={D}: largest error in ulps of the truth per band: {kt.gexp_band_maxima(g, K)}")
    bad = kt.gexp_violations(g, K, fraction=1.0)
    assert bad.size == 0, kt.describe(g, K, bad)
    assert K[0, 0] == 1.0 and not np.any(np.isnan(K)) and np.all(K[0, np.isinf(g.d2)] == 0.0)
    assert np.all(K.ravel()[g.must_zero] == 0.0)


# ---- 2. matrices ------------------------------------------------------------------------------------------------------------
def _kinds_chain(nf, psd=False):
    """psd: the Cosine factor reads the first coordinate alone.  cos(pi |x - y|) is positive definite on the line only (at
    D = 16 the matrices below have eigenvalues near -16), so whatever is factored takes psd=True or a noise that covers it"""
    cos = (P.CosineKernel() @ P.SelectTransform([0])) if psd else P.CosineKernel()
    if nf == 2:     # a chain, a plain term and a chain of one: three classes of launch in one pair
        return 1.3 * wl(P.SEKernel(), 1.3) * cos + 0.4 * P.Matern52Kernel() + 0.2 * P.GammaExponentialKernel(0.7)
    if nf == 3:
        return (0.9 * wl(P.GammaExponentialKernel(1.7), 0.8) * P.RationalQuadraticKernel(0.7) * P.LinearKernel(0.5) +
                1.1 * P.LinearKernel(0.2) * wl(cos, 2.0) * wl(P.SEKernel(), 1.5))
    if nf == 4:
        return 0.9 * wl(P.SEKernel(), 2.0) * cos * P.LinearKernel(0.5) * wl(P.GammaExponentialKernel(0.3), 1.5)
    return 0.8 * (wl(P.SEKernel(), 2.0) * wl(cos, 3.0) * wl(P.Matern32Kernel(), 2.5) * P.GammaExponentialKernel(1.0) *
                  P.RationalQuadraticKernel(1.3) * P.LinearKernel(1.0) * P.ConstantKernel(1.1) * wl(P.GammaExponentialKernel(2.0), 4.0))


def _within(K, Kn, tol):
    err = np.abs(K - Kn)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"    max|K - Kn| = {float(np.max(err)):.3e}   largest fraction of the entry's bound {worst:.3f}")
    return bool(np.all(err <= tol))


@pytest.mark.parametrize("nf,D", [(2, 1), (2, 3), (3, 1), (3, 3), (8, 1), (8, 3), (4, 16)])
def test_cov_var_and_cross_match_the_evaluator(nf, D):
    """tolerance per entry: the per-factor model bounds times the other factors' magnitudes, summed over the chains, for the
    two evaluations compared (kinds_np.np_spec_tolerance)"""
    F = _model(_kinds_chain(nf))
    x, ins = _two_blocks(D, seed=10 * nf + D, n=N2)
    spec, _, _ = P.build_spec(F, x)
    assert max(len(ts) for _, _, ts in kn.chains(spec)) == nf
    K = P.prior_cov(F, x)
    assert K.shape == (200, 200) and _within(K, kn.np_spec_matrix(spec), kd.np_spec_tolerance(spec))
    assert np.array_equal(K, K.T)
    assert np.array_equal(P.prior_var(F, x), np.diag(K))
    Kc = P.prior_cov(F, ins[0], ins[1])                         # the rectangular assembly
    assert np.array_equal(Kc, K[:130, 130:])
    cross = P.build_spec(F, ins[0], None, ins[1])[0]
    assert _within(Kc, kn.np_spec_matrix(cross), kd.np_spec_tolerance(cross))


# ---- 3. bit identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cosine", "gammaexp"])
def test_times_constant_one_is_bit_identical(name):
    k = 1.7 * wl(P.CosineKernel() if name == "cosine" else P.GammaExponentialKernel(1.3), 0.6)
    x, ins = _two_blocks(3, seed=5, n=N2)
    plain, chained = _model(k), _model(k * P.ConstantKernel(1.0))
    assert P.build_spec(chained, x)[0].n_terms == 2 * P.build_spec(plain, x)[0].n_terms
    assert np.array_equal(P.prior_cov(chained, x), P.prior_cov(plain, x))
    assert np.array_equal(P.prior_var(chained, x), P.prior_var(plain, x))
    assert np.array_equal(P.prior_cov(chained, ins[1], ins[0]), P.prior_cov(plain, ins[1], ins[0]))


def test_products_commute_and_a_chain_of_one_equals_itself_in_a_longer_list():
    x, _ = _two_blocks(3, seed=6, n=N2)
    a, b = wl(P.CosineKernel(), 0.7), P.GammaExponentialKernel(0.9)
    assert np.array_equal(P.prior_cov(_model(a * b), x), P.prior_cov(_model(b * a), x))
    for one in (0.6 * wl(P.GammaExponentialKernel(1.3), 0.8), 0.6 * wl(P.CosineKernel(), 0.8)):
        longer = 0.0 * P.SEKernel() * P.Matern32Kernel() + one          # a chain that contributes exact zeros, then the kind
        spec, _, _ = P.build_spec(_model(longer), x)
        assert [len(ts) for _, _, ts in kn.chains(spec)][:2] == [2, 1]
        assert np.array_equal(P.prior_cov(_model(longer), x), P.prior_cov(_model(one), x))


# ---- 4. the anchors of the convention ----------------------------------------------------------------------------------------
def _cov_and_bound(kernel, x):
    """(K, the entrywise model bound of ONE evaluation)"""
    F = _model(kernel)
    return P.prior_cov(F, x), kd.np_spec_tolerance(P.build_spec(F, x)[0], sides=1)


def test_gamma_one_is_the_exponential_kernel():
    x, _ = _two_blocks(3, seed=7, n=N2)
    (Kg, tg), (Km, tm) = _cov_and_bound(P.GammaExponentialKernel(1.0), x), _cov_and_bound(P.Matern12Kernel(), x)
    assert _within(Kg, Km, tg + tm)


def test_gamma_two_is_the_squared_exponential_after_a_scaling_by_root_two():
    """the SE side reads fl(sqrt 2) x: each coordinate carries one more rounding and fl(sqrt 2)^2 is 2 (1 + 1.3e-16), three
    more eps on its d2 than the model's sum of squares has: + 4 eps |d k / d (d2)| d2 = 4 eps (d2 / 2) k"""
    x, _ = _two_blocks(3, seed=8, n=N2)
    (Kg, tg), (Ks, ts) = _cov_and_bound(P.GammaExponentialKernel(2.0), x), _cov_and_bound(P.SEKernel() @ P.ScaleTransform(np.sqrt(2.0)), x)
    assert _within(Kg, Ks, tg + ts + 4.0 * kt.EPS * (-np.log(np.maximum(Ks, 1e-300))) * Ks)


def test_gabor_entries_against_the_entrywise_product_of_two_plain_calls():
    x, _ = _two_blocks(3, seed=9, n=N2)
    t1, t2 = P.ScaleTransform(1.0 / 0.9), P.ARDTransform([0.5, 1.5, 0.25])
    K = P.prior_cov(_model(P.gaborkernel(sqexponential_transform=t1, cosine_transform=t2)), x)
    ref = P.prior_cov(_model(P.SEKernel() @ t1), x) * P.prior_cov(_model(P.CosineKernel() @ t2), x)
    assert np.all(np.abs(K - ref) <= 2.0 * np.spacing(np.abs(ref)))
    assert np.min(K) < -0.05                                    # (the first kernel here whose entries change sign)


# ---- 5. operators on a spectral-mixture GP ---------------------------------------------------------------------------------
def _sm_theta(seed=9, D=2, Q=3):
    rng = np.random.default_rng(seed)
    return dict(alpha=rng.uniform(0.5, 1.5, Q), gamma=rng.uniform(0.3, 1.2, (D, Q)), omega=rng.uniform(0.1, 0.9, (D, Q)))


def _sm_case(D=2):
    rng = np.random.default_rng(10)
    Xs = [np.asfortranarray(rng.standard_normal((D, m))) for m in N2]
    ins = [P.GPPPInput("f", P.ColVecs(X)) for X in Xs]
    return Xs, ins, P.BlockData(ins), rng.standard_normal(200)


def _sm_model(th):
    return _model(P.spectral_mixture_kernel(th["alpha"], th["gamma"], th["omega"]))


def test_logpdf_rand_and_posterior_of_a_spectral_mixture_gp_match_scipy_on_the_evaluators_matrix():
    F = _sm_model(_sm_theta())
    _, _, x, y = _sm_case()
    spec, _, _ = P.build_spec(F, x)
    assert spec.n_terms == 4 * 6 and len(spec.inputs) == 2 * 6
    Cm = kn.np_spec_matrix(spec) + 0.1 * np.eye(200)
    ref = np_logpdf(Cm, y)
    fx = F(x, 0.1)
    assert abs(P.logpdf(fx, y) - ref) <= REL * abs(ref)
    Z = np.asfortranarray(np.random.default_rng(1).standard_normal((200, 3)))
    assert rel(P.rand(None, fx, 3, Z=Z), scipy.linalg.cholesky(Cm, lower=True) @ Z) <= REL
    xs = P.GPPPInput("f", P.ColVecs(np.asfortranarray(np.random.default_rng(2).standard_normal((2, 40)))))
    Ksx = kn.np_spec_matrix(P.build_spec(F, xs, None, x)[0])
    Kss = kn.np_spec_matrix(P.build_spec(F, xs)[0])
    m, v = P.mean_and_var(P.posterior(fx, y)(xs))
    assert rel(m, Ksx @ np.linalg.solve(Cm, y)) <= REL
    assert rel(v, np.diag(Kss - Ksx @ np.linalg.solve(Cm, Ksx.T))) <= REL


def _sm_sparse():
    F = _sm_model(_sm_theta())
    _, _, x, y = _sm_case()
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(1.2 * np.random.default_rng(3).standard_normal((2, 24)))))
    return F, x, z, y


def test_elbo_of_a_spectral_mixture_gp_matches_the_dense_titsias_bound():
    F, x, z, y = _sm_sparse()
    val = P.elbo(P.VFE(F(z, 1e-6)), F(x, 0.1), y)
    Kzz = kn.np_spec_matrix(P.build_spec(F, z)[0]) + 1e-6 * np.eye(24)
    ref = titsias(Kzz, kn.np_spec_matrix(P.build_spec(F, x, None, z)[0]), kg.np_diag(P.build_spec(F, x)[0]), y, 0.1)
    assert abs(val - ref) <= 1e-10 * abs(ref)


# ---- 6. gradients -----------------------------------------------------------------------------------------------------------
def _check_terms(g, noise, y):
    spec = g["_spec"]
    G, Cm = _G(spec, noise, y)
    assert abs(g["logpdf"] - np_logpdf(Cm, y)) <= REL * abs(g["logpdf"])
    gc, gs, gp = g["_raw"]
    ec, _, ep = kn.np_contract(spec, G)
    es = analytic_inscale(spec, G)
    for t in range(spec.n_terms):
        assert abs(gc[t] - ec[t]) <= 1e-8 * max(1.0, abs(ec[t])), (t, gc[t], ec[t])
        assert abs(gp[t] - ep[t]) <= 1e-8 * max(1.0, abs(ep[t])), (t, gp[t], ep[t])
        assert abs(gs[t] - es[t]) <= 1e-8 * max(1.0, abs(es[t])), (t, gs[t], es[t])
    kinds = np.array([spec._terms[t].kind & L.KIND_MASK for t in range(spec.n_terms)])
    return kinds, gp[:spec.n_terms]


# (nf, D, psd, noise): the last case keeps the Cosine on all 16 coordinates, under a noise above the 16.4 its matrix lacks
GRAD_CASES = [(3, 3, True, 0.1), (8, 1, True, 0.1), (4, 16, True, 0.1), (4, 16, False, 25.0)]


@pytest.mark.parametrize("nf,D,psd,noise", GRAD_CASES)
def test_parameter_gradient_outputs_match_the_numpy_contraction(nf, D, psd, noise):
    """coef, inscale and param of sgp_logpdf_grad_param (tolerances of test_gpu_kprod.py's _check_contraction); d / d gamma is
    non-zero, the Cosine's parameter entry exactly 0"""
    x, _ = _two_blocks(D, seed=100 + D, n=N2)
    y = np.random.default_rng(D).standard_normal(200)
    g = P.logpdf_and_gradient(_model(_kinds_chain(nf, psd))(x, noise), y)
    kinds, gp = _check_terms(g, noise, y)
    assert np.all(gp[kinds == L.COSINE] == 0.0) and np.any(kinds == L.COSINE)
    assert np.all(gp[kinds == L.GAMMAEXP] != 0.0) and np.any(kinds == L.GAMMAEXP)


def _with_duplicates(D, seed):
    """two blocks whose points repeat: inside a block, across the blocks, and across a tile boundary"""
    x, ins = _two_blocks(D, seed=seed, n=N2)
    Xs = [np.array(v.x.X if D > 1 else v.x, dtype=np.float64, order="F").reshape(D, -1) for v in ins]
    Xs[0][:, 5] = Xs[0][:, 3]
    Xs[0][:, 129] = Xs[0][:, 0]
    Xs[1][:, 0] = Xs[0][:, 7]
    Xs[1][:, 69] = Xs[1][:, 68]
    ins = [P.GPPPInput("f", X[0].copy() if D == 1 else P.ColVecs(np.asfortranarray(X))) for X in Xs]
    return P.BlockData(ins)


@pytest.mark.parametrize("nf,D,psd,noise", [(2, 1, True, 0.1), (8, 3, True, 0.1)] + GRAD_CASES[:1] + GRAD_CASES[2:])
def test_input_gradients_match_the_evaluator_on_data_with_exact_duplicates(nf, D, psd, noise):
    """sgp_logpdf_grad_param_xs: coincident points take the Cosine's limit -pi^2 / 2 (times a zero difference) and the
    GammaExponential's subgradient 0; bound of test_gpu_kprod_grad.py's _check_against_evaluator"""
    x = _with_duplicates(D, seed=20 * nf + D)
    spec, _, _ = P.build_spec(_model(_kinds_chain(nf, psd)), x)
    assert spec.has_kprod and max(len(ts) for _, _, ts in kn.chains(spec)) == nf
    o, _, _ = _check_against_evaluator(spec, noise, np.random.default_rng(nf + D).standard_normal(200))
    assert all(np.all(np.isfinite(a)) for a in o["gx"])


def test_input_gradients_of_the_spectral_mixture_model():
    """DMAX = 1: every factor reads a one-dimensional projection"""
    _, _, x, y = _sm_case()
    spec, _, _ = P.build_spec(_sm_model(_sm_theta()), x)
    assert max(a.shape[0] for a in spec.inputs) == 1
    _check_against_evaluator(spec, 0.1, y)


def test_diagonal_gradients_where_the_two_views_differ():
    """var(f(a x) + f(b x)): the cross terms of the diagonal read two different views of x (sgp_kernelmatrix_diag_grad_param)"""
    k = 1.3 * P.SEKernel() * wl(P.CosineKernel(), 1.2) + 0.3 * P.LinearKernel(0.4) * P.GammaExponentialKernel(0.8)
    F = P.gppp(lambda GP: (lambda f: {"f": f, "g": P.stretch(f, 0.7) + P.stretch(f, 1.6)})(GP(k)))
    rng = np.random.default_rng(31)
    x = P.BlockData([P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((3, m)) / np.sqrt(3.0)))) for m in N2])
    spec, _, _ = P.build_spec(F, x)
    o, ev = _check_diag(spec, rng.standard_normal(200))
    assert any(np.max(np.abs(e)) > 1e-3 for e in ev["gx"])
    kinds = np.array([spec._terms[t].kind & L.KIND_MASK for t in range(spec.n_terms)])
    assert np.all(o["gp"][:spec.n_terms][kinds == L.COSINE] == 0.0) and np.any(o["gp"][:spec.n_terms][kinds == L.GAMMAEXP] != 0.0)


def test_elbo_gradient_contractions_match_the_evaluator():
    """sgp_elbo_grad_param on the N = 200, M = 24 spectral-mixture model: the value is sgp_elbo's, the term outputs and the
    input gradients of both sides against the evaluator contracting NumPy's own cotangents of the Titsias bound (2e-5 of the
    largest entry: test_gpu_kprod_grad.py's bound for these contractions)"""
    F, x, z, y = _sm_sparse()
    g = P.elbo_and_gradient_param(P.VFE(F(z, 1e-3)), F(x, 0.1), y, inputs=True)
    assert g["elbo"] == P.elbo(P.VFE(F(z, 1e-3)), F(x, 0.1), y)
    zz, xz, xx = (g["_specs"][k] for k in ("zz", "xz", "xx"))
    ref, (dKzz, dKxz, _, _) = titsias(kn.np_spec_matrix(zz) + 1e-3 * np.eye(24), kn.np_spec_matrix(xz), kg.np_diag(xx), y, 0.1,
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


HYPER = dict(v2=0.5, g=1.3)


def _hyper_model(th):
    """a spectral mixture plus v2 * GammaExponential(g) o ARDTransform(v)"""
    k = P.spectral_mixture_kernel(th["alpha"], th["gamma"], th["omega"]) + \
        float(th["v2"]) * (P.GammaExponentialKernel(float(th["g"])) @ P.ARDTransform(th["v"]))
    return _model(k)


def _hyper_theta():
    th = {k: np.array(v) for k, v in _sm_theta().items()}
    th.update(v2=np.array(0.5), g=np.array(1.3), v=np.array([0.8, 1.4]), noise=np.array(0.1))
    return th


def _hyper_gradients(recs):
    """records (seven per block pair: SE, Cosine per mixture component, then the GammaExponential) -> d / d hyper-parameter.
    d_coef / d_param add up over the block pairs; d_transform is the transform's total, the same array on every pair"""
    out = dict(alpha=np.array([sum(r["d_coef"] for i, r in enumerate(recs) if i % 7 == 2 * q) for q in range(3)]),
               gamma=np.stack([recs[2 * q]["d_transform"][0] for q in range(3)], axis=1),
               omega=np.stack([recs[2 * q + 1]["d_transform"][0] for q in range(3)], axis=1),
               v2=sum(r["d_coef"] for i, r in enumerate(recs) if i % 7 == 6),
               g=sum(r["d_param"] for i, r in enumerate(recs) if i % 7 == 6), v=recs[6]["d_transform"])
    assert [r["kind"] for r in recs[:7]] == [L.SE, L.COSINE] * 3 + [L.GAMMAEXP]
    return out


def _central(f, th, name, idx, h=1e-5):
    p, m = ({k: v.copy() for k, v in th.items()} for _ in range(2))
    p[name][idx] += h
    m[name][idx] -= h
    return (f(p) - f(m)) / (2 * h)


def test_host_records_match_central_differences_of_the_hyperparameters():
    """alpha_q, gamma_q, omega_q (through d_transform), the GammaExponential's variance, gamma and ARD factors, and the
    noise; step and tolerance of test_gradient_records_match_central_differences_of_the_hyperparameters (test_gpu_kprod.py)"""
    th = _hyper_theta()
    _, _, x, y = _sm_case()
    lp = lambda t: P.logpdf(_hyper_model(t)(x, float(t["noise"])), y)      # noqa: E731
    g = P.logpdf_and_gradient_param(_hyper_model(th)(x, 0.1), y, inputs=True)
    assert len(g["terms"]) == 21
    got = _hyper_gradients(g["terms"])
    got["noise"] = np.array(g["noise"])
    for name, val in got.items():
        val = np.asarray(val)
        for idx in np.ndindex(val.shape):
            fd = _central(lp, th, name, idx)
            assert abs(val[idx] - fd) <= 1e-6 * max(1.0, abs(fd)), (name, idx, val[idx], fd)


def test_elbo_records_match_central_differences_of_the_hyperparameters():
    """the same through elbo_and_gradient_param: every entry is the sum over K(z, z), K(x, z) and the diagonal of K(x, x)"""
    th = _hyper_theta()
    _, _, x, y = _sm_case()
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(1.2 * np.random.default_rng(3).standard_normal((2, 24)))))

    def bound(t):
        Fm = _hyper_model(t)
        return P.elbo(P.VFE(Fm(z, 1e-3)), Fm(x, 0.1), y)

    F = _hyper_model(th)
    g = P.elbo_and_gradient_param(P.VFE(F(z, 1e-3)), F(x, 0.1), y, inputs=True)
    parts = [_hyper_gradients(g[key]) for key in ("zz_terms", "xz_terms", "xx_terms")]
    for name in ("alpha", "gamma", "omega", "v2", "g", "v"):
        val = np.asarray(sum(np.asarray(p[name]) for p in parts))
        for idx in np.ndindex(val.shape):
            fd = _central(bound, th, name, idx)
            assert abs(val[idx] - fd) <= 1e-6 * max(1.0, abs(fd)), (name, idx, val[idx], fd)


# ---- 7. zeros and overflow ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["se_cosine", "gammaexp_white"])
def test_clusters_1e160_apart_give_exact_zeros_and_finite_values(case):
    """the squared distance between the clusters overflows: an underflowed SE times a Cosine (exactly 1 there) is an exact 0,
    GammaExponential(0.3) is an exact 0 there and WHITE off the diagonal everywhere; nothing is NaN"""
    if case == "se_cosine":
        k = 1.5 * P.SEKernel() * (P.CosineKernel() @ P.SelectTransform([0])) + 0.5 * P.Matern32Kernel()      # (1-D: PSD)
    else:
        k = 1.5 * P.GammaExponentialKernel(0.3) * P.WhiteKernel() + 0.5 * P.Matern32Kernel()
    F = _model(k)
    x, _ = _two_blocks(3, seed=9, n=N2, shift=1e160)
    y = np.random.default_rng(10).standard_normal(200)
    K = P.prior_cov(F, x)
    assert np.all(np.isfinite(K)) and np.all(K[:130, 130:] == 0.0) and np.array_equal(K, K.T)
    assert np.array_equal(P.prior_var(F, x), np.diag(K))
    if case == "gammaexp_white":
        only = P.prior_cov(_model(1.5 * P.GammaExponentialKernel(0.3) * P.WhiteKernel()), x)
        assert np.array_equal(only, 1.5 * np.eye(200))
    g = P.logpdf_and_gradient(F(x, 0.1), y)
    spec = g["_spec"]
    assert np.isfinite(g["logpdf"]) and g["logpdf"] == P.logpdf(F(x, 0.1), y)
    assert all(np.all(np.isfinite(a)) for a in g["_raw"]) and np.all(np.isfinite(g["y"]))
    # pairs (0, 1) and (1, 0): terms 3 .. 8; the chain is the first two of each pair's three
    cross = [t for p in (1, 2) for t in range(3 * p, 3 * p + 2)]
    assert all(spec._terms[t].kind & L.KIND_MASK in ((L.SE, L.COSINE) if case == "se_cosine" else (L.GAMMAEXP, L.WHITE))
               for t in cross)
    for a in g["_raw"]:
        assert np.all(a[cross] == 0.0)
    o = _lp_param_xs(spec, 0.1, y)
    for a in [o["lp"], o["gy"], o["gm"], o["gn"], o["gc"], o["gs"], o["gp"]] + o["gx"]:
        assert np.all(np.isfinite(a))
    assert all(np.all(o[key][cross] == 0.0) for key in ("gc", "gs", "gp"))
    alone = _lp_param_xs(_without_pairs(spec, {(0, 1), (1, 0)}), 0.1, y)      # the far pairs add exact zeros to every point
    for a, b in zip(o["gx"], alone["gx"]):
        assert np.array_equal(a, b)


# ---- 8. batch and pool ---------------------------------------------------------------------------------------------------------
def test_batch_and_pool_members_are_bit_equal_to_their_own_calls():
    rng = np.random.default_rng(8)
    th = _sm_theta()
    kernels = [P.spectral_mixture_kernel(th["alpha"], th["gamma"][:1], th["omega"][:1]),
               2.0 * P.gaborkernel(cosine_transform=P.ScaleTransform(0.5)) + 0.5 * P.GammaExponentialKernel(1.3)]
    for sizes in ((200, 200), (200, 330)):
        mem = [(_atom(k)(np.sort(rng.uniform(-3, 3, n)), 0.1 + 0.05 * i), rng.standard_normal(n))
               for i, (k, n) in enumerate(zip(kernels, sizes))]
        own = np.array([P.logpdf(fx, y) for fx, y in mem])
        assert np.all(np.isfinite(own))
        assert np.array_equal(P.logpdf_batch([s[0] for s in mem], [s[1] for s in mem]), own)
        got, report = P.logpdf_pool([s[0] for s in mem], [s[1] for s in mem], return_report=True)
        assert np.array_equal(got, own) and (sizes[0] == sizes[1] or report["pooled_members"] == 2)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def _raw_spec(terms, D=1, n=8):
    """one block pair over one input of dimension D; terms: (kind, coef, param)"""
    X = np.asfortranarray(np.random.default_rng(12).standard_normal((D, n)))
    return L.Spec([n], [n], [X], {(0, 0): [(k, 0, 0, c, p, None, None) for (k, c, p) in terms]}, True)


def test_unknown_kinds_bad_gammas_and_the_limits_are_refused_by_name():
    TP = L.KIND_TIMES_PREV
    assert _kernelmatrix_rc(_raw_spec([(L.COSINE, 2.0, 0.0), (L.GAMMAEXP | TP, 1.0, 0.5), (L.GAMMAEXP, 1.0, 2.0)])) == 0
    assert _kernelmatrix_rc(_raw_spec([(L.COSINE, 1.0, float("nan"))])) == 0          # the Cosine's param is ignored
    assert _kernelmatrix_rc(_raw_spec([(L.COSINE, 1.0, 0.0), (L.GAMMAEXP | TP, 1.0, 1.0)], D=16)) == 0
    for kind in (9, 15, 18, 9 | TP, 255):
        assert _kernelmatrix_rc(_raw_spec([(L.SE, 1.0, 0.0), (kind, 1.0, 1.0)])) < 0, kind
        assert "unknown kernel kind" in L.last_error(), (kind, L.last_error())
    for gamma in (0.0, -1.0, 2.5, float("nan"), float("inf")):
        for terms in ([(L.GAMMAEXP, 1.0, gamma)], [(L.SE, 1.0, 0.0), (L.GAMMAEXP | TP, 1.0, gamma)]):
            rc = _kernelmatrix_rc(_raw_spec(terms))
            assert rc < 0 and "product" in L.last_error(), (gamma, rc, L.last_error())
    for kind in (L.COSINE, L.GAMMAEXP):
        rc = _kernelmatrix_rc(_raw_spec([(kind, 1.0, 1.0)], D=17))
        assert rc < 0 and "product" in L.last_error(), (kind, rc, L.last_error())
    sp = _raw_spec([(L.COSINE, 1.0, 0.0)])
    sp._terms[0].reserved = 1
    assert _kernelmatrix_rc(sp) < 0 and "product" in L.last_error()


def test_entry_points_without_a_product_instantiation_refuse_a_cosine_spec():
    n = 16
    x = np.linspace(-1.0, 1.0, n)
    spec, _, _ = P.build_spec(_atom(P.CosineKernel()), x)
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
    gx = [np.zeros(a.shape, order="F") for a in spec.inputs]
    assert refused(_call(lib.sgp_logpdf_grad_x, spec, d(m), L.NOISE_SCALAR, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc), d(gs),
                         (PD * 1)(d(gx[0]))))
    assert refused(_call(lib.sgp_kernelmatrix_diag_grad, spec, d(y), d(gc), d(gs)))
    mctx = L.Context(devices=[0, 0])
    try:
        K = np.zeros((n, n), order="F")
        rc = mctx.lib.sgp_kernelmatrix(mctx.handle, spec.ref(mctx), d(K), n)
        assert rc < 0 and "product" in L.last_error() and "multi-GPU" in L.last_error()
    finally:
        mctx.close()
