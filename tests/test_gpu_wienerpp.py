"""The Wiener and PiecewisePolynomial kinds on the device (csrc/kprod.hip: wiener_eval / wiener_derivs / pp_derivs;
include/sthenomi_kprod.h): values against the 60-digit table (tests/wienerpp_truth.py) with the exactness rules, matrices
against the NumPy evaluator (tests/wienerpp_np.py) under the summed error models, the bit identities of the product path, the
operators downstream of assembly, every gradient family, batch / pool members, and the refusals.  Block layouts (129, 1, 70)
and (257,): tile edges, a one-point block, a partial tile.  Every case has N <= 257.

WIENER with i >= 1 is not known to be positive definite beyond the half line, so wherever a matrix is factored such a factor
reads positive 1-D points (the whole input at D = 1, coordinate 0 through a SelectTransform beyond it) and the noise is 0.1;
tests/test_wienerpp_on_numpy.py does not need this, and the cases here were checked to factor on the evaluator's matrix."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import kinds_np as kd
import kprod_grad_np as kg
import kprod_np as kn
import stheno_jl_amd as P
import wienerpp_np as wn
import wienerpp_truth as wt
from oracle import titsias_dense
from stheno_jl_amd import lib as L
from test_gpu_kprod import _G, _atom, _call, _kernelmatrix_rc, _model, rel
from test_gpu_kprod_grad import _check_against_evaluator, _check_diag, _close
from test_gpu_parity import REL
from test_kprod_grad_on_numpy import titsias
from test_kprod_on_numpy import np_logpdf

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]

LAYOUTS = {"three": (129, 1, 70), "one": (257,)}
wl = P.with_lengthscale
W, PP = P.WienerKernel, P.PiecewisePolynomialKernel


@pytest.fixture(autouse=True)
def _evaluators_know_the_kinds(monkeypatch):
    import matern_nu_np
    matern_nu_np.install(monkeypatch)
    wn.install(monkeypatch)


def _blocks(D, seed, n, positive=True):
    """blocks of one process with an exact duplicate inside a block, one across two blocks, and a point at the origin;
    positive: every coordinate in [0, 1) / sqrt(D) (the half line at D = 1), else standard normal / sqrt(D)"""
    rng = np.random.default_rng(seed)
    draw = (lambda m: rng.uniform(0.0, 1.0, (D, m))) if positive else (lambda m: rng.standard_normal((D, m)))
    Xs = [np.asfortranarray(draw(m) / np.sqrt(D)) for m in n]
    Xs[0][:, 5] = Xs[0][:, 3]
    Xs[0][:, 11] = 0.0
    Xs[-1][:, -1] = Xs[0][:, 7]
    ins = [P.GPPPInput("f", X[0].copy() if D == 1 else P.ColVecs(X)) for X in Xs]
    return P.BlockData(ins), ins


def _w(i, D):
    """WIENER i on the half line: the input itself at D = 1, its first coordinate beyond"""
    return W(i) if D == 1 else W(i) @ P.SelectTransform([0])


# ---- 1. values against the table, and the exactness rules ------------------------------------------------------------------
def _table_groups():
    T = wt.load()
    return [(key, D) for key in T for D in T[key] if T[key][D].n]


def _code_param(key):
    return (L.WIENER, float(key[1])) if key[0] == "w" else (L.PIECEWISE0 + key[1], float(key[2]))


def _cross_matrix(kind, param, X, Y):
    """sgp_kernelmatrix of a lone term between the columns of X and of Y"""
    sp = L.Spec([X.shape[1]], [Y.shape[1]], [np.asfortranarray(X), np.asfortranarray(Y)],
                {(0, 0): [(kind, 0, 1, 1.0, param, None, None)]}, False)
    K = np.zeros((sp.N, sp.M), order="F")
    assert _call(L.load().sgp_kernelmatrix, sp, L.dptr(K), sp.N) == 0, L.last_error()
    return K


@pytest.mark.parametrize("key,D", _table_groups(), ids=lambda v: str(v).replace(" ", ""))
def test_values_against_the_table(key, D):
    """a lone term, no coefficient, on the table's own points: entry (i, i) of the cross matrix IS the device's formula on
    pair i.  Bounds: tests/wienerpp_truth.py; no pair is left out"""
    g = wt.load()[key][D]
    kind, param = _code_param(key)
    K = _cross_matrix(kind, param, g.X, g.Y)
    got, tol = np.diag(K).copy(), wt.tolerances(key, g)["k"]
    print(f"\n{key} D={D}: largest error as a fraction of the bound {wt.worst(got, g.truth['k'], tol):.3f}")
    bad = wt.violations(got, g.truth["k"], tol)
    assert bad.size == 0, (bad[:6], got[bad[:6]], g.truth["k"][bad[:6]], tol[bad[:6]])
    assert not np.any(np.isnan(K))
    assert np.array_equal(_cross_matrix(kind, param, g.Y, g.X), K.T)           # symmetric bit for bit
    eq = g.is_cat("equal")
    org = g.is_cat("origin_x") | g.is_cat("origin_y") | g.is_cat("origin_both")
    Kxx = _cross_matrix(kind, param, g.X[:, eq], g.X[:, eq])
    assert np.array_equal(np.diag(Kxx), got[eq]) and np.array_equal(Kxx, Kxx.T)
    if key[0] == "w":
        assert np.all(got[org] == 0.0)                                         # exactly 0 against the origin
        # on the diagonal d == 0 exactly: the single first term |x|^(2 i + 1) / c_i, 2 i + 1 roundings after the square root's
        X = np.sqrt(np.sum(g.X[:, eq] ** 2, 0))
        first = X ** (2 * key[1] + 1) / (1.0, 3.0, 20.0, 252.0)[key[1]]
        assert np.all(np.abs(got[eq] - first) <= ((2 * key[1] + 1) * wt.eps_r(D) + (2 * key[1] + 4) * wt.EPS) * first)
    else:
        assert np.all(got[eq | g.is_cat("origin_both")] == 1.0)                # exactly 1 at d2 == 0
        out = g.is_cat("r1") | g.is_cat("above1") | g.is_cat("far") | g.is_cat("overflow")
        assert np.all(got[out] == 0.0)                                         # exactly 0 for r >= 1 and an overflowed d2


@pytest.mark.parametrize("D", [1, 3, 16])
def test_exact_zeros_beyond_the_support_and_exact_ones_on_the_diagonal(D):
    rng = np.random.default_rng(90 + D)
    X = np.asfortranarray(rng.standard_normal((D, 130)) * (0.6 / np.sqrt(D)))
    X[:, 7] = X[:, 2]
    d2 = ((X[:, :, None] - X[:, None, :]) ** 2).sum(0)
    far, nearby = d2 > 1.0 + 1e-12, d2 < 1.0 - 1e-12
    assert far.sum() > 100 and nearby.sum() > 100
    for q in range(4):
        K = _cross_matrix(L.PIECEWISE0 + q, float(D // 2 + q + 1), X, X)
        assert np.all(K[far] == 0.0) and np.all(K[nearby] > 0.0) and np.all(np.diag(K) == 1.0) and K[7, 2] == 1.0
        assert np.array_equal(K, K.T)


# ---- 2. matrices and the bit identities --------------------------------------------------------------------------------------
def _chain(nf, D):
    nn = P.NeuralNetworkKernel()
    if nf == 1:
        return 1.3 * wl(W(1), 1.5) + 0.7 * PP(1, dim=D) + 0.5 * wl(W(3), 2.0) + 0.4 * wl(PP(3, dim=D), 1.5) + 0.2 * W(0)
    if nf == 2:     # chains, a plain term and a chain of one: three classes of launch in one pair
        return (1.3 * wl(P.SEKernel(), 1.3) * W(2) + 0.4 * P.Matern52Kernel() + 0.2 * PP(0, dim=D) +
                0.6 * nn * wl(PP(2, dim=D), 2.0))
    if nf == 3:
        return (0.9 * wl(W(1), 0.8) * P.RationalQuadraticKernel(0.7) * P.LinearKernel(0.5) +
                1.1 * P.FBMKernel(0.7) * wl(PP(2, dim=1) @ P.SelectTransform([0]), 2.0) * wl(P.GeneralMaternKernel(0.8), 1.2))
    return 0.8 * (wl(P.SEKernel(), 2.0) * wl(W(0), 0.5) * wl(P.Matern32Kernel(), 2.5) * P.FBMKernel(0.5) *
                  P.RationalQuadraticKernel(1.3) * P.LinearKernel(1.0) * wl(PP(1, dim=D), 3.0) * wl(nn, 0.7))


def _within(K, Kn, tol):
    err = np.abs(K - Kn)
    print(f"    max|K - Kn| = {float(np.max(err)):.3e}   largest fraction of the entry's bound "
          f"{float(np.max(err / np.maximum(tol, 1e-300))):.3f}")
    return bool(np.all(err <= tol))


CASES = [(1, 1, "three"), (1, 2, "one"), (1, 16, "three"), (2, 1, "one"), (2, 3, "three"), (3, 2, "three"), (3, 8, "one"),
         (8, 1, "three"), (8, 8, "three"), (2, 16, "one")]


@pytest.mark.parametrize("nf,D,layout", CASES)
def test_cov_var_and_cross_match_the_evaluator_and_keep_the_bit_identities(nf, D, layout):
    """tolerance per entry: the per-factor model bounds times the other factors' magnitudes, summed over the chains, for the
    two evaluations compared (kinds_np.np_spec_tolerance with wienerpp_np's bounds).  Points of both signs: nothing is
    factored here"""
    n = LAYOUTS[layout]
    F = _model(_chain(nf, D))
    x, ins = _blocks(D, seed=10 * nf + D, n=n, positive=False)
    spec, _, _ = P.build_spec(F, x)
    assert max(len(ts) for _, _, ts in kn.chains(spec)) == nf
    K = P.prior_cov(F, x)
    assert K.shape == (sum(n), sum(n)) and _within(K, kn.np_spec_matrix(spec), kd.np_spec_tolerance(spec))
    assert np.array_equal(K, K.T)                                        # exact symmetry
    assert np.array_equal(P.prior_var(F, x), np.diag(K))                 # var == diag(cov) bit for bit
    assert np.array_equal(P.prior_cov(F, x), K)                          # two calls, same bits
    if len(n) > 1:
        Kc = P.prior_cov(F, ins[0], ins[-1])                             # the rectangular assembly
        assert np.array_equal(Kc, K[:n[0], sum(n[:-1]):])
        cross = P.build_spec(F, ins[0], None, ins[-1])[0]
        assert _within(Kc, kn.np_spec_matrix(cross), kd.np_spec_tolerance(cross))


KINDS = {"w0": lambda: W(0), "w1": lambda: W(1), "w2": lambda: W(2), "w3": lambda: W(3),
         "p0": lambda: PP(0, dim=3), "p1": lambda: PP(1, dim=3), "p2": lambda: PP(2, dim=3), "p3": lambda: PP(3, dim=3)}


@pytest.mark.parametrize("name", sorted(KINDS))
def test_times_constant_one_is_bit_identical(name):
    k = 1.7 * wl(KINDS[name](), 1.6)
    x, ins = _blocks(3, seed=5, n=LAYOUTS["three"], positive=False)
    plain, chained = _model(k), _model(k * P.ConstantKernel(1.0))
    assert P.build_spec(chained, x)[0].n_terms == 2 * P.build_spec(plain, x)[0].n_terms
    assert np.array_equal(P.prior_cov(chained, x), P.prior_cov(plain, x))
    assert np.array_equal(P.prior_var(chained, x), P.prior_var(plain, x))
    assert np.array_equal(P.prior_cov(chained, ins[2], ins[0]), P.prior_cov(plain, ins[2], ins[0]))


def test_products_commute_and_mix_with_the_bessel_and_dot_kinds():
    x, _ = _blocks(3, seed=6, n=LAYOUTS["three"], positive=False)
    a, b, c = wl(W(2), 0.7), PP(1, dim=3), wl(P.NeuralNetworkKernel(), 2.0)
    for p, q in ((a, b), (b, c), (a, c), (a, wl(P.SEKernel(), 1.2))):
        assert np.array_equal(P.prior_cov(_model(p * q), x), P.prior_cov(_model(q * p), x))
    gm = P.GeneralMaternKernel(0.8)
    K = P.prior_cov(_model(a * gm * b), x)
    ref = P.prior_cov(_model(a), x) * P.prior_cov(_model(gm), x) * P.prior_cov(_model(b), x)
    assert np.all(np.abs(K - ref) <= 4.0 * np.spacing(np.abs(ref)))
    assert np.array_equal(P.prior_var(_model(a * gm * b), x), np.diag(K))


def test_rational_kernel_is_rq_on_scaled_points_to_the_bit():
    x, _ = _blocks(3, seed=7, n=LAYOUTS["three"], positive=False)
    a = P.prior_cov(_model(1.3 * P.RationalKernel(0.9)), x)
    b = P.prior_cov(_model(1.3 * (P.RationalQuadraticKernel(0.9) @ P.ScaleTransform(np.sqrt(2.0)))), x)
    assert np.array_equal(a, b)
    spec = P.build_spec(_model(1.3 * P.RationalKernel(0.9)), x)[0]
    Z = np.hstack([np.asarray(v) for v in spec.inputs]) / np.sqrt(2.0)    # the raw points, block after block
    d2 = ((Z[:, :, None] - Z[:, None, :]) ** 2).sum(0)
    assert np.max(np.abs(a - 1.3 * (1.0 + d2 / 0.9) ** -0.9)) <= 1e-13     # (1 + d^2 / alpha)^-alpha, written out


def test_batch_and_pool_members_are_bit_equal_to_their_own_calls():
    rng = np.random.default_rng(8)
    kernels = [1.2 * W(1) * wl(P.SEKernel(), 1.5) + 0.3 * PP(2, dim=1), 0.5 * wl(W(3), 3.0) + 0.7 * wl(PP(0, dim=1), 2.0)]
    for sizes in ((200, 200), (200, 257)):
        mem = [(_atom(k)(np.sort(rng.uniform(0.1, 3, n)), 0.1 + 0.05 * i), rng.standard_normal(n))
               for i, (k, n) in enumerate(zip(kernels, sizes))]
        own = np.array([P.logpdf(fx, y) for fx, y in mem])
        assert np.all(np.isfinite(own))
        assert np.array_equal(P.logpdf_batch([s[0] for s in mem], [s[1] for s in mem]), own)
        assert np.array_equal(P.logpdf_pool([s[0] for s in mem], [s[1] for s in mem]), own)


# ---- 3. operators on the evaluator's matrix ----------------------------------------------------------------------------------
OPERATOR_KERNELS = {"w1": lambda D: 1.3 * _w(1, D), "w3": lambda D: 20.0 * wl(_w(3, D), 0.5),
                    "p0": lambda D: 0.9 * PP(0, dim=D), "p3": lambda D: 0.6 * wl(PP(3, dim=D), 2.0),
                    "mixed": lambda D: 1.1 * wl(P.SEKernel(), 1.2) * _w(2, D) + 0.4 * PP(1, dim=D) * P.FBMKernel(0.5),
                    # a MATERN_NU factor inside a chain of the new kinds: the Bessel branch of the mode-3 instantiations
                    "bessel": lambda D: _bessel_chain(D)}


def _bessel_chain(D):
    return (0.9 * wl(P.NeuralNetworkKernel(), 1.5) * wl(P.GeneralMaternKernel(0.8), 1.2) * _w(1, D) +
            0.3 * wl(P.GeneralMaternKernel(2.3), 1.4) * wl(PP(2, dim=D), 3.0))


@pytest.mark.parametrize("name", sorted(OPERATOR_KERNELS))
@pytest.mark.parametrize("D", [1, 3])
def test_logpdf_rand_posterior_and_update_match_scipy_on_the_evaluators_matrix(name, D):
    """noise 0.1; REL = 1e-8 is what the parity suite asks at cond <= |K| / 0.1"""
    F = _model(OPERATOR_KERNELS[name](D))
    n = LAYOUTS["three"]
    x, ins = _blocks(D, seed=40 + D, n=n)
    N = sum(n)
    y = np.random.default_rng(D).standard_normal(N)
    spec, _, _ = P.build_spec(F, x)
    Cm = kn.np_spec_matrix(spec) + 0.1 * np.eye(N)
    ref = np_logpdf(Cm, y)
    fx = F(x, 0.1)
    assert abs(P.logpdf(fx, y) - ref) <= REL * abs(ref)
    Z = np.asfortranarray(np.random.default_rng(1).standard_normal((N, 3)))
    assert rel(P.rand(None, fx, 3, Z=Z), scipy.linalg.cholesky(Cm, lower=True) @ Z) <= REL
    Xs = np.asfortranarray(np.random.default_rng(2).uniform(0.0, 1.0, (D, 40)) / np.sqrt(D))
    xs = P.GPPPInput("f", Xs[0].copy() if D == 1 else P.ColVecs(Xs))
    Ksx = kn.np_spec_matrix(P.build_spec(F, xs, None, x)[0])
    Kss = kn.np_spec_matrix(P.build_spec(F, xs)[0])
    m, v = P.mean_and_var(P.posterior(fx, y)(xs))
    m_ref, v_ref = Ksx @ np.linalg.solve(Cm, y), np.diag(Kss - Ksx @ np.linalg.solve(Cm, Ksx.T))
    assert rel(m, m_ref) <= REL and rel(v, v_ref) <= REL
    # the posterior of the first two blocks extended with the third is the posterior of all three
    n12 = n[0] + n[1]
    head = P.BlockData(ins[:2])
    post = P.update_posterior(P.posterior(F(head, 0.1), y[:n12]), F(ins[2], 0.1), y[n12:])
    m2, v2 = P.mean_and_var(post(xs))
    assert rel(m2, m_ref) <= REL and rel(v2, v_ref) <= REL


@pytest.mark.parametrize("name", sorted(OPERATOR_KERNELS))
def test_elbo_matches_the_dense_titsias_bound(name):
    F = _model(OPERATOR_KERNELS[name](2))
    n = LAYOUTS["three"]
    x, _ = _blocks(2, seed=50, n=n)
    N, M = sum(n), 24
    y = np.random.default_rng(3).standard_normal(N)
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(np.random.default_rng(4).uniform(0.0, 1.0, (2, M)) / np.sqrt(2.0))))
    val = P.elbo(P.VFE(F(z, 0.1)), F(x, 0.1), y)
    Kzz = kn.np_spec_matrix(P.build_spec(F, z)[0]) + 0.1 * np.eye(M)
    # both sides solve with Kzz + Sigma_z and sum N terms: 8 N eps cond(Kzz + Sigma_z), relative (cond <= (|Kzz| + 0.1) / 0.1)
    tol = 8.0 * N * wt.EPS * np.linalg.cond(Kzz)
    ref = titsias_dense.elbo_dense(kn.np_spec_matrix(P.build_spec(F, x)[0]), kn.np_spec_matrix(P.build_spec(F, x, None, z)[0]),
                                   Kzz, np.zeros(N), y, np.full(N, 0.1))
    print(f"    |elbo - ref| / |ref| = {abs(val - ref) / abs(ref):.3e}   bound {tol:.3e}")
    assert abs(val - ref) <= tol * abs(ref)


# ---- 4. gradients ------------------------------------------------------------------------------------------------------------
def _grad_chain(nf, D):
    """_chain with every WIENER factor of i >= 1 on the half line (the matrix is factored)"""
    nn = P.NeuralNetworkKernel()
    if nf == 1:
        return 1.3 * wl(_w(1, D), 1.5) + 0.7 * PP(1, dim=D) + 0.5 * wl(_w(3, D), 2.0) + 0.4 * wl(PP(3, dim=D), 1.5) + 0.2 * W(0)
    if nf == 2:
        return (1.3 * wl(P.SEKernel(), 1.3) * _w(2, D) + 0.4 * P.Matern52Kernel() + 0.2 * PP(0, dim=D) +
                0.6 * nn * wl(PP(2, dim=D), 2.0))
    if nf == 3:
        return (0.9 * wl(_w(1, D), 0.8) * P.RationalQuadraticKernel(0.7) * P.LinearKernel(0.5) +
                1.1 * P.FBMKernel(0.7) * wl(PP(2, dim=1) @ P.SelectTransform([0]), 2.0) * wl(P.GeneralMaternKernel(0.8), 1.2))
    return _chain(8, D)


GRAD_CASES = [(1, 1, "three"), (1, 16, "one"), (2, 3, "three"), (3, 2, "one"), (8, 8, "three"), (8, 1, "one")]


@pytest.mark.parametrize("nf,D,layout", GRAD_CASES)
def test_parameter_gradient_outputs_match_the_numpy_contraction(nf, D, layout):
    """coef, inscale and param of sgp_logpdf_grad_param against the NumPy contraction of the mirror's formulas; data with exact
    duplicates (the tie rule) and a point at the origin; d / d param of both families is exactly 0"""
    n = LAYOUTS[layout]
    x, _ = _blocks(D, seed=100 + D, n=n)
    y = np.random.default_rng(D).standard_normal(sum(n))
    g = P.logpdf_and_gradient(_model(_grad_chain(nf, D))(x, 0.1), y)
    spec = g["_spec"]
    G, Cm = _G(spec, 0.1, y)
    assert abs(g["logpdf"] - np_logpdf(Cm, y)) <= REL * abs(g["logpdf"])
    nt = spec.n_terms
    for got, want in zip(g["_raw"], kn.np_contract(spec, G)):
        assert np.all(np.isfinite(got)) and _close(got[:nt], want)
    kinds = np.array([spec._terms[t].kind & L.KIND_MASK for t in range(nt)])
    gp = g["_raw"][2][:nt]
    assert np.any(np.isin(kinds, wn.WPP_KINDS)) and np.all(gp[np.isin(kinds, wn.WPP_KINDS)] == 0.0)
    assert all(r["d_param"] == 0.0 for r in g["terms"] if r["kind"] in wn.WPP_KINDS)


@pytest.mark.parametrize("nf,D,layout", GRAD_CASES)
def test_input_gradients_match_the_evaluator(nf, D, layout):
    """sgp_logpdf_grad_param_xs: inputs and row scales; bound of test_gpu_kprod_grad.py's _check_against_evaluator"""
    n = LAYOUTS[layout]
    x, _ = _blocks(D, seed=20 * nf + D, n=n)
    spec, _, _ = P.build_spec(_model(_grad_chain(nf, D)), x)
    assert spec.has_kprod and max(len(ts) for _, _, ts in kn.chains(spec)) == nf
    o, _, _ = _check_against_evaluator(spec, 0.1, np.random.default_rng(nf + D).standard_normal(sum(n)))
    assert all(np.all(np.isfinite(a)) for a in o["gx"])


@pytest.mark.parametrize("D,layout", [(1, "three"), (3, "one"), (8, "three"), (16, "one")])
def test_gradients_of_a_chain_with_a_bessel_factor_match_the_evaluator(D, layout):
    """the MATERN_NU branch of grad_kprod_kernel<., 3> and of grad_kprod_inputs_kernel<., 4> at every DMAX"""
    n = LAYOUTS[layout]
    x, _ = _blocks(D, seed=300 + D, n=n)
    y = np.random.default_rng(D).standard_normal(sum(n))
    g = P.logpdf_and_gradient(_model(_bessel_chain(D))(x, 0.1), y)
    spec = g["_spec"]
    kinds = [spec._terms[t].kind & L.KIND_MASK for t in range(spec.n_terms)]
    assert L.MATERN_NU in kinds and L.WIENER in kinds and L.PIECEWISE2 in kinds
    G, Cm = _G(spec, 0.1, y)
    assert abs(g["logpdf"] - np_logpdf(Cm, y)) <= REL * abs(g["logpdf"])
    for got, want in zip(g["_raw"], kn.np_contract(spec, G)):
        assert np.all(np.isfinite(got)) and _close(got[:spec.n_terms], want)
    o, _, _ = _check_against_evaluator(spec, 0.1, y)
    assert all(np.all(np.isfinite(a)) for a in o["gx"])


@pytest.mark.parametrize("two_views", [True, False])
def test_diagonal_gradients_and_the_tie_rule(two_views):
    """sgp_kernelmatrix_diag_grad_param.  two_views: var(f(a x) + f(b x)), whose cross terms read two different views of x (the
    row view gets d k / d x, the column view d k / d y); else var(f(x)): both views are one array and every entry is a tie
    X == Y, d == 0, where the half-and-half rule must add up to the true d k(x, x) / dx"""
    k = (1.3 * P.SEKernel() * wl(W(2), 1.2) + 0.3 * P.LinearKernel(0.4) * PP(1, dim=3) + 0.2 * wl(W(3), 2.0) +
         0.5 * W(0) * wl(PP(3, dim=3), 2.0) + 0.1 * W(1))
    rng = np.random.default_rng(31)
    Xs = [np.asfortranarray(rng.standard_normal((3, m)) / np.sqrt(3.0)) for m in LAYOUTS["three"]]
    Xs[0][:, 4] = 0.0
    if two_views:
        F = P.gppp(lambda GP: (lambda f: {"f": f, "g": P.stretch(f, 0.7) + P.stretch(f, 1.6)})(GP(k)))
        x = P.BlockData([P.GPPPInput("g", P.ColVecs(X)) for X in Xs])
    else:
        F = _model(k)
        x = P.BlockData([P.GPPPInput("f", P.ColVecs(X)) for X in Xs])
    spec, _, _ = P.build_spec(F, x)
    w = rng.standard_normal(200)
    o, ev = _check_diag(spec, w)
    assert any(np.max(np.abs(e)) > 1e-3 for e in ev["gx"])
    kinds = np.array([spec._terms[t].kind & L.KIND_MASK for t in range(spec.n_terms)])
    assert np.all(o["gp"][:spec.n_terms][np.isin(kinds, wn.WPP_KINDS)] == 0.0)
    if not two_views:
        # without lengthscales every factor reads the one array x, and the gradient is the true derivative of
        # sum_i w_i k(x_i, x_i), written out from W(i)(x, x) = |x|^(2 i + 1) / c_i, PP(x, x) = SE(x, x) = 1:
        #     k(x, x) = 1.3 |x|^5 / 20 + 0.2 |x|^7 / 252 + 0.5 |x| + 0.1 |x|^3 / 3,    d |x|^p / dx = p |x|^(p - 2) x
        k1 = 1.3 * P.SEKernel() * W(2) + 0.2 * W(3) + 0.5 * W(0) * PP(3, dim=3) + 0.1 * W(1)
        s1, _, _ = P.build_spec(_model(k1), x)
        assert len(s1.inputs) == len(Xs)
        o1, _ = _check_diag(s1, w)
        off = 0
        for X, a in zip(Xs, o1["gx"]):
            nr = np.sqrt(np.sum(X * X, 0))
            inv = np.where(nr > 0.0, 1.0 / np.where(nr > 0.0, nr, 1.0), 0.0)          # (d |x| / dx := 0 at the origin)
            want = w[off:off + X.shape[1]][None] * (1.3 * 5.0 * nr ** 3 / 20.0 + 0.2 * 7.0 * nr ** 5 / 252.0 + 0.5 * inv + 0.1 * nr)[None] * X
            assert np.max(np.abs(np.asarray(a) - want)) <= 1e-13 * max(1.0, np.max(np.abs(want)))
            off += X.shape[1]


@pytest.mark.parametrize("name", ["w1", "p3", "mixed", "bessel"])
def test_elbo_gradient_contractions_match_the_evaluator(name):
    """sgp_elbo_grad_param: the value is sgp_elbo's, the term outputs and the input gradients of both sides against the
    evaluator contracting NumPy's own cotangents of the Titsias bound (2e-5: test_gpu_kprod_grad.py's bound for these)"""
    F = _model(OPERATOR_KERNELS[name](2) + 0.5 * wl(P.SEKernel(), 1.1) * PP(1, dim=2))
    n = LAYOUTS["three"]
    x, _ = _blocks(2, seed=60, n=n)
    y = np.random.default_rng(5).standard_normal(sum(n))
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(np.random.default_rng(6).uniform(0.0, 1.0, (2, 24)) / np.sqrt(2.0))))
    g = P.elbo_and_gradient_param(P.VFE(F(z, 0.1)), F(x, 0.1), y, inputs=True, scales=True)
    assert g["elbo"] == P.elbo(P.VFE(F(z, 0.1)), F(x, 0.1), y)
    zz, xz, xx = (g["_specs"][k] for k in ("zz", "xz", "xx"))
    ref, (dKzz, dKxz, _, _) = titsias(kn.np_spec_matrix(zz) + 0.1 * np.eye(24), kn.np_spec_matrix(xz), kg.np_diag(xx), y, 0.1,
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
        kinds = np.array([sp._terms[t].kind & L.KIND_MASK for t in range(sp.n_terms)])
        assert np.all(g["_raw"][key][2][:sp.n_terms][np.isin(kinds, wn.WPP_KINDS)] == 0.0)


def _central(f, th, name, idx, h=1e-5):
    p, m = ({k: v.copy() for k, v in th.items()} for _ in range(2))
    p[name][idx] += h
    m[name][idx] -= h
    return (f(p) - f(m)) / (2 * h)


def test_host_records_match_central_differences_of_the_hyperparameters():
    """lengthscales of a WIENER and a PIECEWISE factor (d_inscale), alpha of RationalKernel (d_param of its RQ term), an ARD
    vector (d_transform), a coefficient and the noise, through logpdf_and_gradient_param; step and tolerance of the same test in
    tests/test_gpu_dotkinds.py.  The lengthscale of PIECEWISE moves entries across r = 1, where k and k' are continuous for
    q >= 1"""
    th = dict(lw=np.array(0.8), l=np.array(1.4), al=np.array(1.3), v=np.array([0.8, 1.3]), c=np.array(0.9), noise=np.array(0.1))

    def model(t):
        return _model(float(t["c"]) * wl(_w(1, 2), float(t["lw"])) * wl(P.SEKernel(), float(t["l"])) +
                      0.7 * (PP(2, dim=2) @ P.ARDTransform(t["v"])) * P.RationalKernel(float(t["al"])))

    x, _ = _blocks(2, seed=70, n=LAYOUTS["three"])
    y = np.random.default_rng(7).standard_normal(200)
    lp = lambda t: P.logpdf(model(t)(x, float(t["noise"])), y)      # noqa: E731
    g = P.logpdf_and_gradient_param(model(th)(x, 0.1), y, inputs=True)
    recs = g["terms"]
    pick = lambda kind: [r for r in recs if r["kind"] == kind]      # noqa: E731
    got = dict(lw=-sum(r["d_inscale"] for r in pick(L.WIENER)) / 0.8, c=sum(r["d_coef"] for r in pick(L.WIENER)),
               l=-sum(r["d_inscale"] for r in pick(L.SE)) / 1.4, al=sum(r["d_param"] for r in pick(L.RQ)),
               v=pick(L.PIECEWISE2)[0]["d_transform"], noise=np.array(g["noise"]))
    assert all(r["d_param"] == 0.0 for r in pick(L.WIENER) + pick(L.PIECEWISE2))
    for name, val in got.items():
        val = np.asarray(val)
        for idx in np.ndindex(val.shape):
            fd = _central(lp, th, name, idx)
            assert abs(val[idx] - fd) <= 1e-6 * max(1.0, abs(fd)), (name, idx, val[idx], fd)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def _raw_spec(terms, D=1, n=8):
    X = np.asfortranarray(np.random.default_rng(12).standard_normal((D, n)))
    return L.Spec([n], [n], [X], {(0, 0): [(k, 0, 0, c, p, None, None) for (k, c, p) in terms]}, True)


def test_unknown_kinds_bad_params_and_the_limits_are_refused_by_name():
    TP = L.KIND_TIMES_PREV
    assert _kernelmatrix_rc(_raw_spec([(L.WIENER, 2.0, 3.0), (L.PIECEWISE2 | TP, 1.0, 64.0), (L.PIECEWISE0, 1.0, 1.0)])) == 0
    assert _kernelmatrix_rc(_raw_spec([(L.WIENER, 1.0, 0.0), (L.PIECEWISE3 | TP, 1.0, 12.0)], D=16)) == 0
    for kind in (8, 9, 15, 18, 19, 21, 22, 23, 27, 255, 9 | TP, 15 | TP, 27 | TP):
        assert _kernelmatrix_rc(_raw_spec([(L.SE, 1.0, 0.0), (kind, 1.0, 1.0)])) < 0, kind
        assert "unknown kernel kind" in L.last_error(), (kind, L.last_error())
    for i in (-1.0, 0.5, 4.0, 1.0000000000000002, float("nan"), float("inf")):
        for terms in ([(L.WIENER, 1.0, i)], [(L.SE, 1.0, 0.0), (L.WIENER | TP, 1.0, i)]):
            rc = _kernelmatrix_rc(_raw_spec(terms))
            assert rc < 0 and "product" in L.last_error() and "SGP_WIENER" in L.last_error() and " i " in L.last_error(), (i, L.last_error())
    for q in range(4):
        for j in (0.0, -1.0, 1.5, 65.0, 1e30, float("nan"), float("inf")):
            for terms in ([(L.PIECEWISE0 + q, 1.0, j)], [(L.SE, 1.0, 0.0), ((L.PIECEWISE0 + q) | TP, 1.0, j)]):
                rc = _kernelmatrix_rc(_raw_spec(terms))
                assert rc < 0 and "product" in L.last_error() and "SGP_PIECEWISE" in L.last_error() and " j " in L.last_error(), (q, j, L.last_error())
    for kind in wn.WPP_KINDS:
        rc = _kernelmatrix_rc(_raw_spec([(kind, 1.0, 1.0)], D=17))
        assert rc < 0 and "product" in L.last_error(), (kind, rc, L.last_error())
        rc = _kernelmatrix_rc(_raw_spec([(kind, 1.0, 1.0)] + [(kind | TP, 1.0, 1.0)] * 8))
        assert rc < 0 and "product" in L.last_error(), (kind, rc, L.last_error())
    sp = _raw_spec([(L.WIENER, 1.0, 0.0)])
    sp._terms[0].reserved = 1
    assert _kernelmatrix_rc(sp) < 0 and "product" in L.last_error()


def test_entry_points_without_a_product_instantiation_refuse_a_wiener_spec():
    n = 16
    x = np.linspace(0.1, 1.0, n)
    f = _atom(P.WienerKernel(1))
    spec, _, _ = P.build_spec(f, x)
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
    # sgp_elbo_grad: the kind in K(z, z) and K(x, z)
    z = np.linspace(0.1, 1.0, 4)
    zz, xz = P.build_spec(f, z)[0], P.build_spec(f, x, None, z)[0]
    gz, gzs, gxz, gxs = np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1)
    rc = lib.sgp_elbo_grad(ctx.handle, zz.ref(ctx), xz.ref(ctx), d(np.ones(n)), d(m), L.NOISE_SCALAR, d(nz), L.NOISE_SCALAR,
                           d(np.array([1e-3])), d(y), d(lp), d(gy), d(gm), d(gn), d(np.zeros(n)), d(np.zeros(1)), d(gz), d(gzs),
                           d(gxz), d(gxs))
    assert refused(rc)
    # sgp_posterior_predict_grad_x: a posterior of the kind exists (the posterior path carries it), its gradient call refuses
    post = P.posterior(f(x, 0.1), np.sin(x))
    xt = np.linspace(0.2, 0.8, 4)
    cross, pss = P.build_spec(f, xt, f, x)[0], P.build_spec(f, xt)[0]
    ms, mo, vo = np.zeros(4), np.zeros(4), np.zeros(4)
    gms = [np.zeros(np.asarray(a).shape, order="F") for a in cross.inputs]
    ptrs = (PD * max(1, len(gms)))(*[d(a) for a in gms])
    rc = ctx.predgrad.sgp_posterior_predict_grad_x(post._ensure(), cross.ref(), pss.ref(), d(ms), d(mo), d(vo), ptrs, None, None)
    assert refused(rc)
    # the host mirror raises before either call
    with pytest.raises(NotImplementedError, match="product"):
        P.elbo_and_gradient(P.VFE(f(x[::4], 1e-3)), f(x, 0.1), y)
    with pytest.raises(NotImplementedError, match="product"):
        P.mean_and_var_and_gradient(post(x[:4]))
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_and_gradient_batch([f(x, 0.1)], [y])
    mctx = L.Context(devices=[0, 0])
    try:
        K = np.zeros((n, n), order="F")
        rc = mctx.lib.sgp_kernelmatrix(mctx.handle, spec.ref(mctx), d(K), n)
        assert rc < 0 and "product" in L.last_error() and "multi-GPU" in L.last_error()
    finally:
        mctx.close()
