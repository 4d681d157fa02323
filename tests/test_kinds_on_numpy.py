"""The Cosine and GammaExponential kinds and what the host builds on them (Gabor and spectral-mixture kernels, the
LinearTransform / ARDTransform / SelectTransform steps, MaternKernel, d_transform), without a GPU: the NumPy formulas of
tests/kinds_np.py against the 60-digit table under the error models of tests/kinds_truth.py, the transform steps against their
written formulas and central differences, the expansions of the new constructors, and the host functions over a NumPy double
of the C ABI that knows chains and the two kinds."""
import os
import subprocess

import numpy as np
import pytest

import kinds_np as kd
import kinds_truth as kt
import kprod_np as kn
import np_capi
import stheno_jl_amd as P
from stheno_jl_amd import kernels as KS
from stheno_jl_amd import lib as L
from test_kprod_grad_on_numpy import install_fake
from test_kprod_on_numpy import np_logpdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the formulas against the table -------------------------------------------------------------------------------------
def _within(got, truth, tol):
    return np.flatnonzero(~(np.abs(np.asarray(got) - truth) <= tol))


def test_cosine_formulas_stay_within_the_model():
    g = kt.load()["cosine"]
    k = kd.cosine(g.d2)
    print(f"\nCosine (NumPy): largest error per band (units of 2^-53, fraction of the bound): {kt.cosine_band_maxima(g, k)}")
    bad = kt.cosine_violations(g, k)
    assert bad.size == 0, kt.describe(g, k, bad)
    assert k[0] == 1.0 and np.all(k[np.isinf(g.d2)] == 1.0) and not np.any(np.isnan(k))
    for name, got, truth, tol in (("dk", kd.cosine_dscale(g.d2), g.dk, kt.cosine_dscale_tolerance(g)),
                                  ("kx", kd.cosine_dd2(g.d2), g.kx, kt.cosine_dd2_tolerance(g))):
        bad = _within(got, truth, tol)
        assert bad.size == 0, (name, kt.describe(g, got, bad, truth))
    assert kd.cosine_dd2(np.zeros(1))[0] == -0.5 * np.pi ** 2 and np.all(g.dp == 0.0)
    inf = np.isinf(g.d2)
    assert np.all(kd.cosine_dscale(g.d2)[inf] == 0.0) and np.all(kd.cosine_dd2(g.d2)[inf] == 0.0)
    # the table visits what the model is about: zeros (|k| < 1e-9) and integers up to d = 1e6, both conventions' ends
    assert np.sum(np.abs(g.k) < 1e-9) >= 7 and np.any((g.d >= 1e6) & np.isfinite(g.d) & (g.d < 2e6))
    assert g.d2[0] == 0.0 and np.any((g.d2 > 0) & (g.d2 < 1e-310)) and np.any(inf)


@pytest.mark.parametrize("gamma", kt.GAMMAS)
def test_gammaexp_formulas_stay_within_the_model(gamma):
    g = kt.load()[gamma]
    k = kd.gammaexp(g.d2, gamma)
    print(f"\nGammaExp gamma={gamma} (NumPy): largest error in ulps of the truth per band: {kt.gexp_band_maxima(g, k)}")
    bad = kt.gexp_violations(g, k)
    assert bad.size == 0, kt.describe(g, k, bad)
    assert k[0] == 1.0 and not np.any(np.isnan(k)) and np.all(k[g.must_zero] == 0.0) and np.all(k[np.isinf(g.d2)] == 0.0)
    cols = (("dk", kd.gammaexp_dscale(g.d2, gamma), g.dk, kt.gexp_dscale_tolerance(g)),
            ("kx", kd.gammaexp_dd2(g.d2, gamma), g.kx, kt.gexp_dd2_tolerance(g)),
            ("dp", kd.gammaexp_dparam(g.d2, gamma), g.dp, kt.gexp_dparam_tolerance(g)))
    for name, got, truth, tol in cols:
        bad = _within(got, truth, tol)
        assert bad.size == 0 and not np.any(np.isnan(got)), (name, kt.describe(g, got, bad, truth))
        assert np.all(got[g.must_zero] == 0.0) and got[0] == 0.0
    # the points the table is for: subnormal d2, subnormal k, beyond the underflow, +inf
    tiny = np.finfo(np.float64).tiny
    assert np.any((g.d2 > 0) & (g.d2 < tiny)) and np.any((g.k > 0) & (g.k < tiny)) and g.must_zero.sum() >= 10


def test_gammaexp_anchors_of_the_convention():
    """gamma = 1 is ExponentialKernel, gamma = 2 is SEKernel o ScaleTransform(sqrt 2)"""
    d2 = np.random.default_rng(3).uniform(0.0, 30.0, 200)
    assert np.all(np.abs(kd.gammaexp(d2, 1.0) - np.exp(-np.sqrt(d2))) <= 4 * np.spacing(np.exp(-np.sqrt(d2))) * (1 + np.sqrt(d2)))
    assert np.all(np.abs(kd.gammaexp(d2, 2.0) - np.exp(-0.5 * (2.0 * d2))) <= 4 * np.spacing(np.exp(-d2)) * (1 + d2))


# ---- 2. the transform steps ------------------------------------------------------------------------------------------------
def test_apply_chain_against_the_written_formulas():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((3, 5))
    A = rng.standard_normal((2, 3))
    v = np.array([0.5, 2.0, -1.5])
    assert np.array_equal(KS.apply_chain((P.LinearTransform(A).step(),), X), A @ X)
    assert np.array_equal(KS.apply_chain((P.ARDTransform(v).step(),), X), v[:, None] * X)
    assert np.array_equal(KS.apply_chain((P.SelectTransform([2, 0]).step(),), X), X[[2, 0]])
    chain = (P.SelectTransform([2, 0]).step(), P.ARDTransform([3.0, 0.25]).step(), P.LinearTransform(A[:, :2]).step(), ("scale", 1.5))
    assert np.allclose(KS.apply_chain(chain, X), 1.5 * (A[:, :2] @ (np.array([3.0, 0.25])[:, None] * X[[2, 0]])), rtol=1e-15)
    with pytest.raises(ValueError, match="LinearTransform"):
        KS.apply_chain((P.LinearTransform(A).step(),), X[:2])
    with pytest.raises(ValueError, match="ARDTransform"):
        KS.apply_chain((P.ARDTransform(v).step(),), X[:2])


def test_chain_vjp_and_transform_cotangents_match_central_differences():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((3, 6))
    A, v, idx = rng.standard_normal((2, 2)), np.array([0.7, -1.3]), [2, 0]

    def chain(A, v):
        return (P.SelectTransform(idx).step(), P.ARDTransform(v).step(), P.LinearTransform(A).step(), ("scale", 1.5),
                ("sincos", 0.8))

    W = rng.standard_normal((4, 6))
    value = lambda X, A, v: float(np.sum(W * KS.apply_chain(chain(A, v), X)))      # noqa: E731
    found = []
    gX = KS.chain_vjp(chain(A, v), X, W, found)
    assert len(found) == 2 and found[0].shape == (2,) and found[1].shape == (2, 2)       # chain order: ard, linear
    h = 1e-6

    def fd(arr, f):
        out = np.zeros(arr.shape)
        for i in np.ndindex(arr.shape):
            p, m = arr.copy(), arr.copy()
            p[i] += h
            m[i] -= h
            out[i] = (f(p) - f(m)) / (2 * h)
        return out

    assert np.allclose(gX, fd(X, lambda Z: value(Z, A, v)), atol=1e-8)
    assert np.allclose(found[1], fd(A, lambda B: value(X, B, v)), atol=1e-8)
    assert np.allclose(found[0], fd(v, lambda u: value(X, A, u)), atol=1e-8)
    assert np.all(gX[1] == 0.0)                                # the coordinate SelectTransform drops
    assert np.array_equal(KS.chain_vjp(chain(A, v), X, W), gX)      # (the list is optional)


def test_push_gives_equal_chains_for_equal_maps():
    A = np.array([[1.0, 2.0], [0.5, -1.0]])
    k = P.SEKernel()
    same = [(k @ P.LinearTransform(A)).leaf_products(), (k @ P.LinearTransform(A.copy(order="F"))).leaf_products(),
            (k @ P.LinearTransform([[1, 2], [0.5, -1]])).leaf_products()]
    assert same[0] == same[1] == same[2] and hash(same[0][0][1][0][2]) == hash(same[2][0][1][0][2])
    assert (k @ P.ARDTransform([2, 3])).leaf_products() == (k @ P.ARDTransform(np.array([2.0, 3.0]))).leaf_products()
    assert (k @ P.SelectTransform([0, 2])).leaf_products() == (k @ P.SelectTransform(np.array([0, 2]))).leaf_products() == \
        (k @ P.SelectTransform((0, 2))).leaf_products()
    assert (k @ P.LinearTransform(A)).leaf_products() != (k @ P.LinearTransform(A.T)).leaf_products()
    # a transform applied outside acts first; scalings next to each other still merge
    (_, [(_, _, ch)]), = ((k @ P.ScaleTransform(2.0)) @ P.ScaleTransform(0.5) @ P.SelectTransform([1])).leaf_products()
    assert ch == (("select", (1,)),)
    (_, [(_, _, ch)]), = ((k @ P.LinearTransform(A)) @ P.ARDTransform([1.0, 2.0])).leaf_products()
    assert [s[0] for s in ch] == ["ard", "linear"]
    # equal views are uploaded once
    X = P.ColVecs(np.asfortranarray(np.random.default_rng(1).standard_normal((2, 5))))
    two = P.gppp(lambda GP: {"f": GP(P.SEKernel() @ P.LinearTransform(A) * (P.CosineKernel() @ P.LinearTransform(A.copy())))})
    spec, _, _ = P.build_spec(two, P.GPPPInput("f", X))
    assert len(spec.inputs) == 1 and spec.n_terms == 2
    for bad in (lambda: P.LinearTransform([1.0, 2.0]), lambda: P.ARDTransform([[1.0]]), lambda: P.SelectTransform([-1]),
                lambda: P.SelectTransform([0.5]), lambda: P.SelectTransform([])):
        with pytest.raises(ValueError):
            bad()


# ---- 3. the constructors ---------------------------------------------------------------------------------------------------
def test_kernel_classes_and_their_leaves():
    assert (L.COSINE, L.GAMMAEXP) == (16, 17)
    assert P.CosineKernel().leaf_products() == [(1.0, [(16, 0.0, ())])]
    assert P.GammaExponentialKernel().leaf_products() == [(1.0, [(17, 2.0, ())])]
    assert (0.5 * P.with_lengthscale(P.GammaExponentialKernel(0.7), 2.0)).leaf_products() == [(0.5, [(17, 0.7, (("scale", 0.5),))])]
    for gamma in (0.0, -1.0, 2.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma"):
            P.GammaExponentialKernel(gamma)


def test_matern_kernel_maps_to_the_three_kinds_and_refuses_the_rest():
    assert [P.MaternKernel(nu).leaf_terms()[0][0] for nu in (0.5, 1.5, 2.5)] == [L.MATERN12, L.MATERN32, L.MATERN52]
    assert isinstance(P.MaternKernel(), P.Matern32Kernel) and isinstance(P.MaternKernel(nu=1 / 2), P.Matern12Kernel)
    for nu in (1.0, 3.5, 0.0, float("inf")):
        with pytest.raises(NotImplementedError, match="Matern"):
            P.MaternKernel(nu)


def test_gaborkernel_leaves():
    assert P.gaborkernel().leaf_products() == [(1.0, [(L.SE, 0.0, ()), (L.COSINE, 0.0, ())])]
    got = P.gaborkernel(sqexponential_transform=P.ScaleTransform(2.0), cosine_transform=P.ARDTransform([1.0, 3.0])).leaf_products()
    assert got == [(1.0, [(L.SE, 0.0, (("scale", 2.0),)), (L.COSINE, 0.0, (("ard", (1.0, 3.0)),))])]
    assert (3.0 * P.gaborkernel(cosine_transform=P.ScaleTransform(0.5))).leaf_products() == \
        [(3.0, [(L.SE, 0.0, ()), (L.COSINE, 0.0, (("scale", 0.5),))])]


def _sm_args(D, Q, seed, product=False):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.5, (D, Q) if product else Q), rng.uniform(0.3, 1.2, (D, Q)), rng.uniform(0.1, 0.9, (D, Q)))


def test_spectral_mixture_kernel_leaves():
    al, ga, om = _sm_args(2, 3, 6)
    lp = P.spectral_mixture_kernel(al, ga, om).leaf_products()
    assert len(lp) == 3
    for q, (coef, fs) in enumerate(lp):
        assert coef == al[q] and [f[0] for f in fs] == [L.SE, L.COSINE] and [f[1] for f in fs] == [0.0, 0.0]
        assert fs[0][2] == (("linear", (tuple(ga[:, q]),)),) and fs[1][2] == (("linear", (tuple(om[:, q]),)),)
    lp = P.spectral_mixture_kernel(al, ga, om, h=P.Matern32Kernel()).leaf_products()
    assert [fs[0][0] for _, fs in lp] == [L.MATERN32] * 3
    with pytest.raises(ValueError, match="spectral mixture"):
        P.spectral_mixture_kernel(al[:2], ga, om)
    with pytest.raises(ValueError, match="spectral mixture"):
        P.spectral_mixture_kernel(al, ga, om[:1])


def test_spectral_mixture_product_kernel_leaves_and_its_limit():
    al, ga, om = _sm_args(2, 2, 7, product=True)
    lp = P.spectral_mixture_product_kernel(al, ga, om).leaf_products()
    assert len(lp) == 4 and all(len(fs) == 4 for _, fs in lp)
    combos = [(q0, q1) for q0 in range(2) for q1 in range(2)]       # the distribution's order: dimension 0 outermost
    for (q0, q1), (coef, fs) in zip(combos, lp):
        assert coef == al[0, q0] * al[1, q1]
        assert [f[0] for f in fs] == [L.SE, L.COSINE, L.SE, L.COSINE]
        want = [(0, ga[0, q0]), (0, om[0, q0]), (1, ga[1, q1]), (1, om[1, q1])]
        assert [f[2] for f in fs] == [(("select", (d,)), ("linear", ((float(w),),))) for d, w in want]
    # D = 5: chains of 10 factors, beyond the library's 8: refused by the product message before anything is uploaded
    al, ga, om = _sm_args(5, 1, 8, product=True)
    F = P.gppp(lambda GP: {"f": GP(P.spectral_mixture_product_kernel(al, ga, om))})
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(F, P.GPPPInput("f", P.ColVecs(np.zeros((5, 3), order="F"))))


# ---- 4. the header ---------------------------------------------------------------------------------------------------------
def test_header_compiled_as_c_sees_the_two_kinds(tmp_path):
    src = tmp_path / "kinds.c"
    src.write_text('#include <stdio.h>\n#include "sthenomi_kprod.h"\n'
                   "typedef char cosine_is_16[SGP_COSINE == 16 ? 1 : -1];\ntypedef char gammaexp_is_17[SGP_GAMMAEXP == 17 ? 1 : -1];\n"
                   'int main(void) { printf("%d %d %d\\n", SGP_COSINE, SGP_GAMMAEXP, SGP_LINEAR); return 0; }\n')
    exe = str(tmp_path / "kinds")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True).stdout.split() == ["16", "17", "7"]


# ---- 5. the host functions over a NumPy double that knows chains and the two kinds ------------------------------------------
def _dense_with_chains(self):
    """np_capi._Spec.dense for specs with product chains: kinds_np.factor per term, a continuation multiplies the chain"""
    K = np.zeros((self.N, self.M))
    blk = sl = None

    def flush():
        if blk is not None:
            K[sl] += blk

    for (I, J, kind, ri, ci, coef, param, rs, cs) in self.terms:
        k = kd.factor(kind, self.inputs[ri], self.inputs[ci], param)[0]
        if kind & L.KIND_TIMES_PREV:
            blk = blk * k
            continue
        flush()
        sl = (slice(self.roff[I], self.roff[I + 1]), slice(self.coff[J], self.coff[J + 1]))
        blk = coef * k
        if rs is not None:
            blk = rs[:, None] * blk
        if cs is not None:
            blk = blk * cs[None, :]
    flush()
    return K


def _install(monkeypatch):
    ctx = install_fake(monkeypatch)
    monkeypatch.setattr(np_capi._Spec, "dense", _dense_with_chains)
    return ctx


SM = dict(D=2, Q=3, n=(9, 7))


def _sm_theta():
    al, ga, om = _sm_args(SM["D"], SM["Q"], 9)
    return dict(alpha=al, gamma=ga, omega=om, noise=np.array(0.1))


def _sm_model(th):
    return P.gppp(lambda GP: {"f": GP(P.spectral_mixture_kernel(th["alpha"], th["gamma"], th["omega"]))})


def _sm_formula(th, X, Y):
    """k(x, y) = sum_q alpha_q exp(-(gamma_q' t)^2 / 2) cos(pi omega_q' t), t = x - y: the docstring's formula"""
    T = X[:, :, None] - Y[:, None, :]
    out = 0.0
    for q in range(len(th["alpha"])):
        out = out + th["alpha"][q] * np.exp(-0.5 * np.einsum("d,dij->ij", th["gamma"][:, q], T) ** 2) * \
            np.cos(np.pi * np.einsum("d,dij->ij", th["omega"][:, q], T))
    return out


def _sm_data():
    rng = np.random.default_rng(10)
    Xs = [np.asfortranarray(rng.standard_normal((SM["D"], m))) for m in SM["n"]]
    y = rng.standard_normal(sum(SM["n"]))
    return Xs, y, P.BlockData([P.GPPPInput("f", P.ColVecs(X)) for X in Xs])


def test_host_mirror_of_a_spectral_mixture_model(monkeypatch):
    _install(monkeypatch)
    th = _sm_theta()
    Xs, y, x = _sm_data()
    Xall = np.hstack(Xs)
    F = _sm_model(th)
    Kref = _sm_formula(th, Xall, Xall)
    K = P.prior_cov(F, x)
    assert np.max(np.abs(K - Kref)) <= 1e-14 * np.max(np.abs(Kref))
    assert np.max(np.abs(P.prior_var(F, x) - np.diag(Kref))) <= 1e-14
    Kc = P.prior_cov(F, x.X[0], x.X[1])
    assert np.max(np.abs(Kc - _sm_formula(th, Xs[0], Xs[1]))) <= 1e-14 * np.max(np.abs(Kref))
    lp_np = lambda t: np_logpdf(_sm_formula(t, Xall, Xall) + float(t["noise"]) * np.eye(len(y)), y)      # noqa: E731
    assert abs(P.logpdf(F(x, 0.1), y) - lp_np(th)) <= 1e-12 * abs(lp_np(th))

    g = P.logpdf_and_gradient_param(F(x, 0.1), y, inputs=True)
    assert abs(g["logpdf"] - lp_np(th)) <= 1e-12 * abs(lp_np(th))
    recs = g["terms"]
    # three lower block pairs x three chains x two factors; every factor reads through a LinearTransform
    assert len(recs) == 18 and all("d_transform" in r and r["d_transform"].shape == (1, SM["D"]) for r in recs)
    assert all(r["d_param"] == 0.0 for r in recs)
    h = 1e-6

    def fd(name, idx):
        p, m = ({k: v.copy() for k, v in th.items()} for _ in range(2))
        p[name][idx] += h
        m[name][idx] -= h
        return (lp_np(p) - lp_np(m)) / (2 * h)

    near = lambda a, e: abs(a - e) <= 1e-6 * max(1.0, abs(e))      # noqa: E731
    assert near(g["noise"], fd("noise", ()))
    for q in range(SM["Q"]):
        chain_recs = [r for i, r in enumerate(recs) if (i % 6) // 2 == q]
        assert near(sum(r["d_coef"] for r in chain_recs), fd("alpha", q))
        se = next(r for r in chain_recs if r["kind"] == L.SE)
        co = next(r for r in chain_recs if r["kind"] == L.COSINE)
        for d in range(SM["D"]):
            assert near(se["d_transform"][0, d], fd("gamma", (d, q))), (q, d)
            assert near(co["d_transform"][0, d], fd("omega", (d, q))), (q, d)
        # records of one chain share the transform's total: the same array on every block pair
        assert all(np.array_equal(r["d_transform"], se["d_transform"]) for r in chain_recs if r["kind"] == L.SE)
    # the points themselves, through the projections
    for I in range(2):
        for i in (0, SM["n"][I] - 1):
            for d in range(SM["D"]):
                def lp_at(delta):
                    Z = [X.copy() for X in Xs]
                    Z[I][d, i] += delta
                    Za = np.hstack(Z)
                    return np_logpdf(_sm_formula(th, Za, Za) + 0.1 * np.eye(len(y)), y)
                assert near(np.asarray(g["x"][I])[d, i], (lp_at(h) - lp_at(-h)) / (2 * h))


def test_d_transform_of_an_ard_step_and_of_the_elbo(monkeypatch):
    """ARD factors of a GammaExponential x Cosine model: logpdf and the ELBO against central differences of v and gamma"""
    _install(monkeypatch)
    rng = np.random.default_rng(12)
    Xs, y, x = _sm_data()
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((SM["D"], 5)))))
    th = dict(v=np.array([0.8, 1.4]), w=np.array([0.3, 0.2]), gamma=np.array(1.3))

    def model(t):
        k = 1.2 * (P.GammaExponentialKernel(float(t["gamma"])) @ P.ARDTransform(t["v"])) * (P.CosineKernel() @ P.ARDTransform(t["w"]))
        return P.gppp(lambda GP: {"f": GP(k)})

    def lp_np(t):
        return np_logpdf(kn.np_spec_matrix(P.build_spec(model(t), x)[0]) + 0.1 * np.eye(len(y)), y)

    def bound_np(t):
        from test_kprod_grad_on_numpy import np_bound
        return np_bound(model(t), x, z, y)

    h = 1e-6

    def fd(f, name, idx):
        p, m = ({k: v.copy() for k, v in th.items()} for _ in range(2))
        p[name][idx] += h
        m[name][idx] -= h
        return (f(p) - f(m)) / (2 * h)

    near = lambda a, e: abs(a - e) <= 2e-6 * max(1.0, abs(e))      # noqa: E731
    g = P.logpdf_and_gradient_param(model(th)(x, 0.1), y, inputs=True)
    ge_rec = next(r for r in g["terms"] if r["kind"] == L.GAMMAEXP)
    co_rec = next(r for r in g["terms"] if r["kind"] == L.COSINE)
    assert ge_rec["d_transform"].shape == (2,)
    for d in range(2):
        assert near(ge_rec["d_transform"][d], fd(lp_np, "v", d)) and near(co_rec["d_transform"][d], fd(lp_np, "w", d))
    assert near(sum(r["d_param"] for r in g["terms"] if r["kind"] == L.GAMMAEXP), fd(lp_np, "gamma", ()))
    assert all(r["d_param"] == 0.0 for r in g["terms"] if r["kind"] == L.COSINE)
    assert "d_transform" not in P.logpdf_and_gradient_param(model(th)(x, 0.1), y)["terms"][0]      # inputs=False: not formed
    F = model(th)
    ge = P.elbo_and_gradient_param(P.VFE(F(z, 1e-3)), F(x, 0.1), y, inputs=True)
    for kind, name in ((L.GAMMAEXP, "v"), (L.COSINE, "w")):
        tot = sum(next(r for r in ge[key] if r["kind"] == kind)["d_transform"] for key in ("zz_terms", "xz_terms", "xx_terms"))
        for d in range(2):
            assert near(tot[d], fd(bound_np, name, d)), (name, d)
    dgamma = sum(r["d_param"] for key in ("zz_terms", "xz_terms", "xx_terms") for r in ge[key] if r["kind"] == L.GAMMAEXP)
    assert near(dgamma, fd(bound_np, "gamma", ()))
