"""The NeuralNetwork, FBM and Exponentiated kinds on the host, without a GPU: constructors and their expansions, the limits,
the anchors of the FBM convention, the gradient records of the host functions over a NumPy double of the C ABI that knows the
three kinds (tests/dotkinds_np.py) against central differences, the refusals, and the header's codes."""
import os
import re

import numpy as np
import pytest

import dotkinds_np as dk
import dotkinds_truth as dt
import kprod_np as kn
import np_capi
import stheno_jl_amd as P
from stheno_jl_amd import lib as L
from test_kprod_grad_on_numpy import install_fake, np_bound
from test_kprod_on_numpy import np_logpdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
wl = P.with_lengthscale


def _model(kernel):
    return P.gppp(lambda GP: {"f": GP(kernel)})


def _atom(kernel):
    return P.atomic(P.GP(kernel), P.GPC())


# ---- 1. constructors, encodings, limits ---------------------------------------------------------------------------------------
def test_kernel_classes_and_their_leaves():
    assert (L.NEURALNET, L.FBM, L.EXPONENTIATED) == (24, 25, 26)
    assert P.NeuralNetworkKernel().leaf_products() == [(1.0, [(24, 0.0, ())])]
    assert P.FBMKernel().leaf_products() == [(1.0, [(25, 0.5, ())])]
    assert P.ExponentiatedKernel().leaf_terms() == [(26, 1.0, 0.0, ())]
    assert (0.5 * wl(P.FBMKernel(0.7), 2.0)).leaf_products() == [(0.5, [(25, 0.7, (("scale", 0.5),))])]
    k = 2.0 * (P.NeuralNetworkKernel() * P.SEKernel() + P.ExponentiatedKernel()) @ P.ARDTransform([1.0, 3.0])
    ard = (("ard", (1.0, 3.0)),)
    assert k.leaf_products() == [(2.0, [(24, 0.0, ard), (L.SE, 0.0, ard)]), (2.0, [(26, 0.0, ard)])]
    for t in (P.ScaleTransform(2.0), P.LinearTransform([[1.0, 2.0]]), P.SelectTransform([1])):
        (_, [(kind, h, ch)]), = (P.FBMKernel(0.3) @ t).leaf_products()
        assert (kind, h, ch) == (25, 0.3, (t.step(),))
    for h in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="FBMKernel"):
            P.FBMKernel(h)
    assert P.FBMKernel(1.0).h == 1.0


@pytest.mark.parametrize("name", ["nn", "fbm", "exp"])
def test_the_limits_of_a_chain_are_refused_by_name(name):
    k = {"nn": P.NeuralNetworkKernel, "fbm": lambda: P.FBMKernel(0.5), "exp": P.ExponentiatedKernel}[name]
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(_model(k()), P.GPPPInput("f", P.ColVecs(np.zeros((17, 3), order="F"))))
    nine = k()
    for _ in range(8):
        nine = nine * k()
    with pytest.raises(NotImplementedError, match="product.*limit"):
        P.build_spec(_atom(nine), np.linspace(0, 1, 4))
    five = k() * k() * k() * k() * k()                   # 5 factors x 16 > 64
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(_model(five), P.GPPPInput("f", P.ColVecs(np.zeros((9, 3), order="F"))))
    spec, _, _ = P.build_spec(_model(k() * k() * k() * k()), P.GPPPInput("f", P.ColVecs(np.zeros((16, 3), order="F"))))
    assert spec.has_kprod and spec.n_terms == 4


def test_fbm_at_h_one_is_the_linear_kernel_within_the_model():
    rng = np.random.default_rng(2)
    for D in (1, 3, 16):
        X, Y = rng.standard_normal((D, 40)) * 3.0, rng.standard_normal((D, 30)) * 0.1
        k = dk.derivs(L.FBM, X, Y, 1.0)["k"]
        lin = kn.factor(L.LINEAR, X, Y, 0.0)[0]
        a, b = np.sum(X * X, 0)[:, None], np.sum(Y * Y, 0)[None, :]
        bound = (50.0 + 1.5 * D + 3.5) * dt.EPS * (a + b) + (D + 2) * dt.EPS * (np.abs(X).T @ np.abs(Y))
        assert np.all(np.abs(k - lin) <= bound)


def test_fbm_at_h_half_is_the_wiener_kernel_on_the_half_line():
    x = np.random.default_rng(3).uniform(0.0, 5.0, 50)
    k = dk.derivs(L.FBM, x[None, :], x[None, :], 0.5)["k"]
    assert np.all(np.abs(k - np.minimum(x[:, None], x[None, :])) <= 60.0 * dt.EPS * (x[:, None] + x[None, :]))
    assert np.array_equal(k, k.T)


# ---- 2. the host functions over the double -------------------------------------------------------------------------------------
def _dense_with_chains(self):
    """np_capi._Spec.dense for specs with product chains: kprod_np.factor (as installed) per term"""
    K = np.zeros((self.N, self.M))
    blk = sl = None
    for (I, J, kind, ri, ci, coef, param, rs, cs) in self.terms:
        k = kn.factor(kind, self.inputs[ri], self.inputs[ci], param)[0]
        if kind & L.KIND_TIMES_PREV:
            blk = blk * k
            continue
        if blk is not None:
            K[sl] += blk
        sl = (slice(self.roff[I], self.roff[I + 1]), slice(self.coff[J], self.coff[J + 1]))
        blk = coef * k
        if rs is not None:
            blk = rs[:, None] * blk
        if cs is not None:
            blk = blk * cs[None, :]
    if blk is not None:
        K[sl] += blk
    return K


class _FakeKprod:
    """include/sthenomi_kprod.h on top of the double of its superset: sgp_logpdf_grad_param is sgp_logpdf_grad_param_xs
    without inputs and scales"""

    def __init__(self, grad):
        self.grad = grad

    def sgp_logpdf_grad_param(self, ctx, spec, mean, kind, noise, y, lp, gy, gm, gn, gc, gs, gp):
        return self.grad.sgp_logpdf_grad_param_xs(ctx, spec, mean, kind, noise, y, lp, gy, gm, gn, gc, gs, gp, None, None)


def _install(monkeypatch):
    ctx = install_fake(monkeypatch)
    dk.install(monkeypatch)
    monkeypatch.setattr(np_capi._Spec, "dense", _dense_with_chains)
    ctx.kprod, ctx.is_multi = _FakeKprod(ctx.kprod_grad), False
    return ctx


TH = dict(h=np.array(0.6), l=np.array(1.4), v=np.array([0.8, 1.3]), c=np.array(0.9), c2=np.array(0.3), noise=np.array(0.1))
NS = (9, 7)


def _hyper_model(t):
    k = (float(t["c"]) * P.FBMKernel(float(t["h"])) * wl(P.SEKernel(), float(t["l"])) +
         0.7 * (P.NeuralNetworkKernel() @ P.ARDTransform(t["v"])) + float(t["c2"]) * wl(P.ExponentiatedKernel(), 2.0))
    return _model(k)


def _data():
    rng = np.random.default_rng(10)
    Xs = [np.asfortranarray(rng.standard_normal((2, m))) for m in NS]
    Xs[0][:, 2] = 0.0                               # a point at the origin and an exact duplicate: the zero-base rule
    Xs[1][:, 3] = Xs[0][:, 1]
    return Xs, rng.standard_normal(sum(NS))


def _blockdata(Xs):
    return P.BlockData([P.GPPPInput("f", P.ColVecs(np.asfortranarray(X))) for X in Xs])


def _formula(t, X, Y):
    """the model written out from the definitions (textbook forms: fine at these norms)"""
    s, a, b = X.T @ Y, np.sum(X * X, 0)[:, None], np.sum(Y * Y, 0)[None, :]
    d2 = ((X[:, :, None] - Y[:, None, :]) ** 2).sum(0)
    h, l, v = float(t["h"]), float(t["l"]), t["v"]
    fbm = 0.5 * (dk._pow0(a, h) + dk._pow0(b, h) - dk._pow0(d2, h))
    Xv, Yv = v[:, None] * X, v[:, None] * Y
    sv, av, bv = Xv.T @ Yv, np.sum(Xv * Xv, 0)[:, None], np.sum(Yv * Yv, 0)[None, :]
    return (float(t["c"]) * fbm * np.exp(-0.5 * d2 / (l * l)) + 0.7 * np.arcsin(sv / np.sqrt((1.0 + av) * (1.0 + bv))) +
            float(t["c2"]) * np.exp(s / 4.0))


def _central(f, th, name, idx, h=1e-6):
    p, m = ({k: v.copy() for k, v in th.items()} for _ in range(2))
    p[name][idx] += h
    m[name][idx] -= h
    return (f(p) - f(m)) / (2 * h)


near = lambda a, e: abs(a - e) <= 2e-6 * max(1.0, abs(e))      # noqa: E731


def _hyper_from_records(recs):
    pick = lambda kind: [r for r in recs if r["kind"] == kind]      # noqa: E731
    return dict(h=sum(r["d_param"] for r in pick(L.FBM)), c=sum(r["d_coef"] for r in pick(L.FBM)),
                c2=sum(r["d_coef"] for r in pick(L.EXPONENTIATED)), l=-sum(r["d_inscale"] for r in pick(L.SE)) / float(TH["l"]),
                v=pick(L.NEURALNET)[0].get("d_transform"))


def test_values_and_gradient_records_of_the_host_functions(monkeypatch):
    _install(monkeypatch)
    Xs, y = _data()
    x, Xall = _blockdata(Xs), np.hstack(Xs)
    F = _hyper_model(TH)
    Kref = _formula(TH, Xall, Xall)
    assert np.max(np.abs(P.prior_cov(F, x) - Kref)) <= 1e-13 * np.max(np.abs(Kref))
    assert np.max(np.abs(P.prior_var(F, x) - np.diag(Kref))) <= 1e-13 * np.max(np.abs(Kref))
    lp_np = lambda t: np_logpdf(_formula(t, Xall, Xall) + float(t["noise"]) * np.eye(len(y)), y)      # noqa: E731
    assert abs(P.logpdf(F(x, 0.1), y) - lp_np(TH)) <= 1e-11 * abs(lp_np(TH))

    g0 = P.logpdf_and_gradient(F(x, 0.1), y)                    # the param output of sgp_logpdf_grad_param
    g = P.logpdf_and_gradient_param(F(x, 0.1), y, inputs=True)
    for rec_set in (g0["terms"], g["terms"]):
        got = _hyper_from_records(rec_set)
        for name in ("h", "c", "c2", "l"):
            assert near(got[name], _central(lp_np, TH, name, ())), name
        assert all(r["d_param"] == 0.0 for r in rec_set if r["kind"] in (L.NEURALNET, L.EXPONENTIATED))
    assert near(g["noise"], _central(lp_np, TH, "noise", ()))
    v = _hyper_from_records(g["terms"])["v"]
    for d in range(2):
        assert near(v[d], _central(lp_np, TH, "v", d))
    step = 1e-6
    for I in range(2):
        for i in (0, 1, 2, NS[I] - 1):
            for d in range(2):
                def lp_at(delta):
                    Z = [X.copy() for X in Xs]
                    Z[I][d, i] += delta
                    Za = np.hstack(Z)
                    return np_logpdf(_formula(TH, Za, Za) + 0.1 * np.eye(len(y)), y)
                if I == 0 and i == 2:
                    continue          # the origin: FBM(0.6)'s derivative does not exist there (the library's subgradient is 0)
                assert near(np.asarray(g["x"][I])[d, i], (lp_at(step) - lp_at(-step)) / (2 * step)), (I, i, d)
    assert np.all(np.isfinite(np.asarray(g["x"][0])))


def test_elbo_records_match_central_differences(monkeypatch):
    _install(monkeypatch)
    Xs, y = _data()
    x = _blockdata(Xs)
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(np.random.default_rng(12).standard_normal((2, 5)))))
    bound = lambda t: np_bound(_hyper_model(t), x, z, y)      # noqa: E731
    F = _hyper_model(TH)
    ge = P.elbo_and_gradient_param(P.VFE(F(z, 1e-3)), F(x, 0.1), y, inputs=True)
    parts = [_hyper_from_records(ge[key]) for key in ("zz_terms", "xz_terms", "xx_terms")]
    for name in ("h", "c", "c2", "l"):
        assert near(sum(p[name] for p in parts), _central(bound, TH, name, ())), name
    v = sum(p["v"] for p in parts)
    for d in range(2):
        assert near(v[d], _central(bound, TH, "v", d))


def test_the_dtype_generic_restatement_agrees_with_the_mirror_in_float64(monkeypatch):
    """tests/dotkinds_grad_truth.py run in float64 against the NumPy evaluator (two statements of the same definitions, the
    second in the library's formulation): matrix, term contractions and input gradients of a chain of all three kinds"""
    import dotkinds_grad_truth as DG
    import kprod_grad_np as kg
    import kprod_grad_truth as KT
    dk.install(monkeypatch)
    k = 0.7 * wl(P.NeuralNetworkKernel(), 1.1) * P.FBMKernel(0.6) * wl(P.ExponentiatedKernel(), 2.0) + 0.3 * P.FBMKernel(0.3) * P.LinearKernel(0.2)
    Xs, _ = _data()
    spec = P.build_spec(_model(k), _blockdata(Xs))[0]
    S = KT.read_spec(spec)
    K = kn.np_spec_matrix(spec)
    assert np.max(np.abs(DG.dense(S, np.float64) - K)) <= 1e-13 * np.max(np.abs(K))
    G = np.random.default_rng(5).standard_normal(K.shape)
    G = G + G.T
    R = DG.contract(S, G, np.float64, inputs=True)
    for got, want in zip((R["d_coef"], R["d_inscale"], R["d_param"]), kn.np_contract(spec, G)):
        assert np.max(np.abs(got - want)) <= 1e-11 * max(1.0, np.max(np.abs(want)))
    ev = kg.np_input_grads(spec, G)
    for a, e in zip(R["gx"], ev["row"]):
        assert np.max(np.abs(a - 2.0 * e)) <= 1e-11 * max(1.0, np.max(np.abs(e)))
    assert DG.FLOORS == {fam: float(np.median(v)) for fam, v in DG.MEASURED_FLOAT64.items()} and len(DG.CASES) == 11


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nn", "fbm", "exp"])
def test_host_refuses_what_the_library_does_not_carry_before_any_call(name):
    """each raises NotImplementedError naming "product" on the host, before the library is reached (no GPU here)"""
    k = {"nn": P.NeuralNetworkKernel(), "fbm": P.FBMKernel(0.5), "exp": P.ExponentiatedKernel()}[name]
    x = np.linspace(0.1, 1.0, 4)
    f = _atom(k)
    fx = f(x, 0.1)
    y = np.zeros(4)
    for kw in (dict(inputs=True), dict(scales=True)):
        with pytest.raises(NotImplementedError, match="product"):
            P.logpdf_and_gradient(fx, y, **kw)
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_and_gradient_batch([fx], [y])
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_and_gradient_pool([fx], [y])
    with pytest.raises(NotImplementedError, match="product"):
        P.elbo_and_gradient(P.VFE(f(np.array([0.2, 0.7]))), fx, y)
    with pytest.raises(NotImplementedError, match="product"):
        P.logpdf_f32(f(x.astype(np.float32), 0.1), y.astype(np.float32))
    F = P.gppp(lambda GP: (lambda g: {"g": g, "s": P.stencil(g, np.zeros((1, 2)), [1.0, -1.0])})(GP(k)))
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(F, P.GPPPInput("s", np.linspace(0, 1, 4)))
    Fc = P.gppp(lambda GP: (lambda g: {"g": g, "f": P.patch_convolve(g, patch_shape=(3, 3))})(GP(k)))
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(Fc, P.GPPPInput("f", P.ImageVector(np.zeros((5, 5, 2)))))


def test_prediction_gradients_refuse_the_kinds(monkeypatch):
    _install(monkeypatch)
    f = _atom(P.NeuralNetworkKernel())
    x = np.linspace(0.1, 1.0, 6)
    post = P.posterior(f(x, 0.1), np.sin(x))
    with pytest.raises(NotImplementedError, match="product"):
        P.mean_and_var_and_gradient(post(x[:3]))


# ---- 4. the header ---------------------------------------------------------------------------------------------------------------
def test_header_codes_are_the_host_constants():
    src = open(os.path.join(ROOT, "include", "sthenomi.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(SGP_[A-Z0-9_]+) = (\d+)", src)}
    assert (codes["SGP_NEURALNET"], codes["SGP_FBM"], codes["SGP_EXPONENTIATED"]) == (L.NEURALNET, L.FBM, L.EXPONENTIATED) == (24, 25, 26)
    kinds = sorted(v for k, v in codes.items() if not k.startswith("SGP_NOISE") and k != "SGP_ABI_VERSION")
    assert kinds == [0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 20, 24, 25, 26]
    shim = open(os.path.join(ROOT, "julia", "SthenoMI355X.jl"), encoding="utf-8").read()
    for name, code in (("NeuralNetworkKernel", 24), ("FBMKernel", 25), ("ExponentiatedKernel", 26)):
        assert re.search(r"leaf\(\w*::%s\) = \[\(%d," % (name, code), shim), name
