"""The Wiener and PiecewisePolynomial kinds and the RationalKernel alias without a GPU: the NumPy mirror of the library's
formulation (tests/wienerpp_np.py) against the 60-digit table under the error models of tests/wienerpp_truth.py, the exactness
rules, the host classes and their encodings, the ValueErrors, and the gradient records of the host functions over a NumPy
double of the C ABI (tests/np_capi.py) against central differences."""
import os
import re

import numpy as np
import pytest

import dotkinds_np as dk
import np_capi
import stheno_jl_amd as P
import wienerpp_np as wn
import wienerpp_truth as wt
from stheno_jl_amd import lib as L
from test_dotkinds_on_numpy import _FakeKprod, _dense_with_chains, _central, near
from test_kprod_grad_on_numpy import install_fake, np_bound
from test_kprod_on_numpy import np_logpdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
wl = P.with_lengthscale


def _model(kernel):
    return P.gppp(lambda GP: {"f": GP(kernel)})


def _atom(kernel):
    return P.atomic(P.GP(kernel), P.GPC())


def code_param(key):
    return (L.WIENER, float(key[1])) if key[0] == "w" else (L.PIECEWISE0 + key[1], float(key[2]))


def mirror(key, g):
    """the mirror's k, dg, dx, dy on the group's pairs (pair i: column i of X with column i of Y)"""
    kind, param = code_param(key)
    out = {"k": np.zeros(g.n), "dg": np.zeros(g.n), "dx": np.zeros((g.D, g.n)), "dy": np.zeros((g.D, g.n))}
    for i in range(g.n):
        x, y = g.X[:, i:i + 1], g.Y[:, i:i + 1]
        r = wn.derivs(kind, x, y, param)
        out["k"][i], out["dg"][i] = np.asarray(r["k"]).reshape(-1)[0], np.asarray(r["dk"]).reshape(-1)[0]
        assert np.all(np.asarray(r["dp"]) == 0.0) and np.all(np.asarray(r["c3"]) == 0.0)
        xv, yv = x[:, :, None], y[:, None, :]
        with np.errstate(over="ignore", invalid="ignore"):
            out["dx"][:, i] = (r["c1"][None] * xv + r["c2"][None] * (xv - yv))[:, 0, 0]
            out["dy"][:, i] = (r["c1y"][None] * yv + r["c2"][None] * (yv - xv))[:, 0, 0]
    return out


def _groups():
    T = wt.load()
    return [(key, D) for key in T for D in T[key] if T[key][D].n]


# ---- 1. the mirror against the table ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,D", _groups(), ids=lambda v: str(v).replace(" ", ""))
def test_mirror_stays_within_the_model(key, D):
    g = wt.load()[key][D]
    got, tol = mirror(key, g), wt.tolerances(key, g)
    print(f"\n{key} D={D} ({g.n} pairs): largest error as a fraction of the bound: " +
          ", ".join(f"{n} {wt.worst(got[n], g.truth[n], tol[n]):.3f}" for n in ("k", "dg", "dx", "dy")))
    for n in ("k", "dg", "dx", "dy"):
        bad = wt.violations(got[n], g.truth[n], tol[n])
        assert bad.size == 0, (key, D, n, bad[:6], np.ravel(got[n])[bad[:6]], np.ravel(g.truth[n])[bad[:6]], np.ravel(tol[n])[bad[:6]])


def test_table_covers_the_grid():
    T = wt.load()
    for i in wt.IS:
        assert sorted(T[("w", i)]) == [1, 2, 3, 8, 16]
        for D, g in T[("w", i)].items():
            cats = set(g.cat)
            want = {"equal", "origin_x", "origin_y", "near", "tie", "nearnorm", "huge3", "tiny"} | ({"huge"} if i <= 2 else set())
            assert want | ({"opposite", "half"} if D == 1 else set()) <= cats, (i, D, cats)
            norms = np.sqrt(np.sum(g.X ** 2, 0))
            assert norms.max() >= (0.9e60 if i <= 2 else 0.9e40) and np.all(np.isfinite(g.truth["k"]))
            tie = g.is_cat("tie")
            assert np.array_equal(np.sum(g.X[:, tie] ** 2, 0), np.sum(g.Y[:, tie] ** 2, 0)) and not np.array_equal(g.X[:, tie], g.Y[:, tie])
            if D == 1 and i >= 1:
                assert g.integral.sum() >= 6      # half-line pairs: their truth is the iterated integral
    for D in (1, 2, 3, 8, 16):
        js = {q: sorted(k[2] for k in T if k[0] == "p" and k[1] == q and D in T[k] and T[k][D].n) for q in range(4)}
        for q in range(4):
            assert D // 2 + q + 1 in js[q], (D, q, js)
        if D in (1, 3):
            assert all(js[q][0] == 1 and js[q][-1] == 64 for q in range(4))
        g = T[("p", 0, D // 2 + 1)][D]
        assert {"equal", "origin_x", "near", "r1", "below1", "mid"} <= set(g.cat)
        if D <= 3:
            assert {"below3", "above1", "far", "overflow", "tinyr", "origin_both", "origin_y", "mid9"} <= set(g.cat)
        r1 = g.is_cat("r1")
        assert np.all(np.sum((g.X[:, r1] - g.Y[:, r1]) ** 2, 0) == 1.0)


def test_exactness_rules_of_the_mirror_and_the_table():
    T = wt.load()
    for key in T:
        for D, g in T[key].items():
            if not g.n:
                continue
            got = mirror(key, g)
            assert not any(np.any(np.isnan(v)) for v in got.values()), (key, D)
            eq = g.is_cat("equal")
            org = g.is_cat("origin_x") | g.is_cat("origin_y") | g.is_cat("origin_both")
            if key[0] == "w":
                i = key[1]
                assert np.all(got["k"][org] == 0.0) and np.all(g.truth["k"][org] == 0.0) and np.all(got["dg"][org] == 0.0)
                X = np.sqrt(dk.scalars(g.X[:, eq], g.X[:, eq])[1][:, 0])
                first = [X, X * X * X / 3.0, (X * X * X) * (X * X) / 20.0, (X * X) * (X * X) * ((X * X) * X) / 252.0][i]
                assert np.array_equal(got["k"][eq], first), (i, D)           # d == 0 exactly: the single first term
                # the tie rule: dx + dy of a coincident pair is the true d k(x, x) / dx = (2 i + 1) k x / X^2
                tot = (g.truth["dx"] + g.truth["dy"])[:, eq]
                want = (2 * i + 1) * g.truth["k"][eq][None] * g.X[:, eq] / np.sum(g.X[:, eq] ** 2, 0)[None]
                assert np.all(np.abs(tot - want) <= 1e-14 * np.abs(want))
                assert np.array_equal(g.truth["dx"][:, eq], g.truth["dy"][:, eq])
            else:
                both = eq | g.is_cat("origin_both")
                assert np.all(got["k"][both] == 1.0) and np.all(g.truth["k"][both] == 1.0)
                out = g.is_cat("r1") | g.is_cat("above1") | g.is_cat("far") | g.is_cat("overflow")
                for n in ("k", "dg", "dx", "dy"):
                    assert np.all(got[n][..., out] == 0.0) and np.all(g.truth[n][..., out] == 0.0), (key, D, n)
    # symmetric bit for bit
    rng = np.random.default_rng(4)
    for D in (1, 3, 16):
        X, Y = rng.standard_normal((D, 12)), rng.standard_normal((D, 9)) * 0.3
        for kind, param in [(L.WIENER, i) for i in wt.IS] + [(L.PIECEWISE0 + q, D // 2 + q + 1) for q in range(4)]:
            a, b = wn.derivs(kind, X, Y, param), wn.derivs(kind, Y, X, param)
            assert np.array_equal(a["k"], b["k"].T) and np.array_equal(a["c1"], b["c1y"].T) and np.array_equal(a["c2"], b["c2"].T)


def test_wiener_zero_is_fbm_at_h_half_on_the_half_line_within_the_models():
    x = np.random.default_rng(3).uniform(0.0, 5.0, 50)
    k = wn.derivs(L.WIENER, x[None, :], x[None, :], 0.0)["k"]
    assert np.all(np.abs(k - np.minimum(x[:, None], x[None, :])) <= wt.wiener_rel(0, 1) * k)
    f = dk.derivs(L.FBM, x[None, :], x[None, :], 0.5)["k"]
    assert np.all(np.abs(k - f) <= 60.0 * wt.EPS * (x[:, None] + x[None, :]))


@pytest.mark.parametrize("D", [1, 2, 3, 5])
def test_piecewise_gram_matrices_are_positive_definite_at_their_dimension(D):
    X = np.random.default_rng(20 + D).uniform(0.0, 1.2, (D, 60))
    for q in range(4):
        K = wn.derivs(L.PIECEWISE0 + q, X, X, D // 2 + q + 1)["k"]
        assert np.array_equal(K, K.T) and np.linalg.eigvalsh(K).min() > -1e-12


# ---- 2. host classes, encodings, ValueErrors -----------------------------------------------------------------------------------
def test_kernel_classes_and_their_leaves():
    assert (L.WIENER, L.PIECEWISE0, L.PIECEWISE1, L.PIECEWISE2, L.PIECEWISE3, L.PIECEWISE_J_MAX) == (10, 11, 12, 13, 14, 64)
    for i in range(4):
        assert P.WienerKernel(i).leaf_products() == [(1.0, [(10, float(i), ())])]
    assert P.WienerKernel().leaf_terms() == [(10, 1.0, 0.0, ())]
    assert isinstance(P.WienerKernel(-1), P.WhiteKernel)
    for i in (-2, 4, 0.5, float("nan"), True):
        with pytest.raises(ValueError, match="WienerKernel"):
            P.WienerKernel(i)
    for q in range(4):
        for dim in (1, 2, 3, 8, 16):
            assert P.PiecewisePolynomialKernel(q, dim=dim).leaf_terms() == [(11 + q, 1.0, float(dim // 2 + q + 1), ())]
    assert P.PiecewisePolynomialKernel(dim=3).leaf_terms() == [(11, 1.0, 2.0, ())]
    with pytest.raises(TypeError):
        P.PiecewisePolynomialKernel(1)                       # dim is required
    for q in (-1, 4, 1.5):
        with pytest.raises(ValueError, match="PiecewisePolynomialKernel"):
            P.PiecewisePolynomialKernel(q, dim=2)
    for dim in (0, -1, 2.5, 200):
        with pytest.raises(ValueError, match="PiecewisePolynomialKernel"):
            P.PiecewisePolynomialKernel(0, dim=dim)
    k = 2.0 * (P.WienerKernel(2) * P.SEKernel() + P.PiecewisePolynomialKernel(1, dim=2)) @ P.ARDTransform([1.0, 3.0])
    ard = (("ard", (1.0, 3.0)),)
    assert k.leaf_products() == [(2.0, [(10, 2.0, ard), (L.SE, 0.0, ard)]), (2.0, [(12, 3.0, ard)])]
    assert (0.5 * wl(P.WienerKernel(1), 2.0)).leaf_products() == [(0.5, [(10, 1.0, (("scale", 0.5),))])]


def test_rational_kernel_is_rq_on_points_scaled_by_sqrt_two_to_the_bit():
    a = P.RationalKernel(1.7)
    b = P.RationalQuadraticKernel(1.7) @ P.ScaleTransform(np.sqrt(2.0))
    assert a.leaf_products() == b.leaf_products() == [(1.0, [(L.RQ, 1.7, (("scale", float(np.sqrt(2.0))),))])]
    x = P.GPPPInput("f", P.ColVecs(np.asfortranarray(np.random.default_rng(1).standard_normal((3, 7)))))
    sa, sb = P.build_spec(_model(a), x)[0], P.build_spec(_model(b), x)[0]
    assert sa.n_terms == sb.n_terms == 1 and sa._terms[0].kind == sb._terms[0].kind == L.RQ
    assert sa._terms[0].param == sb._terms[0].param == 1.7
    for u, v in zip(sa.inputs, sb.inputs):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    for al in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="RationalKernel"):
            P.RationalKernel(al)


def test_build_spec_encodes_codes_and_j_and_refuses_a_dimension_beyond_dim():
    X5 = P.GPPPInput("f", P.ColVecs(np.zeros((5, 4), order="F")))
    for q in range(4):
        spec = P.build_spec(_model(P.PiecewisePolynomialKernel(q, dim=5)), X5)[0]
        assert spec.has_kprod and spec.n_terms == 1
        assert (spec._terms[0].kind, spec._terms[0].param) == (11 + q, float(2 + q + 1))
        with pytest.raises(ValueError, match="PiecewisePolynomialKernel.*positive definite"):
            P.build_spec(_model(P.PiecewisePolynomialKernel(q, dim=3)), X5)
        # after its transforms the factor reads 2 coordinates: dim = 2 is enough on 5-dimensional points
        sel = P.PiecewisePolynomialKernel(q, dim=2) @ P.SelectTransform([0, 3])
        assert P.build_spec(_model(sel * P.SEKernel()), X5)[0].n_terms == 2
        with pytest.raises(ValueError, match="PiecewisePolynomialKernel"):
            P.build_spec(_model(P.PiecewisePolynomialKernel(q, dim=1) @ P.SelectTransform([0, 1, 3])), X5)
    spec = P.build_spec(_model(P.WienerKernel(3) * P.PiecewisePolynomialKernel(2, dim=5)), X5)[0]
    assert [(t.kind, t.param) for t in spec._terms[:2]] == [(10, 3.0), (13 | L.KIND_TIMES_PREV, 5.0)]
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(_model(P.WienerKernel(1)), P.GPPPInput("f", P.ColVecs(np.zeros((17, 3), order="F"))))


# ---- 3. the host functions over the double --------------------------------------------------------------------------------------
def _install(monkeypatch):
    ctx = install_fake(monkeypatch)
    wn.install(monkeypatch)
    monkeypatch.setattr(np_capi._Spec, "dense", _dense_with_chains)
    ctx.kprod, ctx.is_multi = _FakeKprod(ctx.kprod_grad), False
    return ctx


TH = dict(l=np.array(1.4), lw=np.array(0.8), c=np.array(0.9), c2=np.array(0.3), al=np.array(1.3), noise=np.array(0.1))
NS = (9, 7)


def _hyper_model(t):
    # (WIENER with i >= 1 is not known to be positive definite beyond the half line: it reads coordinate 0, which is positive)
    k = (float(t["c"]) * wl(P.WienerKernel(1) @ P.SelectTransform([0]), float(t["lw"])) * wl(P.SEKernel(), float(t["l"])) +
         float(t["c2"]) * wl(P.PiecewisePolynomialKernel(2, dim=2), float(t["l"])) * P.RationalKernel(float(t["al"])))
    return _model(k)


def _data():
    rng = np.random.default_rng(10)
    Xs = [np.asfortranarray(rng.uniform(0.1, 1.0, (2, m))) for m in NS]
    Xs[1][:, 3] = Xs[0][:, 1]                       # an exact duplicate across the blocks: the tie rule
    return Xs, rng.standard_normal(sum(NS))


def _blockdata(Xs):
    return P.BlockData([P.GPPPInput("f", P.ColVecs(np.asfortranarray(X))) for X in Xs])


def _formula(t, X, Y):
    """the model written out from the definitions"""
    d2 = ((X[:, :, None] - Y[:, None, :]) ** 2).sum(0)
    l, lw, al = float(t["l"]), float(t["lw"]), float(t["al"])
    A, B = np.abs(X[0])[:, None] / lw, np.abs(Y[0])[None, :] / lw
    m, d = np.minimum(A, B), np.abs(A - B)
    w1 = m ** 3 / 3.0 + m * m * d / 2.0
    r = np.sqrt(d2) / l
    j = 2 // 2 + 2 + 1
    pp = np.maximum(1.0 - r, 0.0) ** (j + 2) * (1.0 + (j + 2) * r + (j * j + 4 * j + 3) / 3.0 * r * r)
    return float(t["c"]) * w1 * np.exp(-0.5 * d2 / (l * l)) + float(t["c2"]) * pp * (1.0 + d2 / al) ** (-al)


def _hyper_from_records(recs):
    pick = lambda kind: [r for r in recs if r["kind"] == kind]      # noqa: E731
    return dict(c=sum(r["d_coef"] for r in pick(L.WIENER)), c2=sum(r["d_coef"] for r in pick(L.PIECEWISE2)),
                lw=-sum(r["d_inscale"] for r in pick(L.WIENER)) / float(TH["lw"]),
                l=-sum(r["d_inscale"] for r in pick(L.SE) + pick(L.PIECEWISE2)) / float(TH["l"]),
                al=sum(r["d_param"] for r in pick(L.RQ)))


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
        for name in ("c", "c2", "lw", "l", "al"):
            assert near(got[name], _central(lp_np, TH, name, ())), name
        assert all(r["d_param"] == 0.0 for r in rec_set if r["kind"] in wn.WPP_KINDS)
    assert near(g["noise"], _central(lp_np, TH, "noise", ()))
    step = 1e-6
    for I in range(2):
        for i in (0, 2, NS[I] - 1):
            for d in range(2):
                def lp_at(delta):
                    Z = [X.copy() for X in Xs]
                    Z[I][d, i] += delta
                    Za = np.hstack(Z)
                    return np_logpdf(_formula(TH, Za, Za) + 0.1 * np.eye(len(y)), y)
                assert near(np.asarray(g["x"][I])[d, i], (lp_at(step) - lp_at(-step)) / (2 * step)), (I, i, d)
    assert np.all(np.isfinite(np.asarray(g["x"][0])))


def test_elbo_records_match_central_differences(monkeypatch):
    _install(monkeypatch)
    Xs, y = _data()
    x = _blockdata(Xs)
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(np.random.default_rng(12).uniform(0.1, 1.0, (2, 5)))))
    bound = lambda t: np_bound(_hyper_model(t), x, z, y)      # noqa: E731
    F = _hyper_model(TH)
    ge = P.elbo_and_gradient_param(P.VFE(F(z, 1e-3)), F(x, 0.1), y, inputs=True, scales=True)
    parts = [_hyper_from_records(ge[key]) for key in ("zz_terms", "xz_terms", "xx_terms")]
    for name in ("c", "c2", "lw", "l", "al"):
        assert near(sum(p[name] for p in parts), _central(bound, TH, name, ())), name
    for key in ("zz_terms", "xz_terms", "xx_terms"):
        assert all(r["d_param"] == 0.0 for r in ge[key] if r["kind"] in wn.WPP_KINDS)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wiener", "pp"])
def test_host_refuses_what_the_library_does_not_carry_before_any_call(name):
    """no new code: the refusals of every product-path kind, each NotImplementedError naming "product" on the host"""
    k = {"wiener": P.WienerKernel(1), "pp": P.PiecewisePolynomialKernel(1, dim=1)}[name]
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
    Fc = P.gppp(lambda GP: (lambda g: {"g": g, "f": P.patch_convolve(g, patch_shape=(3, 3))})(GP(P.WienerKernel(0))))
    with pytest.raises(NotImplementedError, match="product"):
        P.build_spec(Fc, P.GPPPInput("f", P.ImageVector(np.zeros((5, 5, 2)))))


def test_prediction_gradients_refuse_the_kinds(monkeypatch):
    _install(monkeypatch)
    f = _atom(P.WienerKernel(1))
    x = np.linspace(0.1, 1.0, 6)
    post = P.posterior(f(x, 0.1), np.sin(x))
    with pytest.raises(NotImplementedError, match="product"):
        P.mean_and_var_and_gradient(post(x[:3]))


# ---- 5. the headers --------------------------------------------------------------------------------------------------------------
def test_header_codes_are_the_host_constants():
    src = open(os.path.join(ROOT, "include", "sthenomi_kprod.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(SGP_[A-Z0-9_]+) = (\d+)", src)}
    assert codes == {"SGP_WIENER": L.WIENER, "SGP_PIECEWISE0": L.PIECEWISE0, "SGP_PIECEWISE1": L.PIECEWISE1,
                     "SGP_PIECEWISE2": L.PIECEWISE2, "SGP_PIECEWISE3": L.PIECEWISE3}
    assert int(re.search(r"#define SGP_PIECEWISE_J_MAX (\d+)", src).group(1)) == L.PIECEWISE_J_MAX == 64
    assert "8, 9, 15, 18, 19, 21 .. 23 and 27 and above" in src
    shim = open(os.path.join(ROOT, "julia", "SthenoMI355X.jl"), encoding="utf-8").read()
    assert re.search(r"leaf\(::WienerKernel\{I\}\) where \{I\} = \[\(10,", shim)
    assert re.search(r"leaf\(k::PiecewisePolynomialKernel\{D\}\) where \{D\} = \[\(11 \+ D,", shim)
    assert "leaf(k::RationalKernel)" in shim
