"""General-nu Matern (SGP_MATERN_NU = 20, GeneralMaternKernel) without a GPU: the NumPy restatement of the device routine
(tests/matern_nu_np.py) against the 60-digit table within HALF the bound of tests/matern_nu_truth.py, its derivatives against
the table and against central differences, the closed forms at nu = 1/2, 3/2, 5/2, the host class and its leaves, a
scikit-learn golden through the flattener and the evaluator, the header as plain C, and the host functions over the NumPy
double of the C ABI."""
import base64
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

import kernel_truth as kt0
import kprod_np as kn
import matern_nu_np as mn
import matern_nu_truth as mt
import np_capi
import stheno_jl_amd as P
from stheno_jl_amd import lib as L
from test_kprod_grad_on_numpy import install_fake
from test_kprod_on_numpy import np_logpdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
wl = P.with_lengthscale


def _atom(kernel):
    return P.atomic(P.GP(kernel), P.GPC())


# ---- 1. the restatement against the table ----------------------------------------------------------------------------------
def test_the_table_holds_the_grid_of_the_error_model():
    grids = mt.load()
    assert tuple(grids) == mt.NUS and len(mt.NUS) == 14
    for nu, g in grids.items():
        assert len(g) == 19 and g.d2[0] == 0.0 and g.k[0] == 1.0 and g.dk[0] == 0.0
        assert np.isinf(g.d2[-1]) and g.t[-1] == 1e160 and g.k[-1] == 0.0
        assert g.must_zero[-2] and g.must_zero[-1] and np.isfinite(g.d2[-2])           # past the underflow, and overflowed
        assert np.any((g.d2 > 0) & (g.d2 < 1e-310))                                   # d = 1e-160: a subnormal square
        xs = g.x[14:17]                                                                # straddling the change of branch
        assert xs[0] < 2.0 <= xs[2] and np.all(np.abs(xs / 2.0 - 1.0) <= 1.01 * 2.0 ** -20)
        assert g.kx[0] == (-nu / (2.0 * (nu - 1.0)) if nu > 1.0 else 0.0)


@pytest.mark.parametrize("nu", mt.NUS)
def test_restatement_stays_within_half_the_bound(nu):
    """k, kx and dk of the float64 restatement within HALF of (A + 4 x + C n) 2^-53 on every grid point (otherwise the model
    is wrong), and the rules at the ends"""
    g = mt.load()[nu]
    k, dk, kx, its = mn.derivs(g.d2, nu, want_iterations=True)
    live = g.k > np.finfo(np.float64).tiny
    print(f"\nMatern nu={nu} (NumPy): largest error in units of 2^-53 of the truth: k {mt.err_units(g, k)[live].max():.1f} "
          f"kx {mt.err_units(g, kx, g.kx)[live].max():.1f} dk {mt.err_units(g, dk, g.dk)[live].max():.1f}; iterations <= {its.max()}")
    bad = mt.violations(g, k, fraction=0.5)
    assert bad.size == 0, mt.describe(g, k, bad)
    for which, got, truth in (("kx", kx, g.kx), ("dk", dk, g.dk)):
        bad = mt.deriv_violations(g, got, which, fraction=0.5)
        assert bad.size == 0 and not np.any(np.isnan(got)), (which, mt.describe(g, got, bad, truth))
    assert k[0] == 1.0 and dk[0] == 0.0 and kx[0] == g.kx[0]
    for got in (k, dk, kx):
        assert np.all(got[g.must_zero] == 0.0) and got[-1] == 0.0
    assert its.max() <= 100                    # the device's caps (30 and 200) are never what ends a loop


@pytest.mark.parametrize("nu", [0.1, 0.3, 0.75, 1.0, 1.25, 3.7, 12.0, 32.0])
def test_derivatives_match_central_differences_of_the_restatement(nu):
    """kx = d k / d (d2) and dk = d k(g x, g y) / dg at g = 1 = 2 d2 kx, by central differences with a relative step of 1e-6
    (error of the difference: 1e-12 relative from the step, 1e-16 / 1e-6 from the values' roundings times the bound's 200)"""
    d = np.array([1e-3, 0.05, 0.3, 1.0, 1.4, 2.5, 6.0])
    d2 = d * d
    h = 1e-6
    k, dk, kx = mn.derivs(d2, nu)
    fd_x = (mn.matern_nu(d2 * (1 + h), nu) - mn.matern_nu(d2 * (1 - h), nu)) / (2 * h * d2)
    fd_g = (mn.matern_nu(d2 * (1 + h) ** 2, nu) - mn.matern_nu(d2 * (1 - h) ** 2, nu)) / (2 * h)
    tol = 1e-7 * np.maximum(np.abs(kx), k / d2)
    assert np.all(np.abs(kx - fd_x) <= tol), (kx, fd_x)
    assert np.all(np.abs(dk - fd_g) <= tol * d2 * 2), (dk, fd_g)
    assert np.all(kx < 0.0) and np.array_equal(dk, 2.0 * d2 * kx)


@pytest.mark.parametrize("nu,name", [(0.5, "matern12"), (1.5, "matern32"), (2.5, "matern52")])
def test_half_integer_orders_agree_with_the_closed_forms(nu, name):
    """on the closed forms' own table (tests/kernel_truth.py): both are within their bounds of one truth, so they differ by at
    most the sum: (6 + 4 l) ulp of the closed form plus (A + 4 x + C n) 2^-53 relative, x = l"""
    g = kt0.load()[name]
    d2 = g.d2[np.isfinite(g.d2)]
    with np.errstate(over="ignore", invalid="ignore"):
        l = kt0.C_OF[name] * np.sqrt(d2)
        closed = {"matern12": 1.0 + 0 * l, "matern32": 1.0 + l, "matern52": 1.0 + l + l * l / 3.0}[name] * np.exp(-l)
        closed = np.where(np.isfinite(closed), closed, 0.0)
    got = mn.matern_nu(d2, nu)
    truth = g.k[np.isfinite(g.d2)]
    tol = kt0.bound_ulps(name, d2, np.spacing(truth)) * np.spacing(truth) + mt.bound_units(nu, l) * mt.EPS * truth + mt.TINY
    tol = np.where(np.isfinite(tol), tol, 0.0)
    bad = np.flatnonzero(~(np.abs(got - closed) <= tol))
    assert bad.size == 0, [(d2[i], got[i], closed[i]) for i in bad[:5]]
    assert got[d2 == 0.0][0] == 1.0 and len(d2) >= 50


# ---- 2. the host class --------------------------------------------------------------------------------------------------------
def test_general_matern_kernel_and_its_leaves():
    assert (L.MATERN_NU, L.MATERN_NU_MAX) == (20, 32.0) and mn.MATERN_NU == L.MATERN_NU
    k = P.GeneralMaternKernel(1.25)
    assert k.nu == 1.25 and k.leaf_terms() == [(20, 1.0, 1.25, ())] and k.leaf_products() == [(1.0, [(20, 1.25, ())])]
    assert (0.5 * k).leaf_products() == [(0.5, [(20, 1.25, ())])]
    assert (0.5 * wl(k, 2.0)).leaf_products() == [(0.5, [(20, 1.25, (("scale", 0.5),))])]
    assert (k @ P.SelectTransform([1])).leaf_products() == [(1.0, [(20, 1.25, (("select", (1,)),))])]
    prod = 2.0 * P.SEKernel() * P.GeneralMaternKernel(0.3) * wl(P.GeneralMaternKernel(32), 3.0)
    assert isinstance(P.SEKernel() * k, P.KernelProduct)
    assert prod.leaf_products() == [(2.0, [(L.SE, 0.0, ()), (20, 0.3, ()), (20, 32.0, (("scale", 1.0 / 3.0),))])]
    with pytest.raises(NotImplementedError, match="product"):
        prod.leaf_terms()
    spec, _, _ = P.build_spec(_atom(prod + 0.1 * k), np.linspace(0, 1, 5))
    assert spec.has_kprod and not spec.f32_supported()
    assert [T.kind for T in spec._terms[:4]] == [L.SE, 20 | L.KIND_TIMES_PREV, 20 | L.KIND_TIMES_PREV, 20]
    assert [T.param for T in spec._terms[1:4]] == [0.3, 32.0, 1.25]
    assert P.GeneralMaternKernel().nu == 1.5


def test_general_matern_kernel_refuses_orders_outside_its_range():
    for nu in (0.0, -1.0, float("nan"), float("inf"), 32.5):
        with pytest.raises(ValueError, match="nu"):
            P.GeneralMaternKernel(nu)
        with pytest.raises(ValueError, match="nu"):
            mn.constants(nu)
    # MaternKernel keeps mapping to the closed forms and refusing the rest; its message names the class to use
    with pytest.raises(NotImplementedError, match="Matern.*GeneralMaternKernel"):
        P.MaternKernel(1.0)
    assert isinstance(P.MaternKernel(2.5), P.Matern52Kernel)


def test_header_compiled_as_c_sees_the_kind_and_the_cap(tmp_path):
    src = tmp_path / "matern_nu.c"
    src.write_text('#include <stdio.h>\n#include "sthenomi_kprod.h"\n'
                   "typedef char matern_nu_is_20[SGP_MATERN_NU == 20 ? 1 : -1];\n"
                   'int main(void) { printf("%d %g %d\\n", SGP_MATERN_NU, SGP_MATERN_NU_MAX, SGP_ABI_VERSION); return 0; }\n')
    exe = str(tmp_path / "matern_nu")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True).stdout.split() == ["20", "32", "1"]


# ---- 3. scikit-learn golden ---------------------------------------------------------------------------------------------------
def load_golden():
    with open(os.path.join(ROOT, "tests", "golden", "sklearn_matern_nu.json")) as fh:
        g = json.load(fh)
    arr = lambda s: np.frombuffer(base64.b64decode(s), dtype="<f8")      # noqa: E731
    n = g["n"]
    models = [dict(m, K=arr(m["K"]).reshape(n, n), mean=arr(m["mean"]), var=arr(m["var"])) for m in g["models"]]
    return arr(g["x"]).reshape(n, 2), arr(g["y"]), arr(g["xs"]).reshape(7, 2), g["noise"], models


def golden_kernel(m):
    return m["variance"] * wl(P.GeneralMaternKernel(m["nu"]), m["length_scale"])


def test_sklearn_golden_through_flattener_and_evaluator(monkeypatch):
    """K, the log marginal likelihood and the predictive mean and variance at 7 points, at the tolerances of the
    sklearn_kprod.json test (1e-13 of the largest entry, 1e-10 of the likelihood; the predictions, which that golden does
    not hold, at the likelihood's 1e-10)"""
    mn.install(monkeypatch)
    X, y, Xs, noise, models = load_golden()
    assert X.shape == (40, 2) and [m["nu"] for m in models] == [0.8, 1.9]
    x, xs = P.ColVecs(np.asfortranarray(X.T)), P.ColVecs(np.asfortranarray(Xs.T))
    for m in models:
        f = _atom(golden_kernel(m))
        K = kn.np_spec_matrix(P.build_spec(f, x)[0])
        assert np.abs(K - m["K"]).max() <= 1e-13 * np.abs(m["K"]).max()
        lml = np_logpdf(K + noise * np.eye(40), y)
        assert abs(lml - m["lml"]) <= 1e-10 * abs(m["lml"]), (lml, m["lml"])
        Ksx = kn.np_spec_matrix(P.build_spec(f, xs, None, x)[0])
        Kss = kn.np_spec_matrix(P.build_spec(f, xs)[0])
        c = scipy.linalg.cho_factor(K + noise * np.eye(40), lower=True)
        mean, var = Ksx @ scipy.linalg.cho_solve(c, y), np.diag(Kss - Ksx @ scipy.linalg.cho_solve(c, Ksx.T))
        assert np.abs(mean - m["mean"]).max() <= 1e-10 * np.abs(m["mean"]).max()
        assert np.abs(var - m["var"]).max() <= 1e-10 * np.abs(m["var"]).max()


# ---- 4. the host functions over the NumPy double --------------------------------------------------------------------------------
def _dense_with_chains(self):
    """np_capi._Spec.dense for specs with product chains, through kprod_np.factor (extended to kind 20 by mn.install)"""
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


def test_host_functions_over_the_numpy_double(monkeypatch):
    """prior_cov, logpdf and the gradient records of 1.3 Matern(0.8) o (1 / 0.7) * SE + 0.4 Matern(3.7): the records against
    central differences of the variance and the length scale, d_param exactly 0"""
    mn.install(monkeypatch)
    install_fake(monkeypatch)
    monkeypatch.setattr(np_capi._Spec, "dense", _dense_with_chains)
    rng = np.random.default_rng(5)
    X = np.asfortranarray(rng.standard_normal((2, 17)))
    y = rng.standard_normal(17)
    x = P.ColVecs(X)

    def model(v=1.3, ell=0.7):
        return _atom(v * wl(P.GeneralMaternKernel(0.8), ell) * P.SEKernel() + 0.4 * P.GeneralMaternKernel(3.7))

    d2 = mn._sq_dists(X, X)
    Kref = 1.3 * mn.matern_nu(d2 / 0.7 ** 2, 0.8) * np.exp(-0.5 * d2) + 0.4 * mn.matern_nu(d2, 3.7)
    assert np.abs(P.prior_cov(model(), x) - Kref).max() <= 1e-14
    lp = lambda **kw: np_logpdf(kn.np_spec_matrix(P.build_spec(model(**kw), x)[0]) + 0.1 * np.eye(17), y)      # noqa: E731
    assert abs(P.logpdf(model()(x, 0.1), y) - lp()) <= 1e-12 * abs(lp())
    g = P.logpdf_and_gradient_param(model()(x, 0.1), y)
    recs = g["terms"]
    assert [r["kind"] for r in recs] == [20, L.SE, 20] and all(r["d_param"] == 0.0 for r in recs)
    h = 1e-6
    near = lambda a, e: abs(a - e) <= 1e-6 * max(1.0, abs(e))      # noqa: E731
    assert near(recs[0]["d_coef"], (lp(v=1.3 + h) - lp(v=1.3 - h)) / (2 * h))
    dl = (lp(ell=0.7 + h) - lp(ell=0.7 - h)) / (2 * h)
    assert near(-recs[0]["d_inscale"] / 0.7, dl)      # d_inscale is d / d log g of the scale g = 1 / l the factor's inputs carry
