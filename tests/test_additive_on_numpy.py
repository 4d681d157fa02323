"""AdditiveKernel on the host, no GPU: what build_spec makes of it, the float64 restatement of csrc/additive_eval.h against the
long-double formula within the bound the device is held to (tests/additive_ref.py), and the host's refusals, which are raised
before any library call (tests/np_capi.py stands in for the library and does not know the kinds)."""
from math import comb

import numpy as np
import pytest

import additive_ref as R
import np_capi
import stheno_jl_amd as S
from stheno_jl_amd import lib as L


def test_additive_kernel_flattens_to_one_group_per_pair(monkeypatch):
    np_capi.install(monkeypatch)
    X = R.points(4, 9, 1)
    k = S.additive_kernel(S.Matern32Kernel(), [0.5, 0.25, 0.125]) @ S.ARDTransform([1.0, 2.0, 0.5, 4.0]) + 0.3 * S.SEKernel()
    f = S.atomic(S.GP(k), S.GPC())
    spec, _, _ = S.build_spec(f, S.ColVecs(X))
    assert spec.has_additive and not spec.has_kprod and not spec.has_gibbs and not spec.f32_supported()
    assert [(int(t.kind), t.coef, t.param) for t in spec._terms] == [(L.ADDITIVE_MATERN32, 0.5, 1.0), (L.ADDITIVE_MATERN32, 0.25, 2.0),
                                                                     (L.ADDITIVE_MATERN32, 0.125, 3.0), (L.SE, 0.3, 0.0)]
    views = {(t.row_input, t.col_input) for t in spec._terms[:3]}      # one view of the points: one launch group
    assert len(views) == 1 and np.array_equal(spec.inputs[spec._terms[0].row_input], np.array([1.0, 2.0, 0.5, 4.0])[:, None] * X)
    assert (L.ADDITIVE_SE, L.ADDITIVE_MATERN12, L.ADDITIVE_MATERN32, L.ADDITIVE_MATERN52) == (48, 49, 50, 51)
    assert S.AdditiveKernel(S.ExponentialKernel(), 2).leaf_terms() == [(L.ADDITIVE_MATERN12, 1.0, 2.0, ())]


@pytest.mark.parametrize("D,r", [(1, 1), (3, 2), (5, 5), (16, 8)])
@pytest.mark.parametrize("base", [L.SE, L.MATERN12, L.MATERN32, L.MATERN52])
def test_float64_restatement_lies_within_the_bound(base, D, r):
    X = R.points(D, 40, D)
    z, _, _, x = R.coords(base, X, X)
    ref = R.esp_brute(z, r) if D <= 5 else R.esp(z, r)[r]
    got = R.esp(R.coords(base, X, X, dtype=np.float64)[0], r)[r]
    assert np.all(np.abs(got - ref) <= R.units(base, x, r) * R.EPS * ref + R.TINY)
    same = np.all(X[:, :, None] == X[:, None, :], axis=0)
    assert same.sum() >= 44 and np.all(got[same] == comb(D, r))
    assert np.all(got[(x <= 700).sum(0) < r] == 0.0)


def test_host_refusals_name_additive(monkeypatch):
    np_capi.install(monkeypatch)
    x = S.ColVecs(R.points(2, 8, 3, far=3.0))
    ak = S.AdditiveKernel(S.SEKernel(), 2)
    f = S.atomic(S.GP(ak), S.GPC())
    fx, y = f(x, 0.1), np.ones(8)
    with pytest.raises(NotImplementedError, match="additive"):
        (ak * S.SEKernel()).leaf_products()
    with pytest.raises(NotImplementedError, match="additive"):
        S.build_spec(S.derivative(f), x)
    for call in (lambda: S.logpdf_and_gradient(fx, y, scales=True), lambda: S.logpdf_and_gradient_param(fx, y),
                 lambda: S.logpdf_and_gradient_conv(fx, y), lambda: S.logpdf_and_gradient_stencil(fx, y),
                 lambda: S.elbo_and_gradient(S.VFE(f(x, 1e-6)), fx, y), lambda: S.logpdf_f32(fx, y),
                 lambda: S.logpdf_and_gradient(S.atomic(S.GP(ak + S.RationalQuadraticKernel()), S.GPC())(x, 0.1), y)):
        with pytest.raises(NotImplementedError, match="additive"):
            call()
    with pytest.raises(TypeError, match="additive"):
        S.AdditiveKernel(S.with_lengthscale(S.SEKernel(), 2.0), 1)
    with pytest.raises(ValueError, match="additive"):
        S.AdditiveKernel(S.SEKernel(), 9)
