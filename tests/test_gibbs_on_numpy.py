"""GibbsKernel through the host mirror, on the NumPy double (tests/gibbs_np.py): no GPU.

The reference is the formula of include/sthenomi.h written directly in long double; the gradients are held to central
differences of the mirror's own logpdf (step 2^-14: truncation ~ h^2, rounding ~ eps / h, both below the 1e-6 asked)."""
import numpy as np
import pytest

import gibbs_np
import stheno_jl_amd as S
from stheno_jl_amd import lib as L

LD = np.longdouble


def gibbs_ld(X, Y, p):
    """c^(p/2) exp(-s / q) for points (location rows, then the lengthscale row) in long double"""
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD)
    s = ((X[:-1, :, None] - Y[:-1, None, :]) ** 2).sum(0)
    lx, ly = X[-1][:, None], Y[-1][None, :]
    q = lx * lx + ly * ly
    return (2 * lx * ly / q) ** (LD(p) / 2) * np.exp(-s / q)


def ell(a, b):
    return lambda X: a + b * (X * X).sum(0)


def _points(D, n, seed):
    return np.asfortranarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (D, n)))


@pytest.mark.parametrize("D,p", [(1, 1), (2, 2), (4, 1), (15, 16)])
def test_formula_and_flattened_cov(monkeypatch, D, p):
    gibbs_np.install(monkeypatch)
    X = _points(D, 9, D)
    X[:, 3] = X[:, 2]                                  # a coincident pair: exactly 1
    f = S.atomic(S.GP(0.5 * S.GibbsKernel(ell(0.3, 0.2), power=p) + S.SEKernel()), S.GPC())
    spec, _, _ = S.build_spec(f, S.ColVecs(X))
    assert spec.has_gibbs and not spec.has_kprod and not spec.has_deriv and not spec.f32_supported()
    Z = np.vstack([X, ell(0.3, 0.2)(X)])
    assert [(int(t.kind), t.param) for t in spec._terms] == [(L.GIBBS, float(p)), (L.SE, 0.0)]
    assert np.array_equal(spec.inputs[spec._terms[0].row_input], Z)
    ref = 0.5 * gibbs_ld(Z, Z, p) + np.exp(-((X[:, :, None] - X[:, None, :]).astype(LD) ** 2).sum(0) / 2)
    K = S.prior_cov(f, S.ColVecs(X))
    assert np.max(np.abs(K - ref)) <= 64 * 2.0 ** -53 and K[2, 3] == 1.5
    assert np.array_equal(S.prior_var(f, S.ColVecs(X)), np.diag(K))


def test_lengthscale_gradient_against_central_differences(monkeypatch):
    gibbs_np.install(monkeypatch)
    X, y = _points(2, 12, 7), np.random.default_rng(8).standard_normal(12)

    def fx_of(a, b, g=1.0, Z=X):
        l = ell(a, b)                                     # one callable: both terms read one view of the points
        k = 0.8 * (S.GibbsKernel(l, power=2) @ S.ScaleTransform(g)) + 0.3 * S.GibbsKernel(l)
        return S.atomic(S.GP(k), S.GPC())(S.ColVecs(Z), 0.1)

    a, b, h = 0.4, 0.25, 2.0 ** -14
    rec = S.logpdf_and_gradient(fx_of(a, b), y, inputs=True)
    gib = [r for r in rec["terms"] if r["kind"] == L.GIBBS]
    assert len(gib) == 2 and all(r["d_lengthscale"][0].shape == (12,) for r in gib)
    dl = gib[0]["d_lengthscale"][0]                   # both terms read one view: one and the same array
    assert gib[1]["row_input"] == gib[0]["row_input"] and np.array_equal(gib[1]["d_lengthscale"][0], dl)
    near = lambda got, want: abs(got - want) <= 1e-6 * max(1.0, abs(want))      # noqa: E731
    lp = lambda *th: S.logpdf(fx_of(*th), y)                                    # noqa: E731
    assert near(dl.sum(), (lp(a + h, b) - lp(a - h, b)) / (2 * h))
    assert near((dl * (X * X).sum(0)).sum(), (lp(a, b + h) - lp(a, b - h)) / (2 * h))
    # d_inscale: the location coordinates scaled, l held as evaluated -- with l = const the ScaleTransform does exactly that
    rec_c = S.logpdf_and_gradient(fx_of(a, 0.0), y)
    want = (lp(a, 0.0, 1 + h) - lp(a, 0.0, 1 - h)) / (2 * h)
    assert near(rec_c["terms"][0]["d_inscale"], want)
    # x: the partial derivative with l held fixed; the total derivative adds d_lengthscale * grad l
    Xp, Xm = X.copy(), X.copy()
    Xp[1, 5] += h
    Xm[1, 5] -= h
    total = (S.logpdf(fx_of(a, b, Z=Xp), y) - S.logpdf(fx_of(a, b, Z=Xm), y)) / (2 * h)
    assert near(rec["x"][0][1, 5] + dl[5] * 2 * b * X[1, 5], total)


def test_host_refusals_name_gibbs(monkeypatch):
    gibbs_np.install(monkeypatch)
    x = S.ColVecs(_points(1, 6, 3))
    gk = S.GibbsKernel(ell(0.3, 0.2))
    f = S.atomic(S.GP(gk), S.GPC())
    fx, y = f(x, 0.1), np.ones(6)
    with pytest.raises(NotImplementedError, match="Gibbs"):
        (gk * S.SEKernel()).leaf_products()
    with pytest.raises(NotImplementedError, match="Gibbs"):
        S.build_spec(S.derivative(f), x)
    for call in (lambda: S.logpdf_and_gradient(fx, y, scales=True), lambda: S.logpdf_and_gradient_param(fx, y),
                 lambda: S.logpdf_and_gradient_conv(fx, y), lambda: S.logpdf_and_gradient_stencil(fx, y),
                 lambda: S.elbo_and_gradient(S.VFE(f(x, 1e-6)), fx, y), lambda: S.logpdf_f32(fx, y),
                 lambda: S.logpdf_and_gradient(S.atomic(S.GP(gk + S.RationalQuadraticKernel()), S.GPC())(x, 0.1), y)):
        with pytest.raises(NotImplementedError, match="Gibbs"):
            call()
    with pytest.raises(ValueError, match="Gibbs"):
        S.build_spec(S.atomic(S.GP(S.GibbsKernel(lambda X: X[0])), S.GPC()), x)      # not positive
    with pytest.raises(ValueError, match="Gibbs"):
        S.GibbsKernel(ell(1.0, 0.0), power=17)
