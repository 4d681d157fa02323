"""blur(f, variance) through the host mirror, on the NumPy double (tests/blur_np.py): no GPU.

The reference is the formula of include/sthenomi.h written directly in long double, and -- for the formula itself -- an
80-node Gauss-Hermite double sum of the SE kernel against the two footprints."""
import numpy as np
import pytest

import blur_np
import stheno_jl_amd as S
from stheno_jl_amd import lib as L

LD = np.longdouble


def _points(D, n, seed):
    return np.asfortranarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (D, n)))


def test_flattened_spec_of_a_stretched_nested_selected_blur(monkeypatch):
    blur_np.install(monkeypatch)
    X = _points(3, 7, 1)
    f = S.atomic(S.GP(0.5 * (S.SEKernel() @ S.ARDTransform([2.0, 3.0]))), S.GPC())
    s_out, s_in = np.array([0.3, 0.1, 0.2]), (lambda Z: 0.05 * Z * Z)          # the inner node sees the stretched points
    g = S.blur(S.compose(S.blur(S.compose(f, S.Select([2, 0])), s_in), S.Stretch(1.5)), s_out)
    x = S.ColVecs(X)
    spec, _, _ = S.build_spec(S.cross([S.compose(f, S.Select([2, 0])), g]), S.BlockData([x, x]))
    assert spec.has_blur and not spec.has_kprod and not spec.f32_supported()
    kinds = [[int(t.kind) for t in spec._terms[spec._term_ptr[p]:spec._term_ptr[p + 1]]] for p in range(4)]
    assert kinds == [[L.SE], [L.BLUR_SE], [L.BLUR_SE], [L.BLUR_SE]]
    # the blurred view: locations a (1.5 x)[sel], variances a^2 (1.5^2 s_out + s_in(1.5 x))[sel], a = (2, 3), sel = (2, 0)
    a, Xs = np.array([2.0, 3.0])[:, None], 1.5 * X
    want = np.vstack([a * Xs[[2, 0]], a * a * (2.25 * s_out[:, None] + s_in(Xs))[[2, 0]]])
    got = spec.inputs[spec._terms[spec._term_ptr[3]].row_input]
    assert got.shape == (4, 7) and np.max(np.abs(got - want)) <= 4 * 2.0 ** -53 * np.max(np.abs(want))
    plain = spec.inputs[spec._terms[spec._term_ptr[1]].row_input]            # f against g: zero variance rows
    assert np.array_equal(plain, np.vstack([a * X[[2, 0]], np.zeros((2, 7))]))


@pytest.mark.parametrize("D", [1, 3, 8])
def test_prior_cov_against_the_long_double_formula(monkeypatch, D):
    blur_np.install(monkeypatch)
    X, s = _points(D, 9, D), np.linspace(0.1, 0.9, D)
    f = S.atomic(S.GP(0.7 * S.SEKernel()), S.GPC())
    x = S.ColVecs(X)
    K = S.prior_cov(S.cross([f, S.blur(f, s)]), S.BlockData([x, x]))
    Z = [np.vstack([X, 0 * X]), np.vstack([X, s[:, None] + 0 * X])]
    ref = np.block([[LD(0.7) * blur_np.pair(Z[i], Z[j], LD)[3] for j in range(2)] for i in range(2)])
    assert np.max(np.abs(K - ref)) <= 32 * 2.0 ** -53
    se = 0.7 * np.exp(-((X[:, :, None] - X[:, None, :]) ** 2).sum(0) / 2)        # cov(f, f): the plain SE kernel
    assert np.max(np.abs(K[:9, :9] - se)) <= 8 * 2.0 ** -53


def test_formula_against_gauss_hermite(monkeypatch):
    t, w = np.polynomial.hermite.hermgauss(80)
    e, w = np.sqrt(2.0) * t.astype(LD), w.astype(LD) / np.sqrt(LD(np.pi))      # nodes and weights of N(0, 1)

    def gh(mu, s, mup, sp):
        a, b = mu + np.sqrt(LD(s)) * e[:, None], mup + np.sqrt(LD(sp)) * e[None, :]
        return (w[:, None] * w[None, :] * np.exp(-(a - b) ** 2 / 2)).sum()

    k = lambda mu, s, mup, sp: blur_np.pair(np.array([[mu], [s]]), np.array([[mup], [sp]]), LD)[3][0, 0]      # noqa: E731
    for case in [(0.3, 0.7, -0.4, 0.2), (1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 0.0, 0.0)]:
        assert abs(k(*case) - gh(*case)) <= 1e-14
    assert abs(k(1.0, 1.0, 1.0, 1.0) - 1 / np.sqrt(LD(3))) <= 2.0 ** -62 and abs(k(0.0, 1.0, 0.0, 0.0) - 1 / np.sqrt(LD(2))) <= 2.0 ** -62


def test_host_refusals_name_blur(monkeypatch):
    blur_np.install(monkeypatch)
    x = S.ColVecs(_points(2, 6, 3))
    gp = lambda k, m=None: S.atomic(S.GP(k) if m is None else S.GP(m, k), S.GPC())      # noqa: E731
    f = gp(S.SEKernel())
    g = S.blur(f, 0.5)
    fx, y = g(x, 0.1), np.ones(6)
    models = [S.blur(gp(S.Matern32Kernel()), 0.5), S.blur(gp(S.SEKernel() * S.SEKernel()), 0.5),
              S.blur(gp(S.SEKernel() @ S.LinearTransform([[1.0, 1.0], [0.0, 1.0]])), 0.5),
              S.blur(gp(S.GibbsKernel(lambda X: 1.0 + 0 * X[0])), 0.5), S.blur(gp(S.SEKernel(), lambda X: X[0]), 0.5),
              S.blur(S.compose(f, S.Stretch(np.array([[1.0, 1.0], [0.0, 1.0]]))), 0.5), S.blur(S.derivative(f), 0.5),
              S.derivative(g), S.blur(S.stencil(f, np.zeros((2, 1)), np.ones(1)), 0.5),
              S.stencil(g, np.zeros((2, 1)), np.ones(1))]
    for m in models:
        with pytest.raises(NotImplementedError, match="blur"):
            S.build_spec(m, x)
    with pytest.raises(NotImplementedError, match="blur"):
        S.build_spec(S.blur(S.compose(gp(S.SEKernel()), S.Periodic(1.0)), 0.5), S.ColVecs(_points(1, 6, 3)))
    for call in (lambda: S.logpdf_and_gradient(fx, y, scales=True), lambda: S.logpdf_and_gradient_param(fx, y),
                 lambda: S.logpdf_and_gradient_conv(fx, y), lambda: S.logpdf_and_gradient_stencil(fx, y),
                 lambda: S.elbo_and_gradient(S.VFE(g(x, 1e-6)), fx, y), lambda: S.logpdf_f32(fx, y),
                 lambda: S.mean_and_var_and_gradient(S.posterior(fx, y)(x))):
        with pytest.raises(NotImplementedError, match="blur"):
            call()
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="blur"):
            S.blur(f, bad)
    with pytest.raises(ValueError, match="blur"):
        S.build_spec(S.blur(f, lambda X: -X), x)
