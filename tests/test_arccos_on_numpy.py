"""NNGPKernel / NTKKernel through the host mirror, on the NumPy double (tests/arccos_np.py): no GPU.  The reference is the
definition of include/sthenomi.h written out here once more, directly: acos per layer."""
import numpy as np
import pytest

import arccos_np
import stheno_jl_amd as S
from stheno_jl_amd import lib as L


def _points(D, n, seed):
    return np.asfortranarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (D, n)))


def direct(ntk, A, B, depth, bias):
    A, B = (np.vstack([Z, np.full((1, Z.shape[1]), np.sqrt(bias))]) for Z in (A, B))
    na, nb = np.sqrt((A * A).sum(0)), np.sqrt((B * B).sum(0))
    c = np.clip((A.T @ B) / np.outer(na, nb), -1.0, 1.0)
    c[np.all(A[:, :, None] == B[:, None, :], axis=0)] = 1.0      # (acos amplifies the dot product's rounding at c = 1)
    t = c
    for _ in range(depth):
        th = np.arccos(c)
        t, c = (np.sin(th) + (np.pi - th) * c) / np.pi + t * (1 - th / np.pi), (np.sin(th) + (np.pi - th) * c) / np.pi
    return np.outer(na, nb) * (t if ntk else c)


def test_flattening_bias_row_codes_params_and_one_group(monkeypatch):
    arccos_np.install(monkeypatch)
    X, a = _points(2, 7, 1), np.array([2.0, 3.0])
    k = (0.5 * S.NNGPKernel(1, bias=0.25) + 0.3 * S.NNGPKernel(2, bias=0.25) + 0.2 * S.NTKKernel(2, bias=0.25)) @ S.ARDTransform(a)
    spec, _, _ = S.build_spec(S.atomic(S.GP(k + 0.1 * S.SEKernel()), S.GPC()), S.ColVecs(X))
    assert spec.has_arccos and not spec.has_kprod and not spec.f32_supported()
    assert [(int(t.kind), t.coef, t.param) for t in spec._terms] == [(L.NNGP, 0.5, 1.0), (L.NNGP, 0.3, 2.0), (L.NTK, 0.2, 2.0),
                                                                     (L.SE, 0.1, 0.0)]
    assert (L.NNGP, L.NTK) == (64, 65)
    views = {(t.row_input, t.col_input) for t in spec._terms[:3]}      # one view, depths ascending: one launch group
    assert len(views) == 1
    assert np.array_equal(spec.inputs[spec._terms[0].row_input], np.vstack([a[:, None] * X, np.full((1, 7), 0.5)]))
    assert S.NTKKernel(3).leaf_terms() == [(L.NTK, 1.0, 3.0, ())]


@pytest.mark.parametrize("ntk", [False, True])
def test_logpdf_and_elbo_against_the_direct_formula(monkeypatch, ntk):
    arccos_np.install(monkeypatch)
    n, D, depth, bias = 40, 3, 3, 0.5
    X, y = _points(D, n, 2), np.cos(np.arange(n) * 0.7)
    f = S.atomic(S.GP(0.7 * (S.NTKKernel if ntk else S.NNGPKernel)(depth, bias=bias)), S.GPC())
    K = 0.7 * direct(ntk, X, X, depth, bias)
    Lc = np.linalg.cholesky(K + 0.1 * np.eye(n))
    z = np.linalg.solve(Lc, y)
    ref = -0.5 * (z @ z + 2 * np.log(np.diag(Lc)).sum() + n * np.log(2 * np.pi))
    fx = f(S.ColVecs(X), 0.1)
    assert abs(S.logpdf(fx, y) - ref) <= 1e-10 * abs(ref)
    Xz = np.asfortranarray(X[:, 3::8])
    Lz = np.linalg.cholesky(0.7 * direct(ntk, Xz, Xz, depth, bias) + 1e-6 * np.eye(5))
    A = np.linalg.solve(Lz, 0.7 * direct(ntk, Xz, X, depth, bias)) / np.sqrt(0.1)
    Lb = np.linalg.cholesky(np.eye(5) + A @ A.T)
    c = np.linalg.solve(Lb, A @ y) / np.sqrt(0.1)
    want = -0.5 * (n * np.log(2 * np.pi * 0.1) + 2 * np.log(np.diag(Lb)).sum() + y @ y / 0.1 - c @ c
                   + np.diag(K).sum() / 0.1 - (A * A).sum())
    assert abs(S.elbo(S.VFE(f(S.ColVecs(Xz), 1e-6)), fx, y) - want) <= 1e-10 * abs(want)


def test_host_refusals_name_arc_cosine(monkeypatch):
    arccos_np.install(monkeypatch)
    x = S.ColVecs(_points(2, 8, 3))
    k = S.NNGPKernel(2, bias=1.0)
    f = S.atomic(S.GP(k), S.GPC())
    fx, y = f(x, 0.1), np.ones(8)
    with pytest.raises(NotImplementedError, match="arc-cosine"):
        (k * S.SEKernel()).leaf_products()
    for model, pts in ((S.derivative(f), x), (S.blur(f, 0.5), x), (S.stencil(f, np.zeros((2, 1)), np.ones(1)), x),
                       (S.atomic(S.GP(S.NTKKernel(1, bias=1.0)), S.GPC()), S.ColVecs(_points(16, 4, 1)))):
        with pytest.raises(NotImplementedError, match="arc-cosine"):
            S.build_spec(model, pts)
    for call in (lambda: S.logpdf_and_gradient(fx, y, scales=True), lambda: S.logpdf_and_gradient_param(fx, y),
                 lambda: S.logpdf_and_gradient_conv(fx, y), lambda: S.logpdf_and_gradient_stencil(fx, y),
                 lambda: S.elbo_and_gradient(S.VFE(f(x, 1e-6)), fx, y), lambda: S.logpdf_f32(fx, y),
                 lambda: S.mean_and_var_and_gradient(S.posterior(fx, y)(x)),
                 lambda: S.logpdf_and_gradient(S.atomic(S.GP(k + S.RationalQuadraticKernel()), S.GPC())(x, 0.1), y)):
        with pytest.raises(NotImplementedError, match="arc-cosine"):
            call()
    for bad in (lambda: S.NNGPKernel(0), lambda: S.NTKKernel(17), lambda: S.NNGPKernel(1.5), lambda: S.NTKKernel(float("nan")),
                lambda: S.NNGPKernel(float("inf")), lambda: S.NTKKernel(2, bias=-1.0), lambda: S.NNGPKernel(2, bias=float("nan"))):
        with pytest.raises(ValueError, match="arc-cosine"):
            bad()
