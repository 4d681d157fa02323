"""derivative(f) through the host mirror, on the NumPy double (tests/deriv_np.py): no GPU.

1. The flattener.  cov of (h, d h / d x_p, d h / d x_q) as the flattened derivative terms give it equals a long-double
   reference that knows no derivative formula: the covariance of the PLAIN model h, evaluated in long double at shifted
   points, differentiated by Richardson-extrapolated central differences (Romberg table over h0 / 2^k).  Every point, step
   and transformation is dyadic, so the shifted and transformed points are exact in float64 and the reference's only errors
   are the extrapolation's truncation -- estimated by the table itself, |T[K][K] - T[K-1][K-1]| -- and the long-double
   rounding of the difference quotients, eps_ld max|cov| / h_K per level of differencing.  The tolerance is built from those
   two and the float64 rounding of the evaluator under test; no figure in it comes from the result.
2. Every refusal of the host mirror, by name.
3. The chain to a scalar stretch: d / da = (m coef d_coef + d_inscale) / a against central differences of logpdf.
"""
import numpy as np
import pytest

import deriv_np
import stheno_jl_amd as S
from stheno_jl_amd import lib as L

LD = np.longdouble
EPS_LD, EPS = float(np.finfo(LD).eps), 2.0 ** -53
H0, LEVELS = 2.0 ** -3, 6


def _kern_ld(kind, d2):
    r = np.sqrt(d2)
    if kind == L.SE:
        return np.exp(-d2 / 2)
    if kind == L.MATERN32:
        l = np.sqrt(LD(3)) * r
        return (1 + l) * np.exp(-l)
    if kind == L.MATERN52:
        l = np.sqrt(LD(5)) * r
        return (1 + l + l * l / 3) * np.exp(-l)
    raise ValueError(kind)


def _plain_cov_ld(h, X, h2, Y):
    """cov(h(X), h2(Y)) of plain processes in long double, from the flattener's plain terms (its inputs are exact here)"""
    spec, _, _ = S.build_spec(h, S.ColVecs(np.asfortranarray(X)), h2, S.ColVecs(np.asfortranarray(Y)))
    assert not spec.has_deriv and not spec.has_kprod
    K = np.zeros((spec.N, spec.M), dtype=LD)
    for t in range(spec.n_terms):
        T = spec._terms[t]
        assert not T.row_scale and not T.col_scale
        A, B = spec.inputs[T.row_input].astype(LD), spec.inputs[T.col_input].astype(LD)
        d2 = ((A[:, :, None] - B[:, None, :]) ** 2).sum(0)
        K += LD(T.coef) * _kern_ld(T.kind, d2)
    return K


def _romberg(F):
    """(value, truncation estimate) of d F(t) / dt at 0 from central differences at H0 / 2^k, k < LEVELS"""
    T = [[(F(H0 / 2 ** k) - F(-H0 / 2 ** k)) / LD(2 * H0 / 2 ** k)] for k in range(LEVELS)]
    for k in range(1, LEVELS):
        for j in range(1, k + 1):
            T[k].append(T[k][j - 1] + (T[k][j - 1] - T[k - 1][j - 1]) / (LD(4) ** j - 1))
    return T[-1][-1], np.abs(T[-1][-1] - T[-2][-1])


def _reference(h, X, p, h2, Y, q):
    """(d^m cov(h(x), h2(y)) / d x_p d y_q, error bound): p / q None = that side is not differentiated"""
    def shifted(Z, dim, t):
        Z = Z.copy()
        if dim is not None:
            Z[dim, :] += t
        return Z
    scale = float(np.max(np.abs(_plain_cov_ld(h, X, h2, Y)))) + 1.0
    h_min = H0 / 2 ** (LEVELS - 1)
    if p is not None and q is not None:
        def inner(t):
            return _romberg(lambda u: _plain_cov_ld(h, shifted(X, p, u), h2, shifted(Y, q, t)))
        val, est = _romberg(lambda t: inner(t)[0])
        est = est + inner(0.0)[1] / h_min
        floor = 64 * EPS_LD * scale / h_min ** 2
    elif p is not None:
        val, est = _romberg(lambda u: _plain_cov_ld(h, shifted(X, p, u), h2, Y))
        floor = 64 * EPS_LD * scale / h_min
    else:
        val, est = _romberg(lambda t: _plain_cov_ld(h, X, h2, shifted(Y, q, t)))
        floor = 64 * EPS_LD * scale / h_min
    return val, 8 * est + floor


def _dyadic(rng, D, n, lo, hi):
    return np.asfortranarray(rng.integers(int(lo * 64), int(hi * 64), size=(D, n)) / 64.0)


def _models():
    """name -> (D, build(gpc) -> plain process h, separated): separated = the Matern kinds are not analytic at coincident points,
    their two point sets are kept apart (central differences across the kink are not a series in h^2)"""
    def se1(gpc):
        return S.atomic(S.GP(S.SEKernel()), gpc)

    def sums(gpc):
        f1, f2 = S.atomic(S.GP(S.SEKernel()), gpc), S.atomic(S.GP(0.75 * S.SEKernel()), gpc)
        return 2.0 * f1 + S.stretch(f2, 0.5) - 0.25 * f1 + 3.0

    def matrix(gpc):
        return S.stretch(S.atomic(S.GP(S.SEKernel()), gpc), np.array([[1.0, 0.5], [-0.25, 0.75]]))

    def sel(gpc):
        return S.select(S.atomic(S.GP(S.SEKernel()), gpc), [2, 0])

    def shifted(gpc):
        return S.shift(S.stretch(S.atomic(S.GP(S.SEKernel()), gpc), 0.5), np.array([0.25, -1.5]))

    def m52(gpc):
        return S.atomic(S.GP(S.with_lengthscale(S.Matern52Kernel(), 2.0) + 0.5 * S.SEKernel()), gpc)

    def m32(gpc):
        return S.stretch(S.atomic(S.GP(S.Matern32Kernel() @ S.ARDTransform([0.5, 0.25])), gpc), [1.0, 2.0])

    return {"se_1d": (1, se1, False), "sums_scales_known": (2, sums, False), "stretch_matrix": (2, matrix, False),
            "select": (3, sel, False), "shift_stretch": (2, shifted, False), "matern52_lengthscale": (2, m52, True),
            "matern32_ard": (2, m32, True)}


@pytest.mark.parametrize("name", sorted(_models()))
def test_flattened_derivative_terms_match_richardson_reference(name):
    D, build, separated = _models()[name]
    gpc = S.GPC()
    h = build(gpc)
    p, q = 0, D - 1
    dp, dq = S.derivative(h, p), S.derivative(h, q)
    rng = np.random.default_rng(7)
    X = _dyadic(rng, D, 4, -1.0, 1.0)
    Y = _dyadic(rng, D, 3, 2.0, 3.0) if separated else np.asfortranarray(np.hstack([X[:, :1], _dyadic(rng, D, 2, -1.0, 1.0)]))
    rows = S.BlockData([S.ColVecs(X)] * 3)
    cols = S.BlockData([S.ColVecs(Y)] * 3)
    spec, _, _ = S.build_spec(S.cross([h, dp, dq]), rows, S.cross([h, dp, dq]), cols)
    K = deriv_np.dense_from_spec(spec)
    n, m = X.shape[1], Y.shape[1]
    worst = 0.0
    for bi, pi in enumerate((None, p, q)):
        for bj, qj in enumerate((None, p, q)):
            got = K[bi * n:(bi + 1) * n, bj * m:(bj + 1) * m]
            if pi is None and qj is None:
                ref, tol = _plain_cov_ld(h, X, h, Y), 0.0
            else:
                ref, tol = _reference(h, X, pi, h, Y, qj)
            # the evaluator under test is float64: a few roundings of the largest addend of the entry (the plain covariance
            # bounds every term after the Jacobian factors, which are <= 4 here)
            tol = tol + 256 * EPS * (float(np.max(np.abs(ref))) + 1.0)
            err = np.abs(got - ref.astype(np.float64))
            worst = max(worst, float(np.max(err / tol)))
            assert np.all(err <= tol), (name, pi, qj, float(err.max()), float(np.max(tol)))
    print(f"{name}: largest error / tolerance = {worst:.3g}")


def test_select_drops_the_differentiated_coordinate():
    gpc = S.GPC()
    h = S.select(S.atomic(S.GP(S.SEKernel()), gpc), [2, 0])
    X = S.ColVecs(_dyadic(np.random.default_rng(1), 3, 5, -1.0, 1.0))
    spec, _, _ = S.build_spec(S.cross([h, S.derivative(h, 1)]), S.BlockData([X, X]))
    assert spec.n_terms == 1 and not spec.has_deriv          # coordinate 1 is not read: the derivative is the zero process
    K = deriv_np.dense_from_spec(spec)
    assert np.all(K[5:, :] == 0.0) and np.all(K[:, 5:] == 0.0)


def test_matrix_stretch_expands_into_one_term_per_coordinate():
    gpc = S.GPC()
    f = S.atomic(S.GP(S.SEKernel()), gpc)
    A = np.array([[1.0, 0.5], [-0.25, 0.75]])
    X = S.ColVecs(_dyadic(np.random.default_rng(2), 2, 4, -1.0, 1.0))
    spec, _, _ = S.build_spec(S.derivative(S.stretch(f, A), 0), X)
    got = sorted((int(spec._terms[t].param), spec._terms[t].coef) for t in range(spec.n_terms))
    want = sorted((17 * (a + 1) + b + 1, A[a, 0] * A[b, 0]) for a in range(2) for b in range(2))
    assert got == want and all(spec._terms[t].kind == L.DERIV_SE for t in range(spec.n_terms))


def test_constant_mean_differentiates_to_zero_and_known_constant_commutes():
    gpc = S.GPC()
    f = S.atomic(S.GP(2.5, S.SEKernel()), gpc)
    x = np.linspace(0.0, 1.0, 5)
    assert np.all(S.mean_vector(S.derivative(f + 1.0), x) == 0.0)
    assert np.all(S.mean_vector(S.cross([f, S.derivative(f)]), S.BlockData([x, x])) == np.r_[np.full(5, 2.5), np.zeros(5)])


def _refusals():
    def atom(k=None, mean=None):
        gpc = S.GPC()
        return S.atomic(S.GP(*(([mean] if mean is not None else []) + [k or S.SEKernel()])), gpc), gpc
    x1 = np.linspace(0.0, 1.0, 4)
    x2 = S.ColVecs(np.asfortranarray(np.arange(8.0).reshape(2, 4)))
    img = S.ColVecs(np.asfortranarray(np.arange(64.0).reshape(16, 4)))

    def spec_of(node, x):
        return lambda: S.build_spec(node, x)

    f = atom()[0]
    out = {
        "function scale": spec_of(S.derivative(np.sin * f), x1),
        "Periodic warp": spec_of(S.derivative(S.periodic(f, 1.0)), x1),
        "second derivative": spec_of(S.derivative(S.derivative(f)), x1),
        "stencil below": spec_of(S.derivative(S.stencil(f, [0.0, 0.5], [1.0, -1.0])), x1),
        "stencil above": spec_of(S.stencil(S.derivative(f), [0.0, 0.5], [1.0, -1.0]), x1),
        "patch_convolve below": spec_of(S.derivative(S.patch_convolve(atom()[0], (4, 4), (2, 2))), img),
        "patch_convolve above": spec_of(S.patch_convolve(S.derivative(atom()[0]), (4, 4), (2, 2)), img),
        "product of kernels": spec_of(S.derivative(atom(S.SEKernel() * S.Matern32Kernel())[0]), x1),
        "Matern-1/2": spec_of(S.derivative(atom(S.Matern12Kernel())[0]), x1),
        "product-path kind": spec_of(S.derivative(atom(S.RationalQuadraticKernel(2.0))[0]), x1),
        "PeriodicTransform": spec_of(S.derivative(atom(S.SEKernel() @ S.PeriodicTransform(1.0))[0]), x1),
        "callable mean (covariance)": spec_of(S.derivative(atom(mean=np.sin)[0]), x1),
        "callable mean (mean)": lambda: S.mean_vector(S.derivative(atom(mean=np.sin)[0]), x1),
        "dimension 17": spec_of(S.derivative(atom()[0], 3), S.ColVecs(np.asfortranarray(np.ones((17, 3))))),
    }
    g = S.gppp(lambda GP: dict(a=GP(S.SEKernel())))
    gpc = S.GPC()
    out["nested GPPP"] = spec_of(S.derivative(S.atomic(g, gpc)), S.GPPPInput("a", x1))
    del x2
    return out


@pytest.mark.parametrize("case", sorted(_refusals()))
def test_host_refusals_name_the_derivative(case):
    with pytest.raises(NotImplementedError, match="derivative"):
        _refusals()[case]()


def _joint(a, y=None):
    gpc = S.GPC()
    f = S.stretch(S.atomic(S.GP(S.SEKernel() + 0.5 * S.Matern52Kernel()), gpc), a)
    x = np.linspace(-1.0, 1.5, 7)
    fx = S.cross([f, S.derivative(f)])(S.BlockData([x, x + 0.125]), 0.1)
    return fx, (np.sin(3.0 * np.r_[x, x]) if y is None else y)


@pytest.mark.parametrize("what", ["inputs", "scales", "param", "conv", "stencil", "elbo", "f32"])
def test_host_gradient_and_fp32_refusals(monkeypatch, what):
    deriv_np.install(monkeypatch)
    fx, y = _joint(1.5)
    with pytest.raises(NotImplementedError, match="derivative"):
        if what == "inputs":
            S.logpdf_and_gradient(fx, y, inputs=True)
        elif what == "scales":
            S.logpdf_and_gradient(fx, y, scales=True)
        elif what == "param":
            S.logpdf_and_gradient_param(fx, y)
        elif what == "conv":
            S.logpdf_and_gradient_conv(fx, y)
        elif what == "stencil":
            S.logpdf_and_gradient_stencil(fx, y)
        elif what == "elbo":
            S.elbo_and_gradient(S.VFE(fx.f(fx.x, 1e-6)), fx, y)
        else:
            S.logpdf_f32(fx, y)


def test_chain_rule_to_a_scalar_stretch(monkeypatch):
    """d logpdf / da of stretch(f, a) observed with its derivative: sum over the term records of
    (m coef d_coef + d_inscale) / a, m the record's differentiated sides, against central differences of logpdf.  The
    tolerance is the differences' own: |D(2h) - D(h)| bounds the h^2 truncation of D(h) three times over, and a logpdf that is
    right to 64 eps |logpdf| moves the quotient by that over h"""
    deriv_np.install(monkeypatch)
    a, h = 1.5, 2.0 ** -12
    fx, y = _joint(a)
    g = S.logpdf_and_gradient(fx, y)
    assert any(r.get("deriv") == (0, 0) for r in g["terms"]) and any(r.get("deriv") == (0, None) for r in g["terms"])
    got = sum((sum(s is not None for s in r.get("deriv", ())) * r["coef"] * r["d_coef"] + r["d_inscale"]) / a for r in g["terms"])
    lp = lambda v: S.logpdf(_joint(v)[0], y)      # noqa: E731
    d1, d2 = (lp(a + h) - lp(a - h)) / (2 * h), (lp(a + 2 * h) - lp(a - 2 * h)) / (4 * h)
    tol = abs(d2 - d1) + 64 * EPS * abs(g["logpdf"]) / h
    print(f"d/da = {got:.12g}, central difference {d1:.12g}, |difference| / tolerance = {abs(got - d1) / tol:.3g}")
    assert abs(got - d1) <= tol
