"""The kernel formulas of the device (csrc/common.h: exp_nonpos / sqrt_nonneg, kern_eval.h; f32.hip and grad.hip have their
own copies) where standard-normal inputs and an absolute 1e-12 say nothing: against the 60-digit table of
tests/golden/kernel_truth.json in ulps of the truth (tests/kernel_truth.py: the metric, the bounds and where they come
from), at coincident points off the diagonal, at nearly coincident ones under the gradient, and at distances whose
kernel value underflows or whose square overflows.

What the table can and cannot see (tried on builds with a deliberate error, not committed): sqrt_nonneg without its second
Newton step fails the Matern-3/2 cases of test_values_against_the_table in the band d2 >= 1 (1987 ulp; Matern-1/2 and
-5/2 grow tenfold and threefold but stay inside 6 + 4 l); a Taylor coefficient of exp_nonpos wrong by 1e-14 fails the SE
cases in the same band (4 ulp against the bound of 2).  The LAST digit of a coefficient (1/3! off by one ulp moves the
result by under 0.01 ulp) is below what any comparison of doubles can resolve.  Every case is a 1 x n or n x n assembly with n <= 512."""
import math

import numpy as np
import pytest
import scipy.linalg

import kernel_truth as kt
import np_terms
import stheno_jl_amd as P
from test_gpu_parity import REL, _kappa_prime, _oracle_term_grads

pytestmark = pytest.mark.gpu

KERNEL = {"se": P.SEKernel, "matern12": P.Matern12Kernel, "matern32": P.Matern32Kernel, "matern52": P.Matern52Kernel,
          "white": P.WhiteKernel}
COEF = 1.7      # not a power of two: coef * 1 == coef exactly, coef * (1 - 2^-53) != coef


def _atom(kernel):
    return P.atomic(P.GP(kernel), P.GPC())


def _pair_at_offsets(D, coord, t):
    """(x0, xt): one point and len(t) points that differ from it by t in coordinate `coord` alone; the other coordinates
    hold equal non-zero values on both sides (some as large as 1e6), so their differences are exactly 0"""
    if D == 1:
        return np.zeros(1), np.array(t, dtype=np.float64)
    fill = np.array([(1e6, -3.75, 0.1, 12345.678)[j % 4] * (1.0 + j / 7.0) for j in range(D)])
    fill[coord] = 0.0
    X0 = np.asfortranarray(fill[:, None].copy())
    Xt = np.asfortranarray(np.repeat(fill[:, None], len(t), axis=1))
    Xt[coord] = t
    return P.ColVecs(X0), P.ColVecs(Xt)


# ---- 1. fp64 values against the table, once per route ---------------------------------------------------------------------
@pytest.mark.parametrize("D,coord", [(1, 0), (65, 64)], ids=["D1_one_row_kernel", "D65_bigd_kernel"])
@pytest.mark.parametrize("name", kt.KERNELS)
def test_values_against_the_table(name, D, coord):
    """cov(f, [0], t) of a plain atomic GP(kernel): no stretch, no coefficient, the host multiplies nothing -- the entry IS
    the device's kernel formula at d2 = fl(t t)"""
    g = kt.load()[name]
    x0, xt = _pair_at_offsets(D, coord, g.t)
    K = P.prior_cov(_atom(KERNEL[name]()), x0, xt)
    assert K.shape == (1, len(g))
    print(f"\n{name} D={D}: largest error in ulps of the truth per band: {kt.band_maxima(g, K)}")
    bad = kt.violations(g, K)
    assert bad.size == 0, kt.describe(g, K, bad)
    assert K[0, 0] == 1.0


def test_values_against_the_table_through_the_accumulate_launches():
    """D = 16 stages one term per assembly launch: a KernelSum of the four kernels takes four launches, the last three
    read-modify-write.  Against the sum of the truths on the offsets all kernels share, with the summed bound: each
    kernel's own, in its own ulps, plus 2 ulp of the sum (three accumulate roundings and the reference sum's own, half an
    ulp each)."""
    grids = kt.load()
    nc = grids["se"].n_common
    D = 16
    x0, xt = _pair_at_offsets(D, 3, grids["se"].t[:nc])
    f = _atom(P.KernelSum([KERNEL[n]() for n in kt.KERNELS]))
    spec, _, _ = P.build_spec(f, x0, None, xt)
    assert spec.n_terms == 4
    K = P.prior_cov(f, x0, xt).ravel()
    S = np.array([math.fsum(grids[n].k[i] for n in kt.KERNELS) for i in range(nc)])
    tol = sum(grids[n].bound[:nc] * grids[n].ulp[:nc] for n in kt.KERNELS) + 2.0 * np.spacing(S)
    err = np.abs(K - S)
    print(f"\nKernelSum D=16: largest |error| / tolerance = {np.nanmax(err[np.isfinite(tol)] / tol[np.isfinite(tol)]):.3g}")
    assert not np.any(np.isnan(K)) and np.all((K >= 0.0) & (K <= 4.0))
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, [(i, grids["se"].t[i], K[i], S[i], err[i], tol[i]) for i in bad[:8]]
    zero = np.all([grids[n].must_zero[:nc] for n in kt.KERNELS], axis=0)
    assert zero.any() and np.all(K[zero] == 0.0)
    assert K[0] == 4.0


@pytest.mark.parametrize("name", kt.KERNELS)
def test_the_other_assemblies_equal_the_plain_term_on_the_grid(name):
    """prior_var, a one-point zero-offset stencil and a patch that is the whole image are pinned bit-equal to the plain
    term on ordinary inputs (test_gpu_parity / test_gpu_stencil / test_gpu_conv); the same equalities on the grid's
    points carry the table's verdict over to diag_plain_sum, stencil.hip and conv.hip"""
    g = kt.load()[name]
    x0, xt = np.zeros(1), g.t
    f = _atom(KERNEL[name]())
    plain = P.prior_cov(f, x0, xt)
    assert np.array_equal(P.prior_var(f, xt), np.diag(P.prior_cov(f, xt)))

    F = P.gppp(lambda GP: (lambda fp: {"f": fp, "g": P.stencil(fp, np.zeros((1, 1)), [1.0])})(GP(KERNEL[name]())))
    xf, xg, tf, tg = (P.GPPPInput(k, v) for k, v in [("f", x0), ("g", x0), ("f", xt), ("g", xt)])
    assert np.array_equal(P.cov(F(xf), F(tf)), plain)
    assert np.array_equal(P.cov(F(xg), F(tf)), plain)
    assert np.array_equal(P.cov(F(xf), F(tg)), plain)
    assert np.array_equal(P.cov(F(xg), F(tg)), plain)

    Fc = P.gppp(lambda GP: (lambda gp: {"g": gp, "f": P.patch_convolve(gp, patch_shape=(3, 3))})(GP(KERNEL[name]())))
    c0, ct = _pair_at_offsets(9, 4, g.t)
    i0 = P.GPPPInput("f", P.ImageVector(c0.X.reshape(3, 3, 1, order="F")))
    it = P.GPPPInput("f", P.ImageVector(ct.X.reshape(3, 3, -1, order="F")))
    assert np.array_equal(P.cov(Fc(P.GPPPInput("g", c0)), Fc(P.GPPPInput("g", ct))), plain)
    assert np.array_equal(P.cov(Fc(i0), Fc(P.GPPPInput("g", ct))), plain)
    assert np.array_equal(P.cov(Fc(P.GPPPInput("g", c0)), Fc(it)), plain)
    assert np.array_equal(P.cov(Fc(i0), Fc(it)), plain)


# ---- 2. coincident points ------------------------------------------------------------------------------------------------
def _coincident_blocks(D, n_distinct, n_rep_b, n_new_b, seed):
    """block A: n_distinct points, each three times, shuffled; block B: n_rep_b points of A again and n_new_b new ones,
    shuffled.  -> ([XA, XB] as D x n arrays, ids): points with equal ids are the same point"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((D, n_distinct + n_new_b)) / np.sqrt(D)
    ia = rng.permutation(np.repeat(np.arange(n_distinct), 3))
    ib = rng.permutation(np.concatenate([rng.integers(0, n_distinct, n_rep_b), n_distinct + np.arange(n_new_b)]))
    return [np.asfortranarray(base[:, ia]), np.asfortranarray(base[:, ib])], np.concatenate([ia, ib])


def _blockdata(Xs):
    return P.BlockData([P.GPPPInput("f", X[0].copy() if X.shape[0] == 1 else P.ColVecs(X)) for X in Xs])


def _model(name):
    return P.gppp(lambda GP: {"f": GP(COEF * KERNEL[name]())})


@pytest.mark.parametrize("D", [1, 3, 65])
@pytest.mark.parametrize("name", list(KERNEL))
def test_coincident_points_on_and_off_the_diagonal(name, D):
    """repeated measurements at one input: every coincident pair -- inside a block, off its diagonal, across blocks -- has
    the direct differences' d2 = 0 and with it exactly coef * kappa(0) = coef"""
    Xs, ids = _coincident_blocks(D, 50, 40, 30, seed=D)
    F, x = _model(name), _blockdata(Xs)
    K = P.prior_cov(F, x)
    same = ids[:, None] == ids[None, :]
    assert K.shape == (220, 220) and (same.sum() - 220) > 500          # coincident pairs off the diagonal
    assert np.all(K[same] == COEF)
    if name == "white":
        assert np.all(K[~same] == 0.0)
    else:
        assert np.all((K[~same] > 0.0) & (K[~same] < COEF))
    assert np.array_equal(K, K.T)
    assert np.array_equal(P.prior_var(F, x), np.diag(K))
    Kc = P.prior_cov(F, P.GPPPInput("f", x.X[0].x), P.GPPPInput("f", x.X[1].x))        # the cross (rectangular) assembly
    assert np.array_equal(Kc, K[:150, 150:])


def _np_logpdf(K, y):
    c, low = scipy.linalg.cho_factor(K, lower=True)
    a = scipy.linalg.solve_triangular(c, y, lower=True)
    return -0.5 * float(a @ a) - float(np.sum(np.log(np.diag(c)))) - 0.5 * len(y) * math.log(2 * math.pi)


def _dense(spec):
    K = np_terms.dense_from_spec(spec)                      # direct differences, like the device
    return np.tril(K) + np.tril(K, -1).T


@pytest.mark.parametrize("name", kt.KERNELS)
def test_logpdf_with_a_third_of_the_points_duplicated(name):
    """N = 300, noise 0.1; the reference is a SciPy Cholesky of the direct-difference NumPy matrix (the oracle's GEMM-trick
    distances are 1e-8 off at coincident points under Matern-1/2, which is why the oracle comparisons leave it out)"""
    rng = np.random.default_rng(77)
    D = 3
    base = rng.standard_normal((D, 200))
    X = np.asfortranarray(np.concatenate([base, base[:, rng.permutation(200)[:100]]], axis=1)[:, rng.permutation(300)])
    Xs = [X[:, :170], X[:, 170:]]
    F, x = _model(name), _blockdata(Xs)
    y = rng.standard_normal(300)
    spec, _, _ = P.build_spec(F, x)
    ref = _np_logpdf(_dense(spec) + 0.1 * np.eye(300), y)
    lp = P.logpdf(F(x, 0.1), y)
    assert abs(lp - ref) <= REL * abs(ref), (lp, ref)


# ---- 3. gradients at coincident and nearly coincident points --------------------------------------------------------------
@pytest.mark.parametrize("name,D", [(n, 3) for n in kt.KERNELS] + [("matern12", 1), ("matern12", 65), ("matern52", 65)])
def test_gradients_at_coincident_and_nearly_coincident_points(name, D):
    """the data of the coincident-point test plus pairs 1e-8 and 1e-160 apart (d2 = 1e-320 is subnormal; Matern-1/2's
    kappa' = -exp(-d) / 2d is 5e159 there): finite everywhere, and d_coef, d_inscale and the input gradient equal the NumPy
    contraction of G = (alpha alpha' - C^-1) / 2 from the direct-difference matrix.  Matern-1/2 takes the subgradient 0
    at d = 0 on both sides."""
    Xs, ids = _coincident_blocks(D, 50, 40, 30, seed=10 + D)
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(D) / np.sqrt(D)
    p0[0] = 0.0
    p1 = p0.copy()
    p1[0] = 1e-160
    q0 = rng.standard_normal(D) / np.sqrt(D)
    q1 = q0.copy()
    q1[0] += 1e-8
    r1 = q0.copy()
    r1[0] -= 1e-8
    Xs[0] = np.asfortranarray(np.concatenate([Xs[0], np.stack([p0, q0, q1], axis=1)], axis=1))     # q0, q1: inside a block
    Xs[1] = np.asfortranarray(np.concatenate([np.stack([r1, p1], axis=1), Xs[1]], axis=1))         # p0, p1: across blocks
    N = Xs[0].shape[1] + Xs[1].shape[1]
    F, x = _model(name), _blockdata(Xs)
    y = rng.standard_normal(N)
    g = P.logpdf_and_gradient(F(x, 0.1), y, inputs=True)
    spec = g["_spec"]
    gc, gs = g["_raw"]
    assert np.isfinite(g["logpdf"]) and np.all(np.isfinite(gc)) and np.all(np.isfinite(gs))
    assert all(np.all(np.isfinite(a)) for a in g["inputs"]) and np.all(np.isfinite(g["y"])) and np.isfinite(g["noise"])
    C = _dense(spec) + 0.1 * np.eye(N)
    Ci = np.linalg.inv(C)
    al = Ci @ y
    G = 0.5 * (np.outer(al, al) - Ci)
    assert abs(g["logpdf"] - _np_logpdf(C, y)) <= REL * abs(g["logpdf"])
    exp = _oracle_term_grads(spec, G)
    assert len(exp) == spec.n_terms == 4
    for t, (ec, es) in enumerate(exp):
        assert abs(gc[t] - ec) <= 1e-8 * max(1.0, abs(ec)), (t, gc[t], ec)
        assert abs(gs[t] - es) <= 2e-6 * max(1.0, abs(es)), (t, gs[t], es)
    roff = np.concatenate([[0], np.cumsum(spec.row_len)])
    want = [np.zeros_like(a) for a in spec.inputs]
    for (I, J, kind, ri, ci, coef, param, rs, cs) in np_terms.spec_terms(spec):
        Xr, Xc = spec.inputs[ri], spec.inputs[ci]
        df = Xr[:, :, None] - Xc[:, None, :]
        w = G[roff[I]:roff[I + 1], roff[J]:roff[J + 1]] * coef * _kappa_prime(kind, (df ** 2).sum(0))
        want[ri] += 2.0 * 2.0 * (w[None, :, :] * df).sum(2)      # d(d2)/dx = 2 (x - x'), mirror block doubles
    assert len(g["inputs"]) == len(want)
    for k, (a, e) in enumerate(zip(g["inputs"], want)):
        assert a.shape == e.shape
        assert np.abs(a - e).max() <= 1e-8 * max(1.0, np.abs(e).max()), (k, np.abs(a - e).max())


# ---- 4. far points and overflow --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 65])
@pytest.mark.parametrize("name", kt.KERNELS)
def test_far_blocks_are_exact_zeros_and_the_logpdf_splits(name, D):
    """three clusters: around 0, 1e3 away (every kernel underflows: the exp arguments are below -1000) and one point at
    1e200, whose squared distance to everything else overflows to +inf.  The cross entries are exactly 0 -- never NaN --
    and the logpdf is the sum of the clusters' own."""
    rng = np.random.default_rng(3 + D)
    A = rng.standard_normal((D, 150)) / np.sqrt(D)
    B = rng.standard_normal((D, 100)) / np.sqrt(D)
    B[0] += 1e3
    Cp = rng.standard_normal((D, 1)) / np.sqrt(D)
    Cp[D // 2] = 1e200
    Xs = [np.asfortranarray(v) for v in (A, B, Cp)]
    F, x = _model(name), _blockdata(Xs)
    K = P.prior_cov(F, x)
    assert not np.any(np.isnan(K))
    off = np.ones((251, 251), dtype=bool)
    for lo, hi in ((0, 150), (150, 250), (250, 251)):
        off[lo:hi, lo:hi] = False
    assert np.all(K[off] == 0.0)
    assert np.all((K[~off] > 0.0) & (K[~off] <= COEF)) and np.array_equal(K, K.T) and K[250, 250] == COEF
    Kc = P.prior_cov(F, P.GPPPInput("f", x.X[2].x), P.GPPPInput("f", x.X[0].x))          # 1 x 150, every d2 = +inf
    assert np.array_equal(Kc, np.zeros((1, 150)))
    y = rng.standard_normal(251)
    parts = [P.logpdf(F(_blockdata([X]), 0.1), y[lo:hi]) for X, (lo, hi) in zip(Xs, ((0, 150), (150, 250), (250, 251)))]
    lp = P.logpdf(F(x, 0.1), y)
    assert np.isfinite(lp) and abs(lp - sum(parts)) <= REL * abs(sum(parts)), (lp, parts)
    # the gradient kernels have their own formulas (grad.hip): finite, and the far block pairs contribute exact zeros
    g = P.logpdf_and_gradient(F(x, 0.1), y, inputs=True)
    gc, gs = g["_raw"]
    assert abs(g["logpdf"] - sum(parts)) <= REL * abs(sum(parts))
    assert np.all(np.isfinite(gc)) and np.all(np.isfinite(gs)) and all(np.all(np.isfinite(a)) for a in g["inputs"])
    cross = [t for t, term in enumerate(np_terms.spec_terms(g["_spec"])) if term[0] != term[1]]
    assert len(cross) == 6 and np.all(gc[cross] == 0.0) and np.all(gs[cross] == 0.0)


# ---- 5. fp32 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kt.KERNELS)
def test_fp32_values_against_the_table(name):
    """sgp_kernelmatrix_f32 on the grid rounded to float32 (offsets beyond float32 clipped to its largest finite value,
    whose square overflows), against the truth at the rounded offsets: the fp32 suite's absolute tolerance (5e-6 coef,
    test_cov_and_mean_f32), kappa(0) == coef exactly, 0 <= k <= coef, no NaN.  No relative bound is asserted: __expf's error
    at large arguments is nobody's measured number; the measured relative error is printed per band."""
    g = kt.load()[name]
    f = _atom(COEF * KERNEL[name]())
    K = P.prior_cov(f, np.zeros(1, dtype=np.float32), g.t32)
    assert K.dtype == np.float32 and K.shape == (1, len(g))
    K = K.ravel()
    c32 = np.float32(COEF)
    k = K.astype(np.float64) / float(c32)
    with np.errstate(divide="ignore", invalid="ignore"):
        relerr = np.abs(k - g.k32) / g.k32
    tiny32 = float(np.finfo(np.float32).tiny)
    d2 = g.t32.astype(np.float64) ** 2
    for label, m in (("d2 < 1", d2 < 1), ("d2 >= 1, k >= 1e-30", (d2 >= 1) & (g.k32 >= 1e-30)),
                     ("1e-30 > k >= FLT_MIN", (g.k32 < 1e-30) & (g.k32 >= tiny32))):
        print(f"\n{name} fp32, {label}: largest relative error {np.nanmax(relerr[m]) if m.any() else 0.0:.3g}")
    assert not np.any(np.isnan(K))
    assert np.all((K >= 0) & (K <= c32))
    assert np.all(K[g.t32 == 0] == c32) and (g.t32 == 0).sum() >= 1
    assert np.abs(K.astype(np.float64) - COEF * g.k32).max() <= 5e-6 * COEF
    with np.errstate(over="ignore"):
        assert np.isinf(g.t32 * g.t32).sum() >= 1           # the overflowing pair is there
