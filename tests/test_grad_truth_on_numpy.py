"""CPU pin of the gradient reference (tests/grad_truth.py) and of the bounds the GPU file (tests/test_gpu_grad_truth.py)
holds the device to.  No GPU here:

  * one small case (N = 24, D = 3, all four stationary kernels, one of them with a row / column scale) is recomputed at
    40 digits with mpmath; the long-double outputs must agree to 1e-17 of their scale;
  * on every case of the GPU file the reference's float64 run must sit inside its own bound (margin 2 instead of 8) and
    every bound in force must be at least 100 x tighter than the tolerance of the finite-difference era it replaces;
  * the floors in grad_truth.FLOORS are the medians of the recorded float64 figures.

Specs are obtained by running the host mirror on the NumPy double of the C-ABI (tests/np_capi.py); the double's numbers
are not looked at here (tests/test_host_mirror_on_numpy_double.py runs the GPU bodies against them).

`python tests/test_grad_truth_on_numpy.py` prints the float64 figures of every case and family: the lists recorded in
grad_truth.MEASURED_FLOAT64."""
import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (registers the product package, as under pytest)

import grad_truth as T
import np_capi
import test_gpu_grad_truth as GT


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    np_capi.install(monkeypatch)


def test_long_double_is_extended_here():
    assert T.require_extended() is np.longdouble and np.finfo(np.longdouble).eps < 1.1e-19


# ---- mpmath pin ------------------------------------------------------------------------------------------------------
def _mp_kappa(mp, kind, d2):
    """(kappa, kappa', d kappa / dg) in mpmath, written independently of grad_truth.kappa"""
    d = mp.sqrt(d2)
    if kind == T.SE:
        k = mp.exp(-d2 / 2)
        return k, -k / 2, -d2 * k
    if kind == T.MATERN12:
        k = mp.exp(-d)
        return k, (-k / (2 * d) if d > 0 else mp.mpf(0)), -d * k
    if kind == T.MATERN32:
        s = mp.sqrt(3) * d
        return (1 + s) * mp.exp(-s), -mp.mpf(3) / 2 * mp.exp(-s), -3 * d2 * mp.exp(-s)
    s = mp.sqrt(5) * d
    kp = -mp.mpf(5) / 6 * (1 + s) * mp.exp(-s)
    return (1 + s + s * s / 3) * mp.exp(-s), kp, 2 * d2 * kp


def test_long_double_reference_against_mpmath_at_40_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    rng = np.random.default_rng(77)
    n, D = 24, 3
    X = rng.standard_normal((D, n)) / np.sqrt(D) * 1.5
    y, mean = rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    sc = 1.0 + 0.3 * np.sin(X.sum(0))
    coefs = (1.1, 0.7, 0.9, 0.6)
    terms = [(0, 0, kind, 0, 0, coefs[kind], 0.0, sc if kind == T.MATERN32 else None, sc if kind == T.MATERN32 else None)
             for kind in (T.SE, T.MATERN12, T.MATERN32, T.MATERN52)]
    S = dict(terms=terms, inputs=[X], row_len=[n], col_len=[n], symmetric=True)
    noise = 0.15
    R = T.logpdf_grad(S, T.NOISE_SCALAR, noise, mean, y, T.require_extended(), inputs=True, scales=True)

    m = lambda v: mp.mpf(float(v))
    d2 = [[sum((m(X[d, i]) - m(X[d, j])) ** 2 for d in range(D)) for j in range(n)] for i in range(n)]
    kk = {kind: [[_mp_kappa(mp, kind, d2[i][j]) for j in range(n)] for i in range(n)] for kind in range(4)}
    rs = lambda kind, i: m(sc[i]) if kind == T.MATERN32 else mp.mpf(1)
    Cm = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Cm[i, j] = sum(m(coefs[k]) * rs(k, i) * rs(k, j) * kk[k][i][j][0] for k in range(4)) + (m(noise) if i == j else 0)
    Lm = mp.cholesky(Cm)
    Ci = mp.inverse(Cm)
    delta = mp.matrix([m(y[i]) - m(mean[i]) for i in range(n)])
    alpha = Ci * delta
    z = mp.lu_solve(Lm, delta)
    lp = -(n * mp.log(2 * mp.pi) + 2 * sum(mp.log(Lm[i, i]) for i in range(n)) + sum(v * v for v in z)) / 2
    G = [[(alpha[i] * alpha[j] - Ci[i, j]) / 2 for j in range(n)] for i in range(n)]

    def exact(v):           # a long double as the exact sum of two doubles
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))

    def close(got, want, scale):
        assert abs(exact(got) - want) <= mp.mpf("1e-17") * exact(scale), (float(got), float(want), float(scale))

    close(R["value"], lp, T.scale_scalar(R["value"], R["S_value"], n))
    sa = T.scale_entries(R["alpha"], R["S_alpha"] / n)
    for i in range(n):
        close(R["alpha"][i], alpha[i], sa[i])
    close(R["noise"], sum(G[i][i] for i in range(n)), T.scale_scalar(R["noise"], R["S_noise"], n))
    sx = T.scale_entries(R["gx"][0], R["Sn_gx"][0])
    gx = [[mp.mpf(0)] * n for _ in range(D)]
    for t, kind in enumerate((T.SE, T.MATERN12, T.MATERN32, T.MATERN52)):
        w = [[G[i][j] * rs(kind, i) * rs(kind, j) for j in range(n)] for i in range(n)]
        dc = sum(w[i][j] * kk[kind][i][j][0] for i in range(n) for j in range(n))
        ds = m(coefs[kind]) * sum(w[i][j] * kk[kind][i][j][2] for i in range(n) for j in range(n))
        close(R["d_coef"][t], dc, T.scale_scalar(R["d_coef"][t], R["S_coef"][t], n))
        close(R["d_inscale"][t], ds, T.scale_scalar(R["d_inscale"][t], R["S_inscale"][t], n))
        for d in range(D):
            for i in range(n):
                gx[d][i] += 4 * m(coefs[kind]) * sum(w[i][j] * kk[kind][i][j][1] * (m(X[d, i]) - m(X[d, j])) for j in range(n))
        if kind == T.MATERN32:
            ss = T.scale_entries(R["rowscale"][t], R["Sn_rowscale"][t])
            for i in range(n):
                want = 2 * sum(G[i][j] * m(coefs[kind]) * kk[kind][i][j][0] * rs(kind, j) for j in range(n))
                close(R["rowscale"][t][i], want, ss[i])
        else:
            assert R["rowscale"][t] is None
    for d in range(D):
        for i in range(n):
            close(R["gx"][0][d, i], gx[d][i], sx[d, i])


def test_elbo_reference_matches_the_oracle_it_restates():
    """grad_truth.elbo_grad restates oracle/abstractgps.py: elbo_gradient_wrt_cov; its float64 run must agree with that
    (LAPACK) implementation to double rounding on a small dense problem, spec terms written by hand."""
    import oracle.abstractgps as oagp
    import oracle.kernelfunctions as okf
    import oracle.stheno as ost
    rng = np.random.default_rng(5)
    D, n, m = 2, 40, 9
    X, Z = rng.standard_normal((D, n)), rng.standard_normal((D, m))
    y = rng.standard_normal(n)
    sy = 0.1 + rng.random(n)
    term = lambda: [(0, 0, T.MATERN52, 0, 1, 1.0, 0.0, None, None)]
    Szz = dict(terms=[(0, 0, T.MATERN52, 0, 0, 1.0, 0.0, None, None)], inputs=[Z], row_len=[m], col_len=[m], symmetric=True)
    Sxz = dict(terms=term(), inputs=[X, Z], row_len=[n], col_len=[m], symmetric=False)
    Sxx = dict(terms=[(0, 0, T.MATERN52, 0, 0, 1.0, 0.0, None, None)], inputs=[X], row_len=[n], col_len=[n], symmetric=True)
    R = T.elbo_grad(Szz, Sxz, Sxx, T.NOISE_DIAG, sy, T.NOISE_SCALAR, 1e-2, np.zeros(n), y, T.require_extended())
    fo = ost.atomic(oagp.GP(okf.Matern52Kernel()), ost.GPC())
    go = oagp.elbo_gradient_wrt_cov(oagp.VFE(fo(okf.ColVecs(Z), 1e-2)), fo(okf.ColVecs(X), sy), y)
    assert abs(go["elbo"] - float(R["value"])) <= 1e-12 * abs(go["elbo"])
    for key, ref in (("y", R["y"]), ("noise", R["noise"]), ("Kzz", R["dKzz"]), ("Kxz", R["dKxz"]), ("var", R["var"])):
        ref = np.asarray(ref, dtype=np.float64)
        assert np.max(np.abs(go[key] - ref)) <= 1e-10 * np.max(np.abs(ref)), key


# ---- the bounds, on the reference's own float64 run ------------------------------------------------------------------------
def _figures(case):
    """family -> float64 figure in units, for one case of the GPU file"""
    if case in GT.LP_CASES:
        _, (R, *R64) = GT.run_logpdf(case)
        return GT.yardstick(GT.logpdf_units(GT._reference_outputs(r), R) for r in R64)
    _, (R, *R64) = GT.run_elbo(case)
    return GT.yardstick(GT.elbo_units(GT._elbo_reference_outputs(r), R) for r in R64)


@pytest.mark.parametrize("case", GT.LP_CASES + GT.ELBO_CASES, ids=repr)
def test_float64_run_is_inside_its_bound_and_the_bound_is_tight(case):
    f64 = _figures(case)
    old = T.OLD_TOLERANCE["lp" if case in GT.LP_CASES else "elbo"]
    for fam, e in f64.items():
        assert np.isfinite(e)
        assert e <= T.SELF_MARGIN * max(e, T.FLOORS[fam]), (case.id, fam, e)
        bound = T.MARGIN * max(e, T.FLOORS[fam]) * T.EPS            # relative to the scale
        assert bound <= old / 100.0, (case.id, fam, bound, old)


def test_diag_grad_bound_is_tight():
    """(D + 8) eps S at the largest D of the diag_grad cases, against the 1e-10 the ELBO test holds its diagonal terms to"""
    assert (max(c.D for c in GT.DIAG_CASES) + 8) * T.EPS <= 1e-10 / 100.0


def test_floors_are_the_medians_of_the_recorded_float64_figures():
    assert set(T.FLOORS) == set(T.MEASURED_FLOAT64)
    for fam, vals in T.MEASURED_FLOAT64.items():
        assert len(vals) >= 3 and T.FLOORS[fam] == float(np.median(vals)), fam


if __name__ == "__main__":          # the measurement behind grad_truth.FLOORS / MEASURED_FLOAT64
    import pprint

    class _MP:
        def setattr(self, obj, name, value):
            setattr(obj, name, value)

    np_capi.install(_MP())
    lists = {}
    for c in GT.LP_CASES + GT.ELBO_CASES:
        for fam, e in _figures(c).items():
            lists.setdefault(fam, []).append(round(e, 1))
            print(f"{c.id:18s} {fam:15s} {e:10.1f}", flush=True)
    lists = {k: sorted(v) for k, v in lists.items()}
    print("MEASURED_FLOAT64 = ", end="")
    pprint.pprint(lists, width=120, compact=True)
    print("FLOORS = ", end="")
    pprint.pprint({k: float(np.median(v)) for k, v in lists.items()}, width=120)
