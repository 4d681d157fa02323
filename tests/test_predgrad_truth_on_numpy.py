"""CPU pin of the prediction-gradient reference (tests/predgrad_truth.py) and of the bounds the GPU file
(tests/test_gpu_predgrad.py) holds the device to.  No GPU here:

  * the truth against itself: central differences of its own long-double mean and variance at h = 2^-20 agree with its
    analytic gradients to O(h^2), exact and sparse, all four stationary kernels, two views of one atom (a non-zero prior
    part);
  * on every case of the GPU file the reference's float64 runs sit inside their own bound (margin 2 instead of 8);
  * the floors in predgrad_truth.FLOORS are the medians of the recorded float64 figures.

Specs are obtained by running the host mirror on the NumPy double of the C-ABI (tests/np_capi.py with the two entry points of
tests/predgrad_np.py); the double's numbers are looked at in tests/test_predgrad_on_numpy_double.py.

`python tests/test_predgrad_truth_on_numpy.py` prints the float64 figures of every case and family: the lists recorded in
predgrad_truth.MEASURED_FLOAT64."""
import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (registers the product package, as under pytest)

import grad_truth as T
import predgrad_np
import predgrad_truth as PT
import test_gpu_predgrad as GP


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    predgrad_np.install(monkeypatch)


# ---- the truth against itself ------------------------------------------------------------------------------------------------
H = 2.0 ** -20
# every pair is a profile of unit variance of a distance scaled by at most 1.3: its derivatives of order 1, 2, 3 along a
# coordinate are below 1.3^3 * 2 sqrt(3)^3 < 23 (the Matern-3/2 third derivative is the largest); Matern-1/2 is smooth away
# from coincident points, which the random points are not
M3 = 23.0


def _hand_specs(rng, dt):
    """a two-views model written by hand: k = sum_kind c_kind kappa_kind over the views 0.6 x and 1.3 x of one 2-d atom,
    every pair of views a term (the cross-view terms make k(x, x) depend on x)"""
    D, n, ns, m = 2, 14, 5, 6
    X, Xs, Z = (rng.standard_normal((D, k)) for k in (n, ns, m))
    views, coefs = (0.6, 1.3), (0.5, 0.4, 0.3, 0.2)

    def spec(A, B, sym):
        inputs, terms = [], []
        for va in views:
            for vb in views:
                inputs += [np.asarray(A, dtype=dt) * dt(va), np.asarray(B, dtype=dt) * dt(vb)]
                for kind in range(4):
                    terms.append((0, 0, kind, len(inputs) - 2, len(inputs) - 1, coefs[kind] / 4.0, 0.0, None, None))
        return dict(terms=terms, inputs=inputs, row_len=[A.shape[1]], col_len=[B.shape[1]], symmetric=sym)

    return X, Xs, Z, spec, views


def _chain(views, S, arrays):
    """d / d x* from the per-input arrays of a spec built by _hand_specs: row inputs are view va of x*, inputs 0, 2, 4, ..."""
    out = 0
    for q, (va, vb) in enumerate((a, b) for a in views for b in views):
        out = out + va * arrays[2 * q]
    return out


@pytest.mark.parametrize("sparse", [False, True], ids=["exact", "sparse"])
def test_truth_agrees_with_central_differences_of_its_own_values(sparse):
    dt = T.require_extended()
    rng = np.random.default_rng(31 + sparse)
    X, Xs, Z, spec, views = _hand_specs(rng, dt)
    n = X.shape[1]
    y, mean = rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    ms = np.full(Xs.shape[1], 0.2)

    def run(Xt):
        if sparse:
            return PT.sparse_predict_grad(spec(Z, Z, True), T.NOISE_SCALAR, 1e-2, spec(X, Z, False), T.NOISE_SCALAR, 0.15,
                                          mean, y, spec(Xt, Z, False), spec(Xt, Xt, True), ms, dt)
        return PT.predict_grad(spec(X, X, True), T.NOISE_SCALAR, 0.15, mean, y, spec(Xt, X, False), spec(Xt, Xt, True), ms, dt)

    Xs = np.asarray(Xs, dtype=dt)
    R = run(Xs)
    Sc, Sp = spec(Xs, Z if sparse else X, False), spec(Xs, Xs, True)
    d_mean = _chain(views, Sc, R["gm"])
    # the prior spec reads x* on both sides: row inputs 0, 2, .. are view va, column inputs 1, 3, .. view vb
    d_prior = 0
    for q, (va, vb) in enumerate((a, b) for a in views for b in views):
        d_prior = d_prior + va * R["gp"][2 * q] + vb * R["gp"][2 * q + 1]
    d_var = _chain(views, Sc, R["gv"]) + d_prior
    assert np.any(d_prior != 0)
    w_mean = float(np.abs(R["alpha"]).sum())
    # var = k** - sum_jl Q_jl k_j k_l: the third derivative of a product of two profiles has 8 terms, each below M3; k** is
    # four view pairs of coefficients summing to 1.4 / 4 each
    w_var = 8.0 * float(np.abs(R["Q"]).sum()) + 1.4
    eps_ld = float(np.finfo(np.longdouble).eps)
    for d in range(Xs.shape[0]):
        Xp, Xm = Xs.copy(), Xs.copy()
        Xp[d] += dt(H)
        Xm[d] -= dt(H)
        Rp, Rm = run(Xp), run(Xm)
        fd_m = (Rp["mean"] - Rm["mean"]) / dt(2 * H)
        fd_v = (Rp["var"] - Rm["var"]) / dt(2 * H)
        tol_m = H ** 2 * M3 * w_mean / 6 + 64 * eps_ld * float(np.max(R["S_mean"])) / H
        tol_v = H ** 2 * M3 * w_var / 6 + 64 * eps_ld * float(np.max(R["S_var"])) / H
        em, ev = float(np.abs(fd_m - d_mean[d]).max()), float(np.abs(fd_v - d_var[d]).max())
        print(f"d = {d}: mean {em:.3e} (tolerance {tol_m:.3e}), var {ev:.3e} (tolerance {tol_v:.3e})")
        assert em <= tol_m and ev <= tol_v
        assert float(np.abs(d_mean[d]).max()) > 1e4 * tol_m and float(np.abs(d_var[d]).max()) > 1e3 * tol_v


# ---- the bounds, on the reference's own float64 runs ------------------------------------------------------------------------
def _figures(case):
    s, g, (R, *R64) = GP.run_case(case)
    return GP.yardstick(case, R, R64)


@pytest.mark.parametrize("case", GP.ALL_CASES, ids=repr)
def test_float64_runs_are_inside_their_bound(case):
    for fam, e in _figures(case).items():
        assert np.isfinite(e)
        assert e <= PT.SELF_MARGIN * max(e, PT.FLOORS[fam]), (case.id, fam, e)
        assert PT.MARGIN * max(e, PT.FLOORS[fam]) * PT.EPS <= 1e-8 / 100.0        # far tighter than a finite-difference check


@pytest.mark.parametrize("case", GP.ALL_CASES, ids=repr)
def test_the_doubles_gradients_are_inside_the_device_bound(case):
    """the GPU file's body on the NumPy double (LAPACK solves): the same verdict function, so that a mistake in the case list,
    the marshalling or the unit bookkeeping shows here and not first on the device"""
    s, g, (R, *R64) = GP.run_case(case)
    GP.values_check(case, s, g, R, R64)
    GP.hold(case, GP.device_units(case, g, R), GP.yardstick(case, R, R64))
    GP.prior_part_check(case, g, R)


def test_floors_are_the_medians_of_the_recorded_float64_figures():
    assert set(PT.FLOORS) == set(PT.MEASURED_FLOAT64) == {"pred.mean_x", "pred.var_x", "spred.mean_x", "spred.var_x"}
    for fam, vals in PT.MEASURED_FLOAT64.items():
        assert len(vals) >= 3 and PT.FLOORS[fam] == float(np.median(vals)), fam
        assert len(vals) == len([c for c in GP.ALL_CASES if GP.prefix(c) == fam.split(".")[0]])


if __name__ == "__main__":          # the measurement behind predgrad_truth.FLOORS / MEASURED_FLOAT64
    import pprint

    class _MP:
        def setattr(self, obj, name, value, raising=True):
            setattr(obj, name, value)

    predgrad_np.install(_MP())
    lists = {}
    for c in GP.ALL_CASES:
        for fam, e in _figures(c).items():
            lists.setdefault(fam, []).append(round(e, 1))
            print(f"{c.id:18s} {fam:15s} {e:10.1f}", flush=True)
    lists = {k: sorted(v) for k, v in lists.items()}
    print("MEASURED_FLOAT64 = ", end="")
    pprint.pprint(lists, width=120, compact=True)
    print("FLOORS = ", end="")
    pprint.pprint({k: float(np.median(v)) for k, v in lists.items()})
