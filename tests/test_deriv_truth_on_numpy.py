"""The formulas of the derivative kinds, in the library's own operation order (tests/deriv_np.py), against the 80-digit table
(tests/deriv_truth.py) within its first-order bounds: values and input-scale derivatives of all three kinds at
(a, b) in {(1,0), (0,2), (1,1), (1,2)}, D in {1, 3, 16}, distances 0, 1e-160, 1e-8, 1, 40, 1e200, with the exact zeros and
the exact coincident values.  And the gradient truth (tests/deriv_grad_truth.py, on top of tests/grad_truth.py): its
long-double restatement against the table, its floors against the recorded float64 figures, and logpdf_and_gradient on the
NumPy double inside MARGIN x max(e_float64, floor).  No GPU.

`python tests/test_deriv_truth_on_numpy.py` prints the largest error as a fraction of its bound, per kind, and the float64
figures and floors that are written into tests/deriv_grad_truth.py."""
import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (registers the product package, as under pytest)

import deriv_grad_truth as GT
import deriv_np as dn
import deriv_truth as dt
import stheno_jl_amd as S
from stheno_jl_amd import lib as L

KIND = {"se": L.DERIV_SE, "m32": L.DERIV_MATERN32, "m52": L.DERIV_MATERN52}


def fractions(base):
    """(largest value error / bound, largest input-scale error / bound), asserting the exactness rules on the way"""
    worst = [0.0, 0.0]
    for D, G in dt.load()[base].items():
        for (a, b), rec in G["terms"].items():
            k, dk = dn.term(KIND[base], 17 * a + b, G["X"], G["Y"])
            k, dk = np.diag(k), np.diag(dk)
            assert np.all(np.isfinite(k)) and np.all(np.isfinite(dk)), (base, D, a, b)
            for i, (got, want, bound) in enumerate(((k, rec["value"], dt.value_bound(base, D, G, rec)),
                                                    (dk, rec["inscale"], dt.inscale_bound(base, D, G, rec)))):
                err = np.abs(got - want)
                assert np.all(err <= bound), (base, D, (a, b), "value" if i == 0 else "inscale", got, want, bound)
                worst[i] = max(worst[i], float(np.max(err / bound)))
            assert np.all(k[rec["must_zero"]] == 0.0) and np.all(dk[rec["must_zero"]] == 0.0), (base, D, a, b)
            assert np.all(k[rec["exact"][:, 0].astype(int)] == rec["exact"][:, 1]), (base, D, a, b)
            assert np.all(dk[rec["exact"][:, 0].astype(int)] == 0.0), (base, D, a, b)
    return worst


@pytest.mark.parametrize("base", sorted(KIND))
def test_formulas_match_the_table_within_the_first_order_bounds(base):
    v, g = fractions(base)
    print(f"{base}: largest value error / bound = {v:.3g}, largest input-scale error / bound = {g:.3g}")


def test_the_table_covers_what_it_says():
    T = dt.load()
    assert sorted(T) == ["m32", "m52", "se"]
    for base in T:
        assert sorted(T[base]) == [1, 3, 16]
        assert sorted(T[base][1]["terms"]) == [(1, 0), (1, 1)]
        for D in (3, 16):
            assert sorted(T[base][D]["terms"]) == [(0, 2), (1, 0), (1, 1), (1, 2)]
            assert sorted(set(T[base][D]["distance"])) == [0.0, 1e-160, 1e-8, 1.0, 40.0, 1e200]


# ---- the gradient truth ----------------------------------------------------------------------------------------------------
def test_long_double_restatement_matches_the_table():
    """the header's definitions in the derivatives of kappa, which the gradient truth is built from, run in long double,
    against the 80-digit table (kept rounded to float64: its float64 bounds are what the comparison can ask)"""
    LD = GT.T.require_extended()
    for base, per_d in dt.load().items():
        for D, G in per_d.items():
            ok = G["s"] < 1e300            # (the restatement has no clamp: an overflowed s is the library's business)
            for (a, b), rec in G["terms"].items():
                with np.errstate(under="ignore"):
                    k, dk = GT.term(KIND[base], 17 * a + b, G["X"][:, ok].astype(LD), G["Y"][:, ok].astype(LD), LD)
                k, dk = np.diag(k).astype(np.float64), np.diag(dk).astype(np.float64)
                assert np.all(np.abs(k - rec["value"][ok]) <= dt.value_bound(base, D, G, rec)[ok]), (base, D, a, b)
                assert np.all(np.abs(dk - rec["inscale"][ok]) <= dt.inscale_bound(base, D, G, rec)[ok]), (base, D, a, b)


def float64_figures():
    """family -> sorted e_float64 over the final case list"""
    figs = {}
    for name in GT.CASES:
        _, (R, *R64) = GT.case_truth(name, S)
        for fam, e in GT.yardstick(R, R64).items():
            figs.setdefault(fam, []).append(round(float(e), 1))
    return {fam: sorted(v) for fam, v in figs.items()}


def test_floors_are_the_medians_of_the_recorded_float64_figures():
    assert set(GT.FLOORS) == set(GT.MEASURED_FLOAT64) == {"value", "y", "noise", "d_coef", "d_inscale"}
    for fam, vals in GT.MEASURED_FLOAT64.items():
        assert len(vals) == len(GT.CASES) and GT.FLOORS[fam] == float(np.median(vals)), fam


@pytest.mark.parametrize("name", GT.CASES)
def test_numpy_double_gradient_is_inside_the_truth_bound(monkeypatch, name):
    """logpdf_and_gradient through the host mirror on the NumPy double (the library's formulas in float64, LAPACK's
    factorisation) within MARGIN x max(e_float64, floor) of the long-double truth, family by family"""
    dn.install(monkeypatch)
    fx, y = GT.build_case(name, S)
    g = S.logpdf_and_gradient(fx, y)
    _, (R, *R64) = GT.case_truth(name, S)
    gc, gs = g["_raw"]
    nt = g["_spec"].n_terms
    out = dict(value=g["logpdf"], y=g["y"], mean=g["mean"], noise=g["noise"], d_coef=gc[:nt], d_inscale=gs[:nt])
    got, e64 = GT.units(out, R), GT.yardstick(R, R64)
    for fam in sorted(got):
        print(f"{name:8s} {fam:10s} double {got[fam]:9.1f}  float64 {e64[fam]:9.1f}  floor {GT.FLOORS[fam]:8.1f}")
        assert np.isfinite(e64[fam]) and got[fam] <= GT.bound(fam, e64[fam]), (name, fam, got[fam], e64[fam])


if __name__ == "__main__":
    for base in sorted(KIND):
        v, g = fractions(base)
        print(f"{base}: largest value error / bound = {v:.3g}, largest input-scale error / bound = {g:.3g}")
    figs = float64_figures()            # the measurement behind deriv_grad_truth.MEASURED_FLOAT64 / FLOORS
    print("MEASURED_FLOAT64 =", figs)
    print("FLOORS =", {fam: float(np.median(v)) for fam, v in figs.items()})
