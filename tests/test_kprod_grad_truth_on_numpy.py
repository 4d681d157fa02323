"""CPU pin of the product-chain gradient reference (tests/kprod_grad_truth.py) and of the bounds the GPU file
(tests/test_gpu_kprod_grad_truth.py) holds the device to.  No GPU here:

  * grad_truth's outputs did not move by a bit when logpdf_grad / elbo_grad learned to take this module's chains
    (tests/golden/grad_truth_pin.npz);
  * the long-double Bessel routine of kind 20 against mpmath.besselk at 40 digits over the nu and x grid of
    tests/kprod_grad_truth_mp.py: below 2^-59; the pin problem (N = 24, D = 3, M = 6, one chain per kind pair, a function-scaled
    head, the ELBO, the diagonal on one view and on two): every family to 1e-17 of its scale.  Both read the committed values
    of tests/golden/kprod_grad_truth.json and, where mpmath imports, derive them again;
  * the float64 run of the restatement against the existing evaluators (kprod_np, kprod_grad_np, kinds_np, matern_nu_np);
  * central differences of the truth's own long-double logpdf at h = 2^-20, hyper-parameters and points;
  * on every case of the GPU file: the conditioning caps, the recorded float64 figures reproduced to a factor 2, every
    bound in force at least 100 x tighter than the tolerance it sits beside, and the case bodies on the NumPy double of the
    three entry points (tests/test_kprod_grad_on_numpy.py: FakeKprodGrad) wherever the double covers the call;
  * the floors in kprod_grad_truth.FLOORS are the medians of the recorded float64 figures.

`python tests/test_kprod_grad_truth_on_numpy.py` prints BESSEL_MEASURED, MEASURED_FLOAT64 and FLOORS as kprod_grad_truth.py
records them."""
import json
import os

import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (registers the product package, as under pytest)

import kinds_np  # noqa: F401  (teaches kprod_np / kprod_grad_np kinds 16 and 17)
import kprod_grad_np as kg
import kprod_grad_truth as KT
import kprod_grad_truth_mp as KM
import kprod_np as kn
import matern_nu_np
import stheno_jl_amd as P
import test_gpu_kprod_grad_truth as GK
from grad_truth_pin import grad_truth_pin
from test_kprod_grad_on_numpy import install_fake

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    install_fake(monkeypatch)
    matern_nu_np.install(monkeypatch)
    monkeypatch.setattr(GK, "MARGIN_IN_FORCE", KT.SELF_MARGIN)


def _golden():
    with open(os.path.join(HERE, "golden", "kprod_grad_truth.json")) as fh:
        return json.load(fh)


def test_long_double_is_extended_here():
    assert KT.require_extended() is np.longdouble and np.finfo(np.longdouble).eps < 1.1e-19


def test_grad_truth_outputs_did_not_move_by_a_bit():
    """the golden file was written by grad_truth as it was before `ops` was added to logpdf_grad / elbo_grad"""
    want = np.load(os.path.join(HERE, "golden", "grad_truth_pin.npz"))
    got = grad_truth_pin()
    assert set(got) == set(want.files)
    for k in got:
        assert np.array_equal(got[k], want[k]), k


# ---- mpmath pins -------------------------------------------------------------------------------------------------------------
def bessel_figure():
    """largest relative error of the long-double routine (k and kappa') against the committed 40-digit values"""
    dt = KT.require_extended()
    table, worst = _golden()["bessel"], 0.0
    assert [float(s) for s in table] == list(KM.BESSEL_NUS)
    for nu in KM.BESSEL_NUS:
        k, kx, _ = KT.matern_nu_derivs(KM.bessel_points(nu), nu, dt)
        e = table[repr(nu)]
        for got, want in ((k, e["k"]), (kx, e["kx"])):
            want = np.array([dt(s) for s in want])
            assert np.all(want != 0)
            worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
    return worst


def test_bessel_routine_in_long_double_against_mpmath():
    """nu < 1/2, both sides of the half-integers and of the integers, x on both sides of the series / fraction split, of 2 and
    of 600, x up to 999"""
    assert min(KM.BESSEL_NUS) < 0.5 and max(KM.BESSEL_XS) > 990 and min(abs(x - 2.0) for x in KM.BESSEL_XS if x != 2.0) < 1e-5
    worst = bessel_figure()
    print(f"largest relative error {worst:.3e} = {worst / 2.0 ** -64:.1f} units of 2^-64; cap {KT.BESSEL_CAP:.3e}")
    assert worst < KT.BESSEL_CAP
    assert KT.BESSEL_MEASURED is not None and worst <= 2.0 * KT.BESSEL_MEASURED and KT.BESSEL_MEASURED < KT.BESSEL_CAP


def test_pin_problem_in_long_double_against_mpmath():
    """every family of the pin problem agrees with the committed 40-digit values to 1e-17 of its scale (0.09 unit)"""
    dt = KT.require_extended()
    pin, run = _golden()["pin"], KM.long_double_run()
    assert set(pin) == set(run)
    kinds = {kind for ch in KM.pin_problem()["xx"]["chains"] for (_, kind, _, _, _) in ch["factors"]}
    assert {KT.RQ, KT.LINEAR, KT.COSINE, KT.GAMMAEXP, KT.MATERN_NU} <= kinds
    for key in sorted(run):
        got, scale = run[key]
        want = np.array([dt(s) for s in pin[key]])
        assert got.shape == want.shape, key
        err = float(np.max(np.abs(got - want) / np.where(scale > 0, scale, 1)))
        print(f"{key:26s} {err:.3e} of its scale")
        assert np.all((scale > 0) | (got == want)) and err <= 1e-17, (key, err)


def test_committed_values_are_what_mpmath_gives_here():
    pytest.importorskip("mpmath")
    import mpmath as mp
    g = _golden()
    fresh = {"bessel": KM.bessel_table(), "pin": KM.pin_values()}
    for part in ("bessel", "pin"):
        assert set(g[part]) == set(fresh[part])
    pairs = [(g["bessel"][nu][key], fresh["bessel"][nu][key]) for nu in g["bessel"] for key in ("k", "kx")]
    pairs += [(g["pin"][key], fresh["pin"][key]) for key in g["pin"]]
    for want, got in pairs:
        assert len(want) == len(got)
        for a, b in zip(want, got):
            a, b = mp.mpf(a), mp.mpf(b)
            assert abs(a - b) <= mp.mpf("1e-23") * max(abs(a), abs(b)), (a, b)


# ---- the float64 run against the existing evaluators -------------------------------------------------------------------------------
def _close(a, e, tol=1e-8):
    a, e = np.asarray(a, dtype=float), np.asarray(e, dtype=float)
    return float(np.max(np.abs(a - e), initial=0.0)) <= tol * max(1.0, float(np.max(np.abs(e), initial=0.0)))


@pytest.mark.parametrize("case_id", ["kp-D3-nf3", "kp-lim-8x5", "kp-mn-D2", "kp-scaled-mn-D2", "kp-coin-mn1.25", "kp-coin-cosine"])
def test_float64_run_matches_the_existing_evaluators(case_id):
    """the matrix, the three term contractions, the input and scale gradients (symmetric: twice the evaluator's row side) and
    the diagonal's gradients, at the tolerance tests/test_gpu_kprod_grad.py holds the device to against the same evaluators"""
    case = GK.LP_CASES[[c.id for c in GK.LP_CASES].index(case_id)]
    F, x, noise, y = GK.logpdf_problem(case)
    spec, _, _ = P.build_spec(F, x)
    S = KT.read_spec(spec)
    K = KT.dense(S, np.float64)
    assert _close(K, kn.np_spec_matrix(spec), 1e-13)
    rng = np.random.default_rng(5)
    G = rng.standard_normal(K.shape)
    G = G + G.T
    R = KT.contract(S, G, np.float64, inputs=True, scales=True)
    gc, gs, gp = kn.np_contract(spec, G)
    assert _close(R["d_coef"], gc) and _close(R["d_inscale"], gs) and _close(R["d_param"], gp)
    ev = kg.np_input_grads(spec, G)
    for a, e in zip(R["gx"], ev["row"]):
        assert _close(a, 2.0 * e)
    for t in range(spec.n_terms):
        assert (R["rowscale"][t] is None) == (ev["rs"][t] is None)
        if ev["rs"][t] is not None:
            assert _close(R["rowscale"][t], 2.0 * ev["rs"][t])
    w = rng.standard_normal(spec.N)
    Dg, ed = KT.diag_grad(S, w, np.float64), kg.np_diag_grads(spec, w)
    assert _close(KT.diag_of(S, np.float64), kg.np_diag(spec), 1e-13)
    assert _close(Dg["d_coef"], ed["gc"]) and _close(Dg["d_inscale"], ed["gs"]) and _close(Dg["d_param"], ed["gp"])
    for a, e in zip(Dg["gx"], ed["gx"]):
        assert _close(a, e)
    for t in range(spec.n_terms):
        for a, e in ((Dg["rowscale"][t], ed["rs"][t]), (Dg["colscale"][t], ed["cs"][t])):
            assert (a is None) == (e is None)
            if e is not None:
                assert _close(a, e)


def test_float64_cross_block_matches_the_existing_evaluators():
    """a rectangular spec: the column side, and the column scale sums"""
    case = GK.ELBO_CASES[[c.id for c in GK.ELBO_CASES].index("kpelbo-mn-D5")]
    F, x, z, _, _, _ = GK.elbo_problem(case)
    spec, _, _ = P.build_spec(F, x, None, z)
    S = KT.read_spec(spec)
    assert not S["symmetric"] and _close(KT.dense(S, np.float64), kn.np_spec_matrix(spec), 1e-13)
    G = np.random.default_rng(6).standard_normal((spec.N, spec.M))
    R = KT.contract(S, G, np.float64, inputs=True, scales=True)
    gc, gs, gp = kn.np_contract(spec, G)
    assert _close(R["d_coef"], gc) and _close(R["d_inscale"], gs) and _close(R["d_param"], gp)
    ev = kg.np_input_grads(spec, G)
    for a, r, c in zip(R["gx"], ev["row"], ev["col"]):
        assert _close(a, r + c)
    seen = 0
    for t in range(spec.n_terms):
        for a, e in ((R["rowscale"][t], ev["rs"][t]), (R["colscale"][t], ev["cs"][t])):
            assert (a is None) == (e is None)
            if e is not None:
                assert _close(a, e)
                seen += 1
    assert seen >= 2


# ---- the truth against itself ----------------------------------------------------------------------------------------------------
H = 2.0 ** -20


def test_truth_agrees_with_central_differences_of_its_own_logpdf():
    """Central differences of the long-double logpdf of the pin problem at h = 2^-20, for every head's coefficient, every
    factor's input scale and parameter, and coordinates of the points (through the three views), against the analytic
    gradients within h^2 |f'''| / 6 plus the rounding of the differences, 64 eps_ld S / h (S: the absolute sum behind the
    value).  |f'''| is bounded from the values alone: the central differences at 2 h and at h differ by h^2 f''' / 2 to leading
    order, so twice that estimate, 4 |CD(2 h) - CD(h)| / h^2, stands for the bound."""
    dt = KT.require_extended()
    prob = KM.pin_problem()
    S0, y, mean = prob["xx"], prob["y"], prob["mean"]
    X = S0["inputs"][0]

    def value(coef=None, scale=None, param=None, point=None):
        chains = []
        for c, ch in enumerate(S0["chains"]):
            ch = dict(ch)
            if coef is not None and coef[0] == c:
                ch["coef"] = ch["coef"] + coef[1]
            if param is not None:
                ch["factors"] = [(t, k, ri, ci, p + (param[1] if t == param[0] else 0.0)) for (t, k, ri, ci, p) in ch["factors"]]
            chains.append(ch)
        inputs = [a.astype(dt) for a in S0["inputs"]]
        if point is not None:
            d, i, h = point
            Xp = X.astype(dt).copy()
            Xp[d, i] += dt(h)
            inputs = [Xp, dt(0.7) * Xp, dt(0.5) * Xp[:1]]
            # (0.7 and 0.5 as the doubles the problem multiplied with: the products differ from the stored views by roundings
            # that are the same on both sides of the difference)
        if scale is not None:       # the factor's own copy of its view, scaled
            t, h = scale
            for ch in chains:
                fac = []
                for (u, k, ri, ci, p) in ch["factors"]:
                    if u == t:
                        inputs.append(inputs[ri] * (dt(1) + dt(h)))
                        ri = ci = len(inputs) - 1
                    fac.append((u, k, ri, ci, p))
                ch["factors"] = fac
        S = dict(S0, chains=chains, inputs=inputs)
        return _logpdf_value(S, y, mean, dt)

    R = KT.logpdf_grad(S0, KT.NOISE_SCALAR, KM.NOISE, mean, y, dt, inputs=True, scales=True)
    eps_ld = float(np.finfo(np.longdouble).eps)
    round_tol = 64 * eps_ld * float(R["S_value"]) / H
    checks = []
    for c, ch in enumerate(S0["chains"]):
        checks.append((f"coef[{c}]", R["d_coef"][ch["head"]], lambda h, c=c: value(coef=(c, h))))
        for (t, kind, _, _, _) in ch["factors"]:
            checks.append((f"inscale[{t}]", R["d_inscale"][t], lambda h, t=t: value(scale=(t, h))))
            if kind in (KT.RQ, KT.GAMMAEXP, KT.LINEAR, KT.CONST):
                checks.append((f"param[{t}]", R["d_param"][t], lambda h, t=t: value(param=(t, h))))
            else:
                assert R["d_param"][t] == 0
    for d, i in ((0, 0), (1, 5), (2, 11), (0, 23)):
        want = R["gx"][0][d, i] + dt(0.7) * R["gx"][1][d, i] + (dt(0.5) * R["gx"][2][0, i] if d == 0 else 0)
        checks.append((f"x[{d},{i}]", want, lambda h, d=d, i=i: value(point=(d, i, h))))
    assert len(checks) == 6 + 13 + 5 + 4          # heads, factors, factors with a parameter, coordinates
    moved = 0
    for name, want, f in checks:
        cd1 = (f(H) - f(-H)) / dt(2 * H)
        cd2 = (f(2 * H) - f(-2 * H)) / dt(4 * H)
        tol = H ** 2 * (4.0 * float(abs(cd2 - cd1)) / H ** 2) / 6 + round_tol
        err = float(abs(cd1 - want))
        print(f"{name:14s} analytic {float(want):+.12e}  error {err:.2e}  tolerance {tol:.2e}")
        assert err <= tol, (name, err, tol)
        moved += abs(float(want)) > 1e3 * tol
    assert moved >= len(checks) - 4          # the check sees the gradients: nearly all are 1000 tolerances away from 0


def _logpdf_value(S, y, mean, dt):
    n = len(y)
    K = KT.dense(S, dt)
    K = np.tril(K) + np.tril(K, -1).T
    Lm = KT.cholesky(K + KT.noise_matrix(KT.NOISE_SCALAR, KM.NOISE, n, dt))
    z = KT.tri_inverse(Lm) @ (np.asarray(y, np.float64).astype(dt) - np.asarray(mean, np.float64).astype(dt))
    return -(dt(n) * np.log(dt(2) * KT.T._pi(dt)) + dt(2) * np.log(np.diag(Lm)).sum() + z @ z) / dt(2)


# ---- the bounds, on the reference's own float64 runs ------------------------------------------------------------------------------
COND_CAP_LOGPDF, COND_CAP_ELBO = 1e4, 1e6


@pytest.mark.parametrize("case", GK.LP_CASES, ids=repr)
def test_logpdf_cases_are_well_conditioned(case):
    F, x, noise, _ = GK.logpdf_problem(case)
    K = KT.dense(KT.read_spec(P.build_spec(F, x)[0]), np.float64)
    cond = float(np.linalg.cond(K + noise * np.eye(len(K))))
    print(f"{case.id:18s} cond(K + Sigma_y) = {cond:.3e}   largest prior variance {float(np.max(np.diag(K))):.2f}")
    assert cond <= COND_CAP_LOGPDF


@pytest.mark.parametrize("case", GK.ELBO_CASES, ids=repr)
def test_elbo_cases_are_well_conditioned(case):
    F, _, z, _, sz, _ = GK.elbo_problem(case)
    K = KT.dense(KT.read_spec(P.build_spec(F, z)[0]), np.float64)
    cond = float(np.linalg.cond(K + (sz * np.eye(len(K)) if np.ndim(sz) == 0 else sz)))
    print(f"{case.id:18s} cond(Kzz + Sigma_z) = {cond:.3e}")
    assert cond <= COND_CAP_ELBO


def _figures(case):
    """family -> float64 figure in units, for one case of the GPU file"""
    if case in GK.LP_CASES:
        R, *R64 = GK.logpdf_truth(case)
        return GK.yardstick(KT.logpdf_units(KT.logpdf_reference_outputs(r), R) for r in R64)
    R, *R64 = GK.elbo_truth(case)
    return GK.yardstick(KT.elbo_units(KT.elbo_reference_outputs(r), R) for r in R64)


# cases whose bound in force is NOT 100 x inside the tolerance it replaces, and why: {case id: {family: reason}}
_ONE_ROW = ("float64 itself is 1.2e5 / 2.7e5 units off here: the sums of the pairs with the one-row block (129 x 1 and 128 x 1 entries) are "
            "small beside the error of G, which is relative to max |G| of the whole matrix (noise 0.055: alpha ~ y / noise); the "
            "bound in force is still 93 x / 41 x inside 1e-8")
NOT_100X = {"kp-mn-D2": {"kp.d_coef": _ONE_ROW, "kp.d_param": _ONE_ROW}}


@pytest.mark.parametrize("case", GK.LP_CASES + GK.ELBO_CASES, ids=repr)
def test_bound_in_force_is_100x_inside_the_tolerance_beside_it(case):
    f64 = _figures(case)
    for fam, e in f64.items():
        assert np.isfinite(e)
        bound = KT.MARGIN * max(e, KT.FLOORS[fam]) * KT.EPS            # relative to the scale
        old = KT.OLD_TOLERANCE["d_inscale" if fam.endswith("d_inscale") else "other"]
        if fam in NOT_100X.get(case.id, {}):
            assert bound > old / 100.0, (case.id, fam, "listed in NOT_100X but tight")
            continue
        assert bound <= old / 100.0, (case.id, fam, bound, old)


@pytest.mark.parametrize("case", GK.DIAG_CASES + GK.ELBO_CASES, ids=repr)
def test_diagonal_model_bound_is_tight(case):
    """(D + 8 + sum_f amp_f) eps against the 1e-8 the diagonal's gradients are held to beside it"""
    R = GK.run_diag(case)[2] if case in GK.DIAG_CASES else GK.elbo_truth(case)[0]["xx"]
    worst = float(np.max((R["dim"] + 8.0 + R["amp"]) * KT.EPS))
    print(f"{case.id:18s} (D + 8 + sum amp) eps = {worst:.3e}")
    assert worst <= 1e-8 / 100.0


def test_floors_are_the_medians_of_the_recorded_float64_figures():
    fams = {f"kp.{k}" for k in ("value", "y", "noise", "d_coef", "d_inscale", "d_param", "inputs", "scales")}
    fams |= {f"kpelbo.{k}" for k in ("value", "y", "noise", "z_noise", "d_coef", "d_inscale", "d_param", "inputs", "scales")}
    assert set(KT.FLOORS) == set(KT.MEASURED_FLOAT64) == fams
    for fam, vals in KT.MEASURED_FLOAT64.items():
        assert len(vals) >= 3 and KT.FLOORS[fam] == float(np.median(vals)), fam


def test_recorded_float64_figures_are_reproduced_to_a_factor_two():
    lists = {}
    for c in GK.LP_CASES + GK.ELBO_CASES:
        for fam, e in _figures(c).items():
            lists.setdefault(fam, []).append(e)
    assert set(lists) == set(KT.MEASURED_FLOAT64)
    for fam, vals in KT.MEASURED_FLOAT64.items():
        now = sorted(lists[fam])
        assert len(now) == len(vals), fam
        for a, b in zip(now, vals):
            assert max(a, 1.0) <= KT.SELF_MARGIN * max(b, 1.0) and max(b, 1.0) <= KT.SELF_MARGIN * max(a, 1.0), (fam, a, b)


# ---- the GPU file's bodies on the NumPy double, under SELF_MARGIN ----------------------------------------------------------------
# FakeKprodGrad takes a scalar Sigma_y and a scalar Sigma_z and writes every output: the two cases with a dense Sigma_z and
# the NULL-output calls are not covered
DOUBLE_ELBO_CASES = [c for c in GK.ELBO_CASES if c.z_noise == "scalar"]


@pytest.mark.parametrize("case", GK.LP_CASES, ids=repr)
def test_logpdf_body_on_the_numpy_double(case):
    assert GK.MARGIN_IN_FORCE == KT.SELF_MARGIN
    GK.test_logpdf_gradient_against_truth(case)


@pytest.mark.parametrize("case", DOUBLE_ELBO_CASES, ids=repr)
def test_elbo_body_on_the_numpy_double(case):
    GK.test_elbo_gradient_against_truth(case)


@pytest.mark.parametrize("case", GK.DIAG_CASES, ids=repr)
def test_diag_body_on_the_numpy_double(case):
    GK.test_diag_gradient_against_truth(case)


if __name__ == "__main__":          # the measurements behind kprod_grad_truth.BESSEL_MEASURED / MEASURED_FLOAT64 / FLOORS
    import pprint

    class _MP:
        def setattr(self, obj, name, value, raising=True):
            setattr(obj, name, value)

    install_fake(_MP())
    print(f"BESSEL_MEASURED = {bessel_figure():.3e}")
    lists = {}
    for c in GK.LP_CASES + GK.ELBO_CASES:
        for fam, e in _figures(c).items():
            lists.setdefault(fam, []).append(round(e, 1))
            print(f"{c.id:18s} {fam:16s} {e:10.1f}", flush=True)
    lists = {k: sorted(v) for k, v in sorted(lists.items())}
    print("MEASURED_FLOAT64 = ", end="")
    pprint.pprint(lists, width=120, compact=True)
    print("FLOORS = ", end="")
    pprint.pprint({k: float(np.median(v)) for k, v in lists.items()}, width=120)
