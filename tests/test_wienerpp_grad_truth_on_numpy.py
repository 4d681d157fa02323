"""CPU pin of the Wiener / PiecewisePolynomial gradient reference (tests/wienerpp_grad_truth.py) and of the bounds the GPU file
(tests/test_gpu_wienerpp_grad_truth.py) holds the device to.  No GPU here:

  * the long-double `factor` against the committed 60-digit table (tests/golden/wienerpp_truth.json): all 653 pairs, k, dg, dx
    and dy, under the error model of tests/wienerpp_truth.py with eps = 2^-64 plus half a float64 spacing of the table's own
    (rounded) entry; the largest figure is printed; 121 smooth pairs again in mpmath at 40 digits without that term;
  * the pin problem (N = 24, D = 3, M = 6; tests/wienerpp_grad_truth_mp.py): logpdf, the dense Titsias ELBO and the diagonal
    on one view and on two, every family of the long-double run within 1e-17 of its scale of the 40-digit values;
  * the conditions on the inputs of every case, from the reference alone: |r - 1| > 1e-12 for every PIECEWISE factor and pair,
    20 % .. 80 % of a case's pairs beyond each support, equal float64 norms only between identical points for every WIENER
    factor, cond(K + Sigma_y) <= 1e4, cond(Kzz + Sigma_z) <= 1e6;
  * central differences of the truth's own long-double logpdf at h = 2^-20 (coefficients, lengthscales of WIENER and PIECEWISE
    factors, coordinates away from r = 1 and from norm ties);
  * the float64 run against wienerpp_np / kprod_np / kprod_grad_np at the tolerances of tests/test_gpu_wienerpp.py;
  * the recorded MEASURED_FLOAT64 lists to a factor 2, the floors their medians, every bound in force 100 x inside the
    tolerance beside it (1e-8 logpdf, 2e-5 ELBO), and every body of the GPU file on the NumPy double of the entry points
    (scalar and diagonal Sigma_y, scalar and dense Sigma_z)."""
import numpy as np
import pytest

import kprod_grad_np as kg
import kprod_grad_truth as KT
import kprod_np as kn
import matern_nu_np
import stheno_jl_amd as P
import test_gpu_wienerpp_grad_truth as GW
import wienerpp_grad_truth as WG
import wienerpp_np as wn
import wienerpp_truth as wt
from test_kprod_grad_on_numpy import install_fake

SELF_MARGIN = 2.0


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    install_fake(monkeypatch)
    matern_nu_np.install(monkeypatch)
    wn.install(monkeypatch)
    monkeypatch.setattr(GW, "MARGIN_IN_FORCE", SELF_MARGIN)


# ---- the long-double factor against the 60-digit table ---------------------------------------------------------------------------
def test_long_double_factor_against_the_table(monkeypatch):
    dt = KT.require_extended()
    assert np.finfo(dt).eps < 1.1e-19
    table = wt.load()
    monkeypatch.setattr(wt, "EPS", 2.0 ** -64)
    pairs, worst = 0, (0.0, None)
    for key in table:
        kind, param = (WG.WIENER, float(key[1])) if key[0] == "w" else (WG.PIECEWISE0 + key[1], float(key[2]))
        for D, g in table[key].items():
            if not g.n:
                continue
            pairs += g.n
            X, Y = g.X.astype(dt), g.Y.astype(dt)
            with np.errstate(over="ignore", invalid="ignore"):
                f = WG.factor(kind, X, Y, param, dt, diag=True)
                got = dict(k=f["k"], dg=f["dk"], dx=f["c1"] * X + f["c2"] * (X - Y), dy=f["c1y"] * Y + f["c2"] * (Y - X))
                cap = wt.tolerances(key, g)
            for name in ("k", "dg", "dx", "dy"):
                want = g.truth[name]
                with np.errstate(over="ignore", invalid="ignore"):
                    err = np.abs(got[name] - want.astype(dt)).astype(np.float64)
                    bound = np.asarray(cap[name], dtype=np.float64) + 0.5 * np.spacing(np.abs(want))
                    ok = (got[name] == want) | (err <= bound)
                    fig = float(np.max(np.where(got[name] == want, 0.0, err / bound)))
                assert np.all(ok), (key, D, name, np.flatnonzero(~ok.ravel())[:6])
                # the exact zeros are exact (t^64 beyond float64's range, 1e-1022, is a zero of the table and not of long double)
                assert np.all(got[name][want == 0.0].astype(np.float64) == 0.0), (key, D, name)
                if fig > worst[0]:
                    worst = (fig, (key, D, name))
    print(f"long double against the table: {pairs} pair evaluations; largest error / cap {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0 and pairs == 653          # 84 point pairs, each under every kind and parameter it is listed for


def _mp_pair(mp, key, x, y):
    """(k, dg, dx, dy) of one pair at 40 digits, from the header's formulas as functions of the coordinates, differentiated
    by mpmath.diff (the pair is away from ties, the origin, d == 0 and r == 1, where k is smooth)"""
    def k_of(xs, ys):
        X, Y = mp.sqrt(sum(a * a for a in xs)), mp.sqrt(sum(b * b for b in ys))
        d = mp.sqrt(sum((a - b) ** 2 for a, b in zip(xs, ys)))
        if key[0] == "w":
            m, M, i = min(X, Y), max(X, Y), key[1]
            return (m, m ** 3 / 3 + m * m * d / 2, m ** 5 / 20 + m ** 3 * d * (X + Y - m / 2) / 12,
                    m ** 7 / 252 + m ** 4 * d * (5 * M * M + 2 * X * Y + 3 * m * m) / 720)[i]
        q, j = key[1], key[2]
        p = (1, 1 + (j + 1) * d, 1 + (j + 2) * d + mp.mpf(j * j + 4 * j + 3) / 3 * d * d,
             1 + (j + 3) * d + mp.mpf(6 * j * j + 36 * j + 45) / 15 * d * d + mp.mpf(j ** 3 + 9 * j * j + 23 * j + 15) / 15 * d ** 3)[q]
        return (1 - d) ** (j + q) * p if d < 1 else mp.mpf(0)
    D = len(x)
    at = lambda v, c, t: [t if e == c else a for e, a in enumerate(v)]      # noqa: E731
    dx = [mp.diff(lambda t, c=c: k_of(at(x, c, t), y), x[c]) for c in range(D)]
    dy = [mp.diff(lambda t, c=c: k_of(x, at(y, c, t)), y[c]) for c in range(D)]
    dg = mp.diff(lambda g: k_of([g * a for a in x], [g * b for b in y]), mp.mpf(1))
    return k_of(x, y), dg, dx, dy


def test_long_double_factor_against_mpmath_on_pairs_of_the_table():
    """up to six smooth pairs per kind and parameter (no tie, no zero norm, d > 0, |r - 1| > 1e-3, moderate norms), derived again
    at 40 digits from the table's own float64 points and compared WITHOUT the half-spacing of the table's rounding: the cap is the error
    model at eps = 2^-64 alone, plus the 1e-25 mpmath's differences are good for"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    dt = KT.require_extended()
    table = wt.load()
    done, worst = {}, 0.0
    for key in table:
        kind, param = (WG.WIENER, float(key[1])) if key[0] == "w" else (WG.PIECEWISE0 + key[1], float(key[2]))
        for D, g in table[key].items():
            if not g.n:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                nx, ny = np.sqrt(np.sum(g.X ** 2, 0)), np.sqrt(np.sum(g.Y ** 2, 0))
                r = np.sqrt(np.sum((g.X - g.Y) ** 2, 0))
                ok = (nx != ny) & (nx > 1e-3) & (ny > 1e-3) & (r > 1e-3) & (np.abs(r - 1.0) > 1e-3) & (nx < 1e3) & (ny < 1e3)
                if key[0] == "p":
                    ok &= r < 1.0
            X, Y = g.X.astype(dt), g.Y.astype(dt)
            with np.errstate(invalid="ignore", over="ignore"):
                f = WG.factor(kind, X, Y, param, dt, diag=True)
                got = dict(k=f["k"], dg=f["dk"], dx=f["c1"] * X + f["c2"] * (X - Y), dy=f["c1y"] * Y + f["c2"] * (Y - X))
            eps0 = wt.EPS
            try:
                wt.EPS = 2.0 ** -64
                with np.errstate(invalid="ignore", over="ignore"):
                    cap = wt.tolerances(key, g)
            finally:
                wt.EPS = eps0
            for i in np.flatnonzero(ok)[:max(0, 6 - done.get(key, 0))]:
                done[key] = done.get(key, 0) + 1
                x, y = [mp.mpf(float(v)) for v in g.X[:, i]], [mp.mpf(float(v)) for v in g.Y[:, i]]
                k, dg, dx, dy = _mp_pair(mp, key, x, y)
                for name, want in (("k", [k]), ("dg", [dg]), ("dx", dx), ("dy", dy)):
                    have = np.atleast_2d(got[name])[:, i] if name in ("dx", "dy") else [got[name][i]]
                    tol = np.atleast_2d(cap[name])[:, i] if name in ("dx", "dy") else [cap[name][i]]
                    for a, b, t, sp in zip(have, want, tol, np.atleast_1d(np.spacing(np.abs(np.atleast_2d(g.truth[name])[:, i] if name in ("dx", "dy") else g.truth[name][i])))):
                        # the model's `ulp` terms are float64 spacings of the table's entry: they are taken out again
                        t = max(float(t) - (float(sp) if (name != "k" and key[0] == "p") or name in ("dx", "dy") else 0.0), 0.0) + 1e-25 * max(1.0, abs(float(b)))
                        err = abs(mp.mpf(float(a)) + mp.mpf(float(a - dt(float(a)))) - b)
                        worst = max(worst, float(err / t) if t > 0 else (0.0 if err == 0 else np.inf))
                        assert err <= t, (key, D, int(i), name, float(err), t)
    print(f"long double against mpmath at 40 digits: {sum(done.values())} pairs over {len(done)} kinds; largest error / cap {worst:.3f}")
    assert len(done) == len(table) and min(done.values()) >= 2


# ---- the pin problem: chain assembly, the ELBO and the diagonal of the truth against mpmath -------------------------------------
def _pin_golden():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wienerpp_grad_truth.json")) as fh:
        return json.load(fh)["pin"]


def test_pin_problem_in_long_double_against_mpmath():
    """N = 24, D = 3, M = 6 (tests/wienerpp_grad_truth_mp.py): one chain per kind pair, a function-scaled head, logpdf, the
    ELBO in the dense Titsias form (zz, and xz with its column side), the diagonal on one view and on two.  Every family of
    the long-double run agrees with the committed 40-digit values to 1e-17 of its scale, the bound of
    tests/test_kprod_grad_truth_on_numpy.py.  The data hold a duplicate and the origin: ties, d == 0 and X == 0 are inside"""
    import wienerpp_grad_truth_mp as WM
    dt = KT.require_extended()
    pin, run = _pin_golden(), WM.long_double_run()
    assert set(pin) == set(run) and len(run) == 51
    P_ = WM.pin_problem()
    kinds = {(kind, param) for ch in P_["xx"]["chains"] for (_, kind, _, _, param) in ch["factors"]}
    assert {(WG.WIENER, float(i)) for i in range(4)} <= kinds and set(WG.PP) <= {k for k, _ in kinds}
    assert P_["xx"]["chains"][0]["rs"] is not None and not P_["xz"]["symmetric"]
    r = np.sqrt(KT.sqdist(P_["xx"]["inputs"][1], P_["xx"]["inputs"][1]))          # the PIECEWISE view: both sides of r = 1
    assert 0.2 <= np.mean(r >= 1.0) <= 0.8
    for key in sorted(run):
        got, scale = run[key]
        want = np.array([dt(s) for s in pin[key]])
        assert got.shape == want.shape, key
        err = float(np.max(np.abs(got - want) / np.where(scale > 0, scale, 1)))
        print(f"{key:26s} {err:.3e} of its scale")
        assert np.all((scale > 0) | (got == want)) and err <= 1e-17, (key, err)


def test_committed_pin_values_are_what_mpmath_gives_here():
    mp = pytest.importorskip("mpmath")
    import wienerpp_grad_truth_mp as WM
    want, got = _pin_golden(), WM.pin_values()
    assert set(want) == set(got)
    for key in want:
        assert len(want[key]) == len(got[key]), key
        for a, b in zip(want[key], got[key]):
            a, b = mp.mpf(a), mp.mpf(b)
            assert abs(a - b) <= mp.mpf("1e-23") * max(abs(a), abs(b)), (key, a, b)


# ---- the conditions on the inputs ------------------------------------------------------------------------------------------------
COND_CAP_LOGPDF, COND_CAP_ELBO = 1e4, 1e6


@pytest.mark.parametrize("case", WG.CASES, ids=lambda c: c[0])
def test_conditions_on_the_inputs(case):
    F, x, z, noise, sz, y = WG.problem(case)
    sps = WG.specs(case)
    assert all(WG.launch_classes(sp) == GW.DMAX_OF[case[0]] for sp in sps)
    for sp in sps:
        S = KT.read_spec(sp)
        beyond, pairs, nearest = {}, {}, np.inf
        for ch in S["chains"]:
            for (t, kind, ri, ci, param) in ch["factors"]:
                Xr, Xc = S["inputs"][ri], S["inputs"][ci]
                if kind in WG.PP:
                    r = np.sqrt(KT.sqdist(Xr, Xc))
                    nearest = min(nearest, float(np.min(np.abs(r - 1.0))))
                    beyond[kind] = beyond.get(kind, 0) + int(np.sum(r >= 1.0))
                    pairs[kind] = pairs.get(kind, 0) + r.size
                if kind == WG.WIENER:
                    pts = np.hstack([Xr, Xc])
                    nrm = np.sqrt(np.sum(pts * pts, 0))
                    tie = nrm[:, None] == nrm[None, :]
                    same = np.all(pts[:, :, None] == pts[:, None, :], axis=0)
                    assert np.array_equal(tie, same), (case[0], t, "a norm tie between different points")
        for kind in beyond:
            share = beyond[kind] / pairs[kind]
            print(f"{case[0]:18s} PIECEWISE{kind - WG.PIECEWISE0}: {100 * share:.0f} % of {pairs[kind]} pairs beyond the support, "
                  f"smallest |r - 1| {nearest:.2e}")
            assert nearest > 1e-12
            if sp is sps[-1]:                   # the data's own pairs are the case's pairs
                assert 0.2 <= share <= 0.8, (case[0], kind, share)
    K = WG.dense(KT.read_spec(sps[-1]), np.float64)
    cond = float(np.linalg.cond(K + (np.diag(noise) if np.ndim(noise) else noise * np.eye(len(K)))))
    print(f"{case[0]:18s} cond(K + Sigma_y) = {cond:.3e}")
    assert cond <= COND_CAP_LOGPDF
    if z is not None:
        Kz = WG.dense(KT.read_spec(sps[0]), np.float64)
        cz = float(np.linalg.cond(Kz + (sz if np.ndim(sz) else sz * np.eye(len(Kz)))))
        print(f"{case[0]:18s} cond(Kzz + Sigma_z) = {cz:.3e}")
        assert cz <= COND_CAP_ELBO


def test_whole_point_wiener_case_factors_in_long_double_with_the_recorded_coefficient():
    case = WG.CASES[[c[0] for c in WG.CASES].index("wp-wfull-D3")]
    S = KT.read_spec(WG.specs(case)[0])
    assert sorted(ch["coef"] for ch in S["chains"] if ch["factors"][0][1] == WG.WIENER)[0] == WG.WFULL_COEF == 0.05
    assert any(kind == WG.WIENER and S["inputs"][ri].shape[0] == 3 for ch in S["chains"] for (_, kind, ri, _, _) in ch["factors"])
    assert np.all(np.isfinite(np.asarray(WG.truth(case)[0]["value"], dtype=np.float64)))


def test_a_kind_10_factor_reaches_this_modules_factor_through_dense_diag_of_and_contract(monkeypatch):
    """WG.dense, diag_of and contract are DG's code run with WG.factor in its globals: this fails if DG stops calling `factor`
    and testing `DOT` directly in those three functions"""
    seen = []
    real = WG.factor
    X = np.random.default_rng(1).uniform(0.1, 0.9, (1, 5))
    S = KT.hand_spec([dict(I=0, J=0, head=0, coef=1.0, rs=None, cs=None, factors=[(0, WG.WIENER, 0, 0, 1.0)])], [X], [5], [5], True)
    for fn in (WG.dense, WG.diag_of, lambda S, dt: WG.contract(S, np.ones((5, 5)), dt, inputs=True)):
        for f in (WG.dense, WG.diag_of, WG.contract):
            monkeypatch.setitem(f.__globals__, "factor", lambda kind, *a, **k: (seen.append(kind), real(kind, *a, **k))[1])
        n = len(seen)
        out = fn(S, np.float64)
        assert len(seen) > n and seen[-1] == WG.WIENER
    assert np.all(out["gx"][0] != 0.0)          # and the coefficient route carried its point derivatives


# ---- the float64 run against the existing evaluators --------------------------------------------------------------------------------
def _close(a, e, tol=1e-8):
    a, e = np.asarray(a, dtype=float), np.asarray(e, dtype=float)
    return float(np.max(np.abs(a - e), initial=0.0)) <= tol * max(1.0, float(np.max(np.abs(e), initial=0.0)))


@pytest.mark.parametrize("case", WG.CASES, ids=lambda c: c[0])
def test_float64_run_matches_the_existing_evaluators(case):
    sps = WG.specs(case)
    rng = np.random.default_rng(5)
    spec = sps[-1]
    S = KT.read_spec(spec)
    K = WG.dense(S, np.float64)
    assert _close(K, kn.np_spec_matrix(spec), 1e-13)
    G = rng.standard_normal(K.shape)
    G = G + G.T
    R = WG.contract(S, G, np.float64, inputs=True, scales=True)
    for a, e in zip((R["d_coef"], R["d_inscale"], R["d_param"]), kn.np_contract(spec, G)):
        assert _close(a, e)
    ev = kg.np_input_grads(spec, G)
    for a, e in zip(R["gx"], ev["row"]):
        assert _close(a, 2.0 * e)
    if len(sps) == 3:                           # the rectangular spec: the column side takes c1y
        spec = sps[1]
        S = KT.read_spec(spec)
        G = rng.standard_normal((spec.N, spec.M))
        R = WG.contract(S, G, np.float64, inputs=True, scales=True)
        for a, e in zip((R["d_coef"], R["d_inscale"], R["d_param"]), kn.np_contract(spec, G)):
            assert _close(a, e)
        ev = kg.np_input_grads(spec, G)
        for a, r, c in zip(R["gx"], ev["row"], ev["col"]):
            assert _close(a, r + c)


@pytest.mark.parametrize("case", WG.DIAG_CASES, ids=lambda c: c[0])
def test_float64_diagonal_matches_the_existing_evaluator(case):
    spec, w = WG.diag_problem(case)
    S = KT.read_spec(spec)
    Dg, ed = WG.diag_grad(S, w, np.float64), kg.np_diag_grads(spec, w)
    assert _close(WG.diag_of(S, np.float64), kg.np_diag(spec), 1e-13)
    assert _close(Dg["d_coef"], ed["gc"]) and _close(Dg["d_inscale"], ed["gs"]) and _close(Dg["d_param"], ed["gp"])
    for a, e in zip(Dg["gx"], ed["gx"]):
        assert _close(a, e)


# ---- the truth against itself -----------------------------------------------------------------------------------------------------
H = 2.0 ** -20
CD_NOISE = 0.1


def _cd_problem():
    """N = 24, D = 3; every factor reads the points (input 0) or their first coordinate (input 1) directly, so a coordinate can
    be moved.  Coordinates in (0.05, 0.45): every r < 0.7, away from r = 1, and no two norms tie"""
    rng = np.random.default_rng(77)
    X = rng.uniform(0.05, 0.45, (3, 24))
    f = lambda t, kind, inp, param: (t, kind, inp, inp, param)      # noqa: E731
    chains = [dict(I=0, J=0, head=0, coef=1.3, rs=None, cs=None, factors=[f(0, WG.WIENER, 1, 1.0), f(1, KT.SE, 0, 0.0)]),
              dict(I=0, J=0, head=2, coef=0.6, rs=None, cs=None, factors=[f(2, WG.PIECEWISE0 + 2, 0, 4.0)]),
              dict(I=0, J=0, head=3, coef=0.9, rs=None, cs=None, factors=[f(3, WG.WIENER, 0, 2.0), f(4, WG.PIECEWISE0, 0, 2.0)]),
              dict(I=0, J=0, head=5, coef=0.8, rs=None, cs=None, factors=[f(5, WG.WIENER, 1, 3.0), f(6, WG.PIECEWISE0 + 3, 0, 5.0)]),
              dict(I=0, J=0, head=7, coef=0.5, rs=None, cs=None, factors=[f(7, WG.WIENER, 1, 0.0), f(8, WG.PIECEWISE0 + 1, 0, 3.0)])]
    return KT.hand_spec(chains, [X, X[:1]], [24], [24], True), rng.standard_normal(24)


def _logpdf_value(S, y, dt):
    n = len(y)
    K = WG.dense(S, dt)
    Lm = KT.cholesky(np.tril(K) + np.tril(K, -1).T + KT.noise_matrix(KT.NOISE_SCALAR, CD_NOISE, n, dt))
    z = KT.tri_inverse(Lm) @ y.astype(dt)
    return -(dt(n) * np.log(dt(2) * KT.T._pi(dt)) + dt(2) * np.log(np.diag(Lm)).sum() + z @ z) / dt(2)


def test_truth_agrees_with_central_differences_of_its_own_logpdf():
    """tolerance h^2 |f'''| / 6 + 64 eps_ld S / h, |f'''| from the central differences at 2 h and h
    (tests/test_kprod_grad_truth_on_numpy.py)"""
    dt = KT.require_extended()
    S0, y = _cd_problem()
    X = S0["inputs"][0]

    def value(coef=None, scale=None, point=None):
        inputs = [a.astype(dt) for a in S0["inputs"]]
        if point is not None:
            d, i, h = point
            Xp = X.astype(dt).copy()
            Xp[d, i] += dt(h)
            inputs = [Xp, Xp[:1]]
        chains = []
        for c, ch in enumerate(S0["chains"]):
            ch = dict(ch, coef=ch["coef"] + (coef[1] if coef is not None and coef[0] == c else 0.0))
            fac = []
            for (u, k, ri, ci, p) in ch["factors"]:
                if scale is not None and u == scale[0]:          # the factor's own copy of its view, scaled
                    inputs.append(inputs[ri] * (dt(1) + dt(scale[1])))
                    ri = ci = len(inputs) - 1
                fac.append((u, k, ri, ci, p))
            chains.append(dict(ch, factors=fac))
        return _logpdf_value(dict(S0, chains=chains, inputs=inputs), y, dt)

    R = WG.logpdf_grad(S0, KT.NOISE_SCALAR, CD_NOISE, np.zeros(24), y, dt, inputs=True, scales=True)
    round_tol = 64 * float(np.finfo(np.longdouble).eps) * float(R["S_value"]) / H
    checks = []
    for c, ch in enumerate(S0["chains"]):
        checks.append((f"coef[{c}]", R["d_coef"][ch["head"]], lambda h, c=c: value(coef=(c, h))))
        for (t, kind, _, _, _) in ch["factors"]:
            assert R["d_param"][t] == 0
            if kind in WG.WPP:
                checks.append((f"inscale[{t}]", R["d_inscale"][t], lambda h, t=t: value(scale=(t, h))))
    for d, i in ((0, 0), (1, 5), (2, 11), (0, 23)):
        want = R["gx"][0][d, i] + (R["gx"][1][0, i] if d == 0 else 0)
        checks.append((f"x[{d},{i}]", want, lambda h, d=d, i=i: value(point=(d, i, h))))
    assert len(checks) == 5 + 8 + 4
    moved = 0
    for name, want, f in checks:
        cd1 = (f(H) - f(-H)) / dt(2 * H)
        cd2 = (f(2 * H) - f(-2 * H)) / dt(4 * H)
        tol = H ** 2 * (4.0 * float(abs(cd2 - cd1)) / H ** 2) / 6 + round_tol
        err = float(abs(cd1 - want))
        print(f"{name:14s} analytic {float(want):+.12e}  error {err:.2e}  tolerance {tol:.2e}")
        assert err <= tol, (name, err, tol)
        moved += abs(float(want)) > 1e3 * tol
    assert moved >= len(checks) - 3


# ---- the bounds, on the reference's own float64 runs --------------------------------------------------------------------------------
def test_floors_are_the_medians_and_the_recorded_figures_are_reproduced_to_a_factor_two():
    assert WG.FLOORS == {fam: float(np.median(v)) for fam, v in WG.MEASURED_FLOAT64.items()} and len(WG.CASES) == 16
    lists = {}
    for c in WG.CASES:
        for fam, e in WG.reference_figures(c).items():
            lists.setdefault(fam, []).append(e)
    assert set(lists) == set(WG.MEASURED_FLOAT64)
    for fam, vals in WG.MEASURED_FLOAT64.items():
        now = sorted(lists[fam])
        assert len(now) == len(vals), fam
        for a, b in zip(now, vals):
            assert max(a, 1.0) <= SELF_MARGIN * max(b, 1.0) and max(b, 1.0) <= SELF_MARGIN * max(a, 1.0), (fam, a, b)


OLD_TOLERANCE = {"lp": 1e-8, "elbo": 2e-5}          # tests/test_gpu_wienerpp.py


@pytest.mark.parametrize("case", WG.CASES, ids=lambda c: c[0])
def test_bound_in_force_is_100x_inside_the_tolerance_beside_it(case):
    """no exception had to be named"""
    for fam, e in WG.reference_figures(case).items():
        bound = WG.MARGIN * max(e, WG.FLOORS[fam]) * WG.EPS
        print(f"{case[0]:18s} {fam:16s} bound {bound:.2e}   tolerance beside it {OLD_TOLERANCE[case[1]]:.0e}")
        assert np.isfinite(e) and bound <= OLD_TOLERANCE[case[1]] / 100.0, (case[0], fam, bound)


@pytest.mark.parametrize("case", WG.DIAG_CASES, ids=lambda c: c[0])
def test_diagonal_model_bound_is_tight(case):
    R = WG.diag_truth(case)
    worst = float(np.max((R["dim"] + 8.0 + R["amp"]) * WG.EPS))
    print(f"{case[0]:18s} (D + 8 + sum amp) eps = {worst:.3e}")
    assert worst <= 1e-8 / 100.0


# ---- the GPU file's bodies on the NumPy double ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in WG.CASES if c[1] == "lp"], ids=lambda c: c[0])
def test_logpdf_body_on_the_numpy_double(case):
    GW.test_logpdf_gradient_against_truth(case)


@pytest.mark.parametrize("case", [c for c in WG.CASES if c[1] == "elbo"], ids=lambda c: c[0])
def test_elbo_body_on_the_numpy_double(case):
    GW.test_elbo_gradient_against_truth(case)


@pytest.mark.parametrize("case", WG.DIAG_CASES, ids=lambda c: c[0])
def test_diag_body_on_the_numpy_double(case):
    GW.test_diag_gradient_against_truth(case)


@pytest.mark.parametrize("key,D", GW._table_groups(), ids=lambda v: str(v).replace(" ", ""))
def test_table_body_on_the_numpy_double(key, D):
    GW.test_derivative_routines_against_the_table(key, D)
