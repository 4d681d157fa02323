"""CPU pin of the forward-path reference (tests/forward_truth.py) and of the bounds the GPU file
(tests/test_gpu_forward_truth.py) holds the device to.  No GPU here:

  * one small problem (N = 24, N* = 5, M = 6, D = 3, all four stationary kernels, diagonal noise; 16 points and the stacked
    24 of an extension / a VFE update) is recomputed at 40 digits with mpmath, the sparse families in the dense Titsias form
    (another algebra than the reference's Lz / Le form); every long-double family must agree to 1e-17 of its scale;
  * the float64 run against the oracle at the tolerances the GPU suite has used so far;
  * every case body of the GPU file on the NumPy double of the C-ABI (LAPACK solves), held to SELF_MARGIN;
  * the stored MEASURED_FLOAT64 reproduce and FLOORS are their medians;
  * case by case, how much tighter the bound in force is than the tolerance it sits beside;
  * predgrad_truth's outputs after the refactor onto the shared cores, bit for bit (tests/golden/predgrad_truth_pin.npz).

`python tests/test_forward_truth_on_numpy.py` prints the float64 figures of every case and family: the lists recorded in
forward_truth.MEASURED_FLOAT64."""
import os

import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (registers the product package, as under pytest)

import forward_truth as FT
import grad_truth as T
import np_capi
import predgrad_np
import predgrad_truth as PT
import test_extend_on_numpy_double as EX
import test_gpu_forward_truth as G
import test_vfe_update_on_numpy_double as VU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predgrad_truth_pin.npz")


def install(monkeypatch):
    """the NumPy double with the prediction-gradient, extension and VFE-update entry points the other CPU files teach it"""
    ctx = predgrad_np.install(monkeypatch)
    FL = np_capi.FakeLib
    monkeypatch.setattr(FL, "_create0", FL.sgp_posterior_create, raising=False)
    monkeypatch.setattr(FL, "sgp_posterior_create", EX._create)
    monkeypatch.setattr(FL, "sgp_posterior_extend", EX._extend, raising=False)
    monkeypatch.setattr(FL, "_screate0", FL.sgp_sparse_posterior_create, raising=False)
    monkeypatch.setattr(FL, "sgp_sparse_posterior_create", VU._create)
    monkeypatch.setattr(FL, "sgp_sparse_posterior_update", VU._update, raising=False)
    monkeypatch.setattr(FL, "sgp_sparse_posterior_count", VU._count, raising=False)
    ctx.lib.extend_calls, ctx.lib.post_noise, ctx.lib.update_calls, ctx.lib.sums = [], {}, [], {}
    ctx.extend = ctx.vfe_update = ctx.lib
    return ctx


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    install(monkeypatch)


# ---- mpmath pin ----------------------------------------------------------------------------------------------------------
COEFS = (0.5, 0.4, 0.3, 0.2)


def _hand_spec(A, B, sym):
    terms = [(0, 0, kind, 0, 1, COEFS[kind], 0.0, None, None) for kind in range(4)]
    return dict(terms=terms, inputs=[A, B], row_len=[A.shape[1]], col_len=[B.shape[1]], symmetric=sym)


def _mp_kernel(mp, d2):
    d = mp.sqrt(d2)
    s3, s5 = mp.sqrt(3) * d, mp.sqrt(5) * d
    ks = (mp.exp(-d2 / 2), mp.exp(-d), (1 + s3) * mp.exp(-s3), (1 + s5 + s5 * s5 / 3) * mp.exp(-s5))
    return sum(mp.mpf(c) * k for c, k in zip(COEFS, ks))


def _mp_K(mp, A, B):
    K = mp.matrix(A.shape[1], B.shape[1])
    for i in range(A.shape[1]):
        for j in range(B.shape[1]):
            K[i, j] = _mp_kernel(mp, sum((mp.mpf(float(A[d, i])) - mp.mpf(float(B[d, j]))) ** 2 for d in range(A.shape[0])))
    return K


def _ld(x):
    """an mpmath number or matrix as long double (25 digits carry more than its 64 bits)"""
    import mpmath
    if isinstance(x, mpmath.matrix):
        a = np.array([[np.longdouble(mpmath.nstr(x[i, j], 25)) for j in range(x.cols)] for i in range(x.rows)])
        return a[:, 0] if x.cols == 1 else a
    return np.longdouble(mpmath.nstr(x, 25))


def _vec(mp, v):
    return mp.matrix([mp.mpf(float(a)) for a in v])


def _agree(units_by_family):
    for fam, u in units_by_family.items():
        print(f"{fam:16s} {u * T.EPS:.3e} of its scale")
        assert u * T.EPS <= 1e-17, (fam, u * T.EPS)


@pytest.mark.parametrize("n", [16, 24], ids=["create", "stacked"])
def test_long_double_reference_against_mpmath_at_40_digits(n):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    dt = T.require_extended()
    rng = np.random.default_rng(88)
    D, N, ns, M = 3, 24, 5, 6
    X, Xs, Z = (rng.standard_normal((D, k)) / np.sqrt(D) * 1.5 for k in (N, ns, M))
    y, mean, ms = rng.standard_normal(N), 0.1 * rng.standard_normal(N), 0.2 * rng.standard_normal(ns)
    noise = 0.05 + 0.25 * rng.random(N)
    Zr = rng.standard_normal((N, 2))
    X, y, mean, noise, Zr = X[:, :n], y[:n], mean[:n], noise[:n], Zr[:n]          # the create call's 16, or the stacked 24
    log2pi = mp.log(2 * mp.pi)

    # ---- exact: C^-1 by LU, the variance through the inverse (the reference: Cholesky recurrences and V = L^-1 K*')
    R = FT.posterior(_hand_spec(X, X, True), T.NOISE_DIAG, noise, mean, y, _hand_spec(Xs, X, False), _hand_spec(Xs, Xs, True),
                     ms, dt)
    Cm = _mp_K(mp, X, X)
    for i in range(n):
        Cm[i, i] += mp.mpf(float(noise[i]))
    Ci = mp.inverse(Cm)
    delta = _vec(mp, y) - _vec(mp, mean)
    alpha = Ci * delta
    Ks, Kss = _mp_K(mp, Xs, X), _mp_K(mp, Xs, Xs)
    cov = Kss - Ks * Ci * Ks.T
    Lm = mp.cholesky(Cm)
    lp = -(n * log2pi + 2 * sum(mp.log(Lm[i, i]) for i in range(n)) + (delta.T * alpha)[0]) / 2
    out = dict(alpha=_ld(alpha), mean=_ld(_vec(mp, ms) + Ks * alpha), var=np.diag(_ld(cov)).copy(), cov=_ld(cov), logpdf_y=_ld(lp))
    _agree(FT.posterior_units("post" if n == 16 else "ext", out, R))

    # ---- rand
    Rr = FT.rand(_hand_spec(X, X, True), T.NOISE_DIAG, noise, mean, Zr, dt)
    Zm = mp.matrix(n, 2)
    for i in range(n):
        for j in range(2):
            Zm[i, j] = mp.mpf(float(Zr[i, j]))
    draw = Lm * Zm
    for i in range(n):
        for j in range(2):
            draw[i, j] += mp.mpf(float(mean[i]))
    _agree(FT.rand_units(_ld(draw), Rr))

    # ---- sparse, in the dense Titsias form: Qm = Kzz + Kzx S^-1 Kxz, q = N(m, Kxz Kzz^-1 Kzx + S)
    sz = 1e-2
    Rs = FT.sparse_posterior(_hand_spec(Z, Z, True), T.NOISE_SCALAR, sz, _hand_spec(X, Z, False), T.NOISE_DIAG, noise, mean, y,
                             _hand_spec(X, X, True), _hand_spec(Xs, Z, False), _hand_spec(Xs, Xs, True), ms, dt)
    Kzz, Kxz, Ksz = _mp_K(mp, Z, Z), _mp_K(mp, X, Z), _mp_K(mp, Xs, Z)
    for i in range(M):
        Kzz[i, i] += mp.mpf(sz)
    Si = mp.diag([1 / mp.mpf(float(s)) for s in noise])
    Qi = mp.inverse(Kzz + Kxz.T * Si * Kxz)
    Kzzi = mp.inverse(Kzz)
    smean = _vec(mp, ms) + Ksz * (Qi * (Kxz.T * (Si * delta)))
    scov = Kss - Ksz * Kzzi * Ksz.T + Ksz * Qi * Ksz.T
    Qxx = Kxz * Kzzi * Kxz.T
    Cq = Qxx.copy()
    for i in range(n):
        Cq[i, i] += mp.mpf(float(noise[i]))
    Lq = mp.cholesky(Cq)
    quad = (delta.T * mp.inverse(Cq) * delta)[0]
    kxx = _mp_kernel(mp, mp.mpf(0))
    trace = sum((kxx - Qxx[i, i]) / mp.mpf(float(noise[i])) for i in range(n))
    elbo = -(n * log2pi + 2 * sum(mp.log(Lq[i, i]) for i in range(n)) + quad) / 2 - trace / 2
    outs = dict(mean=_ld(smean), var=np.diag(_ld(scov)).copy(), cov=_ld(scov), elbo=_ld(elbo))
    _agree(FT.sparse_units("spost" if n == 16 else "vupd", outs, Rs))


# ---- the float64 run against the oracle at the tolerances of the GPU suite so far -----------------------------------------------
def test_float64_run_against_the_oracle_at_the_old_tolerances():
    import models
    import oracle.abstractgps as oagp
    import oracle.kernelfunctions as okf
    import oracle.stheno as ost
    import stheno_jl_amd as P
    rng = np.random.default_rng(5)
    fo, go = models.gppp_docstring(models.oracle_api())
    fp, gp = models.gppp_docstring(models.product_api())
    Fo, Fp = ost.GPPP(fo, go), P.GPPP(fp, gp)
    D, n1, n2, ns, M = 2, 60, 25, 11, 17
    X1, X2, Xs, Z = (np.asfortranarray(rng.standard_normal((D, k))) for k in (n1, n2, ns, M))
    y = rng.standard_normal(n1 + n2)
    noise = 0.1 + rng.random(n1 + n2)
    Zr = rng.standard_normal((n1 + n2, 2))
    ino = lambda k, x: ost.GPPPInput(k, okf.ColVecs(x))   # noqa: E731
    inp = lambda k, x: P.GPPPInput(k, P.ColVecs(x))       # noqa: E731
    xo, xp = ost.BlockData([ino("f3", X1), ino("f1", X2)]), P.BlockData([inp("f3", X1), inp("f1", X2)])
    to, tp = ino("f2", Xs), inp("f2", Xs)
    zo, zp = ino("f3", Z), inp("f3", Z)
    spec = lambda *a: T.read_spec(P.build_spec(*a)[0])    # noqa: E731
    zero_x, zero_s = np.zeros(n1 + n2), np.zeros(ns)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))   # noqa: E731
    # exact (the stacked data: what an extension is held to)
    po = oagp.posterior(Fo(xo, noise), y)
    R = FT.posterior(spec(Fp, xp), T.NOISE_DIAG, noise, zero_x, y, spec(Fp, tp, Fp, xp), spec(Fp, tp), zero_s, np.float64)
    assert rel(R["alpha"], po.alpha) < 1e-9
    mo, vo = po.mean_and_var(to)
    assert np.max(np.abs(R["mean"] - mo)) < 1e-9 and np.max(np.abs(R["var"] - vo)) < 1e-9
    assert np.max(np.abs(R["cov"] - po.cov(to))) < 1e-9
    lp = oagp.logpdf(Fo(xo, noise), y)
    assert abs(R["logpdf_y"] - lp) <= 1e-10 * abs(lp)
    # rand
    Rr = FT.rand(spec(Fp, xp), T.NOISE_DIAG, noise, zero_x, Zr, np.float64)
    assert rel(Rr["rand"], oagp.rand(Fo(xo, noise), Zr)) < 1e-11
    # sparse (Sigma_z = 1e-6, as the update tests)
    vfe = oagp.VFE(Fo(zo, 1e-6))
    pv = oagp.posterior_vfe(vfe, Fo(xo, noise), y)
    Rs = FT.sparse_posterior(spec(Fp, zp), T.NOISE_SCALAR, 1e-6, spec(Fp, xp, Fp, zp), T.NOISE_DIAG, noise, zero_x, y,
                             spec(Fp, xp), spec(Fp, tp, Fp, zp), spec(Fp, tp), zero_s, np.float64)
    eo = oagp.elbo(vfe, Fo(xo, noise), y)
    assert abs(Rs["elbo"] - eo) <= 1e-9 * abs(eo)
    assert rel(Rs["mean"], pv.mean(to)) < 1e-7
    assert np.max(np.abs(Rs["var"] - pv.var(to))) < 1e-8 and np.max(np.abs(Rs["cov"] - pv.cov(to))) < 1e-8


# ---- every case body of the GPU file on the double, and the reference's own figures ----------------------------------------------
class _MP:
    """what the case bodies use of pytest's monkeypatch, for the script below"""

    def setattr(self, obj, name, value, raising=True):
        setattr(obj, name, value)

    def setenv(self, name, value):
        pass


def _run(case, monkeypatch):
    """(figures of the library that is loaded, figures of the reference's float64 runs) of a case"""
    if case.kind == "post":
        out, (R, *R64), _ = G.run_post(case)
        fn = lambda o, r: FT.posterior_units("post", {k: o[k] for k in ("alpha", "mean", "var", "cov")}, r)   # noqa: E731
    elif case.kind == "ext":
        out, (R, *R64), _ = G.run_ext(case)
        fn = lambda o, r: FT.posterior_units("ext", o, r)   # noqa: E731
    elif case.kind == "rand":
        out, (R, *R64) = G.run_rand(case)
        return FT.rand_units(out, R), G.GT.yardstick(FT.rand_units(r["rand"], R) for r in R64)
    else:
        out, (R, *R64) = G.run_sparse(case, None, monkeypatch) if case.kind == "spost" else G.run_vupd(case, monkeypatch)
        fn = lambda o, r: FT.sparse_units(case.kind, o, r)   # noqa: E731
    return fn(out, R), G.yardstick(fn, R, R64)


def _bound(fam, e):
    return FT.MARGIN * max(e, FT.FLOORS[fam]) * FT.EPS


# families whose bound is less than 100 x tighter than the tolerance beside it, with the reason
# (docs/04_oracle_and_parity.md has the figures)
LESS_THAN_100 = {
    # 513 points on a line (D = 1, the worst-conditioned draw) under the tightest of the old tolerances, 1e-11: the float64
    # reference itself is 398 units from the truth there, and 8 x 398 eps is 28 x inside 1e-11
    ("rand-N513-S1", "rand"): "D = 1 conditioning against a tolerance of 1e-11",
}


@pytest.mark.parametrize("case", G.ALL_CASES, ids=repr)
def test_the_doubles_figures_and_the_tightening_of_every_bound(case, monkeypatch):
    """the GPU file's body on the NumPy double (LAPACK solves) under SELF_MARGIN, so that a mistake in the case list, the
    marshalling or the unit bookkeeping shows here and not first on the device; and how much tighter each bound in force is
    than the tolerance it sits beside"""
    dev, f64 = _run(case, monkeypatch)
    for fam in sorted(dev):
        ratio = FT.OLD_TOLERANCE[fam] / _bound(fam, f64[fam])
        print(f"{case.id:26s} {fam:13s} double {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {FT.FLOORS[fam]:8.1f}  "
              f"tighter x {ratio:.0f}")
        assert np.isfinite(f64[fam])
        assert dev[fam] <= FT.SELF_MARGIN * max(f64[fam], FT.FLOORS[fam]), (case.id, fam, dev[fam], f64[fam])
        if (case.id, fam) in LESS_THAN_100:
            assert ratio >= 1.0, (case.id, fam, ratio)
        else:
            assert ratio >= 100.0, (case.id, fam, ratio)


def _measure(monkeypatch):
    lists = {}
    for c in G.ALL_CASES:
        for fam, e in _run(c, monkeypatch)[1].items():
            lists.setdefault(fam, []).append(e)
            print(f"{c.id:26s} {fam:13s} {e:10.1f}", flush=True)
    return {k: sorted(round(v, 1) for v in vs) for k, vs in lists.items()}


def test_stored_float64_figures_reproduce_and_floors_are_their_medians(monkeypatch):
    """the lists are the figures of this file's script.  Figure by figure they reproduce to the recorded digit where the BLAS
    sums in the recorded order; another summation order moves a figure by its own size at most, so the comparison allows a
    factor SELF_MARGIN on figures above one unit (those below are rounding noise of the comparison itself)"""
    assert set(FT.FLOORS) == set(FT.MEASURED_FLOAT64) == set(FT.OLD_TOLERANCE)
    now = _measure(monkeypatch)
    assert set(now) == set(FT.MEASURED_FLOAT64)
    for fam, vals in FT.MEASURED_FLOAT64.items():
        assert len(vals) >= 4 and FT.FLOORS[fam] == float(np.median(vals)), fam
        assert len(vals) == len(now[fam]), fam
        for a, b in zip(now[fam], vals):
            assert max(a, 1.0) <= FT.SELF_MARGIN * max(b, 1.0) and max(b, 1.0) <= FT.SELF_MARGIN * max(a, 1.0), (fam, a, b)


# ---- predgrad_truth after the refactor ----------------------------------------------------------------------------------
def _predgrad_pin():
    """predict_grad and sparse_predict_grad on a hand-written problem, long double and float64, every output"""
    rng = np.random.default_rng(61)
    D, n, ns, m = 2, 14, 5, 6
    X, Xs, Z = (rng.standard_normal((D, k)) for k in (n, ns, m))
    y, mean, ms = rng.standard_normal(n), 0.1 * rng.standard_normal(n), np.full(ns, 0.2)
    noise = 0.05 + 0.25 * rng.random(n)
    out = {}
    for tag, dt in (("ld", T.require_extended()), ("f64", np.float64)):
        runs = {"exact": PT.predict_grad(_hand_spec(X, X, True), T.NOISE_DIAG, noise, mean, y, _hand_spec(Xs, X, False),
                                         _hand_spec(Xs, Xs, True), ms, dt),
                "sparse": PT.sparse_predict_grad(_hand_spec(Z, Z, True), T.NOISE_SCALAR, 1e-2, _hand_spec(X, Z, False),
                                                 T.NOISE_DIAG, noise, mean, y, _hand_spec(Xs, Z, False), _hand_spec(Xs, Xs, True),
                                                 ms, dt)}
        for name, R in runs.items():
            for key in ("mean", "S_mean", "var", "S_var", "alpha", "B", "Q"):
                out[f"{tag}.{name}.{key}"] = np.ascontiguousarray(R[key])
            for key in ("gm", "Sn_gm", "gv", "Sn_gv", "gp", "S_gp"):
                for k, a in enumerate(R[key]):
                    out[f"{tag}.{name}.{key}.{k}"] = np.ascontiguousarray(a)
    # a long double as two float64 (value and remainder: 106 bits hold its 64), so that no padding byte is compared
    pin = {}
    for k, v in out.items():
        hi = v.astype(np.float64)
        pin[k] = np.stack([hi, (v - hi.astype(v.dtype)).astype(np.float64)])
    return pin


def test_predgrad_truth_outputs_did_not_move_by_a_bit():
    """the golden file was written by the module as it was before exact_core / sparse_core were factored out"""
    T.require_extended()
    want = np.load(GOLDEN)
    got = _predgrad_pin()
    assert set(got) == set(want.files)
    for k in got:
        assert np.array_equal(got[k], want[k]), k


def test_predgrad_truths_recorded_lists_are_what_they_were():
    assert PT.MEASURED_FLOAT64["pred.var_x"][-1] == 96248.1 and PT.FLOORS == {"pred.mean_x": 59.95, "pred.var_x": 630.95,
                                                                              "spred.mean_x": 141.2, "spred.var_x": 45.35}


if __name__ == "__main__":          # the measurement behind forward_truth.FLOORS / MEASURED_FLOAT64
    import pprint
    install(_MP())
    lists = _measure(_MP())
    print("MEASURED_FLOAT64 = ", end="")
    pprint.pprint(lists, width=120, compact=True)
    print("FLOORS = ", end="")
    pprint.pprint({k: float(np.median(v)) for k, v in lists.items()})
