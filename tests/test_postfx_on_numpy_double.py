"""`rand` / `logpdf` of a posterior FiniteGP -> sgp_posterior_rand / sgp_posterior_logpdf (and the sparse forms) WITHOUT a
GPU: which processes the host mirror sends down the new route, what it marshals (the cross and prior specs, the prior mean,
the three noise kinds, vector and matrix Y, S=None), the PosDefException mapping and the fallback to the host route, against
the NumPy double of the C-ABI (tests/np_capi.py).  The double learns the four entry points here from the words of
include/sthenomi_postfx.h: out = mean* + chol(C* + S*) Z, or the logpdf of every column of Y under N(mean*, C* + S*), with
mean* and C* what sgp_posterior_predict / sgp_sparse_posterior_predict answer for the same cross / prior_ss / mean_s;
rc > 0 is the LAPACK info of C* + S*, rc < 0 a refusal (a sharded posterior, sizes that do not match).  Its results are held
to the oracle at the tolerances of tests/test_gpu_parity.py.  That the device route keeps the bits of the host route is
tests/test_gpu_postfx.py's business."""
import numpy as np
import pytest
import scipy.linalg as sla

import models
import np_capi
import oracle.abstractgps as oagp
import oracle.stheno as ost
import stheno_jl_amd as P

L = P.lib
REL = 1e-10            # tests/test_gpu_parity.py: logpdf against the oracle
REL_RAND = 1e-11       # ... and rand with the same Z


def _moments(self, predict, post, cross, prior_ss, mean_s, who):
    """(mean*, C*) through the double's own predict entry point, or an rc < 0"""
    sc, sp = np_capi._Spec(cross), np_capi._Spec(prior_ss)
    n_train = (self.posts[id(post)][0] if predict == "sgp_posterior_predict" else self.sposts[id(post)][0]).shape[0]
    if id(post) in self.sharded:
        return None, None, self._fail(who + ": a posterior of a multi-GPU context (sharded factor) is not sampled or scored on the device")
    if sc.M != n_train or sp.N != sc.N or sp.M != sc.N or not sp.symmetric:
        return None, None, self._fail(who + ": sizes do not match")
    ns = sc.N
    mo, co = np.zeros(ns), np.zeros((ns, ns), order="F")
    rc = getattr(self, predict)(post, cross, prior_ss, mean_s, L.dptr(mo), None, L.dptr(co), ns)
    return mo, co, rc


def _rand(predict, who):
    def fn(self, post, cross, prior_ss, mean_s, kind, noise, Z, ldz, S, out, ldo):
        self.postfx_calls.append({"fn": who, "kind": kind, "cols": int(S), "mean_s": bool(mean_s)})
        m, Cm, rc = _moments(self, predict, post, cross, prior_ss, mean_s, who)
        if rc:
            return rc
        ns = len(m)
        if S < 1 or ldz < ns or ldo < ns:
            return self._fail(who + ": bad sizes")
        Lm, info = np_capi._chol(Cm + np_capi._noise_matrix(kind, noise, ns))
        if info:
            return self._fail("matrix is not positive definite", info)
        np_capi._mat(out, ns, S, ldo)[:, :] = m[:, None] + Lm @ np_capi._mat(Z, ns, S, ldz)
        return 0
    return fn


def _logpdf(predict, who):
    def fn(self, post, cross, prior_ss, mean_s, kind, noise, Y, ldy, ncols, out):
        self.postfx_calls.append({"fn": who, "kind": kind, "cols": int(ncols), "mean_s": bool(mean_s)})
        m, Cm, rc = _moments(self, predict, post, cross, prior_ss, mean_s, who)
        if rc:
            return rc
        ns = len(m)
        if ncols < 1 or ldy < ns:
            return self._fail(who + ": bad sizes")
        Lm, info = np_capi._chol(Cm + np_capi._noise_matrix(kind, noise, ns))
        if info:
            return self._fail("matrix is not positive definite", info)
        Zs = sla.solve_triangular(Lm, np_capi._mat(Y, ns, ncols, ldy) - m[:, None], lower=True, check_finite=False)
        np_capi._vec(out, ncols)[:] = -0.5 * (ns * np_capi.LOG2PI + 2.0 * np.log(np.diag(Lm)).sum() + (Zs * Zs).sum(0))
        return 0
    return fn


ENTRY = {
    "sgp_posterior_rand": _rand("sgp_posterior_predict", "sgp_posterior_rand"),
    "sgp_posterior_logpdf": _logpdf("sgp_posterior_predict", "sgp_posterior_logpdf"),
    "sgp_sparse_posterior_rand": _rand("sgp_sparse_posterior_predict", "sgp_sparse_posterior_rand"),
    "sgp_sparse_posterior_logpdf": _logpdf("sgp_sparse_posterior_predict", "sgp_sparse_posterior_logpdf"),
}


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    ctx = np_capi.install(monkeypatch)
    assert sorted(ENTRY) == L.postfx_symbols()
    for name, fn in ENTRY.items():
        monkeypatch.setattr(np_capi.FakeLib, name, fn, raising=False)
    ctx.lib.postfx_calls, ctx.lib.sharded = [], set()
    ctx.postfx = ctx.lib          # (Context.postfx: libsthenomi_postfx.so; the double serves both libraries)
    return ctx


def _both():
    fo, go = models.gppp_docstring(models.oracle_api())
    fp, gp = models.gppp_docstring(models.product_api())
    return ost.GPPP(fo, go), P.GPPP(fp, gp)


def _inputs(rng, sizes, names):
    xs = [rng.standard_normal(n) for n in sizes]
    return (ost.BlockData([ost.GPPPInput(k, x) for k, x in zip(names, xs)]),
            P.BlockData([P.GPPPInput(k, x) for k, x in zip(names, xs)]))


def _setup(seed, n_star=(7, 6)):
    rng = np.random.default_rng(seed)
    Fo, Fp = _both()
    xo, xp = _inputs(rng, (30, 20), ("f3", "f1"))
    so, sp = _inputs(rng, n_star, ("f2", "f3"))
    y = rng.standard_normal(50)
    return rng, Fo, Fp, xo, xp, so, sp, y


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _host_route(ctx, fn):
    """fn() with the context stripped of the library: the route through cov / mean and the zero-term spec"""
    lib = ctx.__dict__.pop("postfx")
    try:
        return fn()
    finally:
        ctx.postfx = lib


def test_which_processes_take_the_device_route(_numpy_double):
    rng, Fo, Fp, xo, xp, so, sp, y = _setup(1)
    calls = _numpy_double.lib.postfx_calls
    Z = rng.standard_normal((13, 2))
    ys = rng.standard_normal(13)
    # a prior: never
    P.logpdf(Fp(xp, 0.1), y), P.rand(rng, Fp(xp, 0.1))
    assert calls == []
    # the exact posterior
    post = P.posterior(Fp(xp, 0.1), y)
    P.logpdf(post(sp, 0.2), ys), P.rand(None, post(sp, 0.2), 2, Z=Z)
    assert [c["fn"] for c in calls] == ["sgp_posterior_logpdf", "sgp_posterior_rand"]
    # the VFE posterior
    zo, zp = _inputs(rng, (9,), ("f3",))
    spost = P.posterior(P.VFE(Fp(zp, 1e-6)), Fp(xp, 0.1), y)
    assert isinstance(spost, P.ApproxPosteriorGP)
    P.logpdf(spost(sp, 0.2), ys), P.rand(None, spost(sp, 0.2), 2, Z=Z)
    assert [c["fn"] for c in calls[2:]] == ["sgp_sparse_posterior_logpdf", "sgp_sparse_posterior_rand"]
    del calls[:]
    # a posterior conditioned on top of the VFE posterior answers through explicit covariances: the host route
    ex = P.posterior(spost(sp, 0.3), ys)
    assert isinstance(ex, P.finite_gp.ExplicitPosteriorGP)
    q = P.GPPPInput("f1", rng.standard_normal(4))
    P.logpdf(ex(q, 0.2), np.zeros(4)), P.rand(rng, ex(q, 0.2))
    assert calls == []
    # a multi-GPU context: the host route, same answer
    want = P.logpdf(post(sp, 0.2), ys)
    _numpy_double.is_multi = True
    del calls[:]
    got = P.logpdf(post(sp, 0.2), ys)
    assert calls == [] and abs(got - want) <= 1e-12 * abs(want)
    _numpy_double.is_multi = False


def test_fallback_without_the_library_gives_the_same_answer(_numpy_double):
    rng, Fo, Fp, xo, xp, so, sp, y = _setup(2)
    calls = _numpy_double.lib.postfx_calls
    post = P.posterior(Fp(xp, 0.1), y)
    zo, zp = _inputs(rng, (9,), ("f3",))
    spost = P.posterior(P.VFE(Fp(zp, 1e-6)), Fp(xp, 0.1), y)
    Z = rng.standard_normal((13, 3))
    Y = rng.standard_normal((13, 2))
    for p in (post, spost):
        del calls[:]
        lp, r = P.logpdf(p(sp, 0.2), Y), P.rand(None, p(sp, 0.2), 3, Z=Z)
        assert len(calls) == 2
        lp0, r0 = _host_route(_numpy_double, lambda: (P.logpdf(p(sp, 0.2), Y), P.rand(None, p(sp, 0.2), 3, Z=Z)))
        assert len(calls) == 2 and not hasattr(np_capi.FakeContext(), "postfx")
        assert _rel(lp, lp0) < 1e-12 and _rel(r, r0) < 1e-12


def test_noise_kinds_vector_and_matrix_y_and_s_none(_numpy_double):
    rng, Fo, Fp, xo, xp, so, sp, y = _setup(3)
    calls = _numpy_double.lib.postfx_calls
    post = P.posterior(Fp(xp, 0.1), y)
    B = rng.standard_normal((13, 3))
    noises = [(0.3, L.NOISE_SCALAR), (0.1 + rng.random(13), L.NOISE_DIAG), (0.2 * np.eye(13) + 0.05 * B @ B.T, L.NOISE_DENSE)]
    Y = rng.standard_normal((13, 3))
    Z = rng.standard_normal((13, 1))
    for noise, kind in noises:
        del calls[:]
        lp_v, lp_m = P.logpdf(post(sp, noise), Y[:, 0]), P.logpdf(post(sp, noise), Y)
        assert isinstance(lp_v, float) and lp_m.shape == (3,) and abs(lp_v - lp_m[0]) <= 1e-13 * abs(lp_v)
        r_v, r_m = P.rand(None, post(sp, noise), None, Z=Z), P.rand(None, post(sp, noise), 1, Z=Z)
        assert r_v.shape == (13,) and r_m.shape == (13, 1) and np.array_equal(r_v, r_m[:, 0])
        assert [(c["kind"], c["cols"], c["mean_s"]) for c in calls] == [(kind, 1, True), (kind, 3, True), (kind, 1, True), (kind, 1, True)]
        lp0 = _host_route(_numpy_double, lambda: P.logpdf(post(sp, noise), Y))
        assert _rel(lp_m, lp0) < 1e-12
    # S=None draws from the caller's generator, one column
    a = P.rand(np.random.default_rng(5), post(sp, 0.3))
    b = P.rand(None, post(sp, 0.3), 1, Z=np.random.default_rng(5).standard_normal((13, 1)))
    assert a.shape == (13,) and np.array_equal(a, b[:, 0])
    with pytest.raises(ValueError):
        P.logpdf(post(sp, 0.3), np.zeros(12))
    with pytest.raises(ValueError):
        P.logpdf(post(sp, np.ones(12)), np.zeros(13))


def test_float32_models_keep_their_rounding(_numpy_double):
    """all inputs Float32: mean and covariance are rounded to Float32 before they are factored (the one output-type rule), which
    only the host route reproduces -- it stays; Float32 test points on Float64 data: the device route, the sample rounded"""
    rng = np.random.default_rng(4)
    F = P.gppp_sum_model()
    calls = _numpy_double.lib.postfx_calls
    x64, s64 = rng.standard_normal(20), rng.standard_normal(6)
    y = rng.standard_normal(20)
    post32 = P.posterior(F(P.GPPPInput("f3", x64.astype(np.float32)), 0.1), y)
    s32 = P.GPPPInput("f1", s64.astype(np.float32))
    r = P.rand(rng, post32(s32, 0.2), 2)
    lp = P.logpdf(post32(s32, 0.2), np.zeros(6))
    assert calls == [] and r.dtype == np.float32 and isinstance(lp, float)
    post64 = P.posterior(F(P.GPPPInput("f3", x64), 0.1), y)
    r = P.rand(rng, post64(s32, 0.2), 2)
    lp = P.logpdf(post64(s32, 0.2), np.zeros(6))
    assert [c["fn"] for c in calls] == ["sgp_posterior_rand", "sgp_posterior_logpdf"]
    assert r.dtype == np.float32 and isinstance(lp, float)


def test_posdef_exception_carries_the_info_of_the_host_route(_numpy_double):
    rng, Fo, Fp, xo, xp, so, sp, y = _setup(6)
    post = P.posterior(Fp(xp, 0.1), y)
    before = post.mean(sp)
    bad = np.full(13, 0.2)
    bad[8] = -5.0                                  # C*[8, 8] <= k(x, x) = 1: the ninth leading minor is not positive
    with pytest.raises(P.PosDefException) as e0:
        _host_route(_numpy_double, lambda: P.logpdf(post(sp, bad), np.zeros(13)))
    for fn in (lambda: P.logpdf(post(sp, bad), np.zeros(13)), lambda: P.rand(rng, post(sp, bad), 2)):
        with pytest.raises(P.PosDefException) as e:
            fn()
        assert e.value.info == e0.value.info == 9
    assert np.array_equal(post.mean(sp), before)


def test_refusals_become_errors_and_name_the_entry_point(_numpy_double):
    rng, Fo, Fp, xo, xp, so, sp, y = _setup(7)
    post = P.posterior(Fp(xp, 0.1), y)
    _numpy_double.lib.sharded.add(id(post._h))
    with pytest.raises(P.SthenoMIError, match="sgp_posterior_logpdf.*multi-GPU"):
        P.logpdf(post(sp, 0.2), np.zeros(13))
    _numpy_double.lib.sharded.clear()
    # through the ABI signature: a prior spec of another size
    fg = P.finite_gp
    cross, _, _ = P.build_spec(Fp, sp, Fp, xp)
    other = fg._prior_spec(Fp, P.GPPPInput("f1", rng.standard_normal(5)))
    ms, s2, out = np.zeros(13), np.array([0.2]), np.zeros(1)
    fn = L.default_context().postfx.sgp_posterior_logpdf
    assert len(L._SIGS_POSTFX["sgp_posterior_logpdf"][1]) == 10 and len(L._SIGS_POSTFX["sgp_posterior_rand"][1]) == 11
    assert fn(post._h, cross.ref(), other.ref(), L.dptr(ms), L.NOISE_SCALAR, L.dptr(s2), L.dptr(ms), 13, 1, L.dptr(out)) < 0
    assert b"sgp_posterior_logpdf" in _numpy_double.lib.sgp_last_error()
    good = fg._prior_spec(Fp, sp)
    assert fn(post._h, cross.ref(), good.ref(), L.dptr(ms), L.NOISE_SCALAR, L.dptr(s2), L.dptr(ms), 13, 1, L.dptr(out)) == 0


@pytest.mark.parametrize("noise_id", ["scalar", "diag", "dense"])
def test_the_doubles_results_against_the_oracle(_numpy_double, noise_id):
    rng, Fo, Fp, xo, xp, so, sp, y = _setup(8)
    B = rng.standard_normal((13, 2))
    noise = {"scalar": 0.3, "diag": 0.1 + rng.random(13), "dense": 0.2 * np.eye(13) + 0.05 * B @ B.T}[noise_id]
    Y, Z = rng.standard_normal((13, 3)), rng.standard_normal((13, 4))
    po, pp = oagp.posterior(Fo(xo, 0.1), y), P.posterior(Fp(xp, 0.1), y)
    zo, zp = _inputs(rng, (9,), ("f3",))
    vo = oagp.posterior_vfe(oagp.VFE(Fo(zo, 1e-6)), Fo(xo, 0.1), y)
    vp = P.posterior(P.VFE(Fp(zp, 1e-6)), Fp(xp, 0.1), y)
    for o, p in ((po, pp), (vo, vp)):
        lo, lp = oagp.logpdf(o(so, noise), Y), P.logpdf(p(sp, noise), Y)
        assert np.all(np.abs(lp - lo) <= REL * np.abs(lo))
        assert _rel(P.rand(None, p(sp, noise), 4, Z=Z), oagp.rand(o(so, noise), Z)) < REL_RAND
    assert len(_numpy_double.lib.postfx_calls) == 4
