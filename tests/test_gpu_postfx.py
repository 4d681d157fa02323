"""rand / logpdf of a posterior FiniteGP against the kept factor (include/sthenomi_postfx.h: sgp_posterior_rand /
sgp_posterior_logpdf and their sparse forms), on the device (run with -m gpu on an MI355X).

The route these entry points replace is spelled out here through public calls -- post.cov(x*), post.mean(x*), S* added in
NumPy, the zero-term spec with the sum as dense noise, sgp_logpdf / sgp_rand -- and the new route must give ITS bits:
np.array_equal, for every noise kind, at test sizes that end inside a tile (150), on a tile edge (128) and at one point, for
sample counts on both sides of sgp_rand's 128-column pad.  Against the oracle the tolerances are those of
tests/test_gpu_parity.py for the prior: 1e-11 relative for rand with the same Z, REL for logpdf.

Shared set-up: the @gppp docstring model (f3 = f1 + f2) observed at 170 points of f3 and 130 of f1 -- the data straddle a
tile edge -- with test points in two blocks of two different processes."""
import ctypes as C

import numpy as np
import pytest

import models
import oracle.abstractgps as oagp
import oracle.stheno as ost
import stheno_jl_amd as P
from stheno_jl_amd.flatten import zero_spec
from test_gpu_kprod import _golden_on_two_blocks

pytestmark = pytest.mark.gpu

L = P.lib
REL = 1e-10            # tests/test_gpu_parity.py
REL_RAND = 1e-11
N_STAR = {1: (1,), 128: (70, 58), 150: (80, 70)}


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _blocks(names, xs):
    return (ost.BlockData([ost.GPPPInput(k, x) for k, x in zip(names, xs)]),
            P.BlockData([P.GPPPInput(k, x) for k, x in zip(names, xs)]))


class _Case:
    """the model, its data and the exact and VFE posteriors of oracle and product, built once"""

    def __init__(self):
        rng = np.random.default_rng(20251)
        fo, go = models.gppp_docstring(models.oracle_api())
        fp, gp = models.gppp_docstring(models.product_api())
        self.Fo, self.Fp = ost.GPPP(fo, go), P.GPPP(fp, gp)
        self.xo, self.xp = _blocks(("f3", "f1"), [rng.uniform(-4, 4, 170), rng.uniform(-4, 4, 130)])
        self.y = rng.standard_normal(300)
        self.star = {n: _blocks(("f2", "f3"), [rng.uniform(-4, 4, m) for m in sizes]) for n, sizes in N_STAR.items()}
        self.po, self.pp = oagp.posterior(self.Fo(self.xo, 0.1), self.y), P.posterior(self.Fp(self.xp, 0.1), self.y)
        zo, zp = _blocks(("f3",), [np.linspace(-4, 4, 40)])
        self.vo = oagp.posterior_vfe(oagp.VFE(self.Fo(zo, 1e-6)), self.Fo(self.xo, 0.1), self.y)
        self.vp = P.posterior(P.VFE(self.Fp(zp, 1e-6)), self.Fp(self.xp, 0.1), self.y)
        self.rng = rng

    def noise(self, kind, n):
        rng = np.random.default_rng(n + 7)
        if kind == "scalar":
            return 0.3
        if kind == "diag":
            return 0.1 + rng.random(n)
        B = rng.standard_normal((n, 3))
        return 0.2 * np.eye(n) + 0.05 * B @ B.T


@pytest.fixture(scope="module")
def case():
    return _Case()


# ---- the route these entry points replace, through public calls ----------------------------------------------------------
def _host_args(post, xs, noise):
    n = len(xs)
    Cm = np.asfortranarray(post.cov(xs) + P.finite_gp._noise_dense(noise, n))
    m = np.ascontiguousarray(post.mean(xs), dtype=np.float64)
    return n, zero_spec(n), m, Cm


def host_logpdf(post, xs, noise, Y):
    n, spec, m, Cm = _host_args(post, xs, noise)
    Y = np.asfortranarray(np.asarray(Y, dtype=np.float64).reshape(n, -1))
    out = np.zeros(Y.shape[1])
    ctx = L.default_context()
    L.check(ctx.lib.sgp_logpdf(ctx.handle, spec.ref(), L.dptr(m), L.NOISE_DENSE, L.dptr(Cm), L.dptr(Y), n, Y.shape[1],
                               L.dptr(out)), "sgp_logpdf")
    return out


def host_rand(post, xs, noise, Z):
    n, spec, m, Cm = _host_args(post, xs, noise)
    Z = np.asfortranarray(Z)
    out = np.zeros(Z.shape, order="F")
    ctx = L.default_context()
    L.check(ctx.lib.sgp_rand(ctx.handle, spec.ref(), L.dptr(m), L.NOISE_DENSE, L.dptr(Cm), L.dptr(Z), n, Z.shape[1],
                             L.dptr(out), n), "sgp_rand")
    return out


def _bit_equal(post, xs, noise, rng, samples=(1, 3, 130)):
    n = len(xs)
    Y = rng.standard_normal((n, 3))
    assert np.array_equal(np.array([P.logpdf(post(xs, noise), Y[:, 0])]), host_logpdf(post, xs, noise, Y[:, 0]))
    assert np.array_equal(P.logpdf(post(xs, noise), Y), host_logpdf(post, xs, noise, Y))
    for S in samples:
        Z = rng.standard_normal((n, S))
        got = P.rand(None, post(xs, noise), S, Z=Z)
        assert got.shape == (n, S) and np.array_equal(got, host_rand(post, xs, noise, Z)), S


# ---- 1. bit-equality with the host route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "diag", "dense"])
@pytest.mark.parametrize("n", [1, 128, 150])
def test_bit_equal_to_the_host_route(case, n, kind):
    _bit_equal(case.pp, case.star[n][1], case.noise(kind, n), np.random.default_rng(100 + n))


# ---- 2. parity with the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "diag", "dense"])
def test_parity_with_the_oracle(case, kind):
    so, sp = case.star[150]
    noise = case.noise(kind, 150)
    rng = np.random.default_rng(3)
    Y, Z = rng.standard_normal((150, 2)), rng.standard_normal((150, 4))
    lo, lp = oagp.logpdf(case.po(so, noise), Y), P.logpdf(case.pp(sp, noise), Y)
    print(f"\nlogpdf rel {np.max(np.abs(lp - lo) / np.abs(lo)):.3e}")
    assert np.all(np.abs(lp - lo) <= REL * np.abs(lo))
    r = rel(P.rand(None, case.pp(sp, noise), 4, Z=Z), oagp.rand(case.po(so, noise), Z))
    print(f"rand rel {r:.3e}")
    assert r < REL_RAND


# ---- 3. the factorisation identity -------------------------------------------------------------------------------------------
def test_logpdf_of_the_posterior_is_joint_minus_train(case):
    """p(y* | y) = p(y*, y) / p(y) with ONE scalar noise s on the training and the test side; the bound is the rounding of the
    two terms that are subtracted"""
    s = 0.1
    sp = case.star[150][1]
    ys = np.random.default_rng(4).standard_normal(150)
    lp_post = P.logpdf(case.pp(sp, s), ys)
    joint = P.BlockData(list(case.xp.X) + list(sp.X))
    lp_joint = P.logpdf(case.Fp(joint, s), np.concatenate([case.y, ys]))
    lp_train = P.logpdf(case.Fp(case.xp, s), case.y)
    print(f"\nposterior {lp_post!r} joint - train {lp_joint - lp_train!r}")
    assert abs(lp_post - (lp_joint - lp_train)) <= REL * (abs(lp_joint) + abs(lp_train))


# ---- 4. host routing: nothing N*^2 is fetched ---------------------------------------------------------------------------------
def test_the_mirror_does_not_fetch_the_covariance(case, monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("the posterior covariance was fetched")
    monkeypatch.setattr(P.PosteriorGP, "cov", boom)
    monkeypatch.setattr(P.ApproxPosteriorGP, "cov", boom)
    sp = case.star[150][1]
    rng = np.random.default_rng(5)
    for post in (case.pp, case.vp):
        assert isinstance(post, (P.PosteriorGP, P.ApproxPosteriorGP))
        r = P.rand(rng, post(sp, 0.2), 2)
        lp = P.logpdf(post(sp, 0.2), r[:, 0])
        assert r.shape == (150, 2) and np.all(np.isfinite(r)) and np.isfinite(lp)
        assert P.rand(rng, post(sp, 0.2)).shape == (150,)
    with pytest.raises(AssertionError):       # the host route does fetch it
        host_logpdf(case.pp, sp, 0.2, np.zeros(150))


# ---- 5. the VFE posterior ----------------------------------------------------------------------------------------------------
def test_vfe_bit_equal_to_the_host_route(case):
    assert len(case.vp.z) == 40
    _bit_equal(case.vp, case.star[150][1], case.noise("dense", 150), np.random.default_rng(6))


def test_vfe_parity_with_the_oracle(case):
    so, sp = case.star[150]
    noise = case.noise("diag", 150)
    rng = np.random.default_rng(7)
    Y, Z = rng.standard_normal((150, 2)), rng.standard_normal((150, 4))
    lo, lp = oagp.logpdf(case.vo(so, noise), Y), P.logpdf(case.vp(sp, noise), Y)
    print(f"\nlogpdf rel {np.max(np.abs(lp - lo) / np.abs(lo)):.3e}")
    assert np.all(np.abs(lp - lo) <= REL * np.abs(lo))
    r = rel(P.rand(None, case.vp(sp, noise), 4, Z=Z), oagp.rand(case.vo(so, noise), Z))
    print(f"rand rel {r:.3e}")
    assert r < REL_RAND


# ---- 6. a product kernel -------------------------------------------------------------------------------------------------------
def test_product_kernel_bit_equal_to_the_host_route():
    F, x, ins, y = _golden_on_two_blocks()
    post = P.posterior(F(x, 0.1), y)
    xs = P.GPPPInput("f", np.linspace(-3.5, 3.5, 150))
    _bit_equal(post, xs, 0.05 + np.random.default_rng(8).random(150), np.random.default_rng(9), samples=(3,))


# ---- 7. not positive definite ------------------------------------------------------------------------------------------------
def test_not_positive_definite_raises_the_info_of_the_host_route(case):
    """the input: a diagonal S* whose entry 100 is -5 -- C*[100, 100] <= k(x, x) = 2 for f3, so the 101st leading minor of
    C* + S* is negative while the first 100 (S* = 0.2 there) are positive"""
    sp = case.star[150][1]
    bad = np.full(150, 0.2)
    bad[100] = -5.0
    before = case.pp.mean(sp)
    with pytest.raises(P.PosDefException) as e0:
        host_logpdf(case.pp, sp, bad, np.zeros(150))
    with pytest.raises(P.PosDefException) as e1:
        host_rand(case.pp, sp, bad, np.zeros((150, 1)))
    assert e0.value.info == e1.value.info == 101
    with pytest.raises(P.PosDefException) as e2:
        P.logpdf(case.pp(sp, bad), np.zeros(150))
    with pytest.raises(P.PosDefException) as e3:
        P.rand(np.random.default_rng(0), case.pp(sp, bad), 2)
    assert e2.value.info == e3.value.info == 101
    assert np.array_equal(case.pp.mean(sp), before)
    _bit_equal(case.pp, sp, 0.3, np.random.default_rng(10), samples=(1,))      # and a valid call after it


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def _raw(fn, h, Fp, sp, xp, n, cols, ldx=None, prior=None):
    cross, _, _ = P.build_spec(Fp, sp, Fp, xp)
    pss = prior if prior is not None else P.finite_gp._prior_spec(Fp, sp)
    X = np.zeros((n, cols), order="F")
    s2, out = np.array([0.2]), np.zeros((n, cols), order="F")
    args = [h, cross.ref(), pss.ref(), None, L.NOISE_SCALAR, L.dptr(s2), L.dptr(X), n if ldx is None else ldx, cols, L.dptr(out)]
    if fn.endswith("_rand"):
        args.append(n)
    return getattr(L.postfx_lib(), fn)(*args), L.last_error()


def test_refusals_name_the_entry_point(case):
    sp, xp = case.star[150][1], case.xp
    for fn, h in (("sgp_posterior_rand", case.pp._h), ("sgp_posterior_logpdf", case.pp._h),
                  ("sgp_sparse_posterior_rand", case.vp._h), ("sgp_sparse_posterior_logpdf", case.vp._h)):
        train = xp if "sparse" not in fn else case.vp.z
        assert _raw(fn, h, case.Fp, sp, train, 150, 2)[0] == 0
        other = case.star[128][1]
        for rc, msg in (_raw(fn, h, case.Fp, sp, train, 150, 2, prior=P.finite_gp._prior_spec(case.Fp, other)),   # K** of another size
                        _raw(fn, h, case.Fp, sp, other, 150, 2),                                                  # cross against other columns
                        _raw(fn, h, case.Fp, sp, train, 150, 2, ldx=149),                                         # a leading dimension too small
                        _raw(fn, h, case.Fp, sp, train, 150, 0)):                                                 # no columns
            assert rc < 0 and msg.startswith(fn + ":"), (fn, rc, msg)
    rc = L.postfx_lib().sgp_posterior_logpdf(None, None, None, None, 0, None, None, 1, 1, None)
    assert rc < 0 and L.last_error().startswith("sgp_posterior_logpdf:")


def test_a_sharded_posterior_is_refused_and_the_mirror_takes_the_host_route(case):
    sp = case.star[150][1]
    Z = np.random.default_rng(11).standard_normal((150, 2))
    want = P.rand(None, case.pp(sp, 0.2), 2, Z=Z)
    mctx = L.Context(devices=[0, 0])
    prev = L.set_default_context(mctx)
    try:
        post = P.posterior(case.Fp(case.xp, 0.1), case.y)
        rc, msg = _raw("sgp_posterior_rand", post._h, case.Fp, sp, case.xp, 150, 2)
        assert rc < 0 and msg.startswith("sgp_posterior_rand:") and "multi-GPU" in msg
        rc, msg = _raw("sgp_posterior_logpdf", post._h, case.Fp, sp, case.xp, 150, 2)
        assert rc < 0 and "multi-GPU" in msg
        got = P.rand(None, post(sp, 0.2), 2, Z=Z)               # today's route, on the sharded factor
        assert rel(got, want) < 1e-9
        assert np.isfinite(P.logpdf(post(sp, 0.2), got[:, 0]))
        del post
    finally:
        L.set_default_context(prev)
        mctx.close()
    # a destroyed context
    ctx = L.Context(0)
    spec = P.finite_gp._prior_spec(case.Fp, case.xp)
    hd = C.c_void_p()
    s2 = np.array([0.1])
    assert ctx.lib.sgp_posterior_create(ctx.handle, spec.ref(), None, L.NOISE_SCALAR, L.dptr(s2), L.dptr(case.y), None, C.byref(hd)) == 0
    ctx.close()
    rc, msg = _raw("sgp_posterior_logpdf", hd, case.Fp, sp, case.xp, 150, 1)
    assert rc < 0 and "destroyed" in msg
    L.load().sgp_posterior_destroy(hd)


# ---- 9. ragged edges -----------------------------------------------------------------------------------------------------------
def test_one_point_one_sample_and_a_null_mean(case):
    so, sp = case.star[1]
    Z = np.array([[0.7]])
    got = P.rand(None, case.pp(sp, 0.3), 1, Z=Z)
    assert got.shape == (1, 1) and np.array_equal(got, host_rand(case.pp, sp, 0.3, Z))
    assert abs(got[0, 0] - oagp.rand(case.po(so, 0.3), Z)[0, 0]) <= REL_RAND * abs(got[0, 0])
    # mean_s = NULL is the zero prior mean (this model's): bit for bit, at N* = 128 exactly and at 150
    for n in (128, 150):
        sp = case.star[n][1]
        cross, _, _ = P.build_spec(case.Fp, sp, case.Fp, case.xp)
        pss = P.finite_gp._prior_spec(case.Fp, sp)
        Y = np.asfortranarray(np.random.default_rng(12).standard_normal((n, 2)))
        s2, zeros = np.array([0.2]), np.zeros(n)
        outs = []
        for ms in (None, zeros):
            lp, r = np.zeros(2), np.zeros((n, 2), order="F")
            lib = L.postfx_lib()
            assert lib.sgp_posterior_logpdf(case.pp._h, cross.ref(), pss.ref(), L.dptr(ms), L.NOISE_SCALAR, L.dptr(s2), L.dptr(Y), n, 2, L.dptr(lp)) == 0
            assert lib.sgp_posterior_rand(case.pp._h, cross.ref(), pss.ref(), L.dptr(ms), L.NOISE_SCALAR, L.dptr(s2), L.dptr(Y), n, 2, L.dptr(r), n) == 0
            outs.append((lp, r))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        assert np.array_equal(outs[0][0], P.logpdf(case.pp(sp, 0.2), Y))
