"""`update_posterior` -> sgp_posterior_extend WITHOUT a GPU: the host mirror's marshalling (the stacked blocks, the choice
between a scalar and a diagonal noise, the reservation), the hand-over of the handle, the fallback routes and the
PosDefException mapping, against the NumPy double of the C-ABI (tests/np_capi.py).  The double learns the entry point here
from the words of include/sthenomi_extend.h: a successful call leaves what sgp_posterior_create on the stacked data leaves
(every entry point that takes the handle then sees N + n_new points), rc > 0 is the stacked matrix's LAPACK info with the
posterior untouched, rc < 0 a refusal (dense noise, a sharded posterior, a size mismatch, another scalar noise).  The
extension of the factor itself is tests/test_gpu_extend.py's business."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import np_capi
import stheno_jl_amd as P

L = P.lib


def _create(self, ctx, spec, mean, kind, noise, y, alpha_out, out):
    rc = np_capi.FakeLib._create0(self, ctx, spec, mean, kind, noise, y, alpha_out, out)
    if rc == 0:
        self.post_noise[id(np_capi._struct(out))] = (kind, float(noise[0]) if kind == L.NOISE_SCALAR else None)
    return rc


def _extend(self, post, spec_all, mean_all, kind, noise, y_all, n_new, reserve_n, alpha_out, logpdf_out):
    Lm, _ = self.posts[id(post)]
    N = Lm.shape[0]
    self.extend_calls.append({"N": N, "n_new": int(n_new), "kind": kind, "reserve_n": int(reserve_n)})
    if id(post) in self.sharded:
        return self._fail("sgp_posterior_extend: a posterior of a multi-GPU context (sharded factor) cannot be extended")
    if kind not in (L.NOISE_SCALAR, L.NOISE_DIAG):
        return self._fail("sgp_posterior_extend: noise kind must be SCALAR or DIAG (dense noise is not supported)")
    s, m, Cm, rc = self._observed(spec_all, mean_all, kind, noise)
    if rc:
        return rc
    if n_new < 1 or s.N != N + n_new:
        return self._fail("sgp_posterior_extend: spec_all does not have N + n_new points")
    if reserve_n != 0 and reserve_n < s.N:
        return self._fail("sgp_posterior_extend: reserve_n must be 0 or >= N + n_new")
    if kind == L.NOISE_SCALAR and self.post_noise.get(id(post)) != (kind, float(noise[0])):
        return self._fail("sgp_posterior_extend: a scalar noise must be the value the posterior was created with")
    L2, info = np_capi._chol(Cm)
    if info:
        return self._fail("matrix is not positive definite", info)       # the posterior is left exactly as it was
    assert np.allclose(L2[:N, :N], Lm, rtol=0, atol=1e-10)      # the caller's guarantee: the first N points are the old ones
    delta = np_capi._vec(y_all, s.N) - m
    alpha = sla.cho_solve((L2, True), delta, check_finite=False)
    if alpha_out:
        np_capi._vec(alpha_out, s.N)[:] = alpha
    if logpdf_out:
        z = sla.solve_triangular(L2, delta, lower=True, check_finite=False)
        logpdf_out[0] = -0.5 * (s.N * np.log(2 * np.pi) + 2 * np.log(np.diag(L2)).sum() + z @ z)
    self.posts[id(post)] = (L2, alpha)
    self.post_noise[id(post)] = (kind, float(noise[0]) if kind == L.NOISE_SCALAR else None)
    return 0


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    ctx = np_capi.install(monkeypatch)
    monkeypatch.setattr(np_capi.FakeLib, "_create0", np_capi.FakeLib.sgp_posterior_create, raising=False)
    monkeypatch.setattr(np_capi.FakeLib, "sgp_posterior_create", _create)
    monkeypatch.setattr(np_capi.FakeLib, "sgp_posterior_extend", _extend, raising=False)
    ctx.lib.extend_calls, ctx.lib.post_noise, ctx.lib.sharded = [], {}, set()
    ctx.extend = ctx.lib          # (Context.extend: libsthenomi_extend.so; the double serves both libraries)
    return ctx


def _data(rng, n1=60, n2=25, D=2):
    F = P.gppp_sum_model()
    x1 = P.GPPPInput("f3", P.ColVecs(np.asfortranarray(rng.standard_normal((D, n1)))))
    x2 = P.GPPPInput("f1", P.ColVecs(np.asfortranarray(rng.standard_normal((D, n2)))))
    xs = P.GPPPInput("f2", P.ColVecs(np.asfortranarray(rng.standard_normal((D, 11)))))
    return F, x1, x2, xs, rng.standard_normal(n1), rng.standard_normal(n2)


def _same_posterior(a, b, xs, exact=False):
    cmp = np.array_equal if exact else (lambda u, v: np.allclose(u, v, rtol=0, atol=1e-10))
    assert cmp(a.alpha, b.alpha) and cmp(a.mean(xs), b.mean(xs)) and cmp(a.var(xs), b.var(xs)) and cmp(a.cov(xs), b.cov(xs))


def test_marshalling_stacked_blocks_noise_choice_and_reserve(_numpy_double):
    rng = np.random.default_rng(1)
    F, x1, x2, xs, y1, y2 = _data(rng)
    calls = _numpy_double.lib.extend_calls
    # equal scalar noises: the SCALAR kind, no reservation
    post = P.posterior(F(x1, 0.1), y1)
    ref = P.posterior(post(x2, 0.1), y2)                     # the stacked one-shot route (not rerouted)
    assert calls == []
    new = P.update_posterior(post, F(x2, 0.1), y2)
    assert calls == [{"N": 60, "n_new": 25, "kind": L.NOISE_SCALAR, "reserve_n": 0}]
    assert isinstance(new, P.PosteriorGP) and len(new.x) == 85 and [len(b) for b in new.x.X] == [60, 25]
    assert np.ndim(new.noise) == 0 and np.array_equal(new.y, np.concatenate([y1, y2]))
    _same_posterior(new, ref, xs, exact=True)
    lp = P.logpdf(F(new.x, new.noise), new.y)
    assert abs(new.logpdf_y - lp) <= 1e-12 * abs(lp)
    # different scalars -> DIAG with N + n_new values; reserve is passed on, and raised to the stacked size when smaller
    post = P.posterior(F(x1, 0.1), y1)
    new = P.update_posterior(post, F(x2, 0.3), y2, reserve=4096)
    assert calls[-1] == {"N": 60, "n_new": 25, "kind": L.NOISE_DIAG, "reserve_n": 4096}
    assert np.array_equal(new.noise, np.r_[np.full(60, 0.1), np.full(25, 0.3)])
    _same_posterior(new, P.posterior(F(P.BlockData([x1, x2]), new.noise), new.y), xs, exact=True)
    # a further extension of the extended posterior: three blocks, a vector noise on the new side
    x3 = P.GPPPInput("f2", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 7)))))
    v3 = 0.05 + rng.random(7)
    newer = P.update_posterior(new, F(x3, v3), rng.standard_normal(7), reserve=10)
    assert calls[-1] == {"N": 85, "n_new": 7, "kind": L.NOISE_DIAG, "reserve_n": 92}
    assert [len(b) for b in newer.x.X] == [60, 25, 7] and np.array_equal(newer.noise[85:], v3)


def test_the_new_object_takes_the_handle_over(_numpy_double):
    rng = np.random.default_rng(2)
    F, x1, x2, xs, y1, y2 = _data(rng)
    post = P.posterior(F(x1, 0.2), y1)
    h = post._h
    m_old = post.mean(xs)
    new = P.update_posterior(post, F(x2, 0.2), y2)
    assert new._h is h and post._h is None
    assert not np.allclose(new.mean(xs), m_old)
    # the old object rebuilds a factor of its own on demand (PosteriorGP._ensure) and answers as before
    assert np.array_equal(post.mean(xs), m_old) and post._h is not None and post._h is not h
    assert np.array_equal(post.alpha, P.posterior(F(x1, 0.2), y1).alpha)
    # fx2 may be written on the posterior itself, as sequential conditioning writes it
    again = P.update_posterior(post, post(x2, 0.2), y2)
    _same_posterior(again, new, xs, exact=True)


def test_fallback_routes_give_the_stacked_answer(_numpy_double):
    rng = np.random.default_rng(3)
    F, x1, x2, xs, y1, y2 = _data(rng)
    calls = _numpy_double.lib.extend_calls
    B = rng.standard_normal((25, 3))
    S2 = 0.2 * np.eye(25) + 0.01 * B @ B.T
    # dense Sigma_y on the new side, and on the old side
    post = P.posterior(F(x1, 0.1), y1)
    via = P.update_posterior(post, F(x2, S2), y2)
    assert calls == [] and post._h is not None and via.noise.shape == (85, 85)
    _same_posterior(via, P.posterior(post(x2, S2), y2), xs, exact=True)
    A = rng.standard_normal((60, 2))
    postd = P.posterior(F(x1, 0.1 * np.eye(60) + 0.01 * A @ A.T), y1)
    via = P.update_posterior(postd, F(x2, 0.3), y2)
    assert calls == []
    _same_posterior(via, P.posterior(postd(x2, 0.3), y2), xs, exact=True)
    # a multi-GPU context: the sharded factor is not extended
    _numpy_double.is_multi = True
    via = P.update_posterior(post, F(x2, 0.1), y2)
    assert calls == [] and post._h is not None
    _same_posterior(via, P.posterior(post(x2, 0.1), y2), xs, exact=True)
    _numpy_double.is_multi = False
    # a posterior without its observation model: as the sequential-conditioning branch answers
    bare = P.PosteriorGP(post.prior, post.x, post._h, post.alpha, post.delta)
    with pytest.raises(NotImplementedError):
        P.update_posterior(bare, F(x2, 0.1), y2)
    with pytest.raises(NotImplementedError):
        P.posterior(bare(x2, 0.1), y2)
    bare._h = None


def test_posdef_exception_carries_the_stacked_info_and_leaves_the_posterior(_numpy_double):
    rng = np.random.default_rng(4)
    F, x1, x2, xs, y1, y2 = _data(rng)
    post = P.posterior(F(x1, 0.1), y1)
    h, before = post._h, post.mean_and_var(xs)
    dup = P.GPPPInput("f3", P.ColVecs(np.asfortranarray(np.asarray(x1.x.X)[:, :10])))
    with pytest.raises(P.PosDefException) as e:
        P.update_posterior(post, F(dup, -0.5), np.zeros(10))
    with pytest.raises(P.PosDefException) as e1:
        P.posterior(post(dup, -0.5), np.zeros(10))
    assert e.value.info == e1.value.info > 60
    assert post._h is h
    after = post.mean_and_var(xs)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    good = P.update_posterior(post, F(x2, 0.1), y2)           # a following valid extension succeeds
    _same_posterior(good, P.posterior(F(P.BlockData([x1, x2]), 0.1), np.concatenate([y1, y2])), xs, exact=True)


def test_refusals_of_the_entry_point_become_errors(_numpy_double):
    rng = np.random.default_rng(5)
    F, x1, x2, xs, y1, y2 = _data(rng)
    post = P.posterior(F(x1, 0.1), y1)
    _numpy_double.lib.sharded.add(id(post._h))
    with pytest.raises(P.SthenoMIError, match="multi-GPU"):
        P.update_posterior(post, F(x2, 0.1), y2)
    assert post._h is not None
    _numpy_double.lib.sharded.clear()
    # through the ABI signature: size mismatch, dense kind, another scalar noise, a reservation that is too small
    spec = P.finite_gp._prior_spec(F, P.BlockData([x1, x2]))
    yy = np.concatenate([y1, y2])
    fn = L.default_context().extend.sgp_posterior_extend
    assert len(L._SIGS_EXTEND["sgp_posterior_extend"][1]) == 10
    s2, s3 = np.array([0.1]), np.array([0.3])
    d2 = np.asfortranarray(0.1 * np.eye(85))
    assert fn(post._h, spec.ref(), None, L.NOISE_SCALAR, L.dptr(s2), L.dptr(yy), 24, 0, None, None) < 0
    assert fn(post._h, spec.ref(), None, L.NOISE_DENSE, L.dptr(d2), L.dptr(yy), 25, 0, None, None) < 0
    assert fn(post._h, spec.ref(), None, L.NOISE_SCALAR, L.dptr(s3), L.dptr(yy), 25, 0, None, None) < 0
    assert fn(post._h, spec.ref(), None, L.NOISE_SCALAR, L.dptr(s2), L.dptr(yy), 25, 80, None, None) < 0
    assert fn(post._h, spec.ref(), None, L.NOISE_SCALAR, L.dptr(s2), L.dptr(yy), 25, 0, None, None) == 0
    with pytest.raises(TypeError):
        P.update_posterior(F(x1, 0.1), F(x2, 0.1), y2)
    with pytest.raises(ValueError):
        P.update_posterior(post, P.gppp_sum_model()(x2, 0.1), y2)      # another programme's process
