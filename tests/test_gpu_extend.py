"""update_posterior on the device (include/sthenomi_extend.h: sgp_posterior_extend): a kept Cholesky factor extended by the
rows of new data, against the one-shot `posterior` on the stacked data and against the CPU oracle.  Bounds as in
tests/test_gpu_parity.py for the same quantities: 1e-9 absolute for mean / var / cov against the oracle, 1e-9 relative for
alpha, that file's REL for the log marginal likelihood against sgp_logpdf of the stacked data."""
import ctypes as C

import numpy as np
import pytest

import models
import oracle.abstractgps as oagp
import oracle.kernelfunctions as okf
import oracle.stheno as ost
import stheno_jl_amd as P

pytestmark = pytest.mark.gpu

REL = 1e-10          # tests/test_gpu_parity.py
L = P.lib


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def both(recipe):
    fo, go = recipe(models.oracle_api())
    fp, gp = recipe(models.product_api())
    return ost.GPPP(fo, go), P.GPPP(fp, gp)


def _stacked_noise(s1, n1, s2, n2):
    if np.ndim(s1) == 0 and np.ndim(s2) == 0 and float(s1) == float(s2):
        return float(s1)
    return np.concatenate([np.broadcast_to(np.asarray(s1, dtype=float), (n1,)), np.broadcast_to(np.asarray(s2, dtype=float), (n2,))])


def _case(recipe, names, N, n_new, s1, s2, seed, reserve=None, D=1):
    """(extended, one-shot stacked, oracle stacked) posteriors + test inputs of the three kinds"""
    rng = np.random.default_rng(seed)
    Fo, Fp = both(recipe)
    x1 = np.asfortranarray(rng.standard_normal((D, N)))
    x2 = np.asfortranarray(rng.standard_normal((D, n_new)))
    y1, y2 = rng.standard_normal(N), rng.standard_normal(n_new)
    ino = lambda k, x: ost.GPPPInput(k, okf.ColVecs(x))   # noqa: E731
    inp = lambda k, x: P.GPPPInput(k, P.ColVecs(x))       # noqa: E731
    noise = _stacked_noise(s1, N, s2, n_new)
    po = oagp.posterior(Fo(ost.BlockData([ino(names[0], x1), ino(names[1], x2)]), noise), np.concatenate([y1, y2]))
    p_one = P.posterior(Fp(P.BlockData([inp(names[0], x1), inp(names[1], x2)]), noise), np.concatenate([y1, y2]))
    p_old = P.posterior(Fp(inp(names[0], x1), s1), y1)
    p_ext = P.update_posterior(p_old, Fp(inp(names[1], x2), s2), y2, reserve=reserve)
    xs = np.asfortranarray(rng.standard_normal((D, 25)))
    tests = [(ino(k, xs), inp(k, xs)) for k in dict.fromkeys(names)]
    return p_ext, p_one, po, p_old, tests


def _check(p_ext, p_one, po, tests):
    assert len(p_ext.y) == len(p_one.y) == len(po.alpha)
    print(f"alpha: ext vs oracle {rel(p_ext.alpha, po.alpha):.2e}, one-shot vs oracle {rel(p_one.alpha, po.alpha):.2e}")
    assert rel(p_ext.alpha, po.alpha) < 1e-9
    assert rel(p_ext.alpha, p_one.alpha) < 1e-9
    for to, tp in tests:
        mo, vo = po.mean_and_var(to)
        me, ve = p_ext.mean_and_var(tp)
        m1, v1 = p_one.mean_and_var(tp)
        Co, Ce = po.cov(to), p_ext.cov(tp)
        print(f"mean {np.max(np.abs(me - mo)):.2e} var {np.max(np.abs(ve - vo)):.2e} cov {np.max(np.abs(Ce - Co)):.2e}")
        assert np.max(np.abs(me - mo)) < 1e-9 and np.max(np.abs(ve - vo)) < 1e-9
        assert np.max(np.abs(Ce - Co)) < 1e-9
        assert np.max(np.abs(me - m1)) < 1e-9 and np.max(np.abs(ve - v1)) < 1e-9
        assert np.max(np.abs(Ce - p_one.cov(tp))) < 1e-9
    lp = P.logpdf(P.FiniteGP(p_one.prior, p_one.x, p_one.noise), p_one.y)      # sgp_logpdf of the stacked data
    print(f"logpdf: ext {p_ext.logpdf_y!r} sgp_logpdf {lp!r}")
    assert abs(p_ext.logpdf_y - lp) <= REL * abs(lp)


@pytest.mark.parametrize("N,n_new", [(70, 40), (128, 1), (129, 127), (200, 700), (1000, 24)])
def test_extension_matches_stacked_posterior_and_oracle(N, n_new):
    p_ext, p_one, po, _, tests = _case(models.gppp_docstring, ("f3", "f1"), N, n_new, 0.1, 0.3, seed=100 + N)
    _check(p_ext, p_one, po, tests)


def test_gppp_docstring_old_in_f3_new_in_f1_two_dimensional():
    p_ext, p_one, po, _, tests = _case(models.gppp_docstring, ("f3", "f1"), 70, 40, 0.1, 0.3, seed=31, D=2)
    _check(p_ext, p_one, po, tests)


def test_scalar_noise_on_both_sides_stays_scalar():
    p_ext, p_one, po, _, tests = _case(models.gppp_docstring, ("f3", "f3"), 150, 60, 0.2, 0.2, seed=7)
    assert np.ndim(p_ext.noise) == 0 and p_ext.noise == 0.2
    _check(p_ext, p_one, po, tests)


def test_different_scalar_noises_become_a_diagonal():
    p_ext, p_one, po, _, tests = _case(models.gppp_docstring, ("f2", "f3"), 150, 60, 0.2, 0.05, seed=8)
    assert np.shape(p_ext.noise) == (210,)
    _check(p_ext, p_one, po, tests)


def test_non_zero_mean():
    p_ext, p_one, po, _, tests = _case(models.toy_gppp, ("f3", "f1"), 140, 90, 0.1, 0.3, seed=9)
    assert np.max(np.abs(p_ext._mean_x)) > 0.1
    _check(p_ext, p_one, po, tests)


def test_old_posterior_stays_usable_after_the_hand_over():
    p_ext, _, _, p_old, tests = _case(models.gppp_docstring, ("f3", "f1"), 70, 40, 0.1, 0.3, seed=12)
    assert p_old._h is None and p_ext._h is not None
    rng = np.random.default_rng(12)
    Fo, _ = both(models.gppp_docstring)
    x1, _x2, y1 = np.asfortranarray(rng.standard_normal((1, 70))), rng.standard_normal((1, 40)), rng.standard_normal(70)
    po_old = oagp.posterior(Fo(ost.GPPPInput("f3", okf.ColVecs(x1)), 0.1), y1)
    to, tp = tests[0]
    assert np.max(np.abs(p_old.mean(tp) - po_old.mean(to))) < 1e-9       # rebuilt on demand (PosteriorGP._ensure)


def test_chain_of_ten_extensions_against_one():
    rng = np.random.default_rng(77)
    Fo, Fp = both(models.gppp_docstring)
    N, k, steps = 300, 16, 10
    x1 = rng.standard_normal(N)
    x2 = rng.standard_normal(k * steps)
    y1, y2 = rng.standard_normal(N), rng.standard_normal(k * steps)
    one = P.update_posterior(P.posterior(Fp(P.GPPPInput("f3", x1), 0.1), y1), Fp(P.GPPPInput("f1", x2), 0.1), y2)
    chain = P.posterior(Fp(P.GPPPInput("f3", x1), 0.1), y1)
    for i in range(steps):
        sl = slice(i * k, (i + 1) * k)
        chain = P.update_posterior(chain, Fp(P.GPPPInput("f1", x2[sl]), 0.1), y2[sl], reserve=N + k * steps)
    po = oagp.posterior(Fo(ost.BlockData([ost.GPPPInput("f3", x1), ost.GPPPInput("f1", x2)]), 0.1), np.concatenate([y1, y2]))
    xs = rng.standard_normal(25)
    assert rel(chain.alpha, po.alpha) < 1e-9 and rel(one.alpha, po.alpha) < 1e-9
    for name in ("f1", "f2", "f3"):
        mo, vo = po.mean_and_var(ost.GPPPInput(name, xs))
        for p in (chain, one):
            m, v = p.mean_and_var(P.GPPPInput(name, xs))
            assert np.max(np.abs(m - mo)) < 1e-9 and np.max(np.abs(v - vo)) < 1e-9
            assert np.max(np.abs(p.cov(P.GPPPInput(name, xs)) - po.cov(ost.GPPPInput(name, xs)))) < 1e-9
    assert abs(chain.logpdf_y - one.logpdf_y) <= REL * abs(one.logpdf_y)


@pytest.mark.parametrize("N,n0,n_new", [(200, 60, 200), (129, 128, 200), (700, 100, 300)])
def test_in_place_and_reallocating_runs_give_the_same_bits(N, n0, n_new):
    rng = np.random.default_rng(5)
    _, Fp = both(models.gppp_docstring)
    x1, x0, x2 = rng.standard_normal(N), rng.standard_normal(n0), rng.standard_normal(n_new)
    y1, y0, y2 = rng.standard_normal(N), rng.standard_normal(n0), rng.standard_normal(n_new)
    xs = P.GPPPInput("f2", rng.standard_normal(40))
    # a first extension by n0 points outgrows the buffer of N.  With a reservation it moves to one that also holds the second
    # extension, which then runs in place; without, the second extension outgrows the buffer again and reallocates.
    assert -(-(N + n0) // 128) > -(-N // 128) and -(-(N + n0 + n_new) // 128) > -(-(N + n0) // 128)
    outs = []
    for reserve in (N + n0 + n_new, None):
        p = P.posterior(Fp(P.GPPPInput("f3", x1), 0.1), y1)
        p = P.update_posterior(p, Fp(P.GPPPInput("f1", x0), 0.1), y0, reserve=reserve)
        p = P.update_posterior(p, Fp(P.GPPPInput("f1", x2), 0.1), y2)
        outs.append((p.alpha, *p.mean_and_var(xs), p.cov(xs), p.logpdf_y))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_larger_case_split_k_route_and_multi_tile_trailing_block():
    """N = 6000 + 300: the deep products run split over K and the trailing block has several tile columns.  Bound: an error
    at most 4 x that of the one-shot stacked posterior against the oracle, measured here -- both are backward-stable
    factorisations of the same matrix, and the factor leaves room for the different accumulation order."""
    p_ext, p_one, po, _, tests = _case(models.gppp_docstring, ("f3", "f1"), 6000, 300, 0.1, 0.3, seed=600, D=2)
    e_ext, e_one = rel(p_ext.alpha, po.alpha), rel(p_one.alpha, po.alpha)
    print(f"alpha: ext {e_ext:.3e} one-shot {e_one:.3e}")
    figures = [("alpha", e_ext, e_one)]
    for to, tp in tests:
        mo, vo = po.mean_and_var(to)
        me, ve = p_ext.mean_and_var(tp)
        m1, v1 = p_one.mean_and_var(tp)
        figures.append(("mean", np.max(np.abs(me - mo)), np.max(np.abs(m1 - mo))))
        figures.append(("var", np.max(np.abs(ve - vo)), np.max(np.abs(v1 - vo))))
    for what, e, e1 in figures:
        print(f"{what}: extended {e:.3e} one-shot {e1:.3e}")
    for what, e, e1 in figures:
        assert e <= 4.0 * e1, (what, e, e1)


def test_failed_extension_leaves_the_posterior_bit_equal_and_extensible():
    """new points that duplicate old ones under a negative noise: the stacked matrix fails at a leading minor > N"""
    rng = np.random.default_rng(3)
    _, Fp = both(models.gppp_docstring)
    N = 200
    x1, y1 = rng.standard_normal(N), rng.standard_normal(N)
    xs = P.GPPPInput("f1", rng.standard_normal(30))
    for n_dup, reserve in ((20, None), (100, None), (20, 400)):     # in place (220 <= 256), reallocating, in a reserved buffer
        post = P.posterior(Fp(P.GPPPInput("f3", x1), 0.1), y1)
        if reserve:
            post = P.update_posterior(post, Fp(P.GPPPInput("f3", x1[:1] + 0.5), 0.1), y1[:1], reserve=reserve)
        n_old = len(post.y)
        before = post.mean_and_var(xs)
        h = post._h
        dup = Fp(P.GPPPInput("f3", x1[:n_dup]), -0.5)
        with pytest.raises(P.PosDefException) as e_ext:
            P.update_posterior(post, dup, np.zeros(n_dup))
        with pytest.raises(P.PosDefException) as e_one:
            P.posterior(post(dup.x, -0.5), np.zeros(n_dup))
        assert e_ext.value.info == e_one.value.info > n_old
        assert post._h is h
        after = post.mean_and_var(xs)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        good = P.update_posterior(post, Fp(P.GPPPInput("f1", x1[:n_dup] + 0.25), 0.3), y1[:n_dup])
        ref = P.posterior(post(P.GPPPInput("f1", x1[:n_dup] + 0.25), 0.3), y1[:n_dup])
        m, v = good.mean_and_var(xs)
        mr, vr = ref.mean_and_var(xs)
        assert np.max(np.abs(m - mr)) < 1e-9 and np.max(np.abs(v - vr)) < 1e-9


def _raw_extend(h, F, x_all, noise, y_all, n_new, kind=None):
    spec = P.finite_gp._prior_spec(F, x_all)
    k, nbuf = L._noise_args(noise, len(y_all))
    y = np.asarray(y_all, dtype=np.float64)
    rc = L.default_context().extend.sgp_posterior_extend(h, spec.ref(), None, k if kind is None else kind, L.dptr(nbuf),
                                                         L.dptr(y), n_new, 0, None, None)
    return rc, L.last_error()


def test_refusals_and_the_mirrors_fallback():
    rng = np.random.default_rng(4)
    _, Fp = both(models.gppp_docstring)
    N, k = 90, 30
    x1, x2 = rng.standard_normal(N), rng.standard_normal(k)
    y1, y2 = rng.standard_normal(N), rng.standard_normal(k)
    xx = P.BlockData([P.GPPPInput("f3", x1), P.GPPPInput("f1", x2)])
    yy = np.concatenate([y1, y2])
    xs = P.GPPPInput("f2", rng.standard_normal(20))
    post = P.posterior(Fp(P.GPPPInput("f3", x1), 0.1), y1)
    before = post.mean_and_var(xs)
    # dense noise
    rc, msg = _raw_extend(post._h, Fp, xx, 0.1 * np.eye(N + k), yy, k)
    assert rc < 0 and "dense" in msg
    # size mismatch
    rc, msg = _raw_extend(post._h, Fp, xx, 0.1, yy, k + 1)
    assert rc < 0 and "N + n_new" in msg
    # a scalar noise that is not the old one
    rc, msg = _raw_extend(post._h, Fp, xx, 0.2, yy, k)
    assert rc < 0 and "scalar noise" in msg
    after = post.mean_and_var(xs)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the mirror's fallback for a dense Sigma_y: the stacked answer
    S2 = 0.3 * np.eye(k) + 0.01 * np.ones((k, k))
    via = P.update_posterior(post, Fp(P.GPPPInput("f1", x2), S2), y2)
    ref = P.posterior(post(P.GPPPInput("f1", x2), S2), y2)
    assert post._h is not None                                # nothing was handed over
    assert np.array_equal(via.mean(xs), ref.mean(xs))
    # a posterior of a multi-GPU context (one device listed twice): sharded factor
    mctx = L.Context(devices=[0, 0])
    spec1 = P.finite_gp._prior_spec(Fp, P.GPPPInput("f3", x1))
    hm = C.c_void_p()
    s2 = np.array([0.1])
    assert mctx.lib.sgp_posterior_create(mctx.handle, spec1.ref(), None, L.NOISE_SCALAR, L.dptr(s2), L.dptr(y1), None, C.byref(hm)) == 0
    rc, msg = _raw_extend(hm, Fp, xx, 0.1, yy, k)
    assert rc < 0 and "multi-GPU" in msg
    mctx.lib.sgp_posterior_destroy(hm)
    mctx.close()
    # a destroyed context
    ctx = L.Context(0)
    hd = C.c_void_p()
    assert ctx.lib.sgp_posterior_create(ctx.handle, spec1.ref(), None, L.NOISE_SCALAR, L.dptr(s2), L.dptr(y1), None, C.byref(hd)) == 0
    ctx.close()
    rc, msg = _raw_extend(hd, Fp, xx, 0.1, yy, k)
    assert rc < 0 and "destroyed" in msg
    L.load().sgp_posterior_destroy(hd)


def test_mirror_falls_back_to_the_stacked_posterior_on_a_multi_gpu_context():
    """update_posterior with a multi-GPU default context (one device listed twice): the sharded factor is not extended, the
    answer is the stacked one-shot posterior's"""
    rng = np.random.default_rng(6)
    Fo, Fp = both(models.gppp_docstring)
    N, k = 300, 50
    x1, x2 = rng.standard_normal(N), rng.standard_normal(k)
    y1, y2 = rng.standard_normal(N), rng.standard_normal(k)
    xs = rng.standard_normal(20)
    po = oagp.posterior(Fo(ost.BlockData([ost.GPPPInput("f3", x1), ost.GPPPInput("f1", x2)]),
                           _stacked_noise(0.1, N, 0.3, k)), np.concatenate([y1, y2]))
    mctx = L.Context(devices=[0, 0])
    prev = L.set_default_context(mctx)
    try:
        post = P.posterior(Fp(P.GPPPInput("f3", x1), 0.1), y1)
        via = P.update_posterior(post, Fp(P.GPPPInput("f1", x2), 0.3), y2)
        assert post._h is not None and not hasattr(via, "logpdf_y")          # nothing handed over, no extension ran
        assert rel(via.alpha, po.alpha) < 1e-9
        for name in ("f1", "f2", "f3"):
            m, v = via.mean_and_var(P.GPPPInput(name, xs))
            mo, vo = po.mean_and_var(ost.GPPPInput(name, xs))
            assert np.max(np.abs(m - mo)) < 1e-9 and np.max(np.abs(v - vo)) < 1e-9
        del post, via
    finally:
        L.set_default_context(prev)
        mctx.close()
