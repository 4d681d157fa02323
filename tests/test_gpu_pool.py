"""sgp_logpdf_pool / sgp_logpdf_grad_pool (include/sthenomi_pool.h): independent models of DIFFERENT sizes and noise kinds in
one call.  The poolable members are factored by ONE ragged launch of the dataflow kernel (chol_df.hip: chol_pool_kernel; task
order csrc/df_pool.h), each in the geometry of its own call.  The contract: every output of every member is BIT-EQUAL to its
own `logpdf` / `logpdf_and_gradient`, whatever the mix of sizes, the input order and what ran on the context before; a member
that is not positive definite does not lose the others; the report says what was pooled.  The loop it serves is the
member-by-member one around examples/getting_started/script.jl:154-213 of the reference."""
import time

import numpy as np
import pytest

import stheno_jl_amd as P
from oracle import reference_model as orm

pytestmark = pytest.mark.gpu

D = 3
_CACHE = {}


def _member(N, seed, noise="scalar"):
    """one model of N points (built once per (N, seed, noise)) and its own call's value"""
    key = (N, seed, noise)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * seed + N)
        ell, s2 = 0.5 + rng.random(), 0.05 + 0.2 * rng.random()
        f = P.atomic(P.GP(P.with_lengthscale(P.Matern52Kernel(), ell)), P.GPC())
        x = P.ColVecs(np.asfortranarray(rng.standard_normal((D, N))))
        y = rng.standard_normal(N)
        fx = f(x, s2 if noise == "scalar" else 0.05 + rng.random(N))
        _CACHE[key] = [fx, y, None]
    return _CACHE[key]


def _own(N, seed, noise="scalar"):
    m = _member(N, seed, noise)
    if m[2] is None:
        m[2] = P.logpdf(m[0], m[1])
    return m[2]


def _pool(sizes, noise="scalar"):
    ms = [_member(N, b, noise) for b, N in enumerate(sizes)]
    return [m[0] for m in ms], [m[1] for m in ms], np.array([_own(N, b, noise) for b, N in enumerate(sizes)])


TILE_SIZES = (1, 127, 128, 129, 300, 640, 1000)          # T_c = 1, 1, 1, 2, 3, 5, 8


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_members_of_every_tile_count_share_one_launch(order):
    fxs, ys, own = _pool(TILE_SIZES)
    perm = {"ascending": np.arange(7), "descending": np.arange(7)[::-1],
            "shuffled": np.random.default_rng(3).permutation(7)}[order]
    got, infos, rep = P.logpdf_pool([fxs[i] for i in perm], [ys[i] for i in perm], return_infos=True, return_report=True)
    print(order, "pool - own:", got - own[perm], rep)
    assert rep["pool_launches"] == 1 and rep["pooled_members"] == 7 and rep["single_members"] == 0
    assert rep["distinct_sizes"] == 5
    assert np.array_equal(got, own[perm]) and not infos.any()


def test_repeats_and_changing_geometry_keep_the_bits():
    """the state words are zeroed for the right count whatever ran before"""
    fxs, ys, own = _pool(TILE_SIZES)
    f2, y2, own2 = _pool((300, 300, 700))
    for _ in range(2):
        assert np.array_equal(P.logpdf_pool(fxs, ys), own)
    assert np.array_equal(P.logpdf_pool(f2, y2), own2)
    assert np.array_equal(P.logpdf_pool(fxs, ys), own)


def test_members_of_one_shape_take_the_equal_size_kernel_and_keep_the_bits():
    """a pool whose members all share one shape is launched through the equal-size batch's kernel (same order, no table)"""
    for sizes in ((300, 290, 257), (130, 140)):
        fxs, ys, own = _pool(sizes)
        got, rep = P.logpdf_pool(fxs, ys, return_report=True)
        assert rep["pool_launches"] == 1 and rep["pooled_members"] == len(sizes) and rep["distinct_sizes"] == 1
        assert np.array_equal(got, own)
    fxs, ys, _ = _pool((300, 290, 257))
    got = P.logpdf_and_gradient_pool(fxs, ys)
    for g, fx, y in zip(got, fxs, ys):
        _same_gradient(g, P.logpdf_and_gradient(fx, y))


def test_more_than_sixteen_members_are_cut_into_launches_and_keep_input_order():
    sizes = [(200, 456, 640, 1100)[b % 4] for b in range(19)]
    fxs, ys, own = _pool(sizes)
    got, rep = P.logpdf_pool(fxs, ys, return_report=True)
    assert rep["pool_launches"] == 2 and rep["pooled_members"] == 19 and rep["single_members"] == 0
    assert np.array_equal(got, own)


def test_mixed_noise_kinds_means_and_a_block_model_in_one_pool():
    rng = np.random.default_rng(21)
    fxs, ys, _ = _pool((300, 700))
    fd, yd, _ = _pool((130, 520), noise="diag")
    # means given for some members (a constant mean function) and NULL for others (zero mean: the atomic models above)
    fm = P.atomic(P.GP(1.5, P.with_lengthscale(P.Matern52Kernel(), 0.8)), P.GPC())
    xm = P.ColVecs(np.asfortranarray(rng.standard_normal((D, 400))))
    F = P.gppp_sum_model()
    xs = [np.asfortranarray(rng.standard_normal((D, 300))) for _ in range(3)]
    xb = P.BlockData([P.GPPPInput(k, P.ColVecs(v)) for k, v in zip(("f1", "f2", "f3"), xs)])
    yb = rng.standard_normal(900)
    fxs = fxs + fd + [fm(xm, 0.2), F(xb, 0.1)]
    ys = ys + yd + [rng.standard_normal(400), yb]
    own = np.array([P.logpdf(fx, y) for fx, y in zip(fxs, ys)])
    got, rep = P.logpdf_pool(fxs, ys, return_report=True)
    assert rep["pool_launches"] == 1 and rep["pooled_members"] == 6
    assert np.array_equal(got, own)
    np.testing.assert_allclose(got[-1], orm.gppp_sum_logpdf(xs, yb, 0.1), rtol=1e-10)
    # through the C signature: NULL mean pointers for the zero-mean members, a vector for the others
    import ctypes as C
    L = P.lib
    keep = []
    for fx, y in zip(fxs, ys):
        spec, m, kind, nbuf = P.finite_gp._spec_mean_noise(fx)
        m = np.asfortranarray(m, dtype=np.float64)
        keep.append((spec, m if m.any() else None, kind, nbuf, np.asarray(y, dtype=np.float64)))
    assert sum(k[1] is None for k in keep) == 5 and keep[4][1] is not None
    nb = len(keep)

    def ptrs(arrs):
        return (C.POINTER(C.c_double) * nb)(*[L.dptr(a) for a in arrs])

    for k in keep:
        k[0].ref()
    specs = (C.POINTER(L.sgp_cov_spec) * nb)(*[C.pointer(k[0].c) for k in keep])
    kinds = (C.c_int * nb)(*[k[2] for k in keep])
    out = np.zeros(nb)
    ctx = L.default_context()
    rc = ctx.pool.sgp_logpdf_pool(ctx.handle, nb, specs, ptrs([k[1] for k in keep]), kinds, ptrs([k[3] for k in keep]),
                                  ptrs([k[4] for k in keep]), L.dptr(out), None, None)
    assert rc == 0 and np.array_equal(out, own)


@pytest.mark.parametrize("bad", [0, 3])
def test_one_bad_member_does_not_lose_the_others(bad):
    sizes = (130, 300, 700, 1000)
    fxs, ys, own = _pool(sizes)
    fxs = list(fxs)
    fxs[bad] = fxs[bad].f(fxs[bad].x, -3.0)                     # K - 3 I: not positive definite
    with pytest.raises(P.PosDefException) as e:
        P.logpdf(fxs[bad], ys[bad])
    vals, infos, rep = P.logpdf_pool(fxs, ys, return_infos=True, return_report=True)
    assert rep["pool_launches"] == 1 and rep["pooled_members"] == 4
    assert np.isnan(vals[bad]) and infos[bad] == e.value.info and infos[bad] >= 1
    keep = [b for b in range(4) if b != bad]
    assert np.array_equal(vals[keep], own[keep]) and not infos[keep].any()


def _same_gradient(got, ref):
    assert got["logpdf"] == ref["logpdf"]
    assert np.array_equal(got["y"], ref["y"]) and np.array_equal(got["mean"], ref["mean"])
    assert np.array_equal(np.asarray(got["noise"]), np.asarray(ref["noise"]))
    assert np.array_equal(got["_raw"][0], ref["_raw"][0]) and np.array_equal(got["_raw"][1], ref["_raw"][1])


def test_gradient_pool_is_bit_equal_and_honours_null_outputs():
    import ctypes as C
    L = P.lib
    sizes = (130, 300, 700, 300)                 # one C^-1 group of two and two singles
    fxs, ys, _ = _pool(sizes)
    fxs = list(fxs)
    fxs[1] = _member(300, 1, "diag")[0]          # (a diagonal-noise member among scalar ones)
    ys[1] = _member(300, 1, "diag")[1]
    refs = [P.logpdf_and_gradient(fx, y) for fx, y in zip(fxs, ys)]
    got, infos, rep = P.logpdf_and_gradient_pool(fxs, ys, return_infos=True, return_report=True)
    assert rep["pool_launches"] == 1 and rep["pooled_members"] == 4 and rep["distinct_sizes"] == 3
    assert not infos.any()
    for g, r in zip(got, refs):
        _same_gradient(g, r)
    # a NULL array (grad_mean) and a NULL element (grad_y of member 2) through the C signature
    keep = []
    for fx, y in zip(fxs, ys):
        spec = P.finite_gp._prior_spec(fx.f, fx.x)
        kind, nbuf = L._noise_args(fx.noise, len(fx))
        keep.append((spec, np.asfortranarray(P.mean_vector(fx.f, fx.x), dtype=np.float64), kind, nbuf, np.asarray(y, dtype=np.float64)))
    nb = len(keep)

    def ptrs(arrs):
        return (C.POINTER(C.c_double) * nb)(*[L.dptr(a) if a is not None else None for a in arrs])

    for k in keep:
        k[0].ref()
    specs = (C.POINTER(L.sgp_cov_spec) * nb)(*[C.pointer(k[0].c) for k in keep])
    kinds = (C.c_int * nb)(*[k[2] for k in keep])
    lp = np.zeros(nb)
    gy = [np.full(len(k[4]), 7.0) for k in keep]
    gy[2] = None
    gc = [np.full(max(1, k[0].n_terms), 7.0) for k in keep]
    ctx = L.default_context()
    rc = ctx.pool.sgp_logpdf_grad_pool(ctx.handle, nb, specs, ptrs([k[1] for k in keep]), kinds, ptrs([k[3] for k in keep]),
                                       ptrs([k[4] for k in keep]), L.dptr(lp), ptrs(gy), None, None, ptrs(gc), None, None, None)
    assert rc == 0
    for b, r in enumerate(refs):
        assert lp[b] == r["logpdf"]
        if gy[b] is not None:
            assert np.array_equal(gy[b], r["y"])
        assert np.array_equal(gc[b], r["_raw"][0][:len(gc[b])])


def test_a_gradient_pool_of_more_than_sixteen_members_is_cut_into_launches():
    """18 members of two padded sizes (256, 384, 384): a launch of 16 and one of the two smallest, results in input order"""
    ms = [_member((130, 260, 300)[b % 3], b) for b in range(18)]
    fxs, ys = [m[0] for m in ms], [m[1] for m in ms]
    got, infos, rep = P.logpdf_and_gradient_pool(fxs, ys, return_infos=True, return_report=True)
    assert rep["pool_launches"] == 2 and rep["pooled_members"] == 18 and rep["single_members"] == 0
    assert not infos.any()
    for g, fx, y in zip(got, fxs, ys):
        _same_gradient(g, P.logpdf_and_gradient(fx, y))


def test_the_batch_calls_and_the_pool_calls_agree_on_members_of_one_shape():
    """both routes plan one launch of the same three members: the same bits from either, and from the members' own calls"""
    fxs, ys, own = _pool((300, 290, 257))
    by_batch, by_pool = P.logpdf_batch(fxs, ys), P.logpdf_pool(fxs, ys)
    assert np.array_equal(by_batch, by_pool) and np.array_equal(by_batch, own) and np.array_equal(by_pool, own)
    g_batch, g_pool = P.logpdf_and_gradient_batch(fxs, ys), P.logpdf_and_gradient_pool(fxs, ys)
    for gb, gp, fx, y in zip(g_batch, g_pool, fxs, ys):
        ref = P.logpdf_and_gradient(fx, y)
        _same_gradient(gb, gp)
        _same_gradient(gb, ref)
        _same_gradient(gp, ref)


def test_the_error_text_names_the_bad_member_as_its_entry_point_counts_it():
    """infos = NULL through the C signatures: the call returns the first bad member's info and names it "(batch member b)" /
    "(pool member b)", b its index in the caller's arrays; the other members keep their values"""
    import ctypes as C
    L = P.lib
    fxs, ys, own = _pool((130, 130, 130))
    fxs = list(fxs)
    fxs[1] = fxs[1].f(fxs[1].x, -3.0)                           # K - 3 I: not positive definite
    with pytest.raises(P.PosDefException) as e:
        P.logpdf(fxs[1], ys[1])
    keep = []
    for fx, y in zip(fxs, ys):
        spec, m, kind, nbuf = P.finite_gp._spec_mean_noise(fx)
        assert kind == L.NOISE_SCALAR
        keep.append((spec, np.asfortranarray(m, dtype=np.float64), nbuf, np.asarray(y, dtype=np.float64)))

    def ptrs(q):
        return (C.POINTER(C.c_double) * 3)(*[L.dptr(k[q]) for k in keep])

    for k in keep:
        k[0].ref()
    specs = (C.POINTER(L.sgp_cov_spec) * 3)(*[C.pointer(k[0].c) for k in keep])
    kinds = (C.c_int * 3)(*[L.NOISE_SCALAR] * 3)
    ctx = L.default_context()
    out = np.zeros(3)
    rc = ctx.lib.sgp_logpdf_batch(ctx.handle, 3, specs, ptrs(1), L.NOISE_SCALAR, ptrs(2), ptrs(3), L.dptr(out), None)
    print("batch:", rc, L.last_error())
    assert rc == e.value.info and rc >= 1 and "(batch member 1)" in L.last_error()
    assert out[0] == own[0] and out[2] == own[2]
    out = np.zeros(3)
    rc = ctx.pool.sgp_logpdf_pool(ctx.handle, 3, specs, ptrs(1), kinds, ptrs(2), ptrs(3), L.dptr(out), None, None)
    print("pool:", rc, L.last_error())
    assert rc == e.value.info and rc >= 1 and "(pool member 1)" in L.last_error()
    assert out[0] == own[0] and out[2] == own[2]


def test_knobs_switch_the_pool_off_bound_it_and_force_the_rerun(monkeypatch):
    """SGP_BATCH_MAX_N=0: no pool.  =512: the member beyond it runs through its own call, the others pool.
    SGP_DF_TIMEOUT_S tiny: the ragged launch runs into its bounded wait, the entry point reruns on the launch-based schedule
    (with_df_fallback).  Same bits in every case."""
    fxs, ys, own = _pool((300, 700, 400))
    cases = (({"SGP_BATCH_MAX_N": "0"}, dict(pool_launches=0, pooled_members=0, single_members=3)),
             ({"SGP_BATCH_MAX_N": "512"}, dict(pool_launches=1, pooled_members=2, single_members=1)),
             ({"SGP_DF_TIMEOUT_S": "1e-7"}, None))
    for env, want in cases:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = P.lib.Context(0)
        prev = P.lib.set_default_context(ctx)
        try:
            got, rep = P.logpdf_pool(fxs, ys, return_report=True)
            assert np.array_equal(got, own), env
            if want:
                assert {k: rep[k] for k in want} == want, (env, rep)
        finally:
            P.lib.set_default_context(prev)
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)


def test_the_pool_pays_against_the_member_by_member_loop():
    """8 members N = 1536, 1920, ..., 4224 (no two of one padded size: sgp_logpdf_batch would run them one by one).
    t_loop = median of 5 runs of the member-by-member loop, t_pool = median of 5 pool calls; the pool must win by more than
    the spread (max - min) of the loop's own runs."""
    sizes = [1536 + 384 * b for b in range(8)]
    fxs, ys, own = _pool(sizes)
    assert np.array_equal(P.logpdf_pool(fxs, ys), own)          # (also the warm-up of both routes)

    def runs(fn, reps=5):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return np.array(ts)

    t_loop = runs(lambda: [P.logpdf(fx, y) for fx, y in zip(fxs, ys)])
    t_pool = runs(lambda: P.logpdf_pool(fxs, ys))
    print("loop ms", 1e3 * t_loop, "pool ms", 1e3 * t_pool)
    assert np.median(t_pool) < np.median(t_loop) - (t_loop.max() - t_loop.min()), (t_pool, t_loop)
