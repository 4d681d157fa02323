"""`logpdf_pool` / `logpdf_and_gradient_pool` -> sgp_logpdf_pool / sgp_logpdf_grad_pool WITHOUT a GPU: the host mirror's
marshalling (per-member noise kinds, the pointer arrays, the report), its result mapping, the NaN + info convention, the
Float32 route and the argument checks, against the NumPy double of the C-ABI (tests/np_capi.py).  The double learns the two
entry points here from its own single-member functions, as include/sthenomi_pool.h specifies them: member b is exactly the
member's own call with ITS noise kind; NULL arrays / elements skip outputs; results in input order even though the driver
works through the members largest first.  The ragged launch itself is tests/test_gpu_pool.py's business."""
import ctypes as C

import numpy as np
import pytest

import np_capi
import stheno_jl_amd as P

L = P.lib
_DP = C.POINTER(C.c_double)


def _report(self, report, kinds, nspec):
    """the double pools every scalar / diagonal member when there are two or more (one launch), like the driver"""
    pooled = [b for b in range(nspec) if kinds[b] != L.NOISE_DENSE]
    if len(pooled) < 2:
        pooled = []
    if report:
        r = report._obj if hasattr(report, "_obj") else report.contents
        r.pool_launches = 1 if pooled else 0
        r.pooled_members = len(pooled)
        r.single_members = nspec - len(pooled)
        r.distinct_sizes = len({-(-np_capi._Spec(self.pool_specs[b]).N // 128) for b in pooled})


def _order(self, specs, nspec):
    """the driver's order of work: largest member first (results must still land in input order)"""
    self.pool_specs = specs
    return sorted(range(nspec), key=lambda b: -np_capi._Spec(specs[b]).N)


def _logpdf_pool(self, ctx, nspec, specs, means, kinds, noises, ys, out, infos, report):
    self.pool_calls.append(("value", [int(kinds[b]) for b in range(nspec)]))
    o = np.ctypeslib.as_array(out, shape=(nspec,))
    inf = np.ctypeslib.as_array(infos, shape=(nspec,)) if infos else None
    first_bad = 0
    for b in _order(self, specs, nspec):
        one = np.zeros(1)
        n = np_capi._Spec(specs[b]).N
        rc = self.sgp_logpdf(ctx, specs[b], means[b] if means else None, kinds[b], noises[b], ys[b], n, 1, one.ctypes.data_as(_DP))
        if rc < 0:
            return rc
        o[b] = one[0] if rc == 0 else np.nan
        if inf is not None:
            inf[b] = rc
        first_bad = first_bad or rc
    _report(self, report, kinds, nspec)
    return 0 if inf is not None else first_bad


def _grad_pool(self, ctx, nspec, specs, means, kinds, noises, ys, lp_out, gy, gm, gn, gc, gs, infos, report):
    self.pool_calls.append(("grad", [int(kinds[b]) for b in range(nspec)]))
    lp = np.ctypeslib.as_array(lp_out, shape=(nspec,))
    inf = np.ctypeslib.as_array(infos, shape=(nspec,)) if infos else None
    first_bad = 0
    for b in _order(self, specs, nspec):
        one = np.zeros(1)

        def at(arr):
            return arr[b] if arr else None

        rc = self.sgp_logpdf_grad(ctx, specs[b], means[b] if means else None, kinds[b], noises[b], ys[b],
                                  one.ctypes.data_as(_DP), at(gy), at(gm), at(gn), at(gc), at(gs))
        if rc < 0:
            return rc
        lp[b] = one[0] if rc == 0 else np.nan
        if inf is not None:
            inf[b] = rc
        first_bad = first_bad or rc
    _report(self, report, kinds, nspec)
    return 0 if inf is not None else first_bad


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    ctx = np_capi.install(monkeypatch)
    monkeypatch.setattr(np_capi.FakeLib, "sgp_logpdf_pool", _logpdf_pool, raising=False)
    monkeypatch.setattr(np_capi.FakeLib, "sgp_logpdf_grad_pool", _grad_pool, raising=False)
    ctx.lib.pool_calls = []
    ctx.pool = ctx.lib          # (Context.pool: libsthenomi_pool.so; the double serves every library)
    return ctx


def _f(ell=0.7):
    return P.atomic(P.GP(P.with_lengthscale(P.Matern52Kernel(), ell)), P.GPC())


def _members(sizes, rng, noise=lambda b, n, rng: 0.1 + 0.05 * b):
    fxs, ys = [], []
    for b, n in enumerate(sizes):
        x = P.ColVecs(np.asfortranarray(rng.standard_normal((2, n))))
        fxs.append(_f(0.6 + 0.1 * b)(x, noise(b, n, rng)))
        ys.append(rng.standard_normal(n))
    return fxs, ys


def _mixed_noise(b, n, rng):
    return (0.1 + 0.05 * b) if b % 2 == 0 else 0.05 + rng.random(n)


def test_mixed_sizes_and_noise_kinds_go_down_in_one_call_and_keep_input_order(_numpy_double):
    rng = np.random.default_rng(4)
    fxs, ys = _members((20, 150, 7, 131, 64), rng, _mixed_noise)
    got, infos, rep = P.logpdf_pool(fxs, ys, return_infos=True, return_report=True)
    assert _numpy_double.lib.pool_calls == [("value", [L.NOISE_SCALAR, L.NOISE_DIAG, L.NOISE_SCALAR, L.NOISE_DIAG, L.NOISE_SCALAR])]
    assert got.shape == (5,) and infos.dtype == np.int32 and not infos.any()
    assert np.array_equal(got, np.array([P.logpdf(fx, y) for fx, y in zip(fxs, ys)]))
    assert rep == dict(pool_launches=1, pooled_members=5, single_members=0, distinct_sizes=2)
    assert np.array_equal(P.logpdf_pool(fxs, ys), got)                       # plain form: the values alone
    grads, ginfos, grep = P.logpdf_and_gradient_pool(fxs, ys, return_infos=True, return_report=True)
    assert _numpy_double.lib.pool_calls[-1][0] == "grad" and not ginfos.any() and grep["pooled_members"] == 5
    for g, fx, y in zip(grads, fxs, ys):
        ref = P.logpdf_and_gradient(fx, y)
        assert set(g) == set(ref) and g["logpdf"] == ref["logpdf"]
        assert np.array_equal(g["y"], ref["y"]) and np.array_equal(g["mean"], ref["mean"])
        assert np.array_equal(np.asarray(g["noise"]), np.asarray(ref["noise"])) and type(g["noise"]) is type(ref["noise"])
        assert [(t["d_coef"], t["d_inscale"]) for t in g["terms"]] == [(t["d_coef"], t["d_inscale"]) for t in ref["terms"]]


def test_dense_noise_and_posterior_members_go_down_as_dense(_numpy_double):
    rng = np.random.default_rng(5)
    fxs, ys = _members((30, 45, 25), rng)
    Bm = rng.standard_normal((45, 3))
    fxs[1] = fxs[1].f(fxs[1].x, 0.2 * np.eye(45) + 0.01 * Bm @ Bm.T)
    post = P.posterior(fxs[2], ys[2])
    fxs.append(post(fxs[2].x, 0.1))
    ys.append(rng.standard_normal(25))
    got, rep = P.logpdf_pool(fxs, ys, return_report=True)
    assert _numpy_double.lib.pool_calls[-1] == ("value", [L.NOISE_SCALAR, L.NOISE_DENSE, L.NOISE_SCALAR, L.NOISE_DENSE])
    assert np.array_equal(got, np.array([P.logpdf(fx, y) for fx, y in zip(fxs, ys)]))
    assert rep["pooled_members"] == 2 and rep["single_members"] == 2
    g = P.logpdf_and_gradient_pool(fxs[:3], ys[:3])
    assert g[1]["noise"].shape == (45, 45)
    assert np.array_equal(g[1]["noise"], P.logpdf_and_gradient(fxs[1], ys[1])["noise"])
    with pytest.raises(NotImplementedError):
        P.logpdf_and_gradient_pool(fxs, ys)                                  # a posterior has no gradient path


def test_float32_member_is_its_own_call_widened_and_counted_single(_numpy_double):
    rng = np.random.default_rng(6)
    fxs, ys = _members((40, 33, 50), rng)
    x32 = P.ColVecs(np.asfortranarray(rng.standard_normal((2, 33)).astype(np.float32)))
    fxs[1] = _f()(x32, np.float32(0.1))
    ys[1] = rng.standard_normal(33).astype(np.float32)
    own = P.logpdf(fxs[1], ys[1])
    assert isinstance(own, np.float32)
    got, rep = P.logpdf_pool(fxs, ys, return_report=True)
    assert got.dtype == np.float64 and got[1] == float(own)
    assert _numpy_double.lib.pool_calls[-1] == ("value", [L.NOISE_SCALAR, L.NOISE_SCALAR])       # two members went down
    assert rep["single_members"] == 1 and rep["pooled_members"] == 2
    assert got[0] == P.logpdf(fxs[0], ys[0]) and got[2] == P.logpdf(fxs[2], ys[2])
    g, grep = P.logpdf_and_gradient_pool(fxs, ys, return_report=True)
    assert g[1]["logpdf"] == P.logpdf_and_gradient(fxs[1], ys[1])["logpdf"] and grep["single_members"] == 1


def test_bad_member_gives_nan_and_its_info(_numpy_double):
    rng = np.random.default_rng(7)
    fxs, ys = _members((20, 140, 60, 35), rng)
    fxs[1] = fxs[1].f(fxs[1].x, -4.0)
    with pytest.raises(P.PosDefException) as e:
        P.logpdf(fxs[1], ys[1])
    vals, infos = P.logpdf_pool(fxs, ys, return_infos=True)
    assert np.isnan(vals[1]) and infos[1] == e.value.info >= 1 and not infos[[0, 2, 3]].any()
    assert np.array_equal(vals[[0, 2, 3]], np.array([P.logpdf(fxs[b], ys[b]) for b in (0, 2, 3)]))
    assert np.isnan(P.logpdf_pool(fxs, ys)[1])                               # without return_infos: no exception either
    got, ginfos = P.logpdf_and_gradient_pool(fxs, ys, return_infos=True)
    assert np.isnan(got[1]["logpdf"]) and got[1]["info"] == ginfos[1] == e.value.info and got[1]["terms"] is None
    assert got[2]["logpdf"] == P.logpdf_and_gradient(fxs[2], ys[2])["logpdf"]


def test_null_outputs_through_the_abi_signature(_numpy_double):
    rng = np.random.default_rng(8)
    fxs, ys = _members((30, 70, 45), rng, _mixed_noise)
    keep = []
    for fx, y in zip(fxs, ys):
        spec = P.finite_gp._prior_spec(fx.f, fx.x)
        kind, nbuf = L._noise_args(fx.noise, len(fx))
        keep.append((spec, np.asfortranarray(P.mean_vector(fx.f, fx.x), dtype=np.float64), kind, nbuf, np.asarray(y, dtype=np.float64)))
    nb = len(keep)

    def ptrs(arrs):
        return (_DP * nb)(*[L.dptr(a) if a is not None else None for a in arrs])

    specs = (C.POINTER(L.sgp_cov_spec) * nb)(*[C.pointer(k[0].c) for k in keep])
    kinds = (C.c_int * nb)(*[k[2] for k in keep])
    lp = np.zeros(nb)
    gy = [np.full(len(k[4]), 7.0) for k in keep]
    gy[1] = None
    gc = [np.full(max(1, k[0].n_terms), 7.0) for k in keep]
    gn = [np.full(70, 7.0) for _ in keep]
    fn = L.default_context().pool.sgp_logpdf_grad_pool
    args = [None, nb, specs, None, kinds, ptrs([k[3] for k in keep]), ptrs([k[4] for k in keep]), L.dptr(lp), ptrs(gy), None,
            None, ptrs(gc), None, None, None]
    assert len(args) == len(L._SIGS_POOL["sgp_logpdf_grad_pool"][1])
    assert fn(*args) == 0
    for b, (fx, y) in enumerate(zip(fxs, ys)):
        ref = P.logpdf_and_gradient(fx, y)
        assert lp[b] == ref["logpdf"]
        if gy[b] is not None:
            assert np.array_equal(gy[b], ref["y"])
        assert np.array_equal(gc[b], ref["_raw"][0][:len(gc[b])])
        assert np.all(gn[b] == 7.0)                                           # grad_noise == NULL: untouched
    out = np.zeros(nb)
    vargs = [None, nb, specs, None, kinds, ptrs([k[3] for k in keep]), ptrs([k[4] for k in keep]), L.dptr(out), None, None]
    assert len(vargs) == len(L._SIGS_POOL["sgp_logpdf_pool"][1])
    assert L.default_context().pool.sgp_logpdf_pool(*vargs) == 0             # infos and report NULL
    assert np.array_equal(out, lp)


def test_argument_checks_come_before_the_call(_numpy_double):
    rng = np.random.default_rng(9)
    fxs, ys = _members((20, 30), rng)
    for fn in (P.logpdf_pool, P.logpdf_and_gradient_pool):
        with pytest.raises(ValueError):
            fn(fxs, ys[:1])
        with pytest.raises(ValueError):
            fn(fxs, [ys[0], ys[1][:-1]])
    assert _numpy_double.lib.pool_calls == []
    assert P.logpdf_pool([], []).shape == (0,)
    vals, infos, rep = P.logpdf_pool([], [], return_infos=True, return_report=True)
    assert vals.shape == (0,) and infos.shape == (0,) and rep["pool_launches"] == 0
    assert P.logpdf_and_gradient_pool([], []) == []
    sp = P.SparseFiniteGP(fxs[0], _f()(P.ColVecs(np.asfortranarray(rng.standard_normal((2, 5)))), 1e-6))
    for fn in (P.logpdf_pool, P.logpdf_and_gradient_pool):
        with pytest.raises(NotImplementedError):
            fn([sp], [ys[0]])
