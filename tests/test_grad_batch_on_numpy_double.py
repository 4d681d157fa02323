"""`logpdf_and_gradient_batch` -> sgp_logpdf_grad_batch WITHOUT a GPU: the host mirror's marshalling (the pointer arrays of
specs / means / noises / ys / five gradient outputs), its result mapping (the dicts of `logpdf_and_gradient`, mirror terms
folded), the NaN + info convention and the member-by-member routes, against the NumPy double of the C-ABI (tests/np_capi.py).
The double learns the batch entry point here, from its own single-member gradient, as include/sthenomi.h specifies it: member b
is exactly the member's sgp_logpdf_grad call, NULL arrays / elements skip outputs.  The pooled factorisation itself is
tests/test_gpu_grad_batch.py's business."""
import ctypes as C

import numpy as np
import pytest

import np_capi
import stheno_jl_amd as P
from oracle import reference_model as orm

L = P.lib


def _grad_batch(self, ctx, nspec, specs, means, kind, noises, ys, lp_out, gy, gm, gn, gc, gs, infos):
    self.batch_calls.append((nspec, kind))
    lp = np.ctypeslib.as_array(lp_out, shape=(nspec,))
    inf = np.ctypeslib.as_array(infos, shape=(nspec,)) if infos else None
    first_bad = 0
    for b in range(nspec):
        if inf is not None:
            inf[b] = 0
        one = np.zeros(1)

        def at(arr):
            return arr[b] if arr else None

        rc = self.sgp_logpdf_grad(ctx, specs[b], means[b] if means else None, kind, noises[b], ys[b],
                                  one.ctypes.data_as(C.POINTER(C.c_double)), at(gy), at(gm), at(gn), at(gc), at(gs))
        if rc < 0:
            return rc
        if rc > 0:
            lp[b] = np.nan
            if inf is not None:
                inf[b] = rc
            first_bad = first_bad or rc
        else:
            lp[b] = one[0]
    return 0 if inf is not None else first_bad


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    ctx = np_capi.install(monkeypatch)
    monkeypatch.setattr(np_capi.FakeLib, "sgp_logpdf_grad_batch", _grad_batch, raising=False)
    ctx.lib.batch_calls = []
    ctx.batch = ctx.lib          # (Context.batch: libsthenomi_batch.so; the double serves both libraries)
    return ctx


def _gppp_members(B, rng, noise=lambda b, n: 0.1 + 0.05 * b):
    F = P.gppp_sum_model()
    fxs, ys, raw = [], [], []
    for b in range(B):
        xs = [np.asfortranarray(rng.standard_normal((2, n))) for n in (30, 25, 40)]
        x = P.BlockData([P.GPPPInput(k, P.ColVecs(v)) for k, v in zip(("f1", "f2", "f3"), xs)])
        y = rng.standard_normal(95)
        fxs.append(F(x, noise(b, 95)))
        ys.append(y)
        raw.append((xs, y))
    return F, fxs, ys, raw


def _same(got, ref):
    assert set(got) == set(ref)
    assert got["logpdf"] == ref["logpdf"]
    assert np.array_equal(got["y"], ref["y"]) and np.array_equal(got["mean"], ref["mean"])
    assert np.array_equal(np.asarray(got["noise"]), np.asarray(ref["noise"])) and type(got["noise"]) is type(ref["noise"])
    assert [(t["I"], t["J"], t["t"], t["mirror_t"]) for t in got["terms"]] == [(t["I"], t["J"], t["t"], t["mirror_t"])
                                                                             for t in ref["terms"]]
    assert [(t["d_coef"], t["d_inscale"]) for t in got["terms"]] == [(t["d_coef"], t["d_inscale"]) for t in ref["terms"]]


def test_batch_maps_every_member_like_its_own_call(_numpy_double):
    rng = np.random.default_rng(4)
    _, fxs, ys, raw = _gppp_members(4, rng)
    got = P.logpdf_and_gradient_batch(fxs, ys)
    assert _numpy_double.lib.batch_calls == [(4, L.NOISE_SCALAR)]
    assert len(got) == 4
    for g, fx, y, (xs, yy), b in zip(got, fxs, ys, raw, range(4)):
        _same(g, P.logpdf_and_gradient(fx, y))
        assert abs(g["logpdf"] - orm.gppp_sum_logpdf(xs, yy, 0.1 + 0.05 * b)) <= 1e-10 * abs(g["logpdf"])
        assert len(g["terms"]) < g["_spec"].n_terms           # mirror-image pairs folded into the lower ones
    # diagonal noise: one pooled call with the DIAG kind, a vector per member
    _, fxd, ysd, _ = _gppp_members(3, rng, noise=lambda b, n: 0.05 + np.random.default_rng(b).random(n))
    got = P.logpdf_and_gradient_batch(fxd, ysd)
    assert _numpy_double.lib.batch_calls[-1] == (3, L.NOISE_DIAG)
    for g, fx, y in zip(got, fxd, ysd):
        _same(g, P.logpdf_and_gradient(fx, y))
        assert g["noise"].shape == (95,)


def test_bad_member_gives_nan_and_its_info(_numpy_double):
    rng = np.random.default_rng(5)
    F, fxs, ys, _ = _gppp_members(4, rng)
    fxs[1] = F(fxs[1].x, -4.0)
    with pytest.raises(P.PosDefException) as e:
        P.logpdf_and_gradient(fxs[1], ys[1])
    got, infos = P.logpdf_and_gradient_batch(fxs, ys, return_infos=True)
    assert np.isnan(got[1]["logpdf"]) and got[1]["info"] == infos[1] == e.value.info >= 1
    assert got[1]["terms"] is None and got[1]["y"] is None
    assert infos.dtype == np.int32 and not infos[[0, 2, 3]].any()
    for b in (0, 2, 3):
        _same(got[b], P.logpdf_and_gradient(fxs[b], ys[b]))
    assert len(P.logpdf_and_gradient_batch(fxs, ys)) == 4       # without return_infos: no exception either


def test_mixed_and_dense_noise_go_member_by_member(_numpy_double):
    rng = np.random.default_rng(6)
    F, fxs, ys, _ = _gppp_members(3, rng)
    mixed = list(fxs)
    mixed[2] = F(fxs[2].x, 0.05 + rng.random(95))
    Bm = rng.standard_normal((95, 3))
    dense = [F(fx.x, 0.2 * np.eye(95) + 0.01 * Bm @ Bm.T) for fx in fxs]
    for batch in (mixed, dense):
        _numpy_double.lib.batch_calls.clear()
        got = P.logpdf_and_gradient_batch(batch, ys)
        assert _numpy_double.lib.batch_calls == []
        for g, fx, y in zip(got, batch, ys):
            _same(g, P.logpdf_and_gradient(fx, y))
    assert got[0]["noise"].shape == (95, 95)
    bad = list(dense)
    bad[0] = F(fxs[0].x, -4.0 * np.eye(95))
    got, infos = P.logpdf_and_gradient_batch(bad, ys, return_infos=True)
    assert np.isnan(got[0]["logpdf"]) and infos[0] >= 1 and not infos[1:].any()


def test_argument_checks(_numpy_double):
    rng = np.random.default_rng(7)
    _, fxs, ys, _ = _gppp_members(2, rng)
    with pytest.raises(ValueError):
        P.logpdf_and_gradient_batch(fxs, ys[:1])
    with pytest.raises(ValueError):
        P.logpdf_and_gradient_batch(fxs, [ys[0], ys[1][:-1]])
    assert P.logpdf_and_gradient_batch([], []) == []
    res, infos = P.logpdf_and_gradient_batch([], [], return_infos=True)
    assert res == [] and infos.shape == (0,)
    f = P.stretch(P.atomic(P.GP(P.SEKernel()), P.GPC()), 2.0)
    x = P.ColVecs(np.asfortranarray(rng.standard_normal((2, 20))))
    post = P.posterior(f(x, 0.1), rng.standard_normal(20))
    with pytest.raises(NotImplementedError):
        P.logpdf_and_gradient_batch([post(x, 0.1)], [rng.standard_normal(20)])
    sp = P.SparseFiniteGP(f(x, 0.1), f(P.ColVecs(np.asfortranarray(rng.standard_normal((2, 5)))), 1e-6))
    with pytest.raises(NotImplementedError):
        P.logpdf_and_gradient_batch([sp], [rng.standard_normal(20)])


def test_null_outputs_through_the_abi_signature(_numpy_double):
    """the ctypes table of lib.py takes NULL for a whole output array and for single elements: the skipped outputs stay as
    they were, the others are the member's own call's"""
    rng = np.random.default_rng(8)
    _, fxs, ys, _ = _gppp_members(3, rng)
    keep = []
    for fx, y in zip(fxs, ys):
        spec = P.finite_gp._prior_spec(fx.f, fx.x)
        kind, nbuf = L._noise_args(fx.noise, len(fx))
        keep.append((spec, np.asfortranarray(P.mean_vector(fx.f, fx.x), dtype=np.float64), nbuf, np.asarray(y, dtype=np.float64)))
    nb = len(keep)

    def ptrs(arrs):
        return (C.POINTER(C.c_double) * nb)(*[L.dptr(a) if a is not None else None for a in arrs])

    specs = (C.POINTER(L.sgp_cov_spec) * nb)(*[C.pointer(k[0].c) for k in keep])
    lp = np.zeros(nb)
    gy = [np.full(95, 7.0), None, np.full(95, 7.0)]
    gc = [np.full(k[0].n_terms, 7.0) for k in keep]
    gn = [np.full(1, 7.0) for _ in keep]
    fn = L.default_context().batch.sgp_logpdf_grad_batch
    argtypes = L._SIGS_BATCH["sgp_logpdf_grad_batch"][1]
    args = [None, nb, specs, ptrs([k[1] for k in keep]), L.NOISE_SCALAR, ptrs([k[2] for k in keep]),
            ptrs([k[3] for k in keep]), L.dptr(lp), ptrs(gy), None, None, ptrs(gc), None, None]
    assert len(args) == len(argtypes)
    assert fn(*args) == 0
    for b, (fx, y) in enumerate(zip(fxs, ys)):
        ref = P.logpdf_and_gradient(fx, y)
        assert lp[b] == ref["logpdf"]
        if gy[b] is not None:
            assert np.array_equal(gy[b], ref["y"])
        assert np.array_equal(gc[b], ref["_raw"][0][:len(gc[b])])
        assert np.all(gn[b] == 7.0)                            # grad_noise == NULL: untouched
