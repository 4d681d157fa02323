"""P.mean_and_var_and_gradient -> sgp_posterior_predict_grad_x / sgp_sparse_posterior_predict_grad_x WITHOUT a GPU: what the
host mirror marshals (the cross and prior specs, the prior mean, one pointer per spec input), the block layout of what it
returns, the chaining of the spec-input gradients back through stretch / select / periodic / shift, the noise added to the
variance only, and every refusal, against the NumPy double of the C-ABI (tests/np_capi.py).  The double learns the two entry
points from the words of include/sthenomi_predgrad.h (tests/predgrad_np.py).  The chained gradients are held to central
differences of the ORACLE's posterior (oracle.abstractgps), which shares no code with either."""
import numpy as np
import pytest

import models
import np_capi
import oracle.abstractgps as oagp
import oracle.stheno as ost
import predgrad_np
import stheno_jl_amd as P
from test_gpu_predgrad import warped_model

L = P.lib
H = 2.0 ** -17          # central differences of the oracle's float64 posterior: h^2 |f'''| / 6 + eps-level noise / h


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    return predgrad_np.install(monkeypatch)


def _warped():
    fo, go = warped_model(models.oracle_api())
    fp, gp = warped_model(models.product_api())
    return ost.GPPP(fo, go), P.GPPP(fp, gp)


def _data(rng):
    X = [rng.standard_normal((3, 25)), rng.standard_normal((3, 15))]
    Xt = [rng.standard_normal((3, 6)), rng.standard_normal((3, 4))]
    return X, Xt, rng.standard_normal(40)


def _block_data(api, names, Xs):
    return api.BlockData([api.GPPPInput(k, api.ColVecs(np.asfortranarray(x))) for k, x in zip(names, Xs)])


def _kf():
    import oracle.kernelfunctions as okf
    ns = models.oracle_api()
    ns.ColVecs = okf.ColVecs
    return ns


def _omv(post, xs, noise):
    """mean_and_var of the oracle's posterior at xs, the noise added to the variance"""
    m, v = post.mean_and_var(xs)
    return np.asarray(m), np.asarray(v) + noise


def test_chained_gradients_against_central_differences_of_the_oracles_posterior(_numpy_double):
    rng = np.random.default_rng(41)
    Fo, Fp = _warped()
    X, Xt, y = _data(rng)
    oa, pa = _kf(), models.product_api()
    po = oagp.posterior(Fo(_block_data(oa, ("f", "g"), X), 0.1), y)
    pp = P.posterior(Fp(_block_data(pa, ("f", "g"), X), 0.1), y)
    noise_t = 0.1 + rng.random(10)
    g = P.mean_and_var_and_gradient(pp(_block_data(pa, ("g", "f"), Xt), noise_t))
    assert [c["fn"] for c in _numpy_double.lib.predgrad_calls] == ["sgp_posterior_predict_grad_x"]
    assert _numpy_double.lib.predgrad_calls[0] == {"fn": "sgp_posterior_predict_grad_x", "mean_s": True, "var": True,
                                                    "gm": True, "gv": True, "gp": True}
    # layout: one (D, n) array per block of x*, the raw arrays one per spec input
    assert [a.shape for a in g["d_mean"]] == [(3, 6), (3, 4)] == [a.shape for a in g["d_var"]]
    assert len(g["inputs_mean"]) == len(g["inputs_var"]) == len(g["_cross"].inputs)
    assert len(g["inputs_var_prior"]) == len(g["_prior"].inputs)
    # the values: those of mean_and_var, the noise in var only, and the oracle's
    m, v = P.mean_and_var(pp(_block_data(pa, ("g", "f"), Xt), noise_t))
    m0, v0 = P.mean_and_var(pp(_block_data(pa, ("g", "f"), Xt)))
    assert np.array_equal(g["mean"], m) and np.array_equal(g["var"], v)
    assert np.array_equal(m, m0) and np.allclose(v - v0, noise_t, rtol=0, atol=1e-15)
    mo, vo = _omv(po, _block_data(oa, ("g", "f"), Xt), noise_t)
    assert np.max(np.abs(m - mo)) < 1e-10 and np.max(np.abs(v - vo)) < 1e-10
    worst = 0.0
    for blk in range(2):
        for d in range(3):
            Xp, Xm = [a.copy() for a in Xt], [a.copy() for a in Xt]
            Xp[blk][d, :] += H
            Xm[blk][d, :] -= H
            mp, vp = _omv(po, _block_data(oa, ("g", "f"), Xp), noise_t)
            mm, vm = _omv(po, _block_data(oa, ("g", "f"), Xm), noise_t)
            sl = slice(0, 6) if blk == 0 else slice(6, 10)
            worst = max(worst, float(np.abs((mp - mm)[sl] / (2 * H) - g["d_mean"][blk][d]).max()),
                        float(np.abs((vp - vm)[sl] / (2 * H) - g["d_var"][blk][d]).max()))
    print(f"largest difference to the oracle's central differences: {worst:.3e}")
    # h^2 M3 W / 6 with M3 = 340 (tests/test_gpu_predgrad.py) and W up to 1e3 is 3e-6; the oracle's LAPACK posterior carries
    # 1e-12-level noise, / h = 1e-7
    assert worst < 5e-6
    assert max(float(np.abs(a).max()) for a in g["d_mean"] + g["d_var"]) > 1e-2


def test_sparse_posterior_and_shared_input_blocks(_numpy_double):
    rng = np.random.default_rng(42)
    Fo, Fp = _warped()
    X, Xt, y = _data(rng)
    Z = [rng.standard_normal((3, 7))]
    oa, pa = _kf(), models.product_api()
    so = oagp.posterior_vfe(oagp.VFE(Fo(_block_data(oa, ("f",), Z), 1e-6)), Fo(_block_data(oa, ("f", "g"), X), 0.1), y)
    sp = P.posterior(P.VFE(Fp(_block_data(pa, ("f",), Z), 1e-6)), Fp(_block_data(pa, ("f", "g"), X), 0.1), y)
    g = P.mean_and_var_and_gradient(sp(_block_data(pa, ("g", "f"), Xt), 0.05))
    assert [c["fn"] for c in _numpy_double.lib.predgrad_calls] == ["sgp_sparse_posterior_predict_grad_x"]
    worst = 0.0
    for blk in range(2):
        for d in range(3):
            Xp, Xm = [a.copy() for a in Xt], [a.copy() for a in Xt]
            Xp[blk][d, :] += H
            Xm[blk][d, :] -= H
            mp, vp = _omv(so, _block_data(oa, ("g", "f"), Xp), 0.05)
            mm, vm = _omv(so, _block_data(oa, ("g", "f"), Xm), 0.05)
            sl = slice(0, 6) if blk == 0 else slice(6, 10)
            worst = max(worst, float(np.abs((mp - mm)[sl] / (2 * H) - g["d_mean"][blk][d]).max()),
                        float(np.abs((vp - vm)[sl] / (2 * H) - g["d_var"][blk][d]).max()))
    print(f"sparse: largest difference to the oracle's central differences: {worst:.3e}")
    assert worst < 5e-5          # (Sigma_z = 1e-6: the oracle's own values carry more rounding here)
    # a single GPPPInput is one block
    one = P.mean_and_var_and_gradient(sp(P.GPPPInput("f", P.ColVecs(np.asfortranarray(Xt[1])))))
    assert len(one["d_mean"]) == 1 and one["d_mean"][0].shape == (3, 4)
    assert np.allclose(one["d_mean"][0], g["d_mean"][1], rtol=0, atol=1e-12)


def test_float32_test_points_and_float32_models(_numpy_double):
    rng = np.random.default_rng(43)
    F = P.gppp_sum_model()
    x64, s64, y = rng.standard_normal(20), rng.standard_normal(6), rng.standard_normal(20)
    post32 = P.posterior(F(P.GPPPInput("f3", x64.astype(np.float32)), 0.1), y)
    g = P.mean_and_var_and_gradient(post32(P.GPPPInput("f1", s64.astype(np.float32)), 0.2))
    assert len(_numpy_double.lib.predgrad_calls) == 1            # through _ensure() to the fp64 factor, as cov
    assert g["mean"].dtype == np.float32 and g["var"].dtype == np.float32
    assert g["d_mean"][0].shape == (1, 6) and g["d_mean"][0].dtype == np.float64
    post64 = P.posterior(F(P.GPPPInput("f3", x64), 0.1), y)
    g64 = P.mean_and_var_and_gradient(post64(P.GPPPInput("f1", s64), 0.2))
    assert g64["mean"].dtype == np.float64
    assert np.allclose(g["d_mean"][0], g64["d_mean"][0], rtol=0, atol=1e-5)


def _sigma(pt):
    return 1.0 + 0.3 * float(np.sin(np.sum(pt)))


def test_every_refusal_names_its_reason(_numpy_double):
    rng = np.random.default_rng(44)
    x, xt, y = rng.standard_normal(12), rng.standard_normal(4), rng.standard_normal(12)

    def post_of(build, name="f", noise=0.1):
        F = P.gppp(build)
        return F, P.posterior(F(P.GPPPInput(name, x), noise), y)

    # a test-side term with a row scale
    F, post = post_of(lambda GP: (lambda a: {"f": a, "h": _sigma * a})(GP(P.SEKernel())))
    with pytest.raises(NotImplementedError, match="scale"):
        P.mean_and_var_and_gradient(post(P.GPPPInput("h", xt)))
    assert P.mean_and_var_and_gradient(post(P.GPPPInput("f", xt)))["d_mean"][0].shape == (1, 4)   # (the data side may carry one)
    F, post = post_of(lambda GP: (lambda a: {"f": a, "h": _sigma * a})(GP(P.SEKernel())), name="h")
    assert P.mean_and_var_and_gradient(post(P.GPPPInput("f", xt)))["d_var"][0].shape == (1, 4)
    # a test-side prior mean that is a function of the point; a constant one is fine
    F, post = post_of(lambda GP: {"f": GP(np.sin, P.SEKernel()), "c": GP(0.7, P.SEKernel())})
    with pytest.raises(NotImplementedError, match="mean"):
        P.mean_and_var_and_gradient(post(P.GPPPInput("f", xt)))
    g = P.mean_and_var_and_gradient(post(P.GPPPInput("c", xt)))
    assert np.allclose(g["mean"], 0.7) and not np.any(g["d_mean"][0])              # independent of the data: the prior
    # products of kernels, stencils, patches -- on the test side of a model whose data side is plain (the double factors
    # plain terms only)
    F, post = post_of(lambda GP: {"f": GP(P.SEKernel()), "p": GP(P.KernelProduct([P.SEKernel(), P.Matern32Kernel()]))})
    with pytest.raises(NotImplementedError, match="product"):
        P.mean_and_var_and_gradient(post(P.GPPPInput("p", xt)))
    F, post = post_of(lambda GP: (lambda a: {"f": a, "s": P.stencil(a, [0.0, 0.1], [0.5, 0.5])})(GP(P.SEKernel())))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.mean_and_var_and_gradient(post(P.GPPPInput("s", xt)))
    gpc = P.GPC()
    atom = P.atomic(P.GP(P.SEKernel()), gpc)
    Fc = P.GPPP({"f": atom, "c": P.patch_convolve(atom, patch_shape=(2, 2))}, gpc)
    pc = P.posterior(Fc(P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((4, 12))))), 0.1), y)
    with pytest.raises(NotImplementedError, match="patch"):
        P.mean_and_var_and_gradient(pc(P.GPPPInput("c", P.ImageVector(rng.standard_normal((3, 3, 4))))))
    # a multi-GPU context, an explicit posterior, a prior, a SparseFiniteGP
    F, post = post_of(lambda GP: {"f": GP(P.SEKernel())})
    _numpy_double.is_multi = True
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        P.mean_and_var_and_gradient(post(P.GPPPInput("f", xt)))
    _numpy_double.is_multi = False
    spost = P.posterior(P.VFE(F(P.GPPPInput("f", x[:5]), 1e-6)), F(P.GPPPInput("f", x), 0.1), y)
    ex = P.posterior(spost(P.GPPPInput("f", xt), 0.3), y[:4])
    assert isinstance(ex, P.finite_gp.ExplicitPosteriorGP)
    with pytest.raises(NotImplementedError, match="ExplicitPosteriorGP"):
        P.mean_and_var_and_gradient(ex(P.GPPPInput("f", xt)))
    with pytest.raises(NotImplementedError, match="posterior"):
        P.mean_and_var_and_gradient(F(P.GPPPInput("f", xt)))
    calls = len(_numpy_double.lib.predgrad_calls)
    # refusals of the library become errors that name the entry point
    _numpy_double.lib.sharded.add(id(post._h))
    with pytest.raises(P.SthenoMIError, match="sgp_posterior_predict_grad_x.*multi-GPU"):
        P.mean_and_var_and_gradient(post(P.GPPPInput("f", xt)))
    _numpy_double.lib.sharded.clear()
    assert len(_numpy_double.lib.predgrad_calls) == calls + 1


def test_the_abi_signature_and_a_size_mismatch(_numpy_double):
    rng = np.random.default_rng(45)
    F = P.gppp_sum_model()
    x, xt, y = rng.standard_normal(12), rng.standard_normal(4), rng.standard_normal(12)
    post = P.posterior(F(P.GPPPInput("f3", x), 0.1), y)
    cross = P.build_spec(F, P.GPPPInput("f1", xt), F, P.GPPPInput("f3", x))[0]
    good = P.build_spec(F, P.GPPPInput("f1", xt))[0]
    other = P.build_spec(F, P.GPPPInput("f1", rng.standard_normal(5)))[0]
    assert len(L._SIGS_PREDGRAD["sgp_posterior_predict_grad_x"][1]) == 9
    fn = L.default_context().predgrad.sgp_posterior_predict_grad_x
    ms, mo, vo = np.zeros(4), np.zeros(4), np.zeros(4)
    assert fn(post._h, cross.ref(), other.ref(), L.dptr(ms), L.dptr(mo), L.dptr(vo), None, None, None) < 0
    assert b"sgp_posterior_predict_grad_x" in _numpy_double.lib.sgp_last_error()
    assert fn(post._h, cross.ref(), good.ref(), L.dptr(ms), L.dptr(mo), L.dptr(vo), None, None, None) == 0
    m, v = P.mean_and_var(post(P.GPPPInput("f1", xt)))
    assert np.allclose(mo, m) and np.allclose(vo, v - 1e-18)
