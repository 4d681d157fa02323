"""Input-point, function-scale and ELBO gradients through product chains on the device (include/sthenomi_kprod_grad.h;
csrc/kprod.hip: grad_kprod_inputs_kernel, diag_grad_kprod_kernel): against the NumPy evaluator (tests/kprod_grad_np.py), the
bit identities with the entry points they are supersets of, `k * ConstantKernel(1)` against plain `k`, zero factors, the ELBO
against central differences of P.elbo, the diagonal, and the refusals.  Every case has N <= 300, M <= 150."""
import ctypes as C

import numpy as np
import pytest

import kprod_grad_np as kg
import kprod_np as kn
import stheno_jl_amd as P
from stheno_jl_amd import lib as L
from test_gpu_kprod import _G, _chain_kernel, _golden_on_two_blocks, _model, _two_blocks
from test_kprod_on_numpy import golden_kernel

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]

PD = C.POINTER(C.c_double)
# the evaluator's need between `k * ConstantKernel(1)` and plain `k` (tests/test_kprod_grad_on_numpy.py measures 0: the
# NumPy forms differ by multiplications with 1.0).  The device's two kernels sum the same <= 300 products per output in the
# same order; a product formed in another association differs by <= 4 roundings: 300 * 4 * 2^-53 = 1.4e-13 of the largest
# partial sum.  1e-12 covers that with the partial sums up to 7 times the result; bits are not pinned.
TOL_CONST_ONE = 1e-12


def _ptrs(arrs, n=None):
    arrs = list(arrs) + [None] * ((n or 0) - len(arrs))
    return (PD * max(1, len(arrs)))(*[L.dptr(a) if a is not None else None for a in arrs])


def _close(a, e, tol=1e-8):
    """the project's bound for a device gradient against the evaluator (tests/test_gpu_parity.py:790), per array"""
    a, e = np.asarray(a, dtype=float), np.asarray(e, dtype=float)
    err, bound = float(np.max(np.abs(a - e))), tol * max(1.0, float(np.max(np.abs(e))))
    print(f"    max|a - e| = {err:.3e}   bound {bound:.3e}   max|e| = {float(np.max(np.abs(e))):.3e}")
    return err <= bound


def _scale_bufs(spec, side, n):
    vecs = spec.term_row_scale if side == "row" else spec.term_col_scale
    return [np.zeros(len(v)) if v is not None else None for v in vecs] + [None] * (n - len(vecs))


def _lp_param_xs(spec, noise, y, inputs=True, scales=True):
    """sgp_logpdf_grad_param_xs on the default context -> dict of every output"""
    ctx, d = L.default_context(), L.dptr
    n, nt = spec.N, max(1, spec.n_terms)
    o = dict(lp=np.zeros(1), gy=np.zeros(n), gm=np.zeros(n), gn=np.zeros(1), gc=np.zeros(nt), gs=np.zeros(nt), gp=np.zeros(nt),
             gx=[np.zeros(a.shape, order="F") for a in spec.inputs] if inputs else None,
             grs=_scale_bufs(spec, "row", nt) if scales else None)
    m, nz = np.zeros(n), np.array([float(noise)])
    rc = L.kprod_grad_lib().sgp_logpdf_grad_param_xs(
        ctx.handle, spec.ref(ctx), d(m), L.NOISE_SCALAR, d(nz), d(np.ascontiguousarray(y)), d(o["lp"]), d(o["gy"]), d(o["gm"]),
        d(o["gn"]), d(o["gc"]), d(o["gs"]), d(o["gp"]), _ptrs(o["gx"]) if inputs else None,
        _ptrs(o["grs"], nt) if scales else None)
    assert rc == 0, L.last_error()
    return o


def _check_against_evaluator(spec, noise, y, pairs=None):
    """input gradients and row-scale sums of a symmetric spec against 2 x the evaluator's row side"""
    o = _lp_param_xs(spec, noise, y)
    G, _ = _G(spec, noise, y)
    ev = kg.np_input_grads(spec, G, pairs)
    for k, (a, e) in enumerate(zip(o["gx"], ev["row"])):
        assert a.shape == e.shape and np.all(np.isfinite(a))
        assert _close(a, 2.0 * e), ("input", k)
    seen = 0
    for t in range(spec.n_terms):
        if spec.term_row_scale[t] is None:
            assert o["grs"][t] is None
            continue
        assert _close(o["grs"][t], 2.0 * ev["rs"][t]), ("row scale", t)
        seen += 1
    return o, ev, seen


# ---- 1. input gradients and row-scale sums against the evaluator -----------------------------------------------------------
@pytest.mark.parametrize("nf,D", [(2, 1), (2, 3), (3, 1), (3, 3), (8, 1), (8, 3)])
def test_input_gradients_of_chains_match_the_evaluator(nf, D):
    F = _model(_chain_kernel(nf))
    x, _ = _two_blocks(D, seed=10 * nf + D)
    spec, _, _ = P.build_spec(F, x)
    assert spec.has_kprod and max(len(ts) for _, _, ts in kn.chains(spec)) == nf
    _check_against_evaluator(spec, 0.1, np.random.default_rng(nf + D).standard_normal(300))


@pytest.mark.parametrize("nf,D", [(4, 16), (8, 8)])
def test_input_gradients_at_the_limits_of_a_chain(nf, D):
    """4 x 16 = 8 x 8 = 64 row coordinates and 64 accumulators per thread, all 65 KiB of LDS"""
    wl = P.with_lengthscale
    k = _chain_kernel(8) if nf == 8 else 0.9 * wl(P.SEKernel(), 2.0) * P.RationalQuadraticKernel(0.7) * P.LinearKernel(0.5) * \
        wl(P.Matern32Kernel(), 1.5)
    x, _ = _two_blocks(D, seed=100 + D)
    spec, _, _ = P.build_spec(_model(k), x)
    assert max(len(ts) for _, _, ts in kn.chains(spec)) == nf and max(a.shape[0] for a in spec.inputs) == D
    _check_against_evaluator(spec, 0.1, np.random.default_rng(D).standard_normal(300))


def test_input_gradients_of_the_golden_kernel_on_two_blocks():
    F, x, _, y = _golden_on_two_blocks()
    spec, _, _ = P.build_spec(F, x)
    assert spec.n_terms == 20
    _check_against_evaluator(spec, 0.1, y)


def _function_scaled(k=None):
    k = k if k is not None else (1.4 * P.SEKernel() * P.with_lengthscale(P.RationalQuadraticKernel(0.9), 1.2) +
                                 0.3 * P.LinearKernel(0.4) * P.Matern32Kernel())
    sigma = lambda v: 1.0 + 0.5 * float(np.sin(np.sum(v)))      # noqa: E731
    F = P.gppp(lambda GP: (lambda f: {"f": f, "g": sigma * f})(GP(k)))
    rng = np.random.default_rng(21)
    Xs = [np.asfortranarray(rng.standard_normal((3, m)) / np.sqrt(3.0)) for m in (170, 130)]
    x = P.BlockData([P.GPPPInput("g", P.ColVecs(Xs[0])), P.GPPPInput("f", P.ColVecs(Xs[1]))])
    return F, x, rng.standard_normal(300)


def test_function_scaled_process_with_a_product_kernel():
    """heads with a row scale, a column scale, both or neither: the row-scale sums ride along with the input pass"""
    F, x, y = _function_scaled()
    spec, _, _ = P.build_spec(F, x)
    heads = [ts[0] for _, _, ts in kn.chains(spec)]
    scaled = [(spec.term_row_scale[t] is not None, spec.term_col_scale[t] is not None) for t in heads]
    assert scaled == [(True, True)] * 2 + [(True, False)] * 2 + [(False, True)] * 2 + [(False, False)] * 2
    _, _, seen = _check_against_evaluator(spec, 0.1, y)
    assert seen == 4


# ---- 2. bit equalities ---------------------------------------------------------------------------------------------------------
def test_outputs_shared_with_the_parameter_gradient_are_bit_equal_and_repeatable():
    F, x, _, y = _golden_on_two_blocks()
    g = P.logpdf_and_gradient(F(x, 0.1), y)                       # sgp_logpdf_grad_param
    spec = g["_spec"]
    o = _lp_param_xs(spec, 0.1, y)
    gc, gs, gp = g["_raw"]
    assert o["lp"][0] == g["logpdf"] and np.array_equal(o["gy"], g["y"]) and np.array_equal(o["gm"], g["mean"])
    assert o["gn"][0] == g["noise"]
    assert np.array_equal(o["gc"], gc) and np.array_equal(o["gs"], gs) and np.array_equal(o["gp"], gp)
    o2 = _lp_param_xs(spec, 0.1, y)
    for a, b in zip(o["gx"], o2["gx"]):
        assert np.array_equal(a, b)
    assert all(np.array_equal(o[k], o2[k]) for k in ("lp", "gy", "gm", "gn", "gc", "gs", "gp"))


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_specs_without_chains_return_the_bits_of_the_entry_points_they_extend():
    """sgp_logpdf_grad_xs, sgp_elbo_grad_xs and sgp_kernelmatrix_diag_grad_xs through their host functions against the three
    new entry points through theirs, on a function-scaled model with plain kernels; and a second call of the new ones"""
    F, x, y = _function_scaled(1.4 * P.with_lengthscale(P.SEKernel(), 1.2) + 0.3 * P.Matern32Kernel() + 0.2 * P.ConstantKernel(0.7))
    fx = F(x, 0.1)
    assert not P.build_spec(F, x)[0].has_kprod
    old = P.logpdf_and_gradient(fx, y, inputs=True, scales=True)
    new = P.logpdf_and_gradient_param(fx, y, inputs=True, scales=True)
    assert old["logpdf"] == new["logpdf"] and old["noise"] == new["noise"]
    for key in ("y", "mean", "inputs", "x", "_rowscale"):
        assert _same(old[key], new[key]), key
    assert _same(old["_raw"], new["_raw"][:2])
    assert _same([s["d_values"] for s in old["scales"]], [s["d_values"] for s in new["scales"]])
    rng = np.random.default_rng(4)
    z = P.BlockData([P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((3, 90)) / np.sqrt(3.0)))),
                     P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((3, 60)) / np.sqrt(3.0))))])
    vfe = P.VFE(F(z, 1e-3))
    eo = P.elbo_and_gradient(vfe, fx, y, inputs=True, scales=True)
    en = P.elbo_and_gradient_param(vfe, fx, y, inputs=True, scales=True)
    en2 = P.elbo_and_gradient_param(vfe, fx, y, inputs=True, scales=True)
    assert eo["elbo"] == en["elbo"] == en2["elbo"] and eo["noise"] == en["noise"] and eo["z_noise"] == en["z_noise"]
    for key in ("y", "mean", "var", "x", "z", "zz_inputs", "xz_inputs"):
        assert _same(eo[key], en[key]) and _same(en[key], en2[key]), key
    for key in ("zz", "xz", "xx"):                              # xx: sgp_kernelmatrix_diag_grad_xs / _param
        assert _same(eo["_raw"][key], en["_raw"][key][:2]) and _same(en["_raw"][key], en2["_raw"][key]), key
    assert _same([s["d_values"] for s in eo["scales"]], [s["d_values"] for s in en["scales"]])
    # d / d param of a plain spec: SGP_CONST alone
    for key in ("zz", "xz", "xx"):
        sp, gp = en["_specs"][key], en["_raw"][key][2]
        const = np.array([sp._terms[t].kind == L.CONST for t in range(sp.n_terms)])
        assert np.all(gp[:sp.n_terms][~const] == 0.0) and np.any(gp[:sp.n_terms][const] != 0.0)


# ---- 3. k * ConstantKernel(1) against plain k -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se", "matern12", "matern32", "matern52"])
def test_times_constant_one_has_the_gradients_of_the_plain_kernel(name):
    k = {"se": P.SEKernel, "matern12": P.Matern12Kernel, "matern32": P.Matern32Kernel, "matern52": P.Matern52Kernel}[name]
    x, ins = _two_blocks(3, seed=5)
    rng = np.random.default_rng(6)
    y = rng.standard_normal(300)
    plain, chained = _model(1.7 * P.with_lengthscale(k(), 0.6)), _model(1.7 * P.with_lengthscale(k(), 0.6) * P.ConstantKernel(1.0))
    gp_ = P.logpdf_and_gradient(plain(x, 0.1), y, inputs=True)
    gc_ = P.logpdf_and_gradient_param(chained(x, 0.1), y, inputs=True)
    assert gc_["_spec"].has_kprod and gc_["logpdf"] == gp_["logpdf"]
    for a, e in zip(gc_["x"], gp_["x"]):
        assert _close(a, e, TOL_CONST_ONE)
    z = P.BlockData([P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((3, m)) / np.sqrt(3.0)))) for m in (90, 60)])
    ep = P.elbo_and_gradient(P.VFE(plain(z, 1e-3)), plain(x, 0.1), y, inputs=True)
    ec = P.elbo_and_gradient_param(P.VFE(chained(z, 1e-3)), chained(x, 0.1), y, inputs=True)
    assert ec["elbo"] == ep["elbo"]
    for key in ("x", "z"):
        for a, e in zip(ec[key], ep[key]):
            assert _close(a, e, TOL_CONST_ONE), key
    for key in ("y", "mean", "var"):
        assert _close(ec[key], ep[key], TOL_CONST_ONE), key
    assert _close(ec["noise"], ep["noise"], TOL_CONST_ONE)
    for key in ("zz_terms", "xz_terms", "xx_terms"):
        heads = [r for r in ec[key] if r["factor"] == 0]
        assert len(heads) == len(ep[key])
        assert _close([r["d_coef"] for r in heads], [r["d_coef"] for r in ep[key]], TOL_CONST_ONE), key
        assert _close([r["d_inscale"] for r in heads], [r["d_inscale"] for r in ep[key]], TOL_CONST_ONE), key


# ---- 4. zero factors ---------------------------------------------------------------------------------------------------------------
def _without_pairs(spec, drop):
    """the same spec without the terms of the block pairs in `drop`"""
    nb = len(spec.col_len)
    pairs = {}
    for p in range(len(spec.row_len) * nb):
        if (p // nb, p % nb) in drop:
            continue
        pairs[(p // nb, p % nb)] = [(spec._terms[t].kind, spec._terms[t].row_input, spec._terms[t].col_input, spec._terms[t].coef,
                                     spec._terms[t].param, spec.term_row_scale[t], spec.term_col_scale[t])
                                    for t in range(spec._term_ptr[p], spec._term_ptr[p + 1])]
    return L.Spec(spec.row_len, spec.col_len, spec.inputs, pairs, True)


@pytest.mark.parametrize("case", ["white_factor", "far_clusters"])
def test_zero_factors_give_exact_zeros_and_finite_values(case):
    if case == "white_factor":
        k = 1.5 * P.SEKernel() * P.WhiteKernel() * P.RationalQuadraticKernel(0.8) + 0.5 * P.Matern32Kernel()
        x, _ = _two_blocks(3, seed=9)
    else:
        k = 1.5 * P.SEKernel() * P.RationalQuadraticKernel(0.8) * P.LinearKernel(0.3) + 0.5 * P.Matern32Kernel()
        x, _ = _two_blocks(3, seed=9, shift=1e3)
    y = np.random.default_rng(10).standard_normal(300)
    spec, _, _ = P.build_spec(_model(k), x)
    o, _, _ = _check_against_evaluator(spec, 0.1, y)
    for a in [o["lp"], o["gy"], o["gm"], o["gn"], o["gc"], o["gs"], o["gp"]] + o["gx"]:
        assert np.all(np.isfinite(a))
    if case == "far_clusters":
        assert np.all(P.prior_cov(_model(k), x)[:170, 170:] == 0.0)
        alone = _lp_param_xs(_without_pairs(spec, {(0, 1), (1, 0)}), 0.1, y)
        for a, b in zip(o["gx"], alone["gx"]):
            assert np.array_equal(a, b)


# ---- 5. the ELBO ----------------------------------------------------------------------------------------------------------------
TH0 = dict(v1=4.0, l=1.5, r=0.6, v2=0.7, alpha=1.3, l2=0.8, v3=0.1, c=0.25)
STRETCH = 0.8


def hyper_model(th, a=STRETCH):
    """SE(l) * (Periodic(r) o ScaleTransform) + RQ + Polynomial(2, c) below a stretch"""
    k = (th["v1"] * P.with_lengthscale(P.SEKernel(), th["l"]) * (P.PeriodicKernel(th["r"]) @ P.ScaleTransform(1.0 / 0.9)) +
         th["v2"] * P.with_lengthscale(P.RationalQuadraticKernel(th["alpha"]), th["l2"]) +
         th["v3"] * P.PolynomialKernel(2, th["c"]))
    return P.gppp(lambda GP: {"f": P.stretch(GP(k), a)})


def hyper_gradients(recs, th):
    """records in the chain form (five per block pair: SE, Periodic | RQ | Linear, Linear) -> d / d every hyper-parameter"""
    pos = lambda k, key: sum(r[key] for i, r in enumerate(recs) if i % 5 == k)      # noqa: E731
    return dict(v1=pos(0, "d_coef"), l=-pos(0, "d_inscale") / th["l"], r=-pos(1, "d_inscale") / th["r"], v2=pos(2, "d_coef"),
                alpha=pos(2, "d_param"), l2=-pos(2, "d_inscale") / th["l2"], v3=pos(3, "d_coef"),
                c=pos(3, "d_param") + pos(4, "d_param"))


def _elbo_case():
    rng = np.random.default_rng(11)
    xs = [np.sort(rng.uniform(-3.0, 3.0, m)) for m in (170, 130)]
    zs = [np.sort(rng.uniform(-3.0, 3.0, m)) for m in (90, 60)]
    y = np.sin(2.0 * np.concatenate(xs)) + 0.3 * rng.standard_normal(300)
    data = lambda vs: P.BlockData([P.GPPPInput("f", v) for v in vs])      # noqa: E731
    return xs, zs, y, data


ZNOISE = 1e-3


def test_elbo_value_hyperparameters_and_points_of_a_product_model():
    """elbo_out is sgp_elbo's value; every hyper-parameter against central differences of P.elbo (h = 1e-5, 1e-6 max(1, |fd|):
    test_gradient_records_match_central_differences_of_the_hyperparameters); points of x and z against central differences
    with h = 1e-6 at the project's bounds for such checks (tests/test_gpu_parity.py: 2e-5 where the model has no warp chain,
    5e-5 below warps -- this model sits below a stretch and a periodic embedding: 5e-5; the NumPy evaluator needs less on the
    same case, tests/test_kprod_grad_on_numpy.py)"""
    xs, zs, y, data = _elbo_case()

    def bound(th, xv, zv):
        Fm = hyper_model(th)
        return P.elbo(P.VFE(Fm(data(zv), ZNOISE)), Fm(data(xv), 0.1), y)

    F = hyper_model(TH0)
    g = P.elbo_and_gradient_param(P.VFE(F(data(zs), ZNOISE)), F(data(xs), 0.1), y, inputs=True)
    assert g["elbo"] == bound(TH0, xs, zs)
    assert all(sp.has_kprod for sp in g["_specs"].values())
    assert len(g["zz_terms"]) == 15 and len(g["xz_terms"]) == 20 and len(g["xx_terms"]) == 10
    got = {}
    for key in ("zz_terms", "xz_terms", "xx_terms"):
        for name, v in hyper_gradients(g[key], TH0).items():
            got[name] = got.get(name, 0.0) + v
    h = 1e-5
    for name, v0 in TH0.items():
        fd = (bound({**TH0, name: v0 + h}, xs, zs) - bound({**TH0, name: v0 - h}, xs, zs)) / (2 * h)
        print(f"  {name}: got {got[name]:.10e}  fd {fd:.10e}  diff {abs(got[name] - fd):.2e}")
        assert abs(got[name] - fd) <= 1e-6 * max(1.0, abs(fd)), (name, got[name], fd)
    h = 1e-6
    # x: first tile, the tile boundary (points 127 / 128 of 300 lie in block 0), the ragged last tile (block 1)
    for I, i in [(0, 0), (0, 127), (0, 128), (1, 0), (1, 129)]:
        vp, vn = [v.copy() for v in xs], [v.copy() for v in xs]
        vp[I][i] += h
        vn[I][i] -= h
        fd = (bound(TH0, vp, zs) - bound(TH0, vn, zs)) / (2 * h)
        a = np.asarray(g["x"][I]).ravel()[i]
        print(f"  x[{I}][{i}]: got {a:.10e}  fd {fd:.10e}  diff {abs(a - fd):.2e}")
        assert abs(a - fd) <= 5e-5 * max(1.0, abs(fd)), ("x", I, i, a, fd)
    # z in both blocks (M = 150 straddles a tile: point 127 / 128 of the stacked z are block 1's 37 / 38); zz and xz added
    for J, j in [(0, 0), (0, 89), (1, 37), (1, 38), (1, 59)]:
        vp, vn = [v.copy() for v in zs], [v.copy() for v in zs]
        vp[J][j] += h
        vn[J][j] -= h
        fd = (bound(TH0, xs, vp) - bound(TH0, xs, vn)) / (2 * h)
        a = np.asarray(g["z"][J]).ravel()[j]
        print(f"  z[{J}][{j}]: got {a:.10e}  fd {fd:.10e}  diff {abs(a - fd):.2e}")
        assert abs(a - fd) <= 5e-5 * max(1.0, abs(fd)), ("z", J, j, a, fd)


def test_elbo_cotangent_contractions_match_the_evaluator():
    """the zz side (symmetric: row side twice) and the xz side (a row pass for x, a transposed pass for z) of
    sgp_elbo_grad_param against the evaluator contracting NumPy's own cotangents of the Titsias bound"""
    import scipy.linalg as sla
    xs, zs, y, data = _elbo_case()
    F = hyper_model(TH0)
    g = P.elbo_and_gradient_param(P.VFE(F(data(zs), ZNOISE)), F(data(xs), 0.1), y, inputs=True)
    zz, xz = g["_specs"]["zz"], g["_specs"]["xz"]
    Kzz, Kxz = kn.np_spec_matrix(zz) + ZNOISE * np.eye(150), kn.np_spec_matrix(xz)
    # cotangents of the bound with respect to Kzz and Kxz (oracle/abstractgps.py's derivation, in NumPy)
    Lz = np.linalg.cholesky(Kzz)
    A = sla.solve_triangular(Lz, Kxz.T, lower=True) / np.sqrt(0.1)
    Bm = A @ A.T + np.eye(150)
    Le = np.linalg.cholesky(Bm)
    delta = y / np.sqrt(0.1)
    u = sla.cho_solve((Le, True), A @ delta)
    Binv = sla.cho_solve((Le, True), np.eye(150))
    Z = np.eye(150) - Binv - np.outer(u, u)
    S = Bm + Binv - 2.0 * np.eye(150) + np.outer(u, u)
    J = sla.solve_triangular(Lz, np.eye(150), lower=True).T
    dKxz = ((A.T @ Z + np.outer(delta, u)) @ J.T) / np.sqrt(0.1)
    dKzz = -0.5 * J @ S @ J.T
    ez, ex = kg.np_input_grads(zz, dKzz), kg.np_input_grads(xz, dKxz)
    # the cotangents amplify rounding by the conditioning of Kzz + 1e-3 I (~1e5): the project's ELBO bound against its
    # oracle for such contractions, 2e-5 of the largest entry (tests/test_gpu_parity.py:877)
    for k, a in enumerate(g["zz_inputs"]):
        assert _close(a, 2.0 * ez["row"][k], 2e-5), ("zz", k)
    for k, a in enumerate(g["xz_inputs"]):
        assert _close(a, ex["row"][k] + ex["col"][k], 2e-5), ("xz", k)


# ---- 6. the diagonal ----------------------------------------------------------------------------------------------------------------
def _diag_param(spec, w):
    ctx, d = L.default_context(), L.dptr
    nt = max(1, spec.n_terms)
    o = dict(gc=np.zeros(nt), gs=np.zeros(nt), gp=np.zeros(nt), gx=[np.zeros(a.shape, order="F") for a in spec.inputs],
             grs=_scale_bufs(spec, "row", nt), gcs=_scale_bufs(spec, "col", nt))
    rc = L.kprod_grad_lib().sgp_kernelmatrix_diag_grad_param(ctx.handle, spec.ref(ctx), d(w), d(o["gc"]), d(o["gs"]), d(o["gp"]),
                                                             _ptrs(o["gx"]), _ptrs(o["grs"], nt), _ptrs(o["gcs"], nt))
    assert rc == 0, L.last_error()
    return o


def _check_diag(spec, w):
    o, ev = _diag_param(spec, w), kg.np_diag_grads(spec, w)
    n = spec.n_terms
    assert _close(o["gc"][:n], ev["gc"]) and _close(o["gs"][:n], ev["gs"]) and _close(o["gp"][:n], ev["gp"])
    for k, (a, e) in enumerate(zip(o["gx"], ev["gx"])):
        assert _close(a, e), ("input", k)
    for t in range(n):
        for got, want in ((o["grs"][t], ev["rs"][t]), (o["gcs"][t], ev["cs"][t])):
            if want is not None:
                assert got is not None and _close(got, want), ("scale", t)
    return o, ev


def test_diagonal_gradients_where_the_two_views_differ():
    """var(f(a x) + f(b x)): the cross terms of the diagonal read two different views of x"""
    k = 1.3 * P.SEKernel() * P.with_lengthscale(P.RationalQuadraticKernel(0.9), 1.2) + 0.3 * P.LinearKernel(0.4) * P.Matern32Kernel()
    F = P.gppp(lambda GP: (lambda f: {"f": f, "g": P.stretch(f, 0.7) + P.stretch(f, 1.6)})(GP(k)))
    rng = np.random.default_rng(31)
    x = P.BlockData([P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((3, m)) / np.sqrt(3.0)))) for m in (170, 130)])
    spec, _, _ = P.build_spec(F, x)
    assert spec.has_kprod
    o, ev = _check_diag(spec, rng.standard_normal(300))
    assert any(np.max(np.abs(e)) > 1e-3 for e in ev["gx"])      # the distance kinds do not cancel here
    assert np.array_equal(P.prior_var(F, x), kg.np_diag(spec)) or _close(P.prior_var(F, x), kg.np_diag(spec), 1e-13)


def test_diagonal_gradients_of_linear_factors_on_one_view_and_of_scales():
    """LINEAR / Polynomial on one array: the row side gets xc, the column side xr, both added; a function-scaled model for
    the row / column scale outputs"""
    F = _model(0.3 * P.PolynomialKernel(2, 0.25) * P.with_lengthscale(P.SEKernel(), 1.1) + 0.5 * P.LinearKernel(0.2))
    x, _ = _two_blocks(3, seed=41)
    spec, _, _ = P.build_spec(F, x)
    rng = np.random.default_rng(42)
    o, ev = _check_diag(spec, rng.standard_normal(300))
    assert any(np.max(np.abs(e)) > 1e-3 for e in ev["gx"])
    F, x, _ = _function_scaled()
    _check_diag(P.build_spec(F, x)[0], rng.standard_normal(300))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_multi_gpu_context_refuses_the_three_entry_points():
    f = P.atomic(P.GP(P.SEKernel() * P.Matern32Kernel()), P.GPC())
    n = 16
    x, z = np.linspace(0.0, 1.0, n), np.linspace(0.0, 1.0, 4)
    spec, zz, xz = P.build_spec(f, x)[0], P.build_spec(f, z)[0], P.build_spec(f, x, None, z)[0]
    lib, d = L.kprod_grad_lib(), L.dptr
    mctx = L.Context(devices=[0, 0])
    try:
        m, y, nz, lp = np.zeros(n), np.ones(n), np.array([0.1]), np.zeros(1)
        gy, gm, gn, gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(2), np.zeros(2), np.zeros(2)
        rc = lib.sgp_logpdf_grad_param_xs(mctx.handle, spec.ref(mctx), d(m), L.NOISE_SCALAR, d(nz), d(y), d(lp), d(gy), d(gm),
                                          d(gn), d(gc), d(gs), d(gp), None, None)
        assert rc < 0 and "multi-GPU" in L.last_error()
        rc = lib.sgp_kernelmatrix_diag_grad_param(mctx.handle, spec.ref(mctx), d(y), d(gc), d(gs), d(gp), None, None, None)
        assert rc < 0 and "multi-GPU" in L.last_error()
        rc = lib.sgp_elbo_grad_param(mctx.handle, zz.ref(mctx), xz.ref(mctx), d(np.ones(n)), d(m), L.NOISE_SCALAR, d(nz),
                                     L.NOISE_SCALAR, d(np.array([1e-6])), d(y), d(lp), d(gy), d(gm), d(gn), d(np.zeros(n)),
                                     d(np.zeros(1)), d(gc), d(gs), d(gp), d(np.zeros(2)), d(np.zeros(2)), d(np.zeros(2)),
                                     None, None, None, None, None)
        assert rc < 0 and "multi-GPU" in L.last_error()
    finally:
        mctx.close()


def test_patch_and_stencil_specs_are_refused_by_name():
    from test_conv_on_numpy import images
    Fs = P.gppp(lambda GP: (lambda f: {"f": f, "s": P.stencil(f, np.zeros((1, 2)), [1.0, -1.0])})(GP(P.SEKernel())))
    xs = P.GPPPInput("s", np.linspace(0, 1, 8))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.logpdf_and_gradient_param(Fs(xs, 0.1), np.zeros(8))
    spec, _, _ = P.build_spec(Fs, xs)
    ctx, d = L.default_context(), L.dptr
    gc, gs, gp = np.zeros(spec.n_terms), np.zeros(spec.n_terms), np.zeros(spec.n_terms)
    rc = L.kprod_grad_lib().sgp_kernelmatrix_diag_grad_param(ctx.handle, spec.ref(ctx), d(np.ones(8)), d(gc), d(gs), d(gp), None,
                                                             None, None)
    assert rc < 0 and "stencil" in L.last_error()
    Fc = P.gppp(lambda GP: (lambda g: {"g": g, "f": P.patch_convolve(g, patch_shape=(3, 3))})(GP(P.SEKernel())))
    xc = P.GPPPInput("f", images(2))
    with pytest.raises(NotImplementedError, match="patch"):
        P.logpdf_and_gradient_param(Fc(xc, 0.1), np.zeros(2))
    specc, _, _ = P.build_spec(Fc, xc)
    lp = np.zeros(1)
    rc = L.kprod_grad_lib().sgp_logpdf_grad_param_xs(ctx.handle, specc.ref(ctx), None, L.NOISE_SCALAR, d(np.array([0.1])),
                                                     d(np.zeros(2)), d(lp), None, None, None, None, None, None, None, None)
    assert rc < 0 and "patch" in L.last_error()


def test_old_host_functions_still_refuse_and_name_the_new_ones():
    f = P.atomic(P.GP(golden_kernel()), P.GPC())
    x, y = np.linspace(0.0, 1.0, 8), np.zeros(8)
    with pytest.raises(NotImplementedError, match="product.*logpdf_and_gradient_param"):
        P.logpdf_and_gradient(f(x, 0.1), y, inputs=True)
    with pytest.raises(NotImplementedError, match="product.*elbo_and_gradient_param"):
        P.elbo_and_gradient(P.VFE(f(np.zeros(2))), f(x, 0.1), y)
