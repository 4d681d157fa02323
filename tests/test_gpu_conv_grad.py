"""Gradients of logpdf, the diagonal and the ELBO through patch (convolutional) terms on the device
(include/sthenomi_conv_grad.h; kernels in stheno.jl_amd/csrc/conv.hip), through P.logpdf_and_gradient_conv,
P.elbo_and_gradient_conv and the three entry points themselves.

The truth is tests/conv_grad_truth.py: a patch term expanded into the plain terms it is the sum of, run through
tests/grad_truth.py in long double; the bound of a case and output family is MARGIN * max(the same run in float64, the
family's floor) -- from the reference, never from the device.  The shapes are the smallest at which each kernel can go wrong
(conv_grad_truth.CASES says which): lanes idle (P = 36), the lane loop's second trip (P = 72), a zero-padded patch dimension
with two row tiles and every mix of patched and plain sides, the one-sided kernel's second chunk of plain points, the whole
image as one patch, and the staging limit of 3072 pixels with 64-pixel patches."""
import ctypes as C

import numpy as np
import pytest

import conv_grad_truth as CT
import grad_truth as T
import stheno_jl_amd as P
from test_conv_on_numpy import np_patches

pytestmark = pytest.mark.gpu

d = P.lib.dptr


def _case(id):
    return next(c for c in CT.CASES if c.id == id)


# ---- logpdf ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CT.LP_CASES, ids=repr)
def test_logpdf_gradient_against_truth(case):
    F, fx, y = case.build()
    g = P.logpdf_and_gradient_conv(fx, y)
    assert g["_spec"].has_patch
    out = CT.logpdf_outputs(g)
    for v in out.values():
        assert not np.any(np.isnan(v))
    R, *R64 = CT.logpdf_truth(case, g, fx, y)
    CT.hold(case, CT.logpdf_units(out, R), CT.yardstick(CT.logpdf_units(CT.logpdf_reference_outputs(r), R) for r in R64))


def test_whole_image_patch_is_bit_equal_to_the_plain_model():
    """P = 1: the same matrix and the same factorisation as sgp_logpdf_grad on the plain model g at the flattened images --
    value, y, mean and noise bit for bit (the term gradients are held to the truth above: their sums run in another order)"""
    case = _case("whole")
    F, fx, y = case.build()
    g = P.logpdf_and_gradient_conv(fx, y)
    plain = P.logpdf_and_gradient(F(P.GPPPInput("g", P.ColVecs(fx.x.x.X)), fx.noise), y)
    assert g["logpdf"] == plain["logpdf"] and g["noise"] == plain["noise"]
    assert np.array_equal(g["y"], plain["y"]) and np.array_equal(g["mean"], plain["mean"])
    assert len(g["terms"]) == len(plain["terms"]) == 1 and g["terms"][0]["row_geom"] == (3, 3, 3, 3)


def test_two_sided_terms_at_the_staging_limit():
    """64 x 48 = 3072 pixels, 8 x 8 patches (D = 64, P = 2337 a side), N = 2, noise 1: grad_coef and grad_inscale against a
    direct float64 evaluation of sum_pq k and sum_pq dk/dg.  Tolerance 2^-53 S P_r P_c, S the absolute sum of the addends:
    any summation order of the P_r P_c N^2 addends meets it -- it catches staging and indexing errors, not rounding."""
    case = _case("staging-1sided")
    F = CT.model(case.kernel, case.patch, case.n_patches)
    rng = np.random.default_rng(77)
    x = P.GPPPInput("f", P.ImageVector(rng.standard_normal(case.image + (2,))))
    spec = P.build_spec(F, x)[0]
    assert spec.n_terms == 1 and spec.term_geoms[0] == ((64, 48, 8, 8),) * 2
    y, m, nz = rng.standard_normal(2), np.zeros(2), np.array([1.0])
    lp, gy, gm, gn, gc, gs = np.zeros(1), np.zeros(2), np.zeros(2), np.zeros(1), np.zeros(1), np.zeros(1)
    ctx = P.lib.default_context()
    rc = ctx.conv_grad.sgp_logpdf_grad_conv(ctx.handle, spec.ref(), d(m), P.lib.NOISE_SCALAR, d(nz), d(y), d(lp), d(gy), d(gm),
                                            d(gn), d(gc), d(gs))
    P.lib.check(rc, "sgp_logpdf_grad_conv")
    pt = np_patches(spec.inputs[0], spec.term_geoms[0][0])        # (P, 2, 64)
    Pn = pt.shape[0]
    sk, sd = np.zeros((2, 2)), np.zeros((2, 2))
    Sk, Sd = np.zeros((2, 2)), np.zeros((2, 2))
    for i in range(2):
        for j in range(2):
            A, B = pt[:, i, :], pt[:, j, :]
            d2 = np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T), 0.0)
            k = np.exp(-0.5 * d2)
            sk[i, j], sd[i, j], Sk[i, j], Sd[i, j] = k.sum(), (-d2 * k).sum(), np.abs(k).sum(), np.abs(d2 * k).sum()
    coef = spec._terms[0].coef
    Cm = coef * sk + np.eye(2)
    alpha = np.linalg.solve(Cm, y)
    G = 0.5 * (np.outer(alpha, alpha) - np.linalg.inv(Cm))
    for name, got, ref, S in (("grad_coef", gc[0], (G * sk).sum(), (np.abs(G) * Sk).sum()),
                              ("grad_inscale", gs[0], coef * (G * sd).sum(), abs(coef) * (np.abs(G) * Sd).sum())):
        tol = 2.0 ** -53 * S * Pn * Pn
        print(f"{name}: device {got:.15e} direct {ref:.15e} |difference| {abs(got - ref):.2e} tolerance {tol:.2e}")
        assert abs(got - ref) <= tol


# ---- the ELBO --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CT.ELBO_CASES, ids=repr)
def test_elbo_gradient_against_truth(case):
    F, fz, fx, y = case.build()
    g = P.elbo_and_gradient_conv(P.VFE(fz), fx, y, inputs=True)
    assert g["_specs"]["xz"].has_patch and g["_specs"]["xx"].has_patch and not g["_specs"]["zz"].has_patch
    assert g["elbo"] == P.elbo(P.VFE(fz), fx, y)                      # bit for bit sgp_elbo's value
    out = CT.elbo_outputs(g)
    flat = [out["value"], out["y"], out["mean"], out["noise"], out["z_noise"], out["var"]]
    for key in ("zz", "xz"):
        flat += [out[key]["d_coef"], out[key]["d_inscale"]] + [a for a in out[key]["gx"] if a is not None]
    for v in flat + [out["xx"]["d_coef"], out["xx"]["d_inscale"]]:
        assert not np.any(np.isnan(v))
    assert g["x"] is None and len(g["z"]) == 1 and g["z"][0].shape == (case.patch[0] * case.patch[1], case.m)
    var_x = P.finite_gp._kernelmatrix_diag(g["_specs"]["xx"])        # what the call under test was given
    R, *R64 = CT.elbo_truth(case, g, fz, fx, y, var_x)
    assert np.max(np.abs(out["var"] - R["var"]) / np.abs(R["var"])) <= 2 * T.EPS      # -1 / (2 sy): one division
    CT.hold(case, CT.elbo_units(out, R), CT.yardstick(CT.elbo_units(CT.elbo_reference_outputs(r), R) for r in R64))
    if case.truth_xx:
        # the var_x chain (sgp_kernelmatrix_diag_grad_conv with w = d elbo / d var_x): no factorisation, so a model bound,
        # depth * eps * S per sum (conv_grad_truth.diag_depth counts the roundings an addend goes through)
        o, r, bound = out["xx"], R["xx"], CT.diag_depth(case, len(y)) * T.EPS
        assert r["diagonal"].all() and len(o["d_coef"]) == len(r["d_coef"]) == 1
        figs = [float(np.max(np.abs(o[k] - r[k]) / (bound * r[s]))) for k, s in (("d_coef", "S_coef"), ("d_inscale", "S_inscale"))]
        print(f"{case.id:20s} diag_grad_conv: error / (depth eps S) = {max(figs):.3f}")
        assert max(figs) <= 1.0, (case.id, figs)


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    F, fx, y = _case("joint").build()
    a, b = P.logpdf_and_gradient_conv(fx, y), P.logpdf_and_gradient_conv(fx, y)
    assert a["logpdf"] == b["logpdf"] and a["noise"] == b["noise"]
    for p, q in zip((a["y"], a["mean"]) + a["_raw"], (b["y"], b["mean"]) + b["_raw"]):
        assert np.array_equal(p, q)
    F, fz, fx, y = _case("elbo-130x7-diag").build()
    a, b = (P.elbo_and_gradient_conv(P.VFE(fz), fx, y, inputs=True) for _ in range(2))
    assert a["elbo"] == b["elbo"] and a["z_noise"] == b["z_noise"]
    for p, q in zip([a["y"], a["mean"], a["noise"], a["var"], a["z"][0]] + [v for k in ("zz", "xz", "xx") for v in a["_raw"][k]],
                    [b["y"], b["mean"], b["noise"], b["var"], b["z"][0]] + [v for k in ("zz", "xz", "xx") for v in b["_raw"][k]]):
        assert np.array_equal(p, q)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _lp_args(n):
    bufs = [np.zeros(n), np.array([0.1]), np.ones(n), np.zeros(1), np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(4), np.zeros(4)]
    return bufs, (d(bufs[0]), P.lib.NOISE_SCALAR) + tuple(d(a) for a in bufs[1:])


def _elbo_args(n, m, nt=4):
    bufs = ([np.ones(n), np.zeros(n), np.array([0.1]), np.array([1e-2]), np.ones(n), np.zeros(1)] +
            [np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(n), np.zeros(1)] + [np.zeros(nt) for _ in range(4)])
    return bufs, ((d(bufs[0]), d(bufs[1]), P.lib.NOISE_SCALAR, d(bufs[2]), P.lib.NOISE_SCALAR, d(bufs[3])) +
                  tuple(d(a) for a in bufs[4:]))


def test_refusals_by_name():
    ctx = P.lib.default_context()
    lib, new = ctx.lib, ctx.conv_grad
    err = P.lib.last_error
    case = _case("lanes-se-f")
    F, fx, y = case.build()
    n, m = 20, 5
    z = P.GPPPInput("g", P.ColVecs(np.asfortranarray(np.random.default_rng(1).standard_normal((9, m)))))
    xx, zz, xz = P.build_spec(F, fx.x)[0], P.build_spec(F, z)[0], P.build_spec(F, fx.x, None, z)[0]
    # an image gradient: the xz input the patched row side reads
    keep, args = _elbo_args(n, m)
    gx = [np.zeros(a.shape, order="F") for a in xz.inputs]
    img = int(xz._terms[0].row_input)
    ptrs = lambda arrs, skip=None: (C.POINTER(C.c_double) * len(arrs))(*[None if k == skip else d(a) for k, a in enumerate(arrs)])  # noqa: E731
    gz = [np.zeros(a.shape, order="F") for a in zz.inputs]
    rc = new.sgp_elbo_grad_conv(ctx.handle, zz.ref(), xz.ref(), *args, ptrs(gz), ptrs(gx))
    assert rc < 0 and "patch" in err() and "images" in err()
    assert new.sgp_elbo_grad_conv(ctx.handle, zz.ref(), xz.ref(), *args, ptrs(gz), ptrs(gx, skip=img)) == 0
    # the old entry points still refuse patch terms
    keep_lp, lp_args = _lp_args(n)
    assert lib.sgp_logpdf_grad(ctx.handle, xx.ref(), *lp_args) < 0 and "patch" in err()
    assert lib.sgp_kernelmatrix_diag_grad(ctx.handle, xx.ref(), d(np.ones(n)), d(np.zeros(4)), d(np.zeros(4))) < 0 and "patch" in err()
    assert lib.sgp_elbo_grad(ctx.handle, zz.ref(), xz.ref(), *args) < 0 and "patch" in err()
    assert ctx.kprod.sgp_logpdf_grad_param(ctx.handle, xx.ref(), *lp_args, d(np.zeros(4))) < 0 and "patch" in err()
    with pytest.raises(NotImplementedError, match="logpdf_and_gradient_conv"):
        P.logpdf_and_gradient(fx, y)
    assert new.sgp_logpdf_grad_conv(ctx.handle, xx.ref(), *lp_args) == 0
    # a stencil term
    Fs = P.gppp(lambda GP: (lambda g: {"g": g, "d": P.stencil(g, [0.0, 0.1], [-1.0, 1.0])})(GP(P.SEKernel())))
    xs = P.GPPPInput("d", P.ColVecs(np.asfortranarray(np.linspace(0.0, 1.0, n)[None, :])))
    st = P.build_spec(Fs, xs)[0]
    assert st.has_stencil
    assert new.sgp_logpdf_grad_conv(ctx.handle, st.ref(), *lp_args) < 0 and "stencil" in err()
    assert new.sgp_kernelmatrix_diag_grad_conv(ctx.handle, st.ref(), d(np.ones(n)), d(np.zeros(4)), d(np.zeros(4))) < 0 and "stencil" in err()
    with pytest.raises(NotImplementedError, match="stencil"):
        P.logpdf_and_gradient_conv(Fs(xs, 0.1), y)
    # a multi-GPU context (it takes no patch geometry: a plain spec is refused all the same)
    plain = P.build_spec(F, P.GPPPInput("g", P.ColVecs(np.asfortranarray(np.random.default_rng(2).standard_normal((9, n))))))[0]
    mctx = P.lib.Context(devices=[0, 0])
    try:
        assert new.sgp_logpdf_grad_conv(mctx.handle, plain.ref(mctx), *lp_args) < 0 and "multi-GPU" in err()
        assert new.sgp_kernelmatrix_diag_grad_conv(mctx.handle, plain.ref(mctx), d(np.ones(n)), d(np.zeros(4)), d(np.zeros(4))) < 0
        assert "multi-GPU" in err()
        prev = P.lib.set_default_context(mctx)
        try:
            with pytest.raises(NotImplementedError, match="multi-GPU"):
                P.logpdf_and_gradient_conv(fx, y)
        finally:
            P.lib.set_default_context(prev)
    finally:
        mctx.close()
    del keep, keep_lp
