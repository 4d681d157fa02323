"""Gradients of logpdf, the diagonal and the ELBO through stencil terms on the device (include/sthenomi_stencil_grad.h;
kernels in stheno.jl_amd/csrc/stencil.hip), through P.logpdf_and_gradient_stencil, P.elbo_and_gradient_stencil and the three
entry points themselves.

The truth is tests/stencil_grad_truth.py: a stencil term expanded into the Q_r Q_c plain terms it is the sum of, run through
tests/grad_truth.py in long double; the bound of a case and output family is MARGIN * max(the same run in float64, the
family's floor) -- from the reference, never from the device.  The shapes are the smallest at which each kernel can go wrong
(stencil_grad_truth.CASES says which): every padded dimension instantiation (D = 1, 3, 5, 9, 16: CC = 4, 4, 2, 1, 1),
stencils of 1, 2, 15 and 64 points with different ones on the two sides, one-sided terms both ways, n = 5 (idle lanes), a
joint model whose block pairs start off the 64-row / 4 CC-column alignment and cross a 128 tile, coincident shifted points
under Matern-1/2, and the ELBO with inducing points in the plain process and in a stencil process."""
import ctypes as C

import numpy as np
import pytest

import conv_grad_truth as CT
import grad_truth as T
import stencil_grad_truth as ST
import stheno_jl_amd as P

pytestmark = pytest.mark.gpu

d = P.lib.dptr


def _ptrs(arrs, skip=()):
    p = (C.POINTER(C.c_double) * max(1, len(arrs)))(*[None if k in skip else d(a) for k, a in enumerate(arrs)])
    p._keep = arrs          # the table does not own the arrays it points into
    return p


def _zeros_like_inputs(spec):
    return [np.zeros(np.asarray(a).shape, order="F") for a in spec.inputs]


def _lp_call(fn, spec, fx, y, *extra):
    """one logpdf gradient entry point on `spec`: (rc, dict of its outputs)"""
    n = len(y)
    kind, nbuf = P.lib._noise_args(fx.noise, n)
    m = np.ascontiguousarray(P.mean(fx), dtype=np.float64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    nt = max(1, spec.n_terms)
    o = dict(lp=np.zeros(1), gy=np.zeros(n), gm=np.zeros(n), gn=np.zeros(n if kind == P.lib.NOISE_DIAG else 1), gc=np.zeros(nt),
             gs=np.zeros(nt))
    ctx = P.lib.default_context()
    rc = fn(ctx.handle, spec.ref(), d(m), kind, d(nbuf), d(yv), d(o["lp"]), d(o["gy"]), d(o["gm"]), d(o["gn"]), d(o["gc"]),
            d(o["gs"]), *extra)
    return rc, o


# ---- logpdf ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ST.LP_CASES, ids=repr)
def test_logpdf_gradient_against_truth(case):
    F, fx, y = case.build()
    g = P.logpdf_and_gradient_stencil(fx, y, inputs=True)
    assert g["_spec"].has_stencil
    out = ST.logpdf_outputs(g)
    for v in [out[k] for k in ("value", "y", "mean", "noise", "d_coef", "d_inscale")] + out["gx"]:
        assert np.all(np.isfinite(v))
    R, *R64 = ST.logpdf_truth(case, g["_spec"], fx, y)
    ST.hold(case, ST.logpdf_units(out, R), ST.yardstick(ST.logpdf_units(ST.logpdf_reference_outputs(r), R) for r in R64))
    # without the inputs: the same bits on everything else
    h = P.logpdf_and_gradient_stencil(fx, y)
    assert h["inputs"] is None and h["logpdf"] == g["logpdf"]
    assert all(np.array_equal(p, q) for p, q in zip(h["_raw"], g["_raw"]))


def test_the_registration_limits_are_accepted():
    case = ST.case("d16-se-64x2")
    (Ag, wg), _ = case.stencils()
    assert Ag.shape == (P.lib.STENCIL_MAX_DIM, P.lib.STENCIL_MAX_POINTS) == (16, 64) and sum(n for _, n in case.blocks) == 6


def test_coincident_shifted_points_have_the_subgradient_zero():
    """Matern-1/2 on a dyadic grid with dyadic offsets: shifted pairs coincide exactly; every gradient is finite (the truth
    case above holds them to the bound)"""
    case = ST.case("coincident-m12")
    F, fx, y = case.build()
    spec = P.build_spec(F, fx.x)[0]
    S = ST.read_spec(spec)
    Sx, *_ = ST.expand(S)
    hits = sum(int((T.sqdist(Sx["inputs"][a], Sx["inputs"][b]) == 0).sum()) for (_, _, _, a, b, *_) in Sx["terms"] if a != b)
    assert hits >= 50
    g = P.logpdf_and_gradient_stencil(fx, y, inputs=True)
    assert all(np.all(np.isfinite(a)) for a in g["inputs"]) and np.all(np.isfinite(g["_raw"][0])) and np.all(np.isfinite(g["_raw"][1]))


@pytest.mark.parametrize("kernel", sorted(ST.BASE))
def test_unit_stencil_against_the_plain_model(kernel):
    """one point, zero offset, unit weight: the same matrix and the same factorisation as sgp_logpdf_grad_x on the plain
    model -- logpdf_out, grad_y, grad_mean and grad_noise bit for bit; grad_coef, grad_inscale and grad_inputs run their sums
    in another order and agree within the sum of the two truth bounds (each held to one truth, the plain model's)"""
    D, n = 3, 150
    rng = np.random.default_rng(11)
    F = ST.model(kernel, D, ST.unit_stencil(D), ST.fd_stencil(D))
    X = P.ColVecs(np.asfortranarray(rng.standard_normal((D, n))))
    y = rng.standard_normal(n)
    fg, ff = F(P.GPPPInput("g", X), 0.2), F(P.GPPPInput("f", X), 0.2)
    a, b = P.logpdf_and_gradient_stencil(fg, y, inputs=True), P.logpdf_and_gradient(ff, y, inputs=True)
    assert a["_spec"].has_stencil and not b["_spec"].has_stencil
    assert a["logpdf"] == b["logpdf"] and a["noise"] == b["noise"]
    assert np.array_equal(a["y"], b["y"]) and np.array_equal(a["mean"], b["mean"])
    R = T.logpdf_grad(T.read_spec(b["_spec"]), T.NOISE_SCALAR, 0.2, P.mean(ff), y, T.require_extended(), inputs=True)
    R64 = T.logpdf_grad(T.read_spec(b["_spec"]), T.NOISE_SCALAR, 0.2, P.mean(ff), y, np.float64, inputs=True)
    for fam, plain_fam, key, scale in (
            ("st.lp.d_coef", "lp.d_coef", "d_coef", T.scale_scalar(R["d_coef"], R["S_coef"], R["n_rows"])),
            ("st.lp.d_inscale", "lp.d_inscale", "d_inscale", T.scale_scalar(R["d_inscale"], R["S_inscale"], R["n_rows"])),
            ("st.lp.inputs", "lp.inputs", "gx", T.scale_entries(R["gx"][0], R["Sn_gx"][0]))):
        ref = R[key][0] if key == "gx" else R[key]
        pick = (lambda r: r["inputs"][0]) if key == "gx" else (lambda r, k=(0 if key == "d_coef" else 1): r["_raw"][k][:1])
        e64 = T.units(R64[key][0] if key == "gx" else R64[key], ref, scale)
        bound = T.MARGIN * max(e64, ST.FLOORS[fam]) + T.MARGIN * max(e64, T.FLOORS[plain_fam])
        apart = T.units(pick(a), np.asarray(pick(b), dtype=ref.dtype), scale)
        print(f"{kernel} {key}: stencil and plain route {apart:.1f} units apart, the two bounds add up to {bound:.1f}")
        assert apart <= bound


def test_specs_without_stencil_terms_are_bit_equal_to_the_conv_entry_point():
    """a plain spec and a patch spec of conv_grad_truth: the outputs shared with sgp_logpdf_grad_conv, bit for bit"""
    ctx = P.lib.default_context()
    cases = [next(c for c in CT.CASES if c.id == "joint"), next(c for c in CT.CASES if c.id == "lanes-se-fh")]
    specs = []
    for c in cases:
        F, fx, y = c.build()
        specs.append((P.build_spec(F, fx.x)[0], fx, y))
    rng = np.random.default_rng(3)
    Fp = P.gppp(lambda GP: {"f": GP(1.3 * P.with_lengthscale(P.Matern52Kernel(), 0.8)) + GP(0.4 * P.SEKernel())})
    fxp = Fp(P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((3, 150))))), 0.2)
    specs.append((P.build_spec(Fp, fxp.x)[0], fxp, rng.standard_normal(150)))
    assert [s.has_patch for s, _, _ in specs] == [True, True, False] and not any(s.has_stencil for s, _, _ in specs)
    for spec, fx, y in specs:
        rc, a = _lp_call(ctx.conv_grad.sgp_logpdf_grad_conv, spec, fx, y)
        assert rc == 0
        for gin in (None, _ptrs(_zeros_like_inputs(spec), skip=P.finite_gp._patched_inputs(spec))):
            rc, b = _lp_call(ctx.stencil_grad.sgp_logpdf_grad_stencil, spec, fx, y, gin)
            assert rc == 0, P.lib.last_error()
            for k in a:
                assert np.array_equal(a[k], b[k]), k


def test_plain_points_of_a_patch_spec_get_their_logpdf_gradient():
    """sgp_logpdf_grad_stencil on a spec with patch terms: the 7 plain points of conv_grad_truth's joint case (the plain
    side of both one-sided orientations and of the plain pair) against the expanded long-double truth, held as grad_truth
    holds the input gradients of a logpdf: MARGIN * max(the float64 run, the floor of lp.inputs)"""
    c = next(c for c in CT.CASES if c.id == "joint")
    F, fx, y = c.build()
    g = P.logpdf_and_gradient_stencil(fx, y, inputs=True)
    spec = g["_spec"]
    img = P.finite_gp._patched_inputs(spec)
    assert spec.has_patch and img and [a is None for a in g["inputs"]] == [k in img for k in range(len(spec.inputs))]
    S = CT.read_spec(spec)
    Sx, owner, in_map = CT.expand(S)
    runs = [T.logpdf_grad(Sx, T.NOISE_SCALAR, fx.noise, P.mean(fx), y, dt, inputs=True) for dt in (T.require_extended(), np.float64)]
    (gx, Sn), (gx64, _) = (CT.fold_inputs(R, in_map, len(S["inputs"])) for R in runs)
    seen = 0
    for k, a in enumerate(g["inputs"]):
        if a is None:
            continue
        scale = T.scale_entries(gx[k], Sn[k])
        dev, e64 = T.units(a, gx[k], scale), T.units(gx64[k], gx[k], scale)
        print(f"input {k}: device {dev:.1f} units, float64 {e64:.1f}, floor {T.FLOORS['lp.inputs']:.1f}")
        assert dev <= T.MARGIN * max(e64, T.FLOORS["lp.inputs"])
        seen += a.shape[1]
    assert seen == 7 and np.max(np.abs(g["x"][1])) > 0 and not np.any(g["x"][0])     # the images' block: zeros


# ---- the ELBO --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ST.ELBO_CASES, ids=repr)
def test_elbo_gradient_against_truth(case):
    F, fz, fx, y = case.build()
    g = P.elbo_and_gradient_stencil(P.VFE(fz), fx, y, inputs=True)
    assert g["_specs"]["xz"].has_stencil and g["_specs"]["xx"].has_stencil
    assert g["_specs"]["zz"].has_stencil == (case.z[0] != "f")
    assert g["elbo"] == P.elbo(P.VFE(fz), fx, y)                      # bit for bit sgp_elbo's value
    # the diagonal's own input gradient, as the host function asks for it
    xx = g["_specs"]["xx"]
    gdx = _zeros_like_inputs(xx)
    gcd, gsd = np.zeros(max(1, xx.n_terms)), np.zeros(max(1, xx.n_terms))
    ctx = P.lib.default_context()
    w = np.ascontiguousarray(g["var"])
    assert ctx.stencil_grad.sgp_kernelmatrix_diag_grad_stencil(ctx.handle, xx.ref(), d(w), d(gcd), d(gsd), _ptrs(gdx)) == 0
    assert np.array_equal(gcd, g["_raw"]["xx"][0]) and np.array_equal(gsd, g["_raw"]["xx"][1])
    out = ST.elbo_outputs(g, gdx)
    flat = [out["value"], out["y"], out["mean"], out["noise"], out["z_noise"], out["var"]]
    for key in ("zz", "xz", "xx"):
        flat += [out[key]["d_coef"], out[key]["d_inscale"]] + list(out[key]["gx"])
    for v in flat:
        assert np.all(np.isfinite(v))
    assert len(g["x"]) == 1 and g["x"][0].shape == (case.D, 150) and len(g["z"]) == 1 and g["z"][0].shape == (case.D, 20)
    var_x = P.finite_gp._kernelmatrix_diag(xx)        # what the call under test was given
    R, *R64 = ST.elbo_truth(case, g["_specs"], fz, fx, y, var_x)
    assert np.max(np.abs(out["var"] - R["var"]) / np.abs(R["var"])) <= 2 * T.EPS      # -1 / (2 sy): one division
    ST.hold(case, ST.elbo_units(out, R), ST.yardstick(ST.elbo_units(ST.elbo_reference_outputs(r), R) for r in R64))
    # the var_x chain (sgp_kernelmatrix_diag_grad_stencil with w = d elbo / d var_x): no factorisation, so a model bound,
    # depth * eps * S per sum (stencil_grad_truth.diag_depth counts the roundings an addend goes through); both sides of
    # every term read one input here: the input gradient is an exact zero where the truth cancels to rounding
    o, r, bound = out["xx"], R["xx"], ST.diag_depth(case, len(y)) * T.EPS
    assert r["diagonal"].all() and len(o["d_coef"]) == len(r["d_coef"]) == 1
    figs = [float(np.max(np.abs(o[k] - r[k]) / (bound * r[s]))) for k, s in (("d_coef", "S_coef"), ("d_inscale", "S_inscale"))]
    figs += [float(np.max(np.abs(a - e) / (bound * np.maximum(s, np.finfo(np.float64).tiny))))
             for a, e, s in zip(o["gx"], r["gx"], r["S_gx"])]
    print(f"{case.id:22s} diag_grad_stencil: error / (depth eps S) = {max(figs):.3f}")
    assert max(figs) <= 1.0, (case.id, figs)


def test_diagonal_input_gradient_with_two_views_of_one_input():
    """var(g)(x) depends on x where a diagonal term reads two different views of x: cov(g, h) of a cross spec at the same
    points, row side a stretched stencil process -- + on the row input, - on the column input, against the expanded truth
    within depth * eps * S"""
    D, n = 3, 70
    rng = np.random.default_rng(5)

    def build(GP):
        f = GP(1.1 * ST.kernel_of("m52", D))
        return {"f": f, "g": P.stencil(P.stretch(f, 0.8), *ST.quad_stencil(D, 5)), "h": P.stencil(f, *ST.fd_stencil(D))}
    F = P.gppp(build)
    X = P.ColVecs(np.asfortranarray(rng.standard_normal((D, n))))
    spec = P.build_spec(F, P.GPPPInput("g", X), None, P.GPPPInput("h", X))[0]
    assert spec.n_terms == 1 and spec.has_stencil and spec._terms[0].row_input != spec._terms[0].col_input
    w = rng.standard_normal(n)
    gc, gs, gx = np.zeros(1), np.zeros(1), _zeros_like_inputs(spec)
    ctx = P.lib.default_context()
    assert ctx.stencil_grad.sgp_kernelmatrix_diag_grad_stencil(ctx.handle, spec.ref(), d(w), d(gc), d(gs), _ptrs(gx)) == 0
    S = ST.read_spec(spec)
    Sx, owner, weight, in_map = ST.expand(S)
    Rd = T.diag_grad(Sx, w, T.require_extended())
    r = ST.fold_terms(Rd, owner, weight, 1)
    tx, Sg = ST.fold_inputs(Rd, in_map, len(S["inputs"]), S_key="S_gx")
    bound = (3 * D + 8 + 2 + 5 * 2 + 2 + 1 + 8) * T.EPS
    figs = [abs(gc[0] - r["d_coef"][0]) / (bound * r["S_coef"][0]), abs(gs[0] - r["d_inscale"][0]) / (bound * r["S_inscale"][0])]
    figs += [float(np.max(np.abs(a - e) / (bound * s))) for a, e, s in zip(gx, tx, Sg)]
    print("diagonal with two views: error / (depth eps S) =", [f"{float(v):.3f}" for v in figs])
    assert max(figs) <= 1.0 and np.max(np.abs(gx[0])) > 0 and np.max(np.abs(gx[1])) > 0


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    F, fx, y = ST.case("joint-37-150").build()
    a, b = (P.logpdf_and_gradient_stencil(fx, y, inputs=True) for _ in range(2))
    assert a["logpdf"] == b["logpdf"] and a["noise"] == b["noise"]
    for p, q in zip((a["y"], a["mean"]) + a["_raw"] + tuple(a["inputs"]), (b["y"], b["mean"]) + b["_raw"] + tuple(b["inputs"])):
        assert np.array_equal(p, q)
    F, fz, fx, y = ST.case("elbo-150x20g-diag").build()
    a, b = (P.elbo_and_gradient_stencil(P.VFE(fz), fx, y, inputs=True) for _ in range(2))
    assert a["elbo"] == b["elbo"] and a["z_noise"] == b["z_noise"]
    outs = lambda g: ([g["y"], g["mean"], g["noise"], g["var"], g["z"][0], g["x"][0]] + g["zz_inputs"] + g["xz_inputs"] +    # noqa: E731
                      [v for k in ("zz", "xz", "xx") for v in g["_raw"][k]])
    for p, q in zip(outs(a), outs(b)):
        assert np.array_equal(p, q)


# ---- the composed route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["se", "m52"])
def test_matches_the_composed_sum_of_shifts(kernel):
    """the model of test_gpu_stencil.test_matches_the_composed_sum_of_shifts: the host gradients (variance, lengthscale,
    noise, x) of the stencil route and of logpdf_and_gradient(inputs=True) on the composed sum of shift views, each held to
    the long-double truth of the stencil model by its own family's bound -- so the two are within the sum of their bounds"""
    rng = np.random.default_rng(7)
    A, w = rng.standard_normal((2, 6)), rng.standard_normal(6)
    v0, l0 = 1.3, 0.9

    def build(GP):
        f = GP(v0 * P.with_lengthscale(ST.BASE[kernel](), l0))
        fs = w[0] * P.shift(f, A[:, 0])
        for q in range(1, 6):
            fs = fs + w[q] * P.shift(f, A[:, q])
        return {"f": f, "g": P.stencil(f, A, w), "fs": fs}
    F = P.gppp(build)
    n = 200
    X = P.ColVecs(np.asfortranarray(rng.standard_normal((2, n))))
    y = rng.standard_normal(n)
    fg, fs = F(P.GPPPInput("g", X), 0.3), F(P.GPPPInput("fs", X), 0.3)
    a, b = P.logpdf_and_gradient_stencil(fg, y, inputs=True), P.logpdf_and_gradient(fs, y, inputs=True)
    assert len(a["terms"]) == 1 and len(b["terms"]) == 36
    R = ST.logpdf_truth(_Named(f"composed-{kernel}"), a["_spec"], fg, y)[0]
    R64s = ST.logpdf_truth(_Named(f"composed-{kernel}"), a["_spec"], fg, y)[1:]
    e64 = ST.yardstick(ST.logpdf_units(ST.logpdf_reference_outputs(r), R) for r in R64s)
    host = lambda g: dict(v=sum(r["d_coef"] * r["coef"] for r in g["terms"]) / v0,        # noqa: E731
                          l=-sum(r["d_inscale"] for r in g["terms"]) / l0, noise=g["noise"], x=g["x"][0])
    ha, hb = host(a), host(b)
    # the truth's host gradients and their scales, formed as `host` forms them
    coef = a["terms"][0]["coef"]
    ref = dict(v=R["d_coef"][0] * coef / v0, l=-R["d_inscale"][0] / l0, noise=R["noise"], x=R["gx"][0] / l0)
    scale = dict(v=T.scale_scalar(R["d_coef"], R["S_coef"], R["n_rows"])[0] * abs(coef) / v0,
                 l=T.scale_scalar(R["d_inscale"], R["S_inscale"], R["n_rows"])[0] / l0,
                 noise=T.scale_scalar(R["noise"], R["S_noise"], R["n"]), x=T.scale_entries(R["gx"][0], R["Sn_gx"][0]) / l0)
    fams = dict(v=("st.lp.d_coef", "lp.d_coef"), l=("st.lp.d_inscale", "lp.d_inscale"), noise=("lp.noise", "lp.noise"),
                x=("st.lp.inputs", "lp.inputs"))
    for key in ("v", "l", "noise", "x"):
        fa, fb = fams[key]
        bound = ST.bound_of(fa, e64) + T.MARGIN * max(e64[fa], T.FLOORS[fb])
        apart = T.units(ha[key], np.asarray(hb[key], dtype=np.longdouble), scale[key])
        off_a, off_b = T.units(ha[key], ref[key], scale[key]), T.units(hb[key], ref[key], scale[key])
        print(f"{kernel} d/d{key}: the routes are {apart:.1f} units apart (stencil {off_a:.1f}, composed {off_b:.1f} from the "
              f"truth); the two bounds add up to {bound:.1f}")
        assert apart <= bound


class _Named:
    """a case of its own for stencil_grad_truth.logpdf_truth's cache: scalar noise"""
    noise = "scalar"

    def __init__(self, id):
        self.id = id


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    ctx = P.lib.default_context()
    lib, new = ctx.lib, ctx.stencil_grad
    err = P.lib.last_error
    F, fx, y = ST.case("n5").build()
    n = len(y)
    xx = P.build_spec(F, fx.x)[0]
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(np.random.default_rng(1).standard_normal((2, 3)))))
    zz, xz = P.build_spec(F, z)[0], P.build_spec(F, fx.x, None, z)[0]
    assert xx.has_stencil and xz.has_stencil and not zz.has_stencil
    nt = 4
    e_bufs = ([np.ones(n), np.zeros(n), np.array([0.1]), np.array([1e-2]), np.ones(n), np.zeros(1)] +
              [np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(n), np.zeros(1)] + [np.zeros(nt) for _ in range(4)])
    e_args = ((d(e_bufs[0]), d(e_bufs[1]), P.lib.NOISE_SCALAR, d(e_bufs[2]), P.lib.NOISE_SCALAR, d(e_bufs[3])) +
              tuple(d(a) for a in e_bufs[4:]))
    # every other gradient entry point keeps refusing stencil terms
    assert _lp_call(lib.sgp_logpdf_grad, xx, fx, y)[0] < 0 and "stencil" in err()
    assert _lp_call(ctx.conv_grad.sgp_logpdf_grad_conv, xx, fx, y)[0] < 0 and "stencil" in err()
    assert _lp_call(ctx.kprod.sgp_logpdf_grad_param, xx, fx, y, d(np.zeros(nt)))[0] < 0 and "stencil" in err()
    assert lib.sgp_kernelmatrix_diag_grad(ctx.handle, xx.ref(), d(np.ones(n)), d(np.zeros(nt)), d(np.zeros(nt))) < 0 and "stencil" in err()
    assert lib.sgp_elbo_grad(ctx.handle, zz.ref(), xz.ref(), *e_args) < 0 and "stencil" in err()
    assert ctx.conv_grad.sgp_elbo_grad_conv(ctx.handle, zz.ref(), xz.ref(), *e_args, None, None) < 0 and "stencil" in err()
    for call in (lambda: P.logpdf_and_gradient(fx, y), lambda: P.logpdf_and_gradient_conv(fx, y),
                 lambda: P.elbo_and_gradient(P.VFE(F(z, 1e-2)), fx, y)):
        with pytest.raises(NotImplementedError, match="stencil.*logpdf_and_gradient_stencil"):
            call()
    # the new ones take them, with and without the inputs
    assert _lp_call(new.sgp_logpdf_grad_stencil, xx, fx, y, None)[0] == 0
    assert new.sgp_elbo_grad_stencil(ctx.handle, zz.ref(), xz.ref(), *e_args, None, None) == 0
    assert new.sgp_elbo_grad_stencil(ctx.handle, zz.ref(), xz.ref(), *e_args, _ptrs(_zeros_like_inputs(zz)),
                                     _ptrs(_zeros_like_inputs(xz), skip={0})) == 0
    # product chains in the ELBO, as sgp_elbo_grad
    Fk = P.gppp(lambda GP: {"p": GP(P.SEKernel() * P.Matern32Kernel())})
    xp = P.GPPPInput("p", P.ColVecs(np.asfortranarray(np.random.default_rng(2).standard_normal((2, n)))))
    zp = P.GPPPInput("p", z.x)
    kz, kx = P.build_spec(Fk, zp)[0], P.build_spec(Fk, xp, None, zp)[0]
    assert kz.has_kprod
    assert new.sgp_elbo_grad_stencil(ctx.handle, kz.ref(), kx.ref(), *e_args, None, None) < 0 and "product chains" in err()
    # ... while the logpdf gradient carries them, inputs included
    kxx = P.build_spec(Fk, xp)[0]
    assert _lp_call(new.sgp_logpdf_grad_stencil, kxx, Fk(xp, 0.1), y, _ptrs(_zeros_like_inputs(kxx)))[0] == 0, err()
    # a non-NULL grad_inputs entry for an input that holds images
    c = next(c for c in CT.CASES if c.id == "lanes-se-f")
    Fc, fxc, yc = c.build()
    pspec = P.build_spec(Fc, fxc.x)[0]
    img = sorted(P.finite_gp._patched_inputs(pspec))
    assert img
    rc, _ = _lp_call(new.sgp_logpdf_grad_stencil, pspec, fxc, yc, _ptrs(_zeros_like_inputs(pspec)))
    assert rc < 0 and "images" in err()
    assert new.sgp_kernelmatrix_diag_grad_stencil(ctx.handle, pspec.ref(), d(np.ones(len(yc))), d(np.zeros(nt)), d(np.zeros(nt)),
                                                  _ptrs(_zeros_like_inputs(pspec))) < 0 and "images" in err()
    assert _lp_call(new.sgp_logpdf_grad_stencil, pspec, fxc, yc, _ptrs(_zeros_like_inputs(pspec), skip=img))[0] == 0
    # ... and the plain side of a one-sided patch term on the diagonal (a cross spec of as many points as images): not formed
    zc = P.GPPPInput("g", P.ColVecs(np.asfortranarray(np.random.default_rng(4).standard_normal((9, len(yc))))))
    cross = P.build_spec(Fc, fxc.x, None, zc)[0]
    cimg = sorted(P.finite_gp._patched_inputs(cross))
    assert len(cimg) == 1 and len(cross.inputs) == 2
    dargs = (d(np.ones(len(yc))), d(np.zeros(nt)), d(np.zeros(nt)))
    assert new.sgp_kernelmatrix_diag_grad_stencil(ctx.handle, cross.ref(), *dargs, _ptrs(_zeros_like_inputs(cross), skip=cimg)) < 0
    assert "one-sided patch" in err()
    assert new.sgp_kernelmatrix_diag_grad_stencil(ctx.handle, cross.ref(), *dargs, None) == 0
    # a multi-GPU context (it takes no stencil: a plain spec is refused all the same)
    plain = P.build_spec(F, P.GPPPInput("f", fx.x.x))[0]
    mctx = P.lib.Context(devices=[0, 0])
    try:
        m, nz, yv = np.zeros(n), np.array([0.1]), np.ones(n)
        bufs = [np.zeros(1), np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(nt), np.zeros(nt)]
        rc = new.sgp_logpdf_grad_stencil(mctx.handle, plain.ref(mctx), d(m), P.lib.NOISE_SCALAR, d(nz), d(yv),
                                         *[d(a) for a in bufs], None)
        assert rc < 0 and "multi-GPU" in err()
        assert new.sgp_kernelmatrix_diag_grad_stencil(mctx.handle, plain.ref(mctx), d(np.ones(n)), d(np.zeros(nt)),
                                                      d(np.zeros(nt)), None) < 0 and "multi-GPU" in err()
        zp = P.build_spec(F, z)[0]
        xzp = P.build_spec(F, P.GPPPInput("f", fx.x.x), None, z)[0]
        assert new.sgp_elbo_grad_stencil(mctx.handle, zp.ref(mctx), xzp.ref(mctx), *e_args, None, None) < 0 and "multi-GPU" in err()
        prev = P.lib.set_default_context(mctx)
        try:
            with pytest.raises(NotImplementedError, match="multi-GPU"):
                P.logpdf_and_gradient_stencil(F(P.GPPPInput("f", fx.x.x), 0.1), y)
        finally:
            P.lib.set_default_context(prev)
    finally:
        mctx.close()
    del e_bufs
