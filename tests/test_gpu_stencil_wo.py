"""Gradients with respect to a stencil's own weights and offsets on the device (include/sthenomi_stencil_wo.h; kernels in
stheno.jl_amd/csrc/stencil.hip), through P.logpdf_and_gradient_stencil / P.elbo_and_gradient_stencil with stencils=True and
the three entry points themselves.

The truth is tests/stencil_wo_truth.py: the header's four sums contracted directly in long double against the cotangent of
tests/grad_truth.py on the expanded spec; the bound of a case and family is MARGIN * max(the same code in float64, the
family's floor) -- from the reference, never from the device.  The shapes are stencil_grad_truth.CASES unchanged (every
padded dimension, 1 / 2 / 15 / 64 points with different stencils on the two sides, one-sided terms both ways, n = 5, block
pairs off the alignment, coincident Matern-1/2 points, the four ELBO layouts) plus stencil_wo_truth.EXTRA: a pair over two
128-column strips and three 64-row groups, ragged on both, and 64 points against 1 in both orders."""
import numpy as np
import pytest

import conv_grad_truth as CT
import grad_truth as T
import stencil_grad_truth as ST
import stencil_wo_truth as WT
import stheno_jl_amd as P
from test_gpu_stencil_grad import _lp_call, _ptrs

pytestmark = pytest.mark.gpu

d = P.lib.dptr
_tables = P.finite_gp._stencil_tables


def _full_tables(spec):
    """tables with an entry for EVERY side, plain ones included (2 pointers per term): what the refusals are asked with"""
    nt = spec.n_terms
    dims = [np.asarray(spec.inputs[int(spec._terms[t].row_input)]).shape[0] for t in range(nt)]
    gw = [np.zeros(64) for _ in range(2 * nt)]
    go = [np.zeros(64 * dims[k // 2]) for k in range(2 * nt)]
    return _ptrs(gw), _ptrs(go)


def _flat(tables):
    return [a for row in tables for a in row if a is not None]


def _same_tables(a, b):
    return all(np.array_equal(p, q) for ta, tb in zip(a, b) for p, q in zip(_flat(ta), _flat(tb)))


# ---- logpdf ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WT.LP_CASES, ids=repr)
def test_logpdf_tables_against_truth(case):
    F, fx, y = case.build()
    g = P.logpdf_and_gradient_stencil(fx, y, inputs=True, stencils=True)
    spec = g["_spec"]
    assert spec.has_stencil
    gw, go = WT.host_tables(g["_raw_stencils"])
    assert all(np.all(np.isfinite(a)) for a in _flat(gw) + _flat(go))
    R, *R64 = WT.logpdf_runs(case, spec, fx, y)
    (uw, uo), (ew, eo) = WT.units(gw, go, R), WT.yardstick(R, R64)
    WT.hold(case, "wo.lp.weights", uw, ew)
    WT.hold(case, "wo.lp.offsets", uo, eo)
    # every output shared with sgp_logpdf_grad_stencil: the same bits
    h = P.logpdf_and_gradient_stencil(fx, y, inputs=True)
    assert h["logpdf"] == g["logpdf"] and np.array_equal(h["noise"], g["noise"])
    for p, q in zip((h["y"], h["mean"]) + h["_raw"] + tuple(h["inputs"]), (g["y"], g["mean"]) + g["_raw"] + tuple(g["inputs"])):
        assert np.array_equal(p, q)
    # sum_p w_p grad_weights_row[p] = coef grad_coef[t] = sum_q v_q grad_weights_col[q], within the two families' bounds
    Rs, *Rs64 = ST.logpdf_truth(case, spec, fx, y)
    ec = ST.yardstick(ST.logpdf_units(ST.logpdf_reference_outputs(r), Rs) for r in Rs64)["st.lp.d_coef"]
    Bw, Bc = WT.bound_of("wo.lp.weights", ew), ST.bound_of("st.lp.d_coef", {"st.lp.d_coef": ec})
    sc = T.scale_scalar(Rs["d_coef"], Rs["S_coef"], Rs["n_rows"])
    worst = 0.0
    for t, term in enumerate(R):
        coef = float(spec._terms[t].coef)
        for side in (0, 1):
            if term is None or term["sides"][side] is None:
                continue
            w = spec.term_stencils[t][side][1]
            lhs, rhs = float(w @ gw[t][side]), coef * float(g["_raw"][0][t])
            tol = T.EPS * (Bw * float(np.abs(w) @ WT.scales(term, side)[0]) + Bc * abs(coef) * float(sc[t]))
            worst = max(worst, abs(lhs - rhs) / tol)
    print(f"{case.id:22s} sum w dw = coef d_coef: {worst:.3f} of the two bounds")
    assert worst <= 1.0


def test_null_tables_and_null_entries_give_the_same_bits():
    """sgp_logpdf_grad_stencil_wo with both tables NULL, with one of them, and with single entries NULL: the shared outputs
    bit for bit sgp_logpdf_grad_stencil's, the tables that are given bit for bit the full call's"""
    case = WT.EXTRA[0]
    F, fx, y = case.build()
    ctx = P.lib.default_context()
    spec = P.build_spec(F, fx.x)[0]
    rc, ref = _lp_call(ctx.stencil_grad.sgp_logpdf_grad_stencil, spec, fx, y, None)
    assert rc == 0
    gw, go, pw, po = _tables(spec)
    rc, full = _lp_call(ctx.stencil_wo.sgp_logpdf_grad_stencil_wo, spec, fx, y, None, pw, po)
    assert rc == 0, P.lib.last_error()
    gw2, go2, pw2, po2 = _tables(spec)
    go3, po3 = _tables(spec)[1::2]
    po3[0] = None                                    # one entry not asked for
    for extra, given in (((None, None), ()), ((pw2, None), (gw2,)), ((None, po3), (go3,))):
        rc, o = _lp_call(ctx.stencil_wo.sgp_logpdf_grad_stencil_wo, spec, fx, y, None, *extra)
        assert rc == 0, P.lib.last_error()
        for k in ref:
            assert np.array_equal(ref[k], o[k]) and np.array_equal(ref[k], full[k]), k
    assert _same_tables((gw,), (gw2,)) and np.any(gw2[0][0])
    assert not np.any(go3[0][0]) and np.any(go[0][0])            # the skipped entry stays untouched
    assert all(np.array_equal(p, q) for p, q in zip(_flat(go)[1:], _flat(go3)[1:]))


# ---- the diagonal ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WT.WO_CASES, ids=repr)
def test_diagonal_tables_against_truth(case):
    built = case.build()
    F, fx = built[0], built[-2]
    spec = P.build_spec(F, fx.x)[0]
    w = np.ascontiguousarray(WT.diag_weights(case, spec.N))
    nt = max(1, spec.n_terms)
    ctx = P.lib.default_context()
    gc0, gs0 = np.zeros(nt), np.zeros(nt)
    assert ctx.stencil_grad.sgp_kernelmatrix_diag_grad_stencil(ctx.handle, spec.ref(), d(w), d(gc0), d(gs0), None) == 0
    gc, gs = np.zeros(nt), np.zeros(nt)
    gw, go, pw, po = _tables(spec)
    rc = ctx.stencil_wo.sgp_kernelmatrix_diag_grad_stencil_wo(ctx.handle, spec.ref(), d(w), d(gc), d(gs), None, pw, po)
    assert rc == 0, P.lib.last_error()
    assert np.array_equal(gc, gc0) and np.array_equal(gs, gs0)
    gc1, gs1 = np.zeros(nt), np.zeros(nt)
    assert ctx.stencil_wo.sgp_kernelmatrix_diag_grad_stencil_wo(ctx.handle, spec.ref(), d(w), d(gc1), d(gs1), None, None, None) == 0
    assert np.array_equal(gc1, gc0) and np.array_equal(gs1, gs0)
    R, R64 = WT.diag_runs(case, spec, w)
    (uw, uo), (ew, eo) = WT.units(*WT.host_tables((gw, go)), R), WT.yardstick(R, [R64])
    WT.hold(case, "wo.diag.weights", uw, ew)
    WT.hold(case, "wo.diag.offsets", uo, eo)


# ---- the ELBO --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WT.ELBO_CASES, ids=repr)
def test_elbo_tables_against_truth(case):
    F, fz, fx, y = case.build()
    g = P.elbo_and_gradient_stencil(P.VFE(fz), fx, y, inputs=True, stencils=True)
    specs, raw = g["_specs"], g["_raw_stencils"]
    assert all(np.all(np.isfinite(a)) for k in ("zz", "xz", "xx") for tb in raw[k] for a in _flat(tb))
    var_x = P.finite_gp._kernelmatrix_diag(specs["xx"])
    R, *R64 = WT.elbo_runs(case, specs, fz, fx, y, var_x)
    fig = {k: (WT.units(*WT.host_tables(raw[k]), R[k]), WT.yardstick(R[k], [r[k] for r in R64])) for k in ("zz", "xz")}
    ew, eo = max(fig[k][1][0] for k in fig), max(fig[k][1][1] for k in fig)
    WT.hold(case, "wo.elbo.weights", max(fig[k][0][0] for k in fig), ew)
    WT.hold(case, "wo.elbo.offsets", max(fig[k][0][1] for k in fig), eo)
    # every output shared with sgp_elbo_grad_stencil / sgp_kernelmatrix_diag_grad_stencil: the same bits
    h = P.elbo_and_gradient_stencil(P.VFE(fz), fx, y, inputs=True)
    assert h["elbo"] == g["elbo"] and np.array_equal(h["z_noise"], g["z_noise"]) and np.array_equal(h["noise"], g["noise"])
    outs = lambda r: ([r["y"], r["mean"], r["var"], r["z"][0], r["x"][0]] + r["zz_inputs"] + r["xz_inputs"] +    # noqa: E731
                      [v for k in ("zz", "xz", "xx") for v in r["_raw"][k]])
    for p, q in zip(outs(h), outs(g)):
        assert np.array_equal(p, q)
    # a one-term cross spec with different inputs: sum_p grad_offsets_row[:, p] = -sum_i grad_inputs[row][:, i], and the
    # columns with the opposite sign, within the bounds of the two families
    xz = specs["xz"]
    assert xz.n_terms == 1 and xz._terms[0].row_input != xz._terms[0].col_input
    Rs, *Rs64 = ST.elbo_truth(case, specs, fz, fx, y, var_x)
    ei = ST.yardstick(ST.elbo_units(ST.elbo_reference_outputs(r), Rs) for r in Rs64)["st.elbo.inputs"]
    Bo, Bi = WT.bound_of("wo.elbo.offsets", eo), ST.bound_of("st.elbo.inputs", {"st.elbo.inputs": ei})
    go = WT.host_tables(raw["xz"])[1]
    for side, k in ((0, int(xz._terms[0].row_input)), (1, int(xz._terms[0].col_input))):
        if go[0][side] is None:
            continue
        so = WT.scales(R["xz"][0], side)[1]
        si = np.broadcast_to(T.scale_entries(Rs["xz"]["gx"][k], Rs["xz"]["Sn_gx"][k]), Rs["xz"]["gx"][k].shape)
        tol = T.EPS * (Bo * so.sum(axis=1) + Bi * si.sum(axis=1))
        off = np.abs(go[0][side].sum(axis=1) + g["xz_inputs"][k].sum(axis=1)) / np.asarray(tol, dtype=np.float64)
        print(f"{case.id:22s} side {side}: sum_p d offsets = -sum_i d inputs: {off.max():.3f} of the two bounds")
        assert off.max() <= 1.0


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    F, fx, y = ST.case("joint-37-150").build()
    a, b = (P.logpdf_and_gradient_stencil(fx, y, inputs=True, stencils=True) for _ in range(2))
    assert a["logpdf"] == b["logpdf"] and _same_tables(a["_raw_stencils"], b["_raw_stencils"])
    assert all(np.array_equal(p, q) for p, q in zip(a["_raw"], b["_raw"]))
    F, fz, fx, y = ST.case("elbo-150x20g-diag").build()
    a, b = (P.elbo_and_gradient_stencil(P.VFE(fz), fx, y, stencils=True) for _ in range(2))
    assert a["elbo"] == b["elbo"]
    for k in ("zz", "xz", "xx"):
        assert _same_tables(a["_raw_stencils"][k], b["_raw_stencils"][k]), k
    assert len(a["stencils"]) == len(b["stencils"]) == 2
    for p, q in zip(a["stencils"], b["stencils"]):
        assert p["node"] is q["node"] and np.array_equal(p["d_offsets"], q["d_offsets"]) and np.array_equal(p["d_weights"], q["d_weights"])


def test_values_at_the_registration_limits_are_finite():
    case = ST.case("d16-se-64x2")
    (Ag, _), _ = case.stencils()
    assert Ag.shape == (P.lib.STENCIL_MAX_DIM, P.lib.STENCIL_MAX_POINTS) == (16, 64) and [n for _, n in case.blocks] == [3, 3]
    F, fx, y = case.build()
    g = P.logpdf_and_gradient_stencil(fx, y, stencils=True)
    gw, go = g["_raw_stencils"]
    assert sorted(a.shape for a in _flat(go)) == sorted([(64, 16)] * 4 + [(2, 16)] * 4)
    assert all(np.all(np.isfinite(a)) and np.any(a) for a in _flat(gw) + _flat(go))
    assert all(np.all(np.isfinite(e["d_offsets"])) and np.all(np.isfinite(e["d_weights"])) for e in g["stencils"])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    ctx = P.lib.default_context()
    new, err = ctx.stencil_wo, P.lib.last_error
    # a non-NULL entry for a plain side: the (g, f) pair of this case has one
    F, fx, y = ST.case("d3-m12-2x1").build()
    spec = P.build_spec(F, fx.x)[0]
    assert any((a is None) != (b is None) for a, b in spec.term_stencils)
    pw, po = _full_tables(spec)
    assert _lp_call(new.sgp_logpdf_grad_stencil_wo, spec, fx, y, None, pw, None)[0] < 0 and "plain side" in err()
    assert _lp_call(new.sgp_logpdf_grad_stencil_wo, spec, fx, y, None, None, po)[0] < 0 and "plain side" in err()
    nt = spec.n_terms
    dargs = (d(np.ones(len(y))), d(np.zeros(nt)), d(np.zeros(nt)), None)
    assert new.sgp_kernelmatrix_diag_grad_stencil_wo(ctx.handle, spec.ref(), *dargs, pw, po) < 0 and "plain side" in err()
    assert _lp_call(new.sgp_logpdf_grad_stencil_wo, spec, fx, y, None, *_tables(spec)[2:])[0] == 0, err()
    # the ELBO: inducing points in the plain process
    Fe, fz, fxe, ye = ST.case("elbo-150x20f-scalar").build()
    zz, xz = P.build_spec(Fe, fz.x)[0], P.build_spec(Fe, fxe.x, None, fz.x)[0]
    n, ntz, ntx = len(ye), max(1, zz.n_terms), max(1, xz.n_terms)
    e_bufs = ([np.ones(n), np.zeros(n), np.array([0.1]), np.array([1e-2]), np.ascontiguousarray(ye), np.zeros(1)] +
              [np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(n), np.zeros(1)] + [np.zeros(ntz), np.zeros(ntz), np.zeros(ntx), np.zeros(ntx)])
    e_args = ((d(e_bufs[0]), d(e_bufs[1]), P.lib.NOISE_SCALAR, d(e_bufs[2]), P.lib.NOISE_SCALAR, d(e_bufs[3])) +
              tuple(d(a) for a in e_bufs[4:]))
    assert not zz.has_stencil and xz.has_stencil
    assert new.sgp_elbo_grad_stencil_wo(ctx.handle, zz.ref(), xz.ref(), *e_args, None, None, None, None, None, None) == 0, err()
    pwz, poz = _full_tables(zz)
    assert new.sgp_elbo_grad_stencil_wo(ctx.handle, zz.ref(), xz.ref(), *e_args, None, None, pwz, poz, None, None) < 0
    assert "plain side" in err()
    pwx, pox = _full_tables(xz)
    assert new.sgp_elbo_grad_stencil_wo(ctx.handle, zz.ref(), xz.ref(), *e_args, None, None, None, None, pwx, pox) < 0
    assert "plain side" in err()
    # a patch term
    c = next(c for c in CT.CASES if c.id == "lanes-se-f")
    Fc, fxc, yc = c.build()
    pspec = P.build_spec(Fc, fxc.x)[0]
    assert pspec.has_patch
    pw, po = _full_tables(pspec)
    assert _lp_call(new.sgp_logpdf_grad_stencil_wo, pspec, fxc, yc, None, pw, po)[0] < 0 and "patch" in err()
    rc, a = _lp_call(new.sgp_logpdf_grad_stencil_wo, pspec, fxc, yc, None, None, None)
    rc0, b = _lp_call(ctx.stencil_grad.sgp_logpdf_grad_stencil, pspec, fxc, yc, None)
    assert rc == rc0 == 0 and all(np.array_equal(a[k], b[k]) for k in a)
    # a product chain
    Fk = P.gppp(lambda GP: {"p": GP(P.SEKernel() * P.Matern32Kernel())})
    xp = P.GPPPInput("p", P.ColVecs(np.asfortranarray(np.random.default_rng(2).standard_normal((2, 12)))))
    kxx = P.build_spec(Fk, xp)[0]
    assert kxx.has_kprod
    pw, po = _full_tables(kxx)
    yk = np.random.default_rng(3).standard_normal(12)
    assert _lp_call(new.sgp_logpdf_grad_stencil_wo, kxx, Fk(xp, 0.1), yk, None, pw, po)[0] < 0 and "product chain" in err()
    assert _lp_call(new.sgp_logpdf_grad_stencil_wo, kxx, Fk(xp, 0.1), yk, None, None, None)[0] == 0, err()
    zk = P.GPPPInput("p", P.ColVecs(np.asfortranarray(np.random.default_rng(4).standard_normal((2, 3)))))
    kz, kx = P.build_spec(Fk, zk)[0], P.build_spec(Fk, P.GPPPInput("p", P.ColVecs(np.asfortranarray(np.zeros((2, n))))), None, zk)[0]
    assert new.sgp_elbo_grad_stencil_wo(ctx.handle, kz.ref(), kx.ref(), *e_args, None, None, None, None, None, None) < 0
    assert "product chains" in err()
    # the older entry points keep refusing stencil terms
    lib = ctx.lib
    assert _lp_call(lib.sgp_logpdf_grad, spec, fx, y)[0] < 0 and "stencil" in err()
    assert _lp_call(ctx.conv_grad.sgp_logpdf_grad_conv, spec, fx, y)[0] < 0 and "stencil" in err()
    assert lib.sgp_kernelmatrix_diag_grad(ctx.handle, spec.ref(), *dargs[:3]) < 0 and "stencil" in err()
    assert lib.sgp_elbo_grad(ctx.handle, zz.ref(), xz.ref(), *e_args) < 0 and "stencil" in err()
    # a multi-GPU context (it takes no stencil: a plain spec is refused all the same)
    plain = P.build_spec(F, P.GPPPInput("f", P.ColVecs(np.asfortranarray(np.random.default_rng(6).standard_normal((3, 6))))))[0]
    npl = plain.N
    mctx = P.lib.Context(devices=[0, 0])
    try:
        m, nz, yv = np.zeros(npl), np.array([0.1]), np.ones(npl)
        bufs = [np.zeros(1), np.zeros(npl), np.zeros(npl), np.zeros(1), np.zeros(4), np.zeros(4)]
        rc = new.sgp_logpdf_grad_stencil_wo(mctx.handle, plain.ref(mctx), d(m), P.lib.NOISE_SCALAR, d(nz), d(yv),
                                            *[d(a) for a in bufs], None, None, None)
        assert rc < 0 and "multi-GPU" in err()
        assert new.sgp_kernelmatrix_diag_grad_stencil_wo(mctx.handle, plain.ref(mctx), d(np.ones(npl)), d(np.zeros(4)),
                                                         d(np.zeros(4)), None, None, None) < 0 and "multi-GPU" in err()
        prev = P.lib.set_default_context(mctx)
        try:
            with pytest.raises(NotImplementedError, match="multi-GPU"):
                P.logpdf_and_gradient_stencil(F(P.GPPPInput("f", P.ColVecs(np.zeros((3, 4)) + np.arange(4.0))), 0.1), np.zeros(4),
                                              stencils=True)
        finally:
            P.lib.set_default_context(prev)
    finally:
        mctx.close()
    del e_bufs


# ---- end to end ------------------------------------------------------------------------------------------------------------
class _Named:
    """a case of its own for stencil_grad_truth.logpdf_truth's cache: scalar noise"""
    noise = "scalar"

    def __init__(self, id):
        self.id = id


def test_host_gradient_of_a_learnable_quadrature_rule():
    """g = stencil(f, A, w) with 15 points over f = GP(1.3 SE(l)), D = 1, observed at 40 points of g and 30 of f: the node's
    d_offsets / d_weights against the truth pushed through the chain rule written out here -- the library reads the offsets
    as A / l, so dA = (1 / l) sum over terms and sides of the truth's offsets table, dw = the sum of its weights tables --
    with the bounds added over the contributing terms"""
    rng = np.random.default_rng(77)
    ls, Q = 0.7, 15
    A = np.sort(0.8 * rng.standard_normal(Q)).reshape(1, Q)
    w = np.exp(-A[0] ** 2) * (1.0 + 0.1 * rng.standard_normal(Q))
    node = {}

    def build(GP):
        f = GP(1.3 * P.with_lengthscale(P.SEKernel(), ls))
        node["g"] = P.stencil(f, A, w)
        return {"f": f, "g": node["g"]}
    F = P.gppp(build)
    x = P.BlockData([P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((1, 40))))),
                     P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((1, 30)))))])
    fx, y = F(x, 0.2), rng.standard_normal(70)
    g = P.logpdf_and_gradient_stencil(fx, y, stencils=True)
    assert len(g["stencils"]) == 1 and g["stencils"][0]["node"] is node["g"]
    got_o, got_w = g["stencils"][0]["d_offsets"], g["stencils"][0]["d_weights"]
    assert got_o.shape == (1, Q) and got_w.shape == (Q,)
    case = _Named("wo-end-to-end")
    R, *R64 = WT.logpdf_runs(case, g["_spec"], fx, y)
    ew, eo = WT.yardstick(R, R64)
    Bw, Bo = WT.bound_of("wo.lp.weights", ew), WT.bound_of("wo.lp.offsets", eo)
    ref_o, ref_w, tol_o, tol_w, sides = 0, 0, 0, 0, 0
    for term in R:
        for side in (0, 1):
            if term is None or term["sides"][side] is None:
                continue
            sw, so = WT.scales(term, side)
            ref_o, ref_w = ref_o + term["sides"][side]["o"] / np.longdouble(ls), ref_w + term["sides"][side]["w"]
            tol_o, tol_w = tol_o + T.EPS * Bo * so / ls, tol_w + T.EPS * Bw * sw
            sides += 1
    assert sides == 4            # (g, g) twice, (g, f) and (f, g) once each
    off_o = float(np.max(np.abs(got_o - ref_o) / tol_o))
    off_w = float(np.max(np.abs(got_w - ref_w) / tol_w))
    print(f"end to end: d_offsets at {off_o:.3f}, d_weights at {off_w:.3f} of the bounds added over {sides} sides")
    assert off_o <= 1.0 and off_w <= 1.0
    # the records: the mirror pair's term folded in with its sides swapped
    rec = next(r for r in g["terms"] if r["I"] == 1 and r["J"] == 0)
    gw, go = WT.host_tables(g["_raw_stencils"])
    assert rec["d_row_weights"] is None and rec["mirror_t"] is not None
    assert np.array_equal(rec["d_col_weights"], gw[rec["t"]][1] + gw[rec["mirror_t"]][0])
    assert np.array_equal(rec["d_col_offsets"], go[rec["t"]][1] + go[rec["mirror_t"]][0])
