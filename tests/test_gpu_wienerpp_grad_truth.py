"""The gradient kernels of chains that hold the Wiener and PiecewisePolynomial kinds (csrc/kprod.hip: the mode-3
instantiations grad_kprod_kernel<DMAX, 3>, grad_kprod_inputs_kernel<DMAX, 4> and diag_grad_kprod_kernel<3>; csrc/kprod_kinds.h:
wiener_derivs, pp_derivs, dotkind_derivs_w) against an extended-precision truth (tests/wienerpp_grad_truth.py) and against the
committed 60-digit table of the two families (tests/wienerpp_truth.py).

(a) Contractions, through the host mirror (P.logpdf_and_gradient_param, P.elbo_and_gradient_param with inputs=True,
    scales=True): the value, y, mean, noise, every term's d_coef / d_inscale / d_param and every entry of every input and scale
    gradient, in eps = 2^-53 times a scale taken from the truth; the bound of a case and family is MARGIN * max(e_float64 of
    the case, the family's floor), both from the reference.  d_param of every WIENER / PIECEWISE term is exactly 0.  The
    diagonal (sgp_kernelmatrix_diag_grad_param with the caller's w) is held to the model bound of kprod_grad_truth.

        what                                               cases
        grad_kprod_kernel<1, 3>, inputs_kernel<1, 4>       wp-w0-D1, wp-pp0-D1 (j = 1, n = 1: kx carries t^0), wp-w2-pp1-D3 (its
                                                           WIENER chain reads one coordinate), wpelbo-w-D1
        <2, 3>, <2, 4>                                     wp-w1-se-D2, wp-pp-rq-lin-D2, wp-pp1-w0-D2, wpelbo-mixed-D2 (dense Sigma_z)
        <4, 3>, <4, 4>                                     wp-w2-pp1-D3, wp-wfull-D3 (WIENER on the whole point), wp-scaled-D3,
                                                           wpelbo-pp-D3
        <8, 3>, <8, 4>                                     wp-w3-se-D8, wp-pp2-D5
        <16, 3>, <16, 4>                                   wp-pp3-D16, wp-w-fbm-mn-D9 (WIENER x FBM x general-nu Matern: the three
                                                           routes of mode 3 in one chain), wpelbo-D16
        WIENER i = 0, 1, 2, 3                              wp-w0-D1, wp-w1-se-D2, wp-w2-pp1-D3, wp-w3-se-D8
        PIECEWISE q = 0, 1, 2, 3                           wp-pp0-D1, wp-w2-pp1-D3, wp-pp2-D5, wp-pp3-D16
        a head with a function-valued row scale            wp-scaled-D3
        ELBO: alpha == nullptr, both strides, rectangular  the wpelbo-* cases (the xz column side is a second launch with every
                                                           factor's row and column points exchanged: it reads c1 again)
        diag_grad_kprod_kernel<3>, the only reader of c1y  wpdiag-D3-views, wpdiag-D8-views (var(f(a x) + f(b x))), wpdiag-D3-plain;
                                                           d k / d y of part (b)

(b) wiener_derivs and pp_derivs pair by pair: every pair of the table as a column of a raw diagonal spec of one term, row
    input X, column input Y.  var_i = k(xr_i, xc_i), so with w = 1 grad_inputs[0][:, i] is d k / d x of pair i and
    grad_inputs[1][:, i] is d k / d y, and with w = e_i grad_inscale is d k / d g of pair i (one small call per pair).  All
    three are held to wienerpp_truth.tolerances, no pair left out; where the table's truth is an exact zero the device's is.
    The routines are __noinline__: the tile kernels call the same code objects.

The bodies re-run on the NumPy double of the entry points in tests/test_wienerpp_grad_truth_on_numpy.py."""
import numpy as np
import pytest

import kprod_grad_truth as KT
import stheno_jl_amd as P
import wienerpp_grad_truth as WG
import wienerpp_truth as wt
from stheno_jl_amd import lib as L
from test_gpu_kprod_grad_truth import _elbo_outputs, _finite, _logpdf_outputs, _ptrs, _scale_bufs

pytestmark = pytest.mark.gpu

MARGIN_IN_FORCE = WG.MARGIN            # the CPU file runs the bodies under its own margin
# the mode-3 launch classes each case must reach: {DMAX} over its chains with a WIENER or PIECEWISE factor
DMAX_OF = {"wp-w0-D1": {1}, "wp-w1-se-D2": {2}, "wp-w2-pp1-D3": {1, 4}, "wp-w3-se-D8": {8}, "wp-wfull-D3": {4}, "wp-pp0-D1": {1},
           "wp-pp2-D5": {8}, "wp-pp3-D16": {16}, "wp-pp-rq-lin-D2": {2}, "wp-w-fbm-mn-D9": {16}, "wp-scaled-D3": {4},
           "wp-pp1-w0-D2": {2}, "wpelbo-w-D1": {1}, "wpelbo-pp-D3": {4}, "wpelbo-mixed-D2": {2}, "wpelbo-D16": {16},
           "wpdiag-D3-views": {4}, "wpdiag-D8-views": {8}, "wpdiag-D3-plain": {4}}


def hold(case, dev, f64):
    """every family's figure inside MARGIN * max(float64 figure, floor); figures printed first"""
    for fam in sorted(dev):
        print(f"{case[0]:18s} {fam:16s} device {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {WG.FLOORS[fam]:8.1f}")
    bad = {fam: (dev[fam], f64[fam]) for fam in dev if not dev[fam] <= MARGIN_IN_FORCE * max(f64[fam], WG.FLOORS[fam])}
    assert not bad, (case[0], bad)


def _param_zeros(spec, d_param):
    kinds = np.array([spec._terms[t].kind & L.KIND_MASK for t in range(spec.n_terms)])
    assert np.any(np.isin(kinds, WG.WPP)) and np.all(np.asarray(d_param)[np.isin(kinds, WG.WPP)] == 0.0)


@pytest.mark.parametrize("case", [c for c in WG.CASES if c[1] == "lp"], ids=lambda c: c[0])
def test_logpdf_gradient_against_truth(case):
    F, x, _, noise, _, y = WG.problem(case)
    g = P.logpdf_and_gradient_param(F(x, noise), y, inputs=True, scales=True)
    R = WG.truth(case)[0]
    out = _logpdf_outputs(g)
    assert g["_spec"].has_kprod and g["_spec"].n_terms == len(R["d_coef"]) and WG.launch_classes(g["_spec"]) == DMAX_OF[case[0]]
    _finite([out["value"], out["y"], out["mean"], out["noise"], out["d_coef"], out["d_inscale"], out["d_param"]] + list(out["gx"]))
    _param_zeros(g["_spec"], out["d_param"])
    dev = WG.logpdf_units(out, R)
    assert ("kp.scales" in dev) == (case[6] == "scaled")
    hold(case, dev, WG.reference_figures(case))


@pytest.mark.parametrize("case", [c for c in WG.CASES if c[1] == "elbo"], ids=lambda c: c[0])
def test_elbo_gradient_against_truth(case):
    F, x, z, noise, sz, y = WG.problem(case)
    g = P.elbo_and_gradient_param(P.VFE(F(z, sz)), F(x, noise), y, inputs=True, scales=True)
    R = WG.truth(case)[0]
    out = _elbo_outputs(g)
    assert all(sp.has_kprod and WG.launch_classes(sp) == DMAX_OF[case[0]] for sp in g["_specs"].values())
    flat = [out["value"], out["y"], out["mean"], out["noise"], out["z_noise"], out["var"]]
    for key in ("zz", "xz"):
        flat += [out[key]["d_coef"], out[key]["d_inscale"], out[key]["d_param"]] + list(out[key]["gx"])
        _param_zeros(g["_specs"][key], out[key]["d_param"])
    _finite(flat)
    assert np.max(np.abs(out["var"] - R["var"]) / np.abs(R["var"])) <= 2 * KT.EPS      # -1 / (2 sy): one division
    hold(case, KT.elbo_units(out, R), WG.reference_figures(case))


# ---- sgp_kernelmatrix_diag_grad_param ------------------------------------------------------------------------------------------
def _diag_call(spec, w, scales=True):
    ctx, d = L.default_context(), L.dptr
    nt = max(1, spec.n_terms)
    o = dict(d_coef=np.full(nt, np.nan), d_inscale=np.full(nt, np.nan), d_param=np.full(nt, np.nan),
             gx=[np.zeros(np.asarray(a).shape, order="F") for a in spec.inputs],
             rowscale=_scale_bufs(spec, "row", nt) if scales else None, colscale=_scale_bufs(spec, "col", nt) if scales else None)
    rc = ctx.kprod_grad.sgp_kernelmatrix_diag_grad_param(ctx.handle, spec.ref(ctx), d(w), d(o["d_coef"]), d(o["d_inscale"]),
                                                         d(o["d_param"]), _ptrs(o["gx"]),
                                                         _ptrs(o["rowscale"], nt) if scales else None,
                                                         _ptrs(o["colscale"], nt) if scales else None)
    assert rc == 0, L.last_error()
    for key in ("d_coef", "d_inscale", "d_param"):
        o[key] = o[key][:spec.n_terms]
    return o


@pytest.mark.parametrize("case", WG.DIAG_CASES, ids=lambda c: c[0])
def test_diag_gradient_against_truth(case):
    spec, w = WG.diag_problem(case)
    o, R = _diag_call(spec, w), WG.diag_truth(case)
    assert spec.has_kprod and R["diagonal"].any() and WG.launch_classes(spec) == DMAX_OF[case[0]]
    _finite([o["d_coef"], o["d_inscale"], o["d_param"]] + o["gx"])
    _param_zeros(spec, o["d_param"])
    fig = KT.diag_model_figures(o, R)
    if case[3] == "views":
        assert any(np.max(np.abs(e)) > 1e-3 for e in R["gx"])
    for fam in sorted(fig):
        print(f"{case[0]:18s} {fam:16s} error / model bound = {fig[fam]:.3f}")
    assert all(v <= 1.0 for v in fig.values()), (case[0], fig)


# ---- (b) the derivative routines against the table, pair by pair ------------------------------------------------------------------
def _table_groups():
    T = wt.load()
    return [(key, D) for key in T for D in T[key] if T[key][D].n]


def pair_derivatives(key, g):
    """(dg, dx, dy) of every pair of a group from sgp_kernelmatrix_diag_grad_param on the raw spec of the module docstring"""
    kind, param = (L.WIENER, float(key[1])) if key[0] == "w" else (L.PIECEWISE0 + key[1], float(key[2]))
    spec = L.Spec([g.n], [g.n], [g.X, g.Y], {(0, 0): [(kind, 0, 1, 1.0, param, None, None)]}, True)
    o = _diag_call(spec, np.ones(g.n), scales=False)
    assert o["d_param"][0] == 0.0
    dg = np.empty(g.n)
    for i in range(g.n):
        e = np.zeros(g.n)
        e[i] = 1.0
        dg[i] = _diag_call(spec, e, scales=False)["d_inscale"][0]
    return dg, np.asarray(o["gx"][0]), np.asarray(o["gx"][1])


@pytest.mark.parametrize("key,D", _table_groups(), ids=lambda v: str(v).replace(" ", ""))
def test_derivative_routines_against_the_table(key, D):
    g = wt.load()[key][D]
    tol = wt.tolerances(key, g)
    for name, got in zip(("dg", "dx", "dy"), pair_derivatives(key, g)):
        want = g.truth[name]
        assert got.shape == want.shape
        print(f"{key} D={D} {name}: largest error as a fraction of the bound {wt.worst(got, want, tol[name]):.3f} over {got.size} entries")
        bad = wt.violations(got, want, tol[name])
        assert bad.size == 0, (name, bad[:6], got.ravel()[bad[:6]], want.ravel()[bad[:6]], np.asarray(tol[name]).ravel()[bad[:6]])
        assert np.all(got[want == 0.0] == 0.0), name          # beyond the support, against the origin, d == 0: exact zeros
