"""Every gradient kernel instantiation (stheno.jl_amd/csrc/grad.hip) against an extended-precision truth
(tests/grad_truth.py), through the public host calls: P.logpdf_and_gradient(..., inputs=True, scales=...),
P.elbo_and_gradient(..., inputs=True) and sgp_kernelmatrix_diag_grad / _grad_x with the caller's w.

Each case asserts the value, y, mean, noise, every term's d_coef / d_inscale (the raw records) and every entry of
every input and row-scale gradient.  Errors are counted in eps = 2^-53 times a scale taken from the truth; the bound of a
case and output family is MARGIN * max(the same reference run in float64 on this case, the family's floor) -- it comes
from the reference, never from the device (docs/04_oracle_and_parity.md, "Gradient kernels against an extended-precision
truth").  Problems are well conditioned (noise 0.05 .. 0.3, O(1) coefficients, inputs standard_normal / sqrt(D) * 1.5,
Sigma_z = 1e-2) so that the truth, not the condition number, decides.

Shapes: block lengths (129, 1, 128, 70), N = 328 -- every block boundary inside a 128 tile, a single-row block, a block one
tile long that straddles two, a tile with rows of three blocks -- plus single blocks of 1, 128 and 257 rows.
The bodies re-run on the NumPy double of the C-ABI in tests/test_host_mirror_on_numpy_double.py."""
import ctypes as C

import numpy as np
import pytest

import grad_truth as T
import stheno_jl_amd as P

pytestmark = pytest.mark.gpu

LAYOUT = (129, 1, 128, 70)
Z_LAYOUT, X_LAYOUT = (33, 1, 70), (129, 70, 131)
KINDS = ("SEKernel", "Matern12Kernel", "Matern32Kernel", "Matern52Kernel")


def _per(D):
    """terms per launch of launch_grad_block (capi.hip: contract_spec): min(8, max(1, 64 / pow2ceil(D)))"""
    dmax = 1
    while dmax < D:
        dmax *= 2
    return min(8, max(1, 64 // dmax))


def _points(rng, D, n):
    return np.asfortranarray(rng.standard_normal((D, n)) / np.sqrt(D) * 1.5)


def _kernel(i):
    return getattr(P, KINDS[i % 4])()


def _blocks(F, names, xs):
    return P.BlockData([P.GPPPInput(k, P.ColVecs(x)) for k, x in zip(names, xs)])


# ---- models ------------------------------------------------------------------------------------------------------
def _two_atoms(i):
    """two independent atoms of kinds i and i + 1, blocks a b a b: one term per block pair, pairs of different atoms empty"""
    gpc = P.GPC()
    a = np.sqrt(1.3) * P.atomic(P.GP(0.2, _kernel(i)), gpc)
    b = np.sqrt(0.8) * P.atomic(P.GP(-0.1, _kernel(i + 1)), gpc)
    return P.GPPP({"a": a, "b": b}, gpc), ("a", "b", "a", "b")


def _kernel_sum(n, i):
    """one atom whose kernel is a sum of n scaled, lengthscaled kernels of mixed kinds: n terms in every block pair"""
    gpc = P.GPC()
    ks = []
    for t in range(n):
        base = P.ConstantKernel(0.7) if (t % 5 == 4) else P.with_lengthscale(_kernel(i + t), 0.5 + 0.04 * t)
        ks.append(P.ScaledKernel(base, (0.5 + 0.25 * (t % 4)) / (0.875 * n)))          # total variance about 1
    f = P.atomic(P.GP(P.KernelSum(ks)), gpc)
    return P.GPPP({"f": f}, gpc), ("f",) * 4


def _three_atoms(i):
    """f = a + stretch(b, 1.4) + c: three terms in every block pair"""
    gpc = P.GPC()
    a, b, c = (P.atomic(P.GP(_kernel(i + q)), gpc) for q in range(3))
    f = np.sqrt(0.45) * a + np.sqrt(0.3) * P.stretch(b, 1.4) + np.sqrt(0.25) * c
    return P.GPPP({"f": f}, gpc), ("f",) * 4


def _mixed_dims():
    """views of 1, 2 and 5 coordinates in one block pair (three atoms: views of different dimension of ONE atom would
    pair a 1-d with a 2-d point in their cross terms)"""
    gpc = P.GPC()
    a1, a2, a5 = (P.atomic(P.GP(_kernel(q)), gpc) for q in (3, 1, 2))
    f = np.sqrt(0.4) * P.select(a1, [2]) + np.sqrt(0.3) * P.select(a2, [0, 3]) + np.sqrt(0.3) * a5
    return P.GPPP({"f": f}, gpc), ("f",) * 4


def _sigma(pt):
    return 1.0 + 0.3 * float(np.sin(np.sum(pt)))


def _function_scaled(i):
    gpc = P.GPC()
    a = P.atomic(P.GP(_kernel(i)), gpc)
    return P.GPPP({"h": _sigma * a}, gpc), ("h",) * 4


def _one_atom(i):
    gpc = P.GPC()
    return P.GPPP({"f": np.sqrt(1.2) * P.atomic(P.GP(0.1, _kernel(i)), gpc)}, gpc), ("f",)


# ---- the case list -------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, id, family, D, model, layout=LAYOUT, noise="scalar", scales=False, z_noise="scalar", seed=0):
        self.id, self.family, self.D, self.model, self.layout = id, family, D, model, layout
        self.noise, self.scales, self.z_noise, self.seed = noise, scales, z_noise, seed

    def __repr__(self):
        return self.id


def _noise(rng, kind, n, lo=0.05):
    if kind == "scalar":
        return float(lo + 0.25 * rng.random())
    if kind == "diag":
        return lo + 0.25 * rng.random(n)
    Bd = rng.standard_normal((n, 5))
    return np.asfortranarray(0.2 * np.eye(n) + 0.02 * Bd @ Bd.T)


LP_CASES, ELBO_CASES, DIAG_CASES = [], [], []
# term gradients, one term per block pair: every grad_block_kernel<DMAX>, both sides of each pow2ceil step, bigd with a full
# last chunk (80) and a one-coordinate last chunk (65, 81)
for _q, _D in enumerate((1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 64, 65, 80, 81)):
    LP_CASES.append(Case(f"terms-D{_D}", "terms", _D, (lambda q=_q: _two_atoms(q)), noise=("scalar", "diag")[_q % 2]))
# single blocks of 1, 128 and 257 rows
for _q, _n in ((1, 1), (3, 128), (2, 257)):
    LP_CASES.append(Case(f"single-N{_n}", "terms", 3, (lambda q=_q: _one_atom(q)), layout=(_n,)))
# term grouping: a full launch, a second launch with one term, three launches into the same partials
for _D in (1, 8, 16, 32):
    for _n in (_per(_D), _per(_D) + 1, 2 * _per(_D) + 1):
        LP_CASES.append(Case(f"group-D{_D}-T{_n}", "grouping", _D, (lambda n=_n, D=_D: _kernel_sum(n, D))))
LP_CASES.append(Case("mixed-dims-D5", "mixed", 5, _mixed_dims))
# input gradients with 1 and 3 terms (the D of the `terms` cases above carry the one-term runs for their dimensions too)
for _q, _D in enumerate((4, 48)):
    LP_CASES.append(Case(f"inputs-D{_D}-T1", "inputs", _D, (lambda q=_q: _two_atoms(q + 2))))
for _q, _D in enumerate((1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 48)):
    LP_CASES.append(Case(f"inputs-D{_D}-T3", "inputs", _D, (lambda q=_q: _three_atoms(q)), noise=("diag", "scalar")[_q % 2]))
for _q, _D in enumerate((1, 8, 17)):
    LP_CASES.append(Case(f"scales-D{_D}", "scales", _D, (lambda q=_q: _function_scaled(q + 2)), scales=True))
for _q, _kind in enumerate(("scalar", "diag", "dense")):
    LP_CASES.append(Case(f"noise-{_kind}", "noise", 3, (lambda q=_q: _two_atoms(q + 1)), noise=_kind))
# ELBO: zz, xz and xx terms, z and x input gradients; Sigma_z = 1e-2 I and one dense Sigma_z
for _q, _D in enumerate((1, 5, 16, 17)):
    ELBO_CASES.append(Case(f"elbo-D{_D}-T1", "elbo", _D, (lambda q=_q: _two_atoms(q)), noise=("scalar", "diag")[_q % 2]))
    _n = _per(_D) + 1
    ELBO_CASES.append(Case(f"elbo-D{_D}-T{_n}", "elbo", _D, (lambda n=_n, D=_D: _kernel_sum(n, D)),
                           noise=("diag", "scalar")[_q % 2], z_noise=("dense" if _D == 5 else "scalar")))
# diag_grad / _grad_x with the caller's w: a plain atom (one term per diagonal pair, coincident points) and a sum of two
# stretched views of one atom (four terms per diagonal pair, two of them between different points)
for _q, _D in enumerate((1, 8, 17, 65)):
    DIAG_CASES.append(Case(f"diag-D{_D}-plain", "diag", _D, (lambda q=_q: _two_atoms(q + 1))))
    DIAG_CASES.append(Case(f"diag-D{_D}-views", "diag", _D, None, seed=_q))
ALL_CASES = LP_CASES + ELBO_CASES + DIAG_CASES        # a case's seed is its position here: additions go at the end
# the remaining grad_inputs_kernel<DMAX, true> instantiations
for _q, _D in enumerate((2, 4, 16)):
    _c = Case(f"scales-D{_D}", "scales", _D, (lambda q=_q: _function_scaled(q + 1)), scales=True)
    LP_CASES.append(_c)
    ALL_CASES.append(_c)


def _two_views(i):
    gpc = P.GPC()
    a = P.atomic(P.GP(_kernel(i)), gpc)
    b = P.atomic(P.GP(_kernel(i + 1)), gpc)
    return P.GPPP({"a": np.sqrt(1.1) * P.stretch(a, 0.6) + np.sqrt(0.7) * P.stretch(a, 1.3),
                   "b": P.stretch(b, 0.5) + P.stretch(b, 1.4)}, gpc), ("a", "b", "a", "b")


for _c in DIAG_CASES:
    if _c.model is None:
        _c.model = (lambda q=_c.seed: _two_views(q + 2))


def _rng(case):
    return np.random.default_rng(9000 + ALL_CASES.index(case))


# ---- running a case on whatever library is loaded, and on the reference -----------------------------------------------------------
_NOISE_TAG = {"scalar": T.NOISE_SCALAR, "diag": T.NOISE_DIAG, "dense": T.NOISE_DENSE}
_TRUTH = {}          # case id -> (truth in long double, the same run in float64): computed once, shared, never modified


def _RUNS():
    """(dtype, factorisation) of the truth and of the two float64 yardstick runs: the reference's own column recurrence
    and the blocked order of the same operations"""
    return ((T.require_extended(), None), (np.float64, None), (np.float64, T.cholesky_blocked_order))


def run_logpdf(case):
    rng = _rng(case)
    F, names = case.model()
    xs = [_points(rng, case.D, n) for n in case.layout]
    n = sum(case.layout)
    fx = F(_blocks(F, names, xs), _noise(rng, case.noise, n))
    y = rng.standard_normal(n)
    g = P.logpdf_and_gradient(fx, y, inputs=True, scales=case.scales)
    if case.id not in _TRUTH:
        S = T.read_spec(g["_spec"])
        args = (S, _NOISE_TAG[case.noise], fx.noise, P.mean(fx), y)
        _TRUTH[case.id] = tuple(T.logpdf_grad(*args, dt, inputs=True, scales=case.scales, cholesky=ch)
                                for dt, ch in _RUNS())
    return g, _TRUTH[case.id]


def _logpdf_outputs(g):
    """the device's (or the double's) results in the layout of the reference's"""
    gc, gs = g["_raw"]
    nt = g["_spec"].n_terms
    return dict(value=g["logpdf"], y=g["y"], mean=g["mean"], noise=g["noise"], d_coef=gc[:nt], d_inscale=gs[:nt],
                gx=g["inputs"], rowscale=g["_rowscale"])


def _reference_outputs(R):
    return dict(value=R["value"], y=-R["alpha"], mean=R["alpha"], noise=R["noise"], d_coef=R["d_coef"],
                d_inscale=R["d_inscale"], gx=R.get("gx"), rowscale=R.get("rowscale"))


def logpdf_units(out, R):
    """largest error of each output family against the truth R, in units"""
    n = R["n"]
    u = {}
    u["lp.value"] = T.units(out["value"], R["value"], T.scale_scalar(R["value"], R["S_value"], n))
    sc = T.scale_entries(R["alpha"], R["S_alpha"] / n)
    u["lp.y"] = max(T.units(out["y"], -R["alpha"], sc), T.units(out["mean"], R["alpha"], sc))
    if np.ndim(R["noise"]) == 0:
        u["lp.noise"] = T.units(out["noise"], R["noise"], T.scale_scalar(R["noise"], R["S_noise"], n))
    else:
        assert np.shape(out["noise"]) == np.shape(R["noise"])
        u["lp.noise"] = T.units(out["noise"], R["noise"], T.scale_entries(R["noise"], R["S_noise"]))
    assert len(out["d_coef"]) == len(R["d_coef"]) and len(out["d_inscale"]) == len(R["d_inscale"])
    u["lp.d_coef"] = T.units(out["d_coef"], R["d_coef"], T.scale_scalar(R["d_coef"], R["S_coef"], R["n_rows"]))
    u["lp.d_inscale"] = T.units(out["d_inscale"], R["d_inscale"],
                                T.scale_scalar(R["d_inscale"], R["S_inscale"], R["n_rows"]))
    assert len(out["gx"]) == len(R["gx"])
    u["lp.inputs"] = 0.0
    for a, e, s in zip(out["gx"], R["gx"], R["Sn_gx"]):
        assert np.shape(a) == e.shape
        u["lp.inputs"] = max(u["lp.inputs"], T.units(a, e, T.scale_entries(e, s)))
    if R.get("rowscale") is not None:
        assert len(out["rowscale"]) == len(R["rowscale"])
        u["lp.scales"] = 0.0
        for a, e, s in zip(out["rowscale"], R["rowscale"], R["Sn_rowscale"]):
            assert (a is None) == (e is None)
            if e is not None:
                assert np.shape(a) == e.shape
                u["lp.scales"] = max(u["lp.scales"], T.units(a, e, T.scale_entries(e, s)))
    return u


def yardstick(runs):
    """e_float64 of a case: family by family the larger figure of the float64 runs"""
    runs = list(runs)
    return {fam: max(r[fam] for r in runs) for fam in runs[0]}


def hold(case, dev, f64):
    """the verdict: every family's device figure inside MARGIN * max(float64 figure, floor); figures printed first"""
    for fam in sorted(dev):
        print(f"{case.id:18s} {fam:15s} device {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {T.FLOORS[fam]:8.1f}")
    bad = {fam: (dev[fam], f64[fam]) for fam in dev if not dev[fam] <= T.MARGIN * max(f64[fam], T.FLOORS[fam])}
    assert not bad, (case.id, bad)


@pytest.mark.parametrize("case", LP_CASES, ids=repr)
def test_logpdf_gradient_against_truth(case):
    g, (R, *R64) = run_logpdf(case)
    out = _logpdf_outputs(g)
    for v in [out["value"], out["y"], out["mean"], out["noise"], out["d_coef"], out["d_inscale"]] + list(out["gx"]):
        assert not np.any(np.isnan(v))
    if case.scales:
        assert any(a is not None for a in out["rowscale"])
    hold(case, logpdf_units(out, R), yardstick(logpdf_units(_reference_outputs(r), R) for r in R64))


# ---- ELBO ----------------------------------------------------------------------------------------------------------------
def run_elbo(case):
    rng = _rng(case)
    F, names = case.model()
    names = names[:3]
    xs = [_points(rng, case.D, n) for n in X_LAYOUT]
    zs = [_points(rng, case.D, n) for n in Z_LAYOUT]
    n, m = sum(X_LAYOUT), sum(Z_LAYOUT)
    if case.z_noise == "dense":
        Q = rng.standard_normal((m, m))
        sz = np.asfortranarray(1e-2 * np.eye(m) + 1e-2 * (Q @ Q.T) / m)
    else:
        sz = 1e-2
    fx = F(_blocks(F, names, xs), _noise(rng, case.noise, n))
    fz = F(_blocks(F, names, zs), sz)
    y = rng.standard_normal(n)
    g = P.elbo_and_gradient(P.VFE(fz), fx, y, inputs=True)
    if case.id not in _TRUTH:
        Sp = {k: T.read_spec(v) for k, v in g["_specs"].items()}
        args = (Sp["zz"], Sp["xz"], Sp["xx"], _NOISE_TAG[case.noise], fx.noise, _NOISE_TAG[case.z_noise], sz, P.mean(fx), y)
        pair = []
        for dt, ch in _RUNS():
            R = T.elbo_grad(*args, dt, inputs=True, cholesky=ch)
            R["xx"] = T.diag_grad(Sp["xx"], np.asarray(R["var"], dtype=np.float64), dt)
            pair.append(R)
        _TRUTH[case.id] = tuple(pair)
    return g, _TRUTH[case.id]


def _elbo_outputs(g):
    nt = {k: g["_specs"][k].n_terms for k in ("zz", "xz", "xx")}
    return dict(value=g["elbo"], y=g["y"], mean=g["mean"], noise=g["noise"], z_noise=g["z_noise"], var=g["var"],
                zz=dict(d_coef=g["_raw"]["zz"][0][:nt["zz"]], d_inscale=g["_raw"]["zz"][1][:nt["zz"]], gx=g["zz_inputs"]),
                xz=dict(d_coef=g["_raw"]["xz"][0][:nt["xz"]], d_inscale=g["_raw"]["xz"][1][:nt["xz"]], gx=g["xz_inputs"]),
                xx=dict(d_coef=g["_raw"]["xx"][0][:nt["xx"]], d_inscale=g["_raw"]["xx"][1][:nt["xx"]]))


def _elbo_reference_outputs(R):
    return dict(value=R["value"], y=R["y"], mean=-R["y"], noise=R["noise"], z_noise=R["z_noise"], var=R["var"],
                zz=R["zz"], xz=R["xz"], xx=R["xx"])


def elbo_units(out, R):
    n, m = R["n"], R["m"]
    u = {}
    u["elbo.value"] = T.units(out["value"], R["value"], T.scale_scalar(R["value"], R["S_value"], n))
    sc = T.scale_entries(R["y"], R["S_y"] / m)
    u["elbo.y"] = max(T.units(out["y"], R["y"], sc), T.units(out["mean"], -R["y"], sc))
    if np.ndim(R["noise"]) == 0:
        u["elbo.noise"] = T.units(out["noise"], R["noise"], T.scale_scalar(R["noise"], R["S_noise"], n))
    else:
        assert np.shape(out["noise"]) == np.shape(R["noise"])
        u["elbo.noise"] = T.units(out["noise"], R["noise"], T.scale_entries(R["noise"], R["S_noise"]))
    if np.ndim(R["z_noise"]) == 0:
        u["elbo.z_noise"] = T.units(out["z_noise"], R["z_noise"], T.scale_scalar(R["z_noise"], R["S_z_noise"], m))
    else:
        assert np.shape(out["z_noise"]) == np.shape(R["z_noise"])
        u["elbo.z_noise"] = T.units(out["z_noise"], R["z_noise"], T.scale_entries(R["z_noise"], R["S_z_noise"]))
    u["elbo.d_coef"] = u["elbo.d_inscale"] = u["elbo.inputs"] = 0.0
    for key in ("zz", "xz"):
        o, r = out[key], R[key]
        assert len(o["d_coef"]) == len(r["d_coef"]) and len(o["gx"]) == len(r["gx"])
        u["elbo.d_coef"] = max(u["elbo.d_coef"],
                               T.units(o["d_coef"], r["d_coef"], T.scale_scalar(r["d_coef"], r["S_coef"], r["n_rows"])))
        u["elbo.d_inscale"] = max(u["elbo.d_inscale"], T.units(o["d_inscale"], r["d_inscale"],
                                                               T.scale_scalar(r["d_inscale"], r["S_inscale"], r["n_rows"])))
        for a, e, s in zip(o["gx"], r["gx"], r["Sn_gx"]):
            assert np.shape(a) == e.shape
            u["elbo.inputs"] = max(u["elbo.inputs"], T.units(a, e, T.scale_entries(e, s)))
    return u


def diag_model_check(case, D, o, r, with_inputs):
    """sgp_kernelmatrix_diag_grad* involve no factorisation: the bound is a model, (D + 8) eps S for every sum and entry;
    terms of off-diagonal block pairs are exact zeros"""
    bound = (D + 8) * T.EPS
    off = ~r["diagonal"]
    assert len(o["d_coef"]) == len(r["d_coef"]) and len(o["d_inscale"]) == len(r["d_inscale"])
    assert np.all(np.asarray(o["d_coef"])[off] == 0.0) and np.all(np.asarray(o["d_inscale"])[off] == 0.0)
    figs = [float(np.max(np.abs(o[k] - r[k]) / np.where(r[s] > 0, bound * r[s], 1.0), initial=0.0))
            for k, s in (("d_coef", "S_coef"), ("d_inscale", "S_inscale"))]
    if with_inputs:
        assert len(o["gx"]) == len(r["gx"])
        for a, e, s in zip(o["gx"], r["gx"], r["S_gx"]):
            assert np.shape(a) == e.shape and not np.any(np.isnan(a))
            assert np.all(np.asarray(a)[s == 0] == 0.0)
            figs.append(float(np.max(np.abs(a - e) / np.where(s > 0, bound * s, 1.0), initial=0.0)))
    print(f"{case.id:18s} diag_grad: error / ((D + 8) eps S) = {max(figs):.3f}")
    assert max(figs) <= 1.0, (case.id, figs)


@pytest.mark.parametrize("case", ELBO_CASES, ids=repr)
def test_elbo_gradient_against_truth(case):
    g, (R, *R64) = run_elbo(case)
    out = _elbo_outputs(g)
    flat = [out["value"], out["y"], out["mean"], out["noise"], out["z_noise"], out["var"]]
    for key in ("zz", "xz"):
        flat += [out[key]["d_coef"], out[key]["d_inscale"]] + list(out[key]["gx"])
    for v in flat:
        assert not np.any(np.isnan(v))
    assert np.max(np.abs(out["var"] - R["var"]) / np.abs(R["var"])) <= 2 * T.EPS      # -1 / (2 sy): one division
    hold(case, elbo_units(out, R), yardstick(elbo_units(_elbo_reference_outputs(r), R) for r in R64))
    diag_model_check(case, case.D, out["xx"], R["xx"], with_inputs=False)


# ---- sgp_kernelmatrix_diag_grad / _grad_x with the caller's w --------------------------------------------------------------
def run_diag(case):
    rng = _rng(case)
    F, names = case.model()
    xs = [_points(rng, case.D, n) for n in LAYOUT]
    spec, _, _ = P.build_spec(F, _blocks(F, names, xs))
    w = np.ascontiguousarray(rng.standard_normal(spec.N))
    ctx = P.lib.default_context()
    nt = max(1, spec.n_terms)
    res = {}
    for with_x in (False, True):
        gc, gs = np.full(nt, np.nan), np.full(nt, np.nan)
        gx = [np.zeros(np.asarray(a).shape, order="F") for a in spec.inputs]
        if with_x:
            ptrs = (C.POINTER(C.c_double) * max(1, len(gx)))(*[P.lib.dptr(a) for a in gx])
            rc = ctx.lib.sgp_kernelmatrix_diag_grad_x(ctx.handle, spec.ref(), P.lib.dptr(w), P.lib.dptr(gc), P.lib.dptr(gs), ptrs)
        else:
            rc = ctx.lib.sgp_kernelmatrix_diag_grad(ctx.handle, spec.ref(), P.lib.dptr(w), P.lib.dptr(gc), P.lib.dptr(gs))
        P.lib.check(rc, "sgp_kernelmatrix_diag_grad")
        res[with_x] = dict(d_coef=gc[:spec.n_terms], d_inscale=gs[:spec.n_terms], gx=gx)
    if case.id not in _TRUTH:
        _TRUTH[case.id] = (T.diag_grad(T.read_spec(spec), w, T.require_extended()),)
    return res, _TRUTH[case.id][0]


@pytest.mark.parametrize("case", DIAG_CASES, ids=repr)
def test_diag_gradient_against_truth(case):
    res, R = run_diag(case)
    assert R["diagonal"].any() and not R["diagonal"].all()
    for with_x in (False, True):
        assert not np.any(np.isnan(res[with_x]["d_coef"])) and not np.any(np.isnan(res[with_x]["d_inscale"]))
        diag_model_check(case, case.D, res[with_x], R, with_inputs=with_x)
    assert np.array_equal(res[False]["d_coef"], res[True]["d_coef"])
    assert np.array_equal(res[False]["d_inscale"], res[True]["d_inscale"])
