"""Gradients of posterior mean and variance with respect to the test points (include/sthenomi_predgrad.h,
stheno.jl_amd/csrc/predgrad.hip) through P.mean_and_var_and_gradient and through the C boundary.

Truth cases: the raw per-input arrays against an extended-precision truth (tests/predgrad_truth.py), errors counted in
eps = 2^-53 times a scale taken from the truth, bound MARGIN * max(the reference's own float64 figures on the case, the
family's floor) -- from the reference, never from the device.  Models, points, noise and conditioning are those of
tests/test_gpu_grad_truth.py (two atoms, three atoms, a kernel sum, two stretched views: SE and Matern-1/2, 3/2, 5/2 in
rotation).  Shapes: D in {1, 2, 3, 8, 16, 17, 33} (every instantiation of the contraction, a full last chunk of the chunked
kernel and a one-coordinate last chunk), training layout (129, 1, 128, 70) plus one single block of
2 * SGP_PREDGRAD_COL_CHUNK + 70 points (several column chunks and a remainder), test layouts (1,), (129, 1, 70) and (257,),
scalar and diagonal noise; sparse: Z layouts (33, 1, 70) and (SGP_PREDGRAD_COL_CHUNK + 1,).
The bodies re-run on the NumPy double of the C-ABI in tests/test_predgrad_truth_on_numpy.py."""
import ctypes as C

import numpy as np
import pytest

import forward_truth as FT
import grad_truth as T
import predgrad_truth as PT
import stheno_jl_amd as P
import test_gpu_grad_truth as GT

pytestmark = pytest.mark.gpu

CHUNK = P.lib.PREDGRAD_COL_CHUNK
LAYOUT = GT.LAYOUT                                  # (129, 1, 128, 70)
TEST_LAYOUTS = ((129, 1, 70), (257,), (1,))
X_LAYOUT = GT.X_LAYOUT                              # the data of the sparse cases
SIGMA_Z = 1e-2


class Case:
    def __init__(self, id, sparse, D, model, layout, test_layout, noise, z_layout=None):
        self.id, self.sparse, self.D, self.model, self.layout = id, sparse, D, model, layout
        self.test_layout, self.noise, self.z_layout = test_layout, noise, z_layout

    def __repr__(self):
        return self.id


_MODELS = (lambda q: GT._two_atoms(q), lambda q: GT._three_atoms(q), lambda q: GT._kernel_sum(3, q), lambda q: GT._two_views(q))
EXACT_CASES, SPARSE_CASES = [], []
for _q, _D in enumerate((1, 2, 3, 8, 16, 17, 33)):
    EXACT_CASES.append(Case(f"pred-D{_D}", False, _D, (lambda q=_q: _MODELS[q % 4](q)), LAYOUT, TEST_LAYOUTS[_q % 3],
                            ("scalar", "diag")[_q % 2]))
# the two-views model (row and column inputs differ: a non-zero prior part) on several test blocks, small and chunked D
EXACT_CASES.append(Case("pred-views-D2", False, 2, (lambda: GT._two_views(1)), LAYOUT, (129, 1, 70), "diag"))
EXACT_CASES.append(Case("pred-views-D17", False, 17, (lambda: GT._two_views(2)), LAYOUT, (257,), "scalar"))
# one block of several column chunks plus a remainder
EXACT_CASES.append(Case("pred-chunks-D3", False, 3, (lambda: GT._three_atoms(1)), (2 * CHUNK + 70,), (129, 1, 70), "scalar"))
for _q, (_D, _zl) in enumerate(((2, (33, 1, 70)), (8, (CHUNK + 1,)), (17, (33, 1, 70)), (3, (CHUNK + 1,)))):
    _m = (lambda q=_q: (GT._two_atoms, GT._three_atoms, GT._two_views, (lambda i: GT._kernel_sum(3, i)))[q](q))
    SPARSE_CASES.append(Case(f"spred-D{_D}-Z{sum(_zl)}", True, _D, _m, X_LAYOUT, TEST_LAYOUTS[_q % 3],
                             ("scalar", "diag")[_q % 2], z_layout=_zl))
ALL_CASES = EXACT_CASES + SPARSE_CASES              # a case's seed is its position here: additions go at the end

_NOISE_TAG = GT._NOISE_TAG
_TRUTH = {}          # case id -> (truth in long double, two float64 runs): computed once, shared, never modified


def _names(names, layout):
    return tuple(names[i % len(names)] for i in range(len(layout)))


def setup(case):
    """the posterior of a case and post(x*, noise*); everything the truth needs rides along"""
    rng = np.random.default_rng(7100 + ALL_CASES.index(case))
    F, names = case.model()
    xs = [GT._points(rng, case.D, n) for n in case.layout]
    n = sum(case.layout)
    x = GT._blocks(F, _names(names, case.layout), xs)
    noise = GT._noise(rng, case.noise, n)
    y = rng.standard_normal(n)
    ts = [GT._points(rng, case.D, k) for k in case.test_layout]
    xt = GT._blocks(F, _names(names, case.test_layout), ts)
    noise_t = 0.1 + rng.random(sum(case.test_layout))
    if case.sparse:
        zs = [GT._points(rng, case.D, k) for k in case.z_layout]
        z = GT._blocks(F, _names(names, case.z_layout), zs)
        post = P.posterior(P.VFE(F(z, SIGMA_Z)), F(x, noise), y)
        return dict(F=F, x=x, z=z, noise=noise, y=y, post=post, fxs=post(xt, noise_t), xt=xt)
    post = P.posterior(F(x, noise), y)
    return dict(F=F, x=x, noise=noise, y=y, post=post, fxs=post(xt, noise_t), xt=xt)


def truth_of(case, s, g):
    if case.id not in _TRUTH:
        F = s["F"]
        Sc, Sp = T.read_spec(g["_cross"]), T.read_spec(g["_prior"])
        ms = P.mean_vector(F, s["xt"])
        runs = []
        for dt, ch in GT._RUNS():
            if case.sparse:
                Szz = T.read_spec(P.build_spec(F, s["z"])[0])
                Sxz = T.read_spec(P.build_spec(F, s["x"], F, s["z"])[0])
                runs.append(PT.sparse_predict_grad(Szz, T.NOISE_SCALAR, SIGMA_Z, Sxz, _NOISE_TAG[case.noise], s["noise"],
                                                   P.mean_vector(F, s["x"]), s["y"], Sc, Sp, ms, dt, cholesky=ch))
            else:
                St = T.read_spec(P.build_spec(F, s["x"])[0])
                runs.append(PT.predict_grad(St, _NOISE_TAG[case.noise], s["noise"], P.mean_vector(F, s["x"]), s["y"], Sc, Sp,
                                            ms, dt, cholesky=ch))
        _TRUTH[case.id] = tuple(runs)
    return _TRUTH[case.id]


def run_case(case):
    s = setup(case)
    g = P.mean_and_var_and_gradient(s["fxs"])
    return s, g, truth_of(case, s, g)


def prefix(case):
    return "spred" if case.sparse else "pred"


def device_units(case, g, R):
    return PT.family_units(prefix(case), dict(gm=g["inputs_mean"], gv=g["inputs_var"]), R)


def yardstick(case, R, R64):
    return GT.yardstick(PT.family_units(prefix(case), PT.reference_outputs(r), R) for r in R64)


def hold(case, dev, f64):
    """every family's device figure inside MARGIN * max(float64 figure, floor); figures printed first"""
    for fam in sorted(dev):
        print(f"{case.id:18s} {fam:15s} device {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {PT.FLOORS[fam]:8.1f}")
    bad = {fam: (dev[fam], f64[fam]) for fam in dev if not dev[fam] <= PT.MARGIN * max(f64[fam], PT.FLOORS[fam])}
    assert not bad, (case.id, bad)


def prior_part_check(case, g, R):
    """the k**_ii part involves no factorisation: the model bound of the diag_grad cases, (D + 8) eps S entry by entry"""
    bound = (case.D + 8) * T.EPS
    assert len(g["inputs_var_prior"]) == len(R["gp"])
    fig = 0.0
    for a, e, s in zip(g["inputs_var_prior"], R["gp"], R["S_gp"]):
        assert np.shape(a) == e.shape and not np.any(np.isnan(a))
        assert np.all(np.asarray(a)[s == 0] == 0.0)
        fig = max(fig, float(np.max(np.abs(a - e) / np.where(s > 0, bound * s, 1.0), initial=0.0)))
    print(f"{case.id:18s} prior part: error / ((D + 8) eps S) = {fig:.3f}")
    assert fig <= 1.0, (case.id, fig)


def values_check(case, s, g, R, R64):
    """mean and var themselves against the truth (their bits are pinned to the predict call below) under the post.mean /
    post.var (spost.*) bound of tests/forward_truth.py: MARGIN * max(the reference's float64 figure on this case, that
    family's floor), in eps of the scale of the truth; var is the latent variance plus the test noise on both sides"""
    pre = "spost" if case.sparse else "post"
    noise = np.asarray(s["fxs"].noise, dtype=np.float64)
    v_truth = R["var"] + noise.astype(R["var"].dtype)
    scales = {"mean": T.scale_entries(R["mean"], R["S_mean"] / R["n"]),
              "var": T.scale_entries(v_truth, (R["S_var"] + np.abs(noise).astype(R["var"].dtype)) / R["n"])}

    def figures(m, v):
        return {"mean": T.units(m, R["mean"], scales["mean"]), "var": T.units(v, v_truth, scales["var"])}

    dev = figures(g["mean"], g["var"])
    f64 = GT.yardstick(figures(r["mean"], r["var"] + noise) for r in R64)
    for key in ("mean", "var"):
        floor = FT.FLOORS[f"{pre}.{key}"]
        print(f"{case.id:18s} {pre + '.' + key:15s} device {dev[key]:10.1f}  float64 {f64[key]:10.1f}  floor {floor:8.1f}")
        assert dev[key] <= FT.MARGIN * max(f64[key], floor), (case.id, key, dev[key], f64[key])


@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_prediction_gradient_against_truth(case):
    s, g, (R, *R64) = run_case(case)
    for v in list(g["inputs_mean"]) + list(g["inputs_var"]) + list(g["inputs_var_prior"]) + [g["mean"], g["var"]]:
        assert not np.any(np.isnan(v))
    values_check(case, s, g, R, R64)
    hold(case, device_units(case, g, R), yardstick(case, R, R64))
    prior_part_check(case, g, R)
    if "views" in case.id:
        assert any(np.any(a != 0.0) for a in g["inputs_var_prior"])       # row and column views differ: a non-zero prior part
    # the chained gradients: one (D, n) array per block of x*
    assert [a.shape for a in g["d_mean"]] == [(case.D, k) for k in case.test_layout]
    assert [a.shape for a in g["d_var"]] == [(case.D, k) for k in case.test_layout]


# ---- shared outputs: the bits of the predict call, and of a second call ------------------------------------------------------
@pytest.mark.parametrize("case", [EXACT_CASES[2], EXACT_CASES[5], SPARSE_CASES[0], SPARSE_CASES[1]], ids=repr)
def test_mean_and_var_keep_the_bits_of_predict_and_two_calls_agree(case):
    s = setup(case)
    g1 = P.mean_and_var_and_gradient(s["fxs"])
    g2 = P.mean_and_var_and_gradient(s["fxs"])
    m, v = P.mean_and_var(s["fxs"])
    assert np.array_equal(g1["mean"], m) and np.array_equal(g1["var"], v)
    # ... and raw, through the two C entry points
    post, fn = s["post"], ("sgp_sparse_posterior_predict" if case.sparse else "sgp_posterior_predict")
    cross, pss = g1["_cross"], g1["_prior"]
    ms = np.ascontiguousarray(P.mean_vector(s["F"], s["xt"]))
    ns = cross.N
    mo, vo, mo2, vo2 = np.zeros(ns), np.zeros(ns), np.zeros(ns), np.zeros(ns)
    ctx = P.lib.default_context()
    rc = getattr(ctx.lib, fn)(post._ensure(), cross.ref(), pss.ref(), P.lib.dptr(ms), P.lib.dptr(mo), P.lib.dptr(vo), None, ns)
    P.lib.check(rc, fn)
    rc = getattr(ctx.predgrad, fn + "_grad_x")(post._ensure(), cross.ref(), pss.ref(), P.lib.dptr(ms), P.lib.dptr(mo2),
                                               P.lib.dptr(vo2), None, None, None)
    P.lib.check(rc, fn + "_grad_x")
    assert np.array_equal(mo, mo2) and np.array_equal(vo, vo2)
    for key in ("inputs_mean", "inputs_var", "inputs_var_prior", "d_mean", "d_var"):
        assert all(np.array_equal(a, b) for a, b in zip(g1[key], g2[key])), key


# ---- an extended posterior: ld != n_pad after update_posterior with reserve, and one without --------------------------------
@pytest.mark.parametrize("reserve", [None, 700], ids=["no-reserve", "reserve"])
def test_gradient_after_update_posterior(reserve):
    case = Case(f"pred-extended-{reserve}", False, 3, (lambda: GT._three_atoms(2)), (129, 70), (129, 1, 70), "scalar")
    rng = np.random.default_rng(7300)
    F, names = case.model()
    x1 = GT._blocks(F, ("f", "f"), [GT._points(rng, 3, n) for n in case.layout])
    x2 = GT._blocks(F, ("f",), [GT._points(rng, 3, 61)])
    noise = 0.15
    y1, y2 = rng.standard_normal(len(x1)), rng.standard_normal(len(x2))
    post = P.update_posterior(P.posterior(F(x1, noise), y1), F(x2, noise), y2, reserve=reserve)
    xt = GT._blocks(F, ("f",) * 3, [GT._points(rng, 3, k) for k in case.test_layout])
    fxs = post(xt, 0.2)
    g = P.mean_and_var_and_gradient(fxs)
    m, v = P.mean_and_var(fxs)
    assert np.array_equal(g["mean"], m) and np.array_equal(g["var"], v)
    St = T.read_spec(P.build_spec(F, post.x)[0])
    Sc, Sp = T.read_spec(g["_cross"]), T.read_spec(g["_prior"])
    runs = [PT.predict_grad(St, T.NOISE_SCALAR, noise, P.mean_vector(F, post.x), post.y, Sc, Sp, P.mean_vector(F, xt), dt,
                            cholesky=ch) for dt, ch in GT._RUNS()]
    R, R64 = runs[0], runs[1:]
    hold(case, device_units(case, g, R), yardstick(case, R, R64))
    prior_part_check(case, g, R)


# ---- edge pairs ------------------------------------------------------------------------------------------------------------
def _one_kind(i, mean=0.0):
    gpc = P.GPC()
    return P.GPPP({"f": P.atomic(P.GP(mean, GT._kernel(i)), gpc)}, gpc)


def test_matern12_at_a_training_point_is_finite_and_contributes_zero():
    rng = np.random.default_rng(7400)
    F = _one_kind(1)
    X = GT._points(rng, 2, 70)
    post = P.posterior(F(P.GPPPInput("f", P.ColVecs(X)), 0.1), rng.standard_normal(70))
    Xt = np.asfortranarray(np.concatenate([X[:, :5], GT._points(rng, 2, 4)], axis=1))
    g = P.mean_and_var_and_gradient(post(P.GPPPInput("f", P.ColVecs(Xt)), 0.1))
    for a in g["d_mean"] + g["d_var"]:
        assert np.all(np.isfinite(a))
    # one training point, the test point on top of it: its only pair contributes 0, so the whole gradient is an exact 0
    x0 = np.asfortranarray(np.array([[0.3], [-0.7]]))
    post1 = P.posterior(F(P.GPPPInput("f", P.ColVecs(x0)), 0.1), np.array([0.8]))
    Xt = np.asfortranarray(np.concatenate([x0, x0 + 1.0], axis=1))
    g = P.mean_and_var_and_gradient(post1(P.GPPPInput("f", P.ColVecs(Xt))))
    assert np.all(g["d_mean"][0][:, 0] == 0.0) and np.all(g["d_var"][0][:, 0] == 0.0)
    assert np.all(g["d_mean"][0][:, 1] != 0.0) and np.all(np.isfinite(g["d_var"][0]))


@pytest.mark.parametrize("kind", range(4), ids=GT.KINDS)
def test_a_far_test_point_gives_exact_zeros(kind):
    rng = np.random.default_rng(7500 + kind)
    F = _one_kind(kind)
    X = GT._points(rng, 3, 70)
    post = P.posterior(F(P.GPPPInput("f", P.ColVecs(X)), 0.1), rng.standard_normal(70))
    Xt = np.asfortranarray(np.concatenate([GT._points(rng, 3, 2), np.full((3, 1), 1e3)], axis=1))   # unit lengthscale
    g = P.mean_and_var_and_gradient(post(P.GPPPInput("f", P.ColVecs(Xt))))
    for a in g["d_mean"] + g["d_var"]:
        assert not np.any(np.isnan(a))
        assert np.all(a[:, 2] == 0.0) and np.any(a[:, :2] != 0.0)


# ---- cross-check of the host chaining on the device path: central differences of the library's own mean_and_var ----------
def warped_model(api):
    """stretch, select, periodic and shift in one process over 3-d points"""
    gpc = api.GPC()
    a = api.atomic(api.GP(api.SEKernel()), gpc)
    b = api.atomic(api.GP(api.Matern52Kernel()), gpc)
    c = api.atomic(api.GP(0.3, api.Matern32Kernel()), gpc)
    f = (api.stretch(api.shift(a, np.array([0.3, -0.2, 0.1])), np.array([0.5, 1.2, 0.8]))
         + api.select(api.periodic(b, 0.4), 1) + api.select(api.stretch(c, 0.9), [2, 0]))
    return {"f": f, "g": api.stretch(a, 0.7)}, gpc


# Step and tolerance of the central differences.  (f(x + h) - f(x - h)) / 2h misses f'(x) by at most h^2 max|f'''| / 6 plus
# E / h, E the error of one evaluation of f.
#   * mean_i = m + sum_j alpha_j k(x, x_j): every pair is a unit-variance SE / Matern-3/2 / Matern-5/2 profile of a warped
#     distance.  Along one coordinate the profiles' derivatives of order 1, 2, 3 are below 1.8, 3 and 2 sqrt(3)^3 = 10.4 (the
#     Matern-3/2 third derivative a^3 (2 - a r) e^(-a r), a = sqrt 3, is the largest); the warps' scales are at most
#     2 pi 0.4 = 2.52 (the periodic warp, whose own higher derivatives bring the profile's lower orders in: Faa di Bruno
#     with |w'|, |w''|, |w'''| <= 2.52, 2.52^2, 2.52^3).  So |d^3 k / dx^3| <= 2.52^3 (10.4 + 3 * 3 + 1.8) < 340 = FD_M3
#     and |f'''| <= FD_M3 sum_j |alpha_j|.
#   * var_i = k(x, x) - sum_jl C^-1_jl k(x, x_j) k(x, x_l): the third derivative of a product of two profiles has 8 terms,
#     products of derivatives each below FD_M3 in all (the profiles themselves are below 1), so
#     |f'''| <= 8 FD_M3 sum_jl |C^-1_jl|; k(x, x) is constant here (every atom enters a process once).
#   * E = 256 eps S, S the absolute sum of the addends of the value (predgrad_truth's S_mean, S_var): the allowance for the
#     rounding of the library's solves on this well-conditioned problem (noise 0.1, 60 points), far inside the 1e-9 S the
#     truth cases hold the values to.
# h = 2^-17 puts both parts between 1e-8 and 1e-5, against gradients of order 0.1 to 1.
FD_H = 2.0 ** -17
FD_M3 = 340.0


def fd_tolerance(weight, S):
    return FD_H ** 2 * FD_M3 * weight / 6.0 + 256.0 * T.EPS * S / FD_H


def test_chained_gradients_against_central_differences_of_mean_and_var():
    import models
    rng = np.random.default_rng(7600)
    fs, gpc = warped_model(models.product_api())
    F = P.GPPP(fs, gpc)
    X = [GT._points(rng, 3, 40), GT._points(rng, 3, 20)]
    x = P.BlockData([P.GPPPInput("f", P.ColVecs(X[0])), P.GPPPInput("g", P.ColVecs(X[1]))])
    post = P.posterior(F(x, 0.1), rng.standard_normal(60))
    Xt = [GT._points(rng, 3, 7), GT._points(rng, 3, 5)]

    def at(Xs):
        return post(P.BlockData([P.GPPPInput("g", P.ColVecs(np.asfortranarray(Xs[0]))),
                                 P.GPPPInput("f", P.ColVecs(np.asfortranarray(Xs[1])))]), 0.05)

    g = P.mean_and_var_and_gradient(at(Xt))
    # the weights of the tolerance, from the float64 reference on this problem
    R = PT.predict_grad(T.read_spec(P.build_spec(F, x)[0]), T.NOISE_SCALAR, 0.1, P.mean_vector(F, x), post.y,
                        T.read_spec(g["_cross"]), T.read_spec(g["_prior"]), P.mean_vector(F, at(Xt).x), np.float64)
    assert not any(np.any(a) for a in g["inputs_var_prior"])          # k(x, x) is constant in this model
    tol_m = fd_tolerance(float(np.abs(R["alpha"]).sum()), float(np.max(R["S_mean"])))
    tol_v = fd_tolerance(8.0 * float(np.abs(R["Q"]).sum()), float(np.max(R["S_var"])))
    worst_m = worst_v = 0.0
    for blk in range(2):
        for d in range(3):
            Xp = [a.copy() for a in Xt]
            Xm = [a.copy() for a in Xt]
            Xp[blk][d, :] += FD_H
            Xm[blk][d, :] -= FD_H
            mp, vp = P.mean_and_var(at(Xp))
            mm, vm = P.mean_and_var(at(Xm))
            off = 0 if blk == 0 else 7
            n = Xt[blk].shape[1]
            fd_m = (mp - mm)[off:off + n] / (2 * FD_H)
            fd_v = (vp - vm)[off:off + n] / (2 * FD_H)
            worst_m = max(worst_m, float(np.abs(fd_m - g["d_mean"][blk][d]).max()))
            worst_v = max(worst_v, float(np.abs(fd_v - g["d_var"][blk][d]).max()))
    print(f"central differences: mean {worst_m:.3e} (tolerance {tol_m:.3e}), var {worst_v:.3e} (tolerance {tol_v:.3e})")
    assert worst_m <= tol_m and worst_v <= tol_v
    # the check can see a wrong gradient
    assert max(float(np.abs(a).max()) for a in g["d_mean"]) > 100 * tol_m
    assert max(float(np.abs(a).max()) for a in g["d_var"]) > 100 * tol_v


# ---- refusals through the C boundary ---------------------------------------------------------------------------------------
def _raw_call(post_handle, cross, pss, ns, sparse=False):
    ctx = P.lib.default_context()
    fn = "sgp_sparse_posterior_predict_grad_x" if sparse else "sgp_posterior_predict_grad_x"
    ms, mo, vo = np.zeros(ns), np.zeros(ns), np.zeros(ns)
    gm = [np.zeros(np.asarray(a).shape, order="F") for a in cross.inputs]
    ptrs = (C.POINTER(C.c_double) * max(1, len(gm)))(*[P.lib.dptr(a) for a in gm])
    rc = getattr(ctx.predgrad, fn)(post_handle, cross.ref(), pss.ref() if pss is not None else None, P.lib.dptr(ms),
                                   P.lib.dptr(mo), P.lib.dptr(vo), ptrs, None, None)
    return rc, P.lib.last_error()


def test_refusals_through_the_c_boundary():
    rng = np.random.default_rng(7700)
    F = _one_kind(0)
    x = P.GPPPInput("f", P.ColVecs(GT._points(rng, 2, 30)))
    xt = P.GPPPInput("f", P.ColVecs(GT._points(rng, 2, 6)))
    post = P.posterior(F(x, 0.1), rng.standard_normal(30))
    cross = P.build_spec(F, xt, F, x)[0]
    pss = P.build_spec(F, xt)[0]
    rc, err = _raw_call(post._ensure(), cross, pss, 6)
    assert rc == 0, err
    # sizes: a cross spec against other training points, a prior spec of another size
    other = P.build_spec(F, xt, F, P.GPPPInput("f", P.ColVecs(GT._points(rng, 2, 29))))[0]
    rc, err = _raw_call(post._ensure(), other, pss, 6)
    assert rc < 0 and "sgp_posterior_predict_grad_x" in err and "sizes do not match" in err
    rc, err = _raw_call(post._ensure(), cross, P.build_spec(F, P.GPPPInput("f", P.ColVecs(GT._points(rng, 2, 5))))[0], 6)
    assert rc < 0 and "sizes do not match" in err
    # a product of kernels
    gpc = P.GPC()
    Fp = P.GPPP({"f": P.atomic(P.GP(P.KernelProduct([P.SEKernel(), P.Matern32Kernel()])), gpc)}, gpc)
    rc, err = _raw_call(post._ensure(), P.build_spec(Fp, xt, Fp, x)[0], P.build_spec(Fp, xt)[0], 6)
    assert rc < 0 and "product" in err
    # a stencil and a patch (convolutional) model
    gpc = P.GPC()
    base = P.atomic(P.GP(P.SEKernel()), gpc)
    Fs = P.GPPP({"f": P.stencil(base, np.array([[0.0, 0.1], [0.0, -0.1]]), [0.5, 0.5])}, gpc)
    rc, err = _raw_call(post._ensure(), P.build_spec(Fs, xt, Fs, x)[0], P.build_spec(Fs, xt)[0], 6)
    assert rc < 0 and "stencil" in err
    gpc = P.GPC()
    Fc = P.GPPP({"f": P.patch_convolve(P.atomic(P.GP(P.SEKernel()), gpc), patch_shape=(2, 2))}, gpc)
    imgs = P.GPPPInput("f", P.ImageVector(rng.standard_normal((3, 3, 30))))
    imt = P.GPPPInput("f", P.ImageVector(rng.standard_normal((3, 3, 6))))
    rc, err = _raw_call(post._ensure(), P.build_spec(Fc, imt, Fc, imgs)[0], P.build_spec(Fc, imt)[0], 6)
    assert rc < 0 and "patch" in err
    # the posterior answers as before
    rc, err = _raw_call(post._ensure(), cross, pss, 6)
    assert rc == 0, err


def test_a_destroyed_context_is_refused():
    rng = np.random.default_rng(7800)
    F = _one_kind(0)
    x = P.GPPPInput("f", P.ColVecs(GT._points(rng, 2, 30)))
    xt = P.GPPPInput("f", P.ColVecs(GT._points(rng, 2, 6)))
    cross, pss = P.build_spec(F, xt, F, x)[0], P.build_spec(F, xt)[0]
    spec = P.build_spec(F, x)[0]
    L = P.lib
    lib = L.load()
    ctx2 = L.Context(0)
    y, s2, h = rng.standard_normal(30), np.array([0.1]), C.c_void_p()
    rc = lib.sgp_posterior_create(ctx2.handle, spec.ref(), None, L.NOISE_SCALAR, L.dptr(s2), L.dptr(y), None, C.byref(h))
    L.check(rc, "sgp_posterior_create")
    ctx2.close()
    rc, err = _raw_call(h, cross, pss, 6)
    assert rc < 0 and "destroyed" in err
    lib.sgp_posterior_destroy(h)
