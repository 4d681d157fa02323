"""The arc-cosine kinds on the device (csrc/arccos.hip; include/sthenomi.h: SGP_NNGP, SGP_NTK).  Values against the DEFINITION in
60 digits (mpmath: acos per layer, no angle tricks): an entry is right to U units of 2^-53 of |w| n_x n_y (NNGP) or of
|w| (L + 1) n_x n_y (NTK), U the per-entry first-order bound of docs/03_kernels.md, 3.2j (bound_units).  Gradients of the host's logpdf_and_gradient against
tests/grad_truth.py in long double (ops: tests/arccos_np.py), inside its margin: MARGIN x max(the float64 runs' figure, the
family's floor).  Shapes: a symmetric 129-point block (one tile and one row) and a 130 x 5 cross pair (one tile and a row pair)."""
import ctypes as C
import functools

import mpmath
import numpy as np
import pytest

import arccos_np
import grad_truth as T
import stheno_jl_amd as P
import test_gpu_grad_truth as GT
from stheno_jl_amd import lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::DeprecationWarning")]
LD, EPS, TINY = np.longdouble, 2.0 ** -53, 2.0 ** -1070
PD = C.POINTER(C.c_double)
DEPTHS = (1, 2, 16)
SPECIAL = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 128)


def bound_units(D, depth, ntk, th, ts):
    """docs/03_kernels.md, 3.2j, per entry and to first order, in units of 2^-53 of |w| n_x n_y (times L + 1 for the NTK): th =
    [theta_0 .. theta_L] and ts = [t_0 .. t_L] of the pair in truth.  Library functions count 4 units relative (2 ulp), an
    operation 1; the error of the carried angle passes a layer with its true factor kappa_0 sin theta_l / sin theta_{l+1}"""
    lam, pi, sin, cos = 4.0, np.pi, np.sin, np.cos
    dth = (D + 6) + (D + 4) * sin(th[0]) + lam * th[0]                                  # the unit vectors and the atan2
    dc = dt = sin(th[0]) * dth + (2 * lam + 1) * (1 - cos(th[0])) + abs(cos(th[0]))     # t_0 = 1 - 2 sin^2 h_0
    for l in range(depth):
        a, nxt = th[l], th[l + 1]
        A, k0 = 1 - cos(a), 1 - a / pi
        eta = (2 * lam + 1) * A + (1 - cos(nxt)) + (a * ((2 * lam + 1) * A + abs(cos(a))) + (2 * lam + 1) * sin(a)
                                                    + 2 * (sin(a) - a * cos(a))) / pi       # of the deficit s
        dc = k0 * sin(a) * dth + eta + abs(cos(nxt))
        dt = k0 * dt + abs(ts[l]) * (dth / pi + 2) + dc + abs(ts[l + 1])
        if nxt > 0:                                                                      # (0: a coincident pair, exact)
            dth = (k0 * sin(a) * dth + eta) / sin(nxt) + (1.273 + lam) * nxt             # back to the angle: sqrt and asin
    top = depth + 1 if ntk else 1
    return ((dt if ntk else dc) + (D + 7) * abs(ts[depth] if ntk else cos(th[depth]))) / top


@functools.lru_cache(maxsize=None)
def points(D):
    """(Z: D x 129, the symmetric block; W: D x 5, the cross pair's columns; Zx: D x 130, its rows -- Z and one more point)"""
    rng = np.random.default_rng(D)
    Z = rng.standard_normal((D, 129))
    Z[:, 0] = 0.0
    Z[0, 0], Z[min(1, D - 1), 0] = (3.0, 4.0) if D > 1 else (5.0, 5.0)      # norm 5 exactly
    Z[:, 1] = Z[:, 0]                                         # bit-coincident
    Z[:, 128] = Z[:, 2]                                       # ... across the tile edge
    Z[:, 3] = Z[:, 4] + 1e-15 * rng.standard_normal(D)        # 1e-15 apart
    Z[:, 5] = -Z[:, 6]                                        # exactly antipodal
    Z[:, 7] = -Z[:, 8] + 1e-9 * rng.standard_normal(D)        # nearly antipodal
    Z[:, 9] = 0.0                                             # norm 0
    Z[:, 10] *= 1e-150 / np.linalg.norm(Z[:, 10])
    Z[:, 11] *= 1e150 / np.linalg.norm(Z[:, 11])
    Z[:, 12] = 2.0 * Z[:, 2]                                  # parallel, another norm
    W = np.stack([Z[:, 2], Z[:, 4] - 1e-15, -Z[:, 6], 0 * Z[:, 0], Z[:, 11]], axis=1)
    return np.asfortranarray(Z), np.asfortranarray(W), np.asfortranarray(np.hstack([Z, rng.standard_normal((D, 1))]))


@functools.lru_cache(maxsize=None)
def truth(D):
    """{(i, j): (n_x n_y, [c_1 .. c_16], [t_1 .. t_16], [theta_0 .. theta_16] and [t_0 .. t_16] as floats for the bound)} in 60
    digits from the definition, for the pairs the value test reads:
    rows SPECIAL and every 5th against every 2nd column of the symmetric block; every pair of the 130 x 5 cross block, keyed
    (i, ~j)"""
    mpmath.mp.dps = 60
    Z, W, Zx = points(D)
    mp = lambda v: [mpmath.mpf(float(a)) for a in v]      # noqa: E731

    def one(x, y):
        nx, ny = mpmath.sqrt(mpmath.fsum(a * a for a in x)), mpmath.sqrt(mpmath.fsum(a * a for a in y))
        c = mpmath.fdot(x, y) / (nx * ny) if nx * ny != 0 else mpmath.mpf(0)
        c = max(min(c, 1), -1)
        t, cs, ts, ths, tf = c, [], [], [], [float(c)]
        for _ in range(16):
            th = mpmath.acos(c)
            k1 = (mpmath.sqrt(1 - c * c) + (mpmath.pi - th) * c) / mpmath.pi
            t, c = k1 + t * (1 - th / mpmath.pi), k1
            cs.append(c), ts.append(t), ths.append(float(th)), tf.append(float(t))
        return nx * ny, cs, ts, ths + [float(mpmath.acos(c))], tf
    cols, Wm = [mp(Zx[:, j]) for j in range(130)], [mp(W[:, j]) for j in range(5)]
    rows = sorted(set(SPECIAL) | set(range(0, 129, 5)))
    out = {(i, j): one(cols[i], cols[j]) for i in rows for j in sorted(set(SPECIAL) | set(range(0, 129, 2)))}
    out.update({(i, ~j): one(cols[i], Wm[j]) for i in range(130) for j in range(5)})
    return out


def call(fn, spec, *args):
    ctx = L.default_context()
    return fn(ctx.handle, spec.ref(ctx), *args)


def matrix(spec):
    K = np.zeros((spec.N, spec.M), order="F")
    assert call(L.load().sgp_kernelmatrix, spec, L.dptr(K), spec.N) == 0, L.last_error()
    return K


def sym_spec(Z, terms, s=None):
    return L.Spec([Z.shape[1]], [Z.shape[1]], [Z], {(0, 0): [(k, 0, 0, c, float(d), s, s) for (k, c, d) in terms]}, True)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("D", [1, 3, 16])
@pytest.mark.parametrize("kind", [L.NNGP, L.NTK])
def test_values_against_60_digits_and_exact_cases(kind, D, depth):
    """MI355X: at most 0.252 of the bound (NNGP, D = 3, L = 2); 0.216 for the NTK (D = 3, L = 1), 0.043 to 0.046 at L = 16"""
    (Z, W, Zx), ref, ntk = points(D), truth(D), kind == L.NTK
    top = depth + 1 if ntk else 1
    s, sx, cw = np.linspace(0.5, 1.5, 129), np.linspace(1.5, 0.5, 130), np.linspace(2.0, 1.0, 5)
    spec = sym_spec(Z, [(kind, -0.75, depth)], s)
    K = matrix(spec)
    Kx = matrix(L.Spec([130], [5], [Zx, W], {(0, 0): [(kind, 0, 1, 1.25, float(depth), sx, cw)]}, False))
    worst = 0.0
    for (i, j), (nn, cs, ts, th, tf) in ref.items():
        got, w = (K[i, j], -0.75 * s[i] * s[j]) if j >= 0 else (Kx[i, ~j], 1.25 * sx[i] * cw[~j])
        want = w * nn * (ts if ntk else cs)[depth - 1]
        frac = float(abs(mpmath.mpf(got) - want) / (bound_units(D, depth, ntk, th, tf) * EPS * abs(w) * nn * top + TINY))
        assert frac <= 1.0, (i, j, got, float(want), frac)
        worst = max(worst, frac)
    print(f"kind {kind} D {D} L {depth}: largest value error / bound = {worst:.3g}")
    diag = np.zeros(129)
    assert call(L.load().sgp_kernelmatrix_diag, spec, L.dptr(diag)) == 0, L.last_error()
    assert np.array_equal(diag, np.diag(K)) and np.array_equal(K, K.T)
    assert np.all(K[9] == 0.0) and np.all(Kx[:, 3] == 0.0) and np.all(Kx[9] == 0.0)      # a point of norm 0: exact zeros
    K1 = matrix(sym_spec(Z, [(kind, 1.0, depth)]))                                     # no weights: the bare n_x n_y T
    same = np.all(Z[:, :, None] == Z[:, None, :], axis=0)
    assert same.sum() >= 129 + 4 and np.array_equal(K1[same], np.broadcast_to(np.diag(K1)[:, None], K1.shape)[same])
    assert K1[0, 1] == 25.0 * top and K[0, 1] == (25.0 * top) * ((-0.75 * s[0]) * s[1])
    if ntk:      # c_l = 1 at every layer: t_L = L + 1 times the NNGP entry, which no depth changes
        N1 = matrix(sym_spec(Z, [(L.NNGP, 1.0, depth)]))
        assert np.array_equal(K1[same], (depth + 1) * N1[same])


@pytest.mark.parametrize("terms", [[(L.NNGP, 1.0, 1), (L.NNGP, 0.5, 2), (L.NNGP, 2.0, 16), (L.NTK, -0.25, 16)],
                                   [(L.NTK, 1.0, 1), (L.NNGP, -0.5, 1), (L.NTK, 2.0, 3), (L.NNGP, 0.25, 3)]])
def test_a_group_is_the_sum_of_its_terms_in_their_order(terms):
    """one launch, one recursion for all depths, against one launch per term.  The coefficients are powers of two, so every
    product is exact and fma(v, coef, acc) is the rounded sum"""
    Z = points(3)[0]
    want = 0.0
    for term in terms:
        want = want + matrix(sym_spec(Z, [term]))
    assert np.array_equal(matrix(sym_spec(Z, terms)), want)


@pytest.mark.parametrize("D,Ln,Lt", [(1, 1, 1), (2, 2, 3), (6, 4, 2), (15, 16, 16)])
def test_host_gradients_against_grad_truth(D, Ln, Lt):
    """(NNGP + NTK) o ARD(a) with a first-layer bias, under Select(perm) o Stretch(diag b): the host's chain back to the user's
    points drops the bias row and carries a, b and the scatter of perm; d_transform is the cotangent of a.  Points 0 and 128
    coincide (sin theta_0 = 0: the NTK's convention) across the tile edge.  MI355X: at most 0.22 of the margin (the input rows at
    D = 6); 0.16 at D = 15, L = 16"""
    n = 129
    rng = np.random.default_rng(100 + D)
    X = np.asfortranarray(rng.standard_normal((D, n)))
    X[:, 128] = X[:, 0]
    a, b, perm = np.linspace(0.8, 1.3, D), np.linspace(1.2, 0.7, D), np.roll(np.arange(D), 1)
    k = (0.7 * P.NNGPKernel(Ln, bias=0.5) + 0.4 * P.NTKKernel(Lt, bias=0.5)) @ P.ARDTransform(a)
    f = P.compose(P.compose(P.atomic(P.GP(k), P.GPC()), P.Select(perm)), P.Stretch(np.diag(b)))
    fx, y = f(P.ColVecs(X), 0.1), np.cos(np.arange(n) * 0.37)
    g = P.logpdf_and_gradient(fx, y, inputs=True)
    assert sorted((int(r["kind"]), r["coef"]) for r in g["terms"]) == [(L.NNGP, 0.7), (L.NTK, 0.4)]
    S = T.read_spec(g["_spec"])
    R, *R64 = (T.logpdf_grad(S, T.NOISE_SCALAR, 0.1, P.mean(fx), y, dt, inputs=True, cholesky=ch, ops=arccos_np)
               for dt, ch in ((T.require_extended(), None), (np.float64, None), (np.float64, T.cholesky_blocked_order)))
    assert abs(P.logpdf(fx, y) - R["value"]) <= 1e-10 * abs(R["value"])
    dev = GT.logpdf_units(GT._logpdf_outputs(g), R)
    e64 = [GT.logpdf_units(GT._reference_outputs(r), R) for r in R64]
    bound = {fam: T.MARGIN * max(max(e[fam] for e in e64), T.FLOORS[fam]) for fam in dev}
    print(f"D {D}:", {fam: (round(dev[fam], 1), round(bound[fam], 1)) for fam in dev})
    assert all(dev[fam] <= bound[fam] for fam in dev)
    (view,) = {r["row_input"] for r in g["terms"]}
    gz, Sz = R["gx"][view][:D], R["Sn_gx"][view][:D]            # the truth in the kernel's coordinates, bias row dropped
    want, Sn = np.zeros((D, n), dtype=gz.dtype), np.zeros((D, n), dtype=gz.dtype)
    want[perm], Sn[perm] = (a * b[perm])[:, None] * gz, (a * b[perm])[:, None] * Sz
    assert g["x"][0].shape == (D, n) and T.units(g["x"][0], want, T.scale_entries(want, Sn)) <= bound["lp.inputs"]
    Xin = (b[:, None] * X)[perm]                                # what the ARD step reads
    want, Sn = (gz * Xin).sum(1), (Sz * np.abs(Xin)).sum(1)
    for r in g["terms"]:
        assert T.units(r["d_transform"], want, T.scale_entries(want, Sn)) <= bound["lp.inputs"]


@pytest.mark.parametrize("D", [3, 16])
def test_c_level_gradients_of_a_six_term_group_without_bias(D):
    """sgp_logpdf_grad_x on one group of 6 terms (the contraction takes them 4 + 2) with an exactly antipodal pair across the tile
    edge (the NTK's convention at l = 0), against grad_truth; sgp_logpdf_grad returns the same grad_coef / grad_inscale bits"""
    n, d = 129, L.dptr
    X = np.asfortranarray(np.random.default_rng(200 + D).standard_normal((D, n)))
    X[:, 128] = -X[:, 0]
    spec = sym_spec(X, [(L.NNGP, 0.5, 1), (L.NTK, 0.3, 1), (L.NNGP, -0.2, 2), (L.NTK, 0.25, 3), (L.NNGP, 0.4, 3), (L.NTK, 0.1, 5)])
    y, m, nz = np.cos(np.arange(n) * 0.37), np.zeros(n), np.array([0.1])
    o = dict(lp=np.zeros(1), gy=np.zeros(n), gm=np.zeros(n), gn=np.zeros(1), gc=np.zeros(6), gs=np.zeros(6), gx=np.zeros((D, n), order="F"))
    head = lambda q: (d(m), 0, d(nz), d(y), d(q["lp"]), d(q["gy"]), d(q["gm"]), d(q["gn"]), d(q["gc"]), d(q["gs"]))      # noqa: E731
    assert call(L.load().sgp_logpdf_grad_x, spec, *head(o), (PD * 1)(d(o["gx"]))) == 0, L.last_error()
    o2 = {k: np.zeros_like(v) for k, v in o.items()}
    assert call(L.load().sgp_logpdf_grad, spec, *head(o2)) == 0, L.last_error()
    assert np.array_equal(o["gc"], o2["gc"]) and np.array_equal(o["gs"], o2["gs"]) and o["lp"][0] == o2["lp"][0]
    S = T.read_spec(spec)
    R, *R64 = (T.logpdf_grad(S, T.NOISE_SCALAR, 0.1, m, y, dt, inputs=True, cholesky=ch, ops=arccos_np)
               for dt, ch in ((T.require_extended(), None), (np.float64, None), (np.float64, T.cholesky_blocked_order)))
    dev = GT.logpdf_units(dict(value=o["lp"][0], y=o["gy"], mean=o["gm"], noise=o["gn"][0], d_coef=o["gc"], d_inscale=o["gs"],
                               gx=[o["gx"]], rowscale=None), R)
    e64 = [GT.logpdf_units(GT._reference_outputs(r), R) for r in R64]
    bound = {fam: T.MARGIN * max(max(e[fam] for e in e64), T.FLOORS[fam]) for fam in dev}
    print(f"D {D}:", {fam: (round(dev[fam], 1), round(bound[fam], 1)) for fam in dev})
    assert all(dev[fam] <= bound[fam] for fam in dev)


def test_logpdf_rand_and_posterior_against_numpy():
    n, D, depth, bias = 200, 3, 4, 0.3
    rng = np.random.default_rng(9)
    X, Xs, y = rng.standard_normal((D, n)), rng.standard_normal((D, 30)), np.sin(np.arange(n) * 0.2)
    f = P.atomic(P.GP(0.6 * P.NNGPKernel(depth, bias=bias) + 0.2 * P.NTKKernel(depth, bias=bias)), P.GPC())

    def dense(A, B):
        A, B = (np.vstack([V, np.full((1, V.shape[1]), np.sqrt(bias))]) for V in (A, B))
        return (0.6 * arccos_np.value(L.NNGP, A, B, depth, LD) + 0.2 * arccos_np.value(L.NTK, A, B, depth, LD)).astype(np.float64)
    Cm = dense(X, X) + 0.1 * np.eye(n)
    Lc = np.linalg.cholesky(Cm)
    z = np.linalg.solve(Lc, y)
    ref = -0.5 * (z @ z + 2 * np.log(np.diag(Lc)).sum() + n * np.log(2 * np.pi))
    fx = f(P.ColVecs(np.asfortranarray(X)), 0.1)
    assert abs(P.logpdf(fx, y) - ref) <= 1e-10 * abs(ref)
    Zd = rng.standard_normal((n, 2))
    draw = Lc @ Zd
    assert np.max(np.abs(P.rand(None, fx, 2, Z=Zd) - draw)) <= 1e-10 * np.max(np.abs(draw))
    V = np.linalg.solve(Lc, dense(X, Xs))
    m, v = P.mean_and_var(P.posterior(fx, y)(P.ColVecs(np.asfortranarray(Xs))))
    assert np.max(np.abs(m - V.T @ z)) <= 1e-10 * np.max(np.abs(V.T @ z))
    var = np.diag(dense(Xs, Xs)) - (V * V).sum(0)
    assert np.max(np.abs(v - var)) <= 1e-10 * np.max(np.abs(np.diag(dense(Xs, Xs))))
    # the batch and pool forms of sgp_logpdf_grad: every member's own call, bit for bit
    fxs, ys = [fx, f(P.ColVecs(np.asfortranarray(X)), 0.2), f(P.ColVecs(np.asfortranarray(Xs)), 0.1)], [y, y, y[:30]]
    own = [P.logpdf_and_gradient(a, b) for a, b in zip(fxs, ys)]
    for got in (P.logpdf_and_gradient_batch(fxs[:2], ys[:2]), P.logpdf_and_gradient_pool(fxs, ys)):
        for o, q in zip(own, got):
            assert o["logpdf"] == q["logpdf"] and all(np.array_equal(a, b) for a, b in zip(o["_raw"], q["_raw"]))


def test_refusals_name_arc_cosine_and_codes_66_to_71_are_unknown():
    n, lib, d, ctx, TP = 16, L.load(), L.dptr, L.default_context(), L.KIND_TIMES_PREV
    Z = {dim: np.asfortranarray(np.random.default_rng(dim).uniform(0.1, 1.0, (dim, n))) for dim in (2, 17)}
    K = np.zeros((n, n), order="F")

    def spec_of(terms, dim=2, reserved=0, symmetric=True, param=2.0):
        sp = L.Spec([n], [n], [Z[dim]], {(0, 0): [(k, 0, 0, 1.0, param, None, None) for k in terms]}, symmetric)
        sp._terms[0].reserved = reserved
        return sp

    def refused(rc, what, word="arc-cosine"):
        assert rc < 0 and word in L.last_error(), (what, rc, L.last_error())

    km = lambda sp: call(lib.sgp_kernelmatrix, sp, d(K), n)      # noqa: E731
    for code in range(66, 72):
        refused(km(spec_of([code])), code, "unknown kernel kind")
    for param in (0.0, 1.5, float("nan"), -1.0, 17.0, 1e30):
        refused(km(spec_of([L.NNGP], param=param)), param)
    for sp in (spec_of([L.NTK], dim=17), spec_of([L.SE, L.NNGP | TP]), spec_of([L.NTK, L.SE | TP]), spec_of([L.NNGP], reserved=1)):
        refused(km(sp), sp)
    spec, cross = spec_of([L.NTK]), spec_of([L.NTK], symmetric=False)
    assert km(spec) == 0
    m, y, nz, lp, w = np.zeros(n), np.ones(n), np.array([0.1]), np.zeros(1), np.ones(n)
    gy, gm, gn, gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1)
    gx, rsc = np.zeros((2, n), order="F"), np.zeros(n)
    ptrs, scl, nulls = (PD * 1)(d(gx)), (PD * 1)(d(rsc)), (PD * 2)()
    head = (d(m), 0, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(gc), d(gs))
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    K32, o32, Zr = np.zeros((n, n), dtype=np.float32, order="F"), np.zeros((n, 1), dtype=np.float32, order="F"), np.zeros((n, 1), order="F")
    assert call(lib.sgp_logpdf_grad_xs, spec, *head, ptrs, None) == 0, L.last_error()
    for where, name, args in [
            (lib, "sgp_logpdf_grad_xs", head + (ptrs, scl)), (ctx.kprod, "sgp_logpdf_grad_param", head + (d(gp),)),
            (ctx.kprod_grad, "sgp_logpdf_grad_param_xs", head + (d(gp), ptrs, nulls)), (ctx.conv_grad, "sgp_logpdf_grad_conv", head),
            (ctx.stencil_grad, "sgp_logpdf_grad_stencil", head + (ptrs,)),
            (ctx.stencil_wo, "sgp_logpdf_grad_stencil_wo", head + (ptrs, nulls, nulls)),
            (lib, "sgp_kernelmatrix_diag_grad", (d(w), d(gc), d(gs))), (lib, "sgp_kernelmatrix_diag_grad_x", (d(w), d(gc), d(gs), ptrs)),
            (lib, "sgp_kernelmatrix_f32", (f32(K32), n)), (lib, "sgp_logpdf_f32", (d(m), 0, d(nz), d(y), d(lp))),
            (lib, "sgp_rand_f32", (d(m), 0, d(nz), d(Zr), n, 1, f32(o32), n)),
            (lib, "sgp_posterior_mean_var_f32", (d(m), 0, d(nz), d(y), cross.ref(ctx), spec.ref(ctx), d(m), f32(o32), f32(o32))),
            (lib, "sgp_elbo_grad", (cross.ref(ctx), d(w), d(m), 0, d(nz), 0, d(nz), d(y), d(lp), d(gy), d(gm), d(gn), d(rsc), d(gp),
                                    d(gc), d(gs), d(gc), d(gs)))]:
        refused(call(getattr(where, name), spec, *args), name)
    g = P.atomic(P.GP(P.NTKKernel(2, bias=1.0)), P.GPC())      # the prediction gradients against kept factors of the host's making
    xh = np.linspace(-1.0, 1.0, n)
    fx = g(xh, 0.1)
    for post in (P.posterior(fx, y), P.posterior(P.VFE(g(xh[::2], 1e-6)), fx, y)):
        fn = getattr(ctx.predgrad, post._stem + "_predict_grad_x")
        refused(fn(post._ensure(), cross.ref(ctx), spec.ref(ctx), d(m), d(gy), d(gm), None, None, None), post._stem)
