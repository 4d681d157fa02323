"""Every product-chain gradient kernel instantiation (stheno.jl_amd/csrc/kprod.hip) against an extended-precision truth
(tests/kprod_grad_truth.py), through the host mirror where it reaches (P.logpdf_and_gradient_param,
P.elbo_and_gradient_param with inputs=True) and through the C entry points where it does not (the diagonal with the caller's
w, NULL outputs).

Each case asserts the value, y, mean, noise, every term's d_coef / d_inscale / d_param (the raw records) and every entry of
every input and scale gradient.  Errors are counted in eps = 2^-53 times a scale taken from the truth; the bound of a case and
output family is MARGIN * max(e_float64 of the case, the family's floor), e_float64 the larger of the column-order and the
blocked-order float64 run of the same restatement -- it comes from the reference, never from the device
(docs/04_oracle_and_parity.md, "Product-chain gradients against the same kind of truth").  The diagonal's bound is the model
stated in tests/kprod_grad_truth.py.  Problems are well conditioned (noise 0.05 .. 0.3, total prior variance about 1, inputs
standard_normal / sqrt(D) * 1.5, Sigma_z = 1e-2; Cosine and Linear factors always beside a decaying one): the CPU file
(tests/test_kprod_grad_truth_on_numpy.py) caps cond(K + Sigma_y) at 1e4 and cond(Kzz + Sigma_z) at 1e6.

Shapes: block lengths (129, 1, 128, 70), N = 328, for every multi-block case; single blocks of 1, 128 and 257; the ELBO has
inducing blocks (33, 1, 70) against data blocks (129, 70, 131).

    what                                                                  cases
    grad_kprod_kernel<1>, <2>, <4>, <8>, <16>, MN = false                 kp-D1-nf2, kp-D2-nf3, kp-D3-nf3, kp-D5-nf2 and
                                                                          kp-D8-nf3, kp-D9-nf2 and kp-D16-nf3
    the same five with MN = true                                          kp-mn-D1 (nu 0.3), -D2 (1.25), -D3 (3.7), -D5 (0.3),
                                                                          -D8 (1.25), -D9 (32), -D16 (3.7)
    factors x DMAX = 64 exactly                                           kp-lim-8x8, kp-lim-4x16, kp-lim-8x5
    factors of different dimension in one chain (d < T.dim zero fill)     kp-select-D5 (views of 1, 2 and 5 coordinates)
    a pair whose chains do not fit one assembly launch (kprod_group cut)  kp-D16-nf3 (two chains of three at D = 16)
    a plain term, a chain, a chain of one; SGP_CONST's d / d param        kp-D1-nf2, kp-D5-nf2, kp-D9-nf2
    grad_kprod_inputs_kernel<DMAX, 0> for all five DMAX                   the kp-D* cases (every case asks for the inputs)
    grad_kprod_inputs_kernel<DMAX, 1>                                     kp-cg-D1, -D2, -D3, -D5, -D9 (Cosine / GammaExp)
    grad_kprod_inputs_kernel<DMAX, 2>                                     the kp-mn-D* cases (D = 8 and 16 among them)
    head with a row scale, a column scale, both, neither; gsv             kp-scaled-D3, kp-scaled-mn-D2, kp-scaled-D9
    LINEAR first, middle, last; two LINEAR factors (Polynomial 2)         kp-D8-nf3, kp-D2-nf3, kp-D3-nf3; kp-D16-nf3 and kp-lim-8x5
    coincident points inside a block and across blocks                    kp-coin-rq, -cosine, -gammaexp, -mn1.25, -mn0.3
    single blocks of 1, 128 and 257 rows                                  kp-single-N1, -N128, -N257
    Periodic (host: SE on the sin / cos embedding, 8 coordinates at D = 4)  kp-periodic-D4
    ELBO: alpha == nullptr, both strides, rectangular pairs,              kpelbo-D1, -D5 (dense Sigma_z), -D16 and
    grad_inputs_zz, xz both sides, gsr / gsc                              kpelbo-mn-D1, -D5, -D16 (function-scaled models)
    diag_grad_kprod_kernel<false> / <true>, plain and two views           kpdiag-D1-plain, -D8-plain (MN), -D16-plain,
                                                                          kpdiag-D1-views (MN), -D8-views, -D16-views (MN)
    NULL grad_param, NULL grad_inputs, NULL scale outputs                 test_null_outputs_leave_the_others_bit_equal
    grad_kprod_reduce_kernel with more than 256 partials                  kpelbo-partials

kpelbo-partials: sgp_elbo_grad_param contracts the cross block K(x, z) of one block pair in one grid (capi.hip: contract_spec,
trc x tcc tiles of the pair), so 16 400 data points in one block against 129 inducing points in one block leave 129 x 2 = 258
partials for grad_kprod_reduce_kernel's strided loop; the partials buffer holds rup(N) / 128 x rup(M) / 128 x 24 doubles
(contract_spec's `need`).  Its truth is the long-double run like every other case's (O(N M^2), M = 129).

The bodies re-run on the NumPy double of the entry points in tests/test_kprod_grad_truth_on_numpy.py."""
import ctypes as C

import numpy as np
import pytest

import kprod_grad_truth as KT
import stheno_jl_amd as P
from stheno_jl_amd import lib as L

pytestmark = pytest.mark.gpu

LAYOUT = (129, 1, 128, 70)
Z_LAYOUT, X_LAYOUT = (33, 1, 70), (129, 70, 131)
MARGIN_IN_FORCE = KT.MARGIN            # the CPU file runs the bodies under SELF_MARGIN
wl = P.with_lengthscale
SE, M12, M32, M52 = P.SEKernel, P.Matern12Kernel, P.Matern32Kernel, P.Matern52Kernel
RQ, LIN, COS, GEXP, GM, CONST = (P.RationalQuadraticKernel, P.LinearKernel, P.CosineKernel, P.GammaExponentialKernel,
                                 P.GeneralMaternKernel, P.ConstantKernel)


def _cos(s, coord=0):
    """cos(pi s |x_c - x'_c|): the Cosine kernel is positive definite on a line only, so it reads one coordinate (as the
    spectral mixtures' 1-D projections do)"""
    return (COS() @ P.ScaleTransform(s)) @ P.SelectTransform([coord])


# ---- kernels (total prior variance about 1 at these inputs) -------------------------------------------------------------------
def k_nf2():
    """a chain, a plain term, a chain of one and a constant: four classes of launch in one pair"""
    return 0.5 * wl(SE(), 1.3) * M32() + 0.2 * M52() + 0.2 * RQ(0.7) + 0.1 * CONST(0.7)


def k_lin_first():
    return 0.25 * LIN(0.4) * wl(SE(), 1.2) * wl(M32(), 1.5) + 0.5 * wl(M52(), 0.8) * RQ(0.9) * wl(SE(), 2.0)


def k_lin_middle():
    return 0.25 * wl(M52(), 0.8) * LIN(0.5) * RQ(0.9) + 0.5 * wl(SE(), 1.1) * wl(M12(), 2.5) * RQ(1.4)


def k_lin_last():
    return 0.25 * wl(SE(), 1.0) * wl(M12(), 1.5) * LIN(0.2) + 0.5 * RQ(0.7) * wl(M32(), 1.2) * wl(SE(), 1.8)


def k_two_chains_of_three():
    """at D = 16 they do not fit one assembly launch (6 x 16 > 64); Polynomial(2, c): two LINEAR factors"""
    return 0.5 * wl(M52(), 0.8) * RQ(0.7) * wl(SE(), 1.5) + 0.05 * P.PolynomialKernel(2, 0.5) * wl(SE(), 1.0)


def k_eight():
    return 0.3 * (wl(SE(), 2.0) * wl(M12(), 3.0) * wl(M32(), 2.5) * M52() * RQ(1.3) * LIN(1.0) * CONST(1.1) * wl(SE(), 4.0))


def k_eight_poly():
    return 0.05 * (wl(SE(), 2.0) * wl(M12(), 3.0) * wl(M32(), 2.5) * RQ(1.3) * P.PolynomialKernel(2, 0.8) * _cos(0.3) *
                  wl(GEXP(1.4), 3.0))


def k_four():
    return 0.4 * wl(SE(), 2.0) * RQ(0.7) * LIN(0.5) * wl(M32(), 1.5)


def k_select():
    """views of 1, 2 and 5 coordinates in ONE chain: DMAX = 8, the narrow factors zero-filled"""
    return (0.6 * (SE() @ P.SelectTransform([2])) * (M32() @ P.SelectTransform([0, 3])) * wl(RQ(0.9), 1.5) +
            0.4 * (wl(M52(), 0.7) @ P.SelectTransform([1, 4])) * wl(SE(), 1.4))


def k_cg():
    """Cosine and GammaExponential chains without kind 20 (NK = 1)"""
    return 0.6 * wl(SE(), 1.2) * _cos(0.5) + 0.4 * wl(GEXP(1.3), 1.1) * wl(M32(), 2.0)


def k_mn(nu):
    """a kind-20 factor in every chain (MN = true, NK = 2)"""
    return 0.6 * wl(GM(nu), 1.1) * wl(SE(), 1.6) + 0.4 * wl(GEXP(1.5), 1.2) * wl(GM(nu), 2.0) * _cos(0.3)


def k_scaled():
    return 0.7 * SE() * wl(RQ(0.9), 1.2) + 0.15 * LIN(0.4) * M32()


def k_scaled_line():
    """k_scaled with the lengthscales of points on a line (D = 1: 104 inducing points within a few units of each other)"""
    return 0.7 * wl(SE(), 0.5) * wl(RQ(0.9), 0.4) + 0.15 * LIN(0.4) * wl(M32(), 0.4)


def k_periodic():
    """PeriodicKernel is flattened on the host into an SE factor on the sin / cos embedding of every coordinate (D = 4: a view
    of 8 coordinates beside factors of 4 under DMAX = 8)"""
    return 0.6 * P.PeriodicKernel(1.5) * wl(SE(), 1.4) + 0.4 * wl(M32(), 1.2) * RQ(0.9)


def k_scaled_mn():
    return 0.7 * wl(GM(1.25), 1.2) * wl(SE(), 1.5) + 0.3 * wl(GEXP(1.2), 1.4) * _cos(0.4)


COIN = {"rq": lambda: 0.6 * RQ(0.8) * wl(SE(), 1.5) + 0.4 * wl(RQ(1.6), 0.9),
        "cosine": lambda: 0.6 * wl(SE(), 1.2) * _cos(0.6) + 0.4 * wl(M52(), 1.1) * _cos(0.3),
        "gammaexp": lambda: 0.6 * GEXP(1.3) * wl(SE(), 1.5) + 0.4 * wl(GEXP(0.7), 1.4),
        "mn1.25": lambda: 0.6 * GM(1.25) * wl(SE(), 1.5) + 0.4 * wl(GM(2.2), 0.9),
        "mn0.3": lambda: 0.6 * GM(0.3) * wl(SE(), 1.5) + 0.4 * wl(GM(0.75), 1.3) * wl(M12(), 2.0)}


# ---- models ------------------------------------------------------------------------------------------------------------------
def _sigma(pt):
    return 1.0 + 0.3 * float(np.sin(np.sum(pt)))


def _plain(kernel):
    return P.gppp(lambda GP: {"f": GP(kernel)}), ("f",) * 4


def _scaled(kernel):
    """blocks g f g f: heads with a row scale, a column scale, both and neither"""
    return P.gppp(lambda GP: (lambda f: {"f": f, "g": _sigma * f})(GP(kernel))), ("g", "f", "g", "f")


def _two_views(kernel):
    """var(f(a x) + f(b x)): the cross terms of the diagonal read two different views of x; a function scale on top"""
    return (P.gppp(lambda GP: (lambda f: {"f": f, "g": _sigma * (np.sqrt(0.5) * P.stretch(f, 0.7) + np.sqrt(0.5) * P.stretch(f, 1.3))})
                   (GP(kernel))), ("g", "f", "g", "f"))


class Case:
    def __init__(self, id, D, kernel, model=_plain, layout=LAYOUT, z_noise="scalar", coincident=False, x_layout=X_LAYOUT,
                 z_layout=Z_LAYOUT, noise=None):
        self.id, self.D, self.kernel, self.model, self.layout = id, D, kernel, model, layout
        self.z_noise, self.coincident, self.x_layout, self.z_layout, self.noise = z_noise, coincident, x_layout, z_layout, noise

    def __repr__(self):
        return self.id


LP_CASES = [Case("kp-D1-nf2", 1, k_nf2), Case("kp-D2-nf3", 2, k_lin_middle), Case("kp-D3-nf3", 3, k_lin_last),
            Case("kp-D5-nf2", 5, k_nf2), Case("kp-D8-nf3", 8, k_lin_first), Case("kp-D9-nf2", 9, k_nf2),
            Case("kp-D16-nf3", 16, k_two_chains_of_three)]
for _D, _nu in ((1, 0.3), (2, 1.25), (3, 3.7), (5, 0.3), (8, 1.25), (9, 32.0), (16, 3.7)):
    LP_CASES.append(Case(f"kp-mn-D{_D}", _D, (lambda nu=_nu: k_mn(nu))))
LP_CASES += [Case("kp-lim-8x8", 8, k_eight), Case("kp-lim-4x16", 16, k_four), Case("kp-lim-8x5", 5, k_eight_poly),
             Case("kp-select-D5", 5, k_select)]
for _D in (1, 2, 3, 5, 9):
    LP_CASES.append(Case(f"kp-cg-D{_D}", _D, k_cg))
LP_CASES += [Case("kp-scaled-D3", 3, k_scaled, model=_scaled), Case("kp-scaled-mn-D2", 2, k_scaled_mn, model=_scaled)]
for _name in COIN:
    LP_CASES.append(Case(f"kp-coin-{_name}", 3, COIN[_name], coincident=True))
for _n, _k in ((1, k_nf2), (128, k_lin_last), (257, k_cg)):
    LP_CASES.append(Case(f"kp-single-N{_n}", 3, _k, layout=(_n,)))
ELBO_CASES = [Case("kpelbo-D1", 1, k_scaled_line, model=_scaled), Case("kpelbo-D5", 5, k_lin_middle, model=_scaled, z_noise="dense"),
              Case("kpelbo-D16", 16, k_four, model=_scaled),
              Case("kpelbo-mn-D1", 1, (lambda: k_mn(0.3)), model=_scaled),
              Case("kpelbo-mn-D5", 5, (lambda: k_mn(1.25)), model=_scaled, z_noise="dense"),
              Case("kpelbo-mn-D16", 16, k_scaled_mn, model=_scaled),
              Case("kpelbo-partials", 2, (lambda: 0.6 * wl(SE(), 1.0) * wl(RQ(0.9), 1.5) + 0.4 * wl(M32(), 1.2) * wl(SE(), 2.0)),
                   x_layout=(16400,), z_layout=(129,), noise=0.2)]
DIAG_CASES = [Case("kpdiag-D1-plain", 1, k_scaled, model=_scaled), Case("kpdiag-D8-plain", 8, k_scaled_mn, model=_scaled),
              Case("kpdiag-D16-plain", 16, k_four, model=_scaled),
              Case("kpdiag-D1-views", 1, (lambda: k_mn(0.3)), model=_two_views),
              Case("kpdiag-D8-views", 8, k_lin_first, model=_two_views),
              Case("kpdiag-D16-views", 16, (lambda: k_mn(3.7)), model=_two_views)]
ALL_CASES = LP_CASES + ELBO_CASES + DIAG_CASES        # a case's seed is its position here: additions go at the end


def _add_later(cases, case):
    """a case added after the list was first recorded: into its family's list and at the end of ALL_CASES, in one step, so
    that every earlier case keeps its seed"""
    cases.append(case)
    ALL_CASES.append(case)


_add_later(LP_CASES, Case("kp-scaled-D9", 9, k_scaled, model=_scaled))          # the row-scale sums under DMAX = 16
_add_later(LP_CASES, Case("kp-periodic-D4", 4, k_periodic))                     # Periodic through the mirror: SE on the embedding


def _rng(case):
    return np.random.default_rng(7000 + ALL_CASES.index(case))


def _points(rng, D, layout, coincident=False):
    n = sum(layout)
    X = rng.standard_normal((D, n)) / np.sqrt(D) * 1.5
    if coincident:          # a third of the points are copies: the last third of the first third (across blocks), and inside
        third = n // 3      # the first block
        X[:, n - third:] = X[:, :third]
        X[:, 100:129] = X[:, :29]
    off = np.concatenate([[0], np.cumsum(layout)])
    return [np.asfortranarray(X[:, off[i]:off[i + 1]]) for i in range(len(layout))]


def _blocks(names, xs):
    return P.BlockData([P.GPPPInput(k, P.ColVecs(x)) for k, x in zip(names, xs)])


# ---- running a case on whatever library is loaded, and on the reference -------------------------------------------------------
_TRUTH = {}          # case id -> (truth in long double, the two float64 runs): computed once, shared, never modified


def _RUNS():
    return ((KT.require_extended(), None), (np.float64, None), (np.float64, KT.cholesky_blocked_order))


def logpdf_problem(case):
    rng = _rng(case)
    F, names = case.model(case.kernel())
    xs = _points(rng, case.D, case.layout, case.coincident)
    n = sum(case.layout)
    noise = float(0.05 + 0.25 * rng.random())
    x = _blocks(names[:len(case.layout)], xs)
    return F, x, noise, rng.standard_normal(n)


def logpdf_truth(case):
    if case.id not in _TRUTH:
        F, x, noise, y = logpdf_problem(case)
        S = KT.read_spec(P.build_spec(F, x)[0])
        fx = F(x, noise)
        _TRUTH[case.id] = tuple(KT.logpdf_grad(S, KT.NOISE_SCALAR, noise, P.mean(fx), y, dt, inputs=True, scales=True, cholesky=ch)
                                for dt, ch in _RUNS())
    return _TRUTH[case.id]


def run_logpdf(case):
    F, x, noise, y = logpdf_problem(case)
    g = P.logpdf_and_gradient_param(F(x, noise), y, inputs=True, scales=True)
    return g, logpdf_truth(case)


def _logpdf_outputs(g):
    gc, gs, gp = g["_raw"]
    nt = g["_spec"].n_terms
    return dict(value=g["logpdf"], y=g["y"], mean=g["mean"], noise=g["noise"], d_coef=gc[:nt], d_inscale=gs[:nt], d_param=gp[:nt],
                gx=g["inputs"], rowscale=g["_rowscale"])


def yardstick(runs):
    """e_float64 of a case: family by family the larger figure of the float64 runs"""
    runs = list(runs)
    return {fam: max(r[fam] for r in runs) for fam in runs[0]}


def hold(case, dev, f64):
    """the verdict: every family's figure inside MARGIN * max(float64 figure, floor); figures printed first"""
    m = MARGIN_IN_FORCE
    for fam in sorted(dev):
        print(f"{case.id:18s} {fam:16s} device {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {KT.FLOORS[fam]:8.1f}")
    bad = {fam: (dev[fam], f64[fam]) for fam in dev if not dev[fam] <= m * max(f64[fam], KT.FLOORS[fam])}
    assert not bad, (case.id, bad)


def _finite(vals):
    for v in vals:
        if v is not None:
            assert not np.any(np.isnan(v))


@pytest.mark.parametrize("case", LP_CASES, ids=repr)
def test_logpdf_gradient_against_truth(case):
    g, (R, *R64) = run_logpdf(case)
    out = _logpdf_outputs(g)
    assert g["_spec"].has_kprod and g["_spec"].n_terms == len(R["d_coef"])
    _finite([out["value"], out["y"], out["mean"], out["noise"], out["d_coef"], out["d_inscale"], out["d_param"]] + list(out["gx"]))
    dev = KT.logpdf_units(out, R)
    assert ("kp.scales" in dev) == (case.model is _scaled)
    hold(case, dev, yardstick(KT.logpdf_units(KT.logpdf_reference_outputs(r), R) for r in R64))


# ---- NULL outputs through the C entry point ------------------------------------------------------------------------------------------
PD = C.POINTER(C.c_double)


def _ptrs(arrs, n=None):
    arrs = list(arrs) + [None] * ((n or 0) - len(arrs))
    return (PD * max(1, len(arrs)))(*[L.dptr(a) if a is not None else None for a in arrs])


def _scale_bufs(spec, side, n):
    vecs = spec.term_row_scale if side == "row" else spec.term_col_scale
    return [np.zeros(len(v)) if v is not None else None for v in vecs] + [None] * (n - len(vecs))


def test_null_outputs_leave_the_others_bit_equal():
    """sgp_logpdf_grad_param_xs with NULL grad_param, NULL grad_inputs and NULL scale outputs, then with NULL y / mean / noise /
    coef / inscale outputs: what is still asked for is bit for bit what the full call (held to the truth above) returns"""
    case = LP_CASES[[c.id for c in LP_CASES].index("kp-scaled-mn-D2")]
    F, x, noise, y = logpdf_problem(case)
    full = _logpdf_outputs(P.logpdf_and_gradient_param(F(x, noise), y, inputs=True, scales=True))
    spec, _, _ = P.build_spec(F, x)
    ctx, d = L.default_context(), L.dptr
    n, nt = spec.N, max(1, spec.n_terms)
    m, nz, yv = np.zeros(n), np.array([noise]), np.ascontiguousarray(y)
    lp, gy, gm, gn, gc, gs = np.zeros(1), np.zeros(n), np.zeros(n), np.zeros(1), np.zeros(nt), np.zeros(nt)
    rc = L.kprod_grad_lib().sgp_logpdf_grad_param_xs(ctx.handle, spec.ref(ctx), d(m), L.NOISE_SCALAR, d(nz), d(yv), d(lp), d(gy),
                                                     d(gm), d(gn), d(gc), d(gs), None, None, None)
    assert rc == 0, L.last_error()
    assert lp[0] == full["value"] and gn[0] == full["noise"]
    assert np.array_equal(gy, full["y"]) and np.array_equal(gm, full["mean"])
    assert np.array_equal(gc[:spec.n_terms], full["d_coef"]) and np.array_equal(gs[:spec.n_terms], full["d_inscale"])
    lp2, gp = np.zeros(1), np.zeros(nt)
    gx = [np.zeros(np.asarray(a).shape, order="F") for a in spec.inputs]
    grs = _scale_bufs(spec, "row", nt)
    rc = L.kprod_grad_lib().sgp_logpdf_grad_param_xs(ctx.handle, spec.ref(ctx), None, L.NOISE_SCALAR, d(nz), d(yv), d(lp2), None,
                                                     None, None, None, None, d(gp), _ptrs(gx), _ptrs(grs, nt))
    assert rc == 0, L.last_error()
    assert lp2[0] == full["value"] and np.array_equal(gp[:spec.n_terms], full["d_param"])
    for a, b in zip(gx, full["gx"]):
        assert np.array_equal(a, b)
    seen = 0
    for a, b in zip(grs, full["rowscale"]):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, b)
            seen += 1
    assert seen >= 1


# ---- ELBO ----------------------------------------------------------------------------------------------------------------
def elbo_problem(case):
    rng = _rng(case)
    F, names = case.model(case.kernel())
    xs = _points(rng, case.D, case.x_layout)
    zs = _points(rng, case.D, case.z_layout)
    n, m = sum(case.x_layout), sum(case.z_layout)
    if case.z_noise == "dense":
        Q = rng.standard_normal((m, m))
        sz = np.asfortranarray(1e-2 * np.eye(m) + 1e-2 * (Q @ Q.T) / m)
    else:
        sz = 1e-2
    noise = case.noise if case.noise is not None else float(0.05 + 0.25 * rng.random())
    x, z = _blocks(names[:len(case.x_layout)], xs), _blocks(names[:len(case.z_layout)], zs)
    return F, x, z, noise, sz, rng.standard_normal(n)


def elbo_truth(case):
    if case.id not in _TRUTH:
        F, x, z, noise, sz, y = elbo_problem(case)
        Szz, Sxz, Sxx = (KT.read_spec(sp) for sp in (P.build_spec(F, z)[0], P.build_spec(F, x, None, z)[0], P.build_spec(F, x)[0]))
        tag = KT.NOISE_DENSE if case.z_noise == "dense" else KT.NOISE_SCALAR
        fx = F(x, noise)
        _TRUTH[case.id] = tuple(KT.elbo_grad(Szz, Sxz, Sxx, KT.NOISE_SCALAR, noise, tag, sz, P.mean(fx), y, dt, inputs=True,
                                             cholesky=ch) for dt, ch in _RUNS())
    return _TRUTH[case.id]


def run_elbo(case):
    F, x, z, noise, sz, y = elbo_problem(case)
    g = P.elbo_and_gradient_param(P.VFE(F(z, sz)), F(x, noise), y, inputs=True, scales=True)
    return g, elbo_truth(case)


def _elbo_outputs(g):
    nt = {k: g["_specs"][k].n_terms for k in ("zz", "xz", "xx")}
    S = g["_scale_arrays"]
    side = lambda k, rs, cs: dict(d_coef=g["_raw"][k][0][:nt[k]], d_inscale=g["_raw"][k][1][:nt[k]],      # noqa: E731
                                  d_param=g["_raw"][k][2][:nt[k]], rowscale=rs, colscale=cs)
    return dict(value=g["elbo"], y=g["y"], mean=g["mean"], noise=g["noise"], z_noise=g["z_noise"], var=g["var"],
                zz=dict(side("zz", S[0], None), gx=g["zz_inputs"]), xz=dict(side("xz", S[1], S[2]), gx=g["xz_inputs"]),
                xx=dict(side("xx", S[3], S[4]), gx=g["_xx_inputs"]))


def hold_diag(case, fig):
    for fam in sorted(fig):
        print(f"{case.id:18s} {fam:16s} error / model bound = {fig[fam]:.3f}")
    assert all(v <= 1.0 for v in fig.values()), (case.id, fig)


@pytest.mark.parametrize("case", ELBO_CASES, ids=repr)
def test_elbo_gradient_against_truth(case):
    g, (R, *R64) = run_elbo(case)
    out = _elbo_outputs(g)
    assert all(sp.has_kprod for sp in g["_specs"].values())
    flat = [out["value"], out["y"], out["mean"], out["noise"], out["z_noise"], out["var"]]
    for key in ("zz", "xz"):
        flat += [out[key]["d_coef"], out[key]["d_inscale"], out[key]["d_param"]] + list(out[key]["gx"])
    _finite(flat)
    assert np.max(np.abs(out["var"] - R["var"]) / np.abs(R["var"])) <= 2 * KT.EPS      # -1 / (2 sy): one division
    dev = KT.elbo_units(out, R)
    assert ("kpelbo.scales" in dev) == (case.model is _scaled)
    hold(case, dev, yardstick(KT.elbo_units(KT.elbo_reference_outputs(r), R) for r in R64))
    hold_diag(case, KT.diag_model_figures(out["xx"], R["xx"]))


# ---- sgp_kernelmatrix_diag_grad_param with the caller's w ----------------------------------------------------------------------
def run_diag(case):
    rng = _rng(case)
    F, names = case.model(case.kernel())
    xs = _points(rng, case.D, LAYOUT)
    spec, _, _ = P.build_spec(F, _blocks(names, xs))
    w = np.ascontiguousarray(rng.standard_normal(spec.N))
    ctx, d = L.default_context(), L.dptr
    nt = max(1, spec.n_terms)
    o = dict(d_coef=np.full(nt, np.nan), d_inscale=np.full(nt, np.nan), d_param=np.full(nt, np.nan),
             gx=[np.zeros(np.asarray(a).shape, order="F") for a in spec.inputs],
             rowscale=_scale_bufs(spec, "row", nt), colscale=_scale_bufs(spec, "col", nt))
    rc = ctx.kprod_grad.sgp_kernelmatrix_diag_grad_param(ctx.handle, spec.ref(ctx), d(w), d(o["d_coef"]), d(o["d_inscale"]),
                                                         d(o["d_param"]), _ptrs(o["gx"]), _ptrs(o["rowscale"], nt),
                                                         _ptrs(o["colscale"], nt))
    assert rc == 0, L.last_error()
    for key in ("d_coef", "d_inscale", "d_param"):
        o[key] = o[key][:spec.n_terms]
    if case.id not in _TRUTH:
        _TRUTH[case.id] = (KT.diag_grad(KT.read_spec(spec), w, KT.require_extended()),)
    return spec, o, _TRUTH[case.id][0]


@pytest.mark.parametrize("case", DIAG_CASES, ids=repr)
def test_diag_gradient_against_truth(case):
    spec, o, R = run_diag(case)
    assert spec.has_kprod and R["diagonal"].any() and not R["diagonal"].all()
    _finite([o["d_coef"], o["d_inscale"], o["d_param"]] + o["gx"])
    mn = any(kind == KT.MATERN_NU for ch in KT.read_spec(spec)["chains"] for (_, kind, _, _, _) in ch["factors"])
    assert mn == (case.id in ("kpdiag-D8-plain", "kpdiag-D1-views", "kpdiag-D16-views"))
    fig = KT.diag_model_figures(o, R)
    assert "kpdiag.scales" in fig
    if case.model is _two_views:
        assert any(np.max(np.abs(e)) > 1e-3 for e in R["gx"])      # the distance kinds do not cancel between two views
    hold_diag(case, fig)
