"""Extended-precision truth for sgp_logpdf_grad through derivative terms (include/sthenomi.h: SGP_DERIV_*), on top of
tests/grad_truth.py (imported, not edited).  TEST INFRASTRUCTURE ONLY.

`dense` and `contract` below are the `ops` of grad_truth.logpdf_grad for a spec that may hold derivative terms: the
plain terms go through grad_truth.kappa, a derivative term through `term`, a dtype-generic statement of the header's
DEFINITIONS in kappa', kappa'' and kappa''' of the base kernel -- not the library's (A, B, GA, GB, GC) forms, nothing of
tests/deriv_np.py, no clamp, no rescaling.  Run in np.longdouble it is the truth, run in np.float64 (with the column
recurrence and with LAPACK's blocked order of the factorisation) it is the yardstick e_float64.  The bound of every output
family is the project's: MARGIN x max(e_float64 of the case, floor), in units of 2^-53 of grad_truth's scales, the floors
being the medians of the float64 figures over the final case list (CASES below) -- measured on the CPU by
`python tests/test_deriv_truth_on_numpy.py`, which prints the two dicts that follow."""
import numpy as np

import grad_truth as T

DERIV_SE, DERIV_M32, DERIV_M52 = 32, 34, 35
PARAM_BASE = 17

# the sorted float64 figures of CASES per family, and their medians (python tests/test_deriv_truth_on_numpy.py)
MEASURED_FLOAT64 = {'value': [3.0, 5.3, 9.7, 10.7, 16.4, 23.8],
                    'y': [39.9, 73.1, 77.2, 87.6, 91.8, 147.8],
                    'noise': [11.8, 38.7, 38.8, 57.8, 60.5, 85.4],
                    'd_coef': [89.3, 104.4, 145.2, 163.6, 220.8, 223.0],
                    'd_inscale': [60.0, 89.6, 94.6, 167.6, 181.6, 183.7]}
FLOORS = {fam: float(np.median(v)) for fam, v in MEASURED_FLOAT64.items()}


def is_deriv(kind):
    return int(kind) in (DERIV_SE, DERIV_M32, DERIV_M52)


def kappa_derivatives(kind, s, dt):
    """(kappa', kappa'', kappa''') of the base kernel at s > 0, in dtype dt; at s == 0 the entries that do not exist are 0 and
    `term` does not read them"""
    s = np.asarray(s, dtype=dt)
    pos = s > 0
    safe = np.where(pos, s, dt(1))
    if kind == DERIV_SE:
        E = np.exp(-s / dt(2))
        return -E / dt(2), E / dt(4), -E / dt(8)
    r = np.sqrt(safe)
    if kind == DERIV_M32:
        q = np.sqrt(dt(3))
        E = np.exp(-q * np.sqrt(s))
        k2 = np.where(pos, dt(3) * q / dt(4) * E / r, dt(0))
        k3 = np.where(pos, -dt(3) * q / dt(8) * E * (q * r + dt(1)) / (r * safe), dt(0))
        return -dt(3) / dt(2) * E, k2, k3
    q = np.sqrt(dt(5))
    l = q * np.sqrt(s)
    E = np.exp(-l)
    k3 = np.where(pos, -dt(25) * q / dt(24) * E / r, dt(0))
    return -dt(5) / dt(6) * (dt(1) + l) * E, dt(25) / dt(12) * E, k3


def term(kind, param, X, Y, dt):
    """(value, input-scale derivative at g = 1) of a derivative term per pair of points, as include/sthenomi.h defines them:
         (p+1, 0)    2 k' u_p                          (4 s k'' + 2 k') u_p
         (0, q+1)   -2 k' u_q                         -(4 s k'' + 2 k') u_q
         (p+1, q+1) -4 k'' u_p u_q - 2 k' delta_pq    -8 s k''' u_p u_q - 8 k'' u_p u_q - 4 s k'' delta_pq
    with the limits at a coincident pair (u = 0): 0, 0 and -2 k'(0) delta_pq; every input-scale derivative 0"""
    a, b = divmod(int(param), PARAM_BASE)
    u = X[:, :, None] - Y[:, None, :]
    s = np.zeros(u.shape[1:], dtype=dt)
    for d in range(u.shape[0]):
        s = s + u[d] * u[d]
    k1, k2, k3 = kappa_derivatives(int(kind), s, dt)
    two, four, eight = dt(2), dt(4), dt(8)
    if b == 0 or a == 0:
        sign, uu = (dt(1), u[a - 1]) if b == 0 else (dt(-1), u[b - 1])
        return sign * two * k1 * uu, sign * (four * s * k2 + two * k1) * uu
    up, uq = u[a - 1], u[b - 1]
    same = dt(1) if a == b else dt(0)
    val = -four * k2 * up * uq - two * k1 * same
    dval = -eight * s * k3 * up * uq - eight * k2 * up * uq - four * s * k2 * same
    return val, dval


def _values(kind, param, X, Y, dt):
    if is_deriv(kind):
        return term(kind, param, X, Y, dt)
    k, _, dk = T.kappa(kind, T.sqdist(X, Y), param, dt)
    return k, dk


def dense(S, dt):
    terms, inputs = T._cast(S, dt)
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    coff = np.concatenate([[0], np.cumsum(S["col_len"])]).astype(int)
    K = np.zeros((roff[-1], coff[-1]), dtype=dt)
    for (I, J, kind, ri, ci, coef, param, rs, cs) in terms:
        blk = coef * _values(kind, param, inputs[ri], inputs[ci], dt)[0]
        if rs is not None:
            blk = rs[:, None] * blk
        if cs is not None:
            blk = blk * cs[None, :]
        K[roff[I]:roff[I + 1], coff[J]:coff[J + 1]] += blk
    return K


def contract(S, G, dt, inputs=False, scales=False):
    """grad_truth.contract's d_coef, d_inscale, S_coef, S_inscale and n_rows for a spec with derivative terms (the input-point
    and scale gradients are refused through such terms: not stated here)"""
    assert not inputs and not scales
    terms, X_in = T._cast(S, dt)
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    coff = np.concatenate([[0], np.cumsum(S["col_len"])]).astype(int)
    nt = len(terms)
    out = dict(d_coef=np.zeros(nt, dt), S_coef=np.zeros(nt, dt), d_inscale=np.zeros(nt, dt), S_inscale=np.zeros(nt, dt),
               n_rows=np.ones(nt, dt))
    for t, (I, J, kind, ri, ci, coef, param, rs, cs) in enumerate(terms):
        k, dk = _values(kind, param, X_in[ri], X_in[ci], dt)
        w = G[roff[I]:roff[I + 1], coff[J]:coff[J + 1]]
        if rs is not None:
            w = w * rs[:, None]
        if cs is not None:
            w = w * cs[None, :]
        a = w * k
        out["d_coef"][t], out["S_coef"][t] = a.sum(), np.abs(a).sum()
        a = w * dk
        out["d_inscale"][t], out["S_inscale"][t] = coef * a.sum(), abs(coef) * np.abs(a).sum()
        out["n_rows"][t] = max(X_in[ri].shape[1], 1)
    return out


class _Ops:
    dense, contract = staticmethod(dense), staticmethod(contract)


def read_spec(spec):
    """grad_truth.read_spec (a lib.Spec -> plain data)"""
    return T.read_spec(spec)


def runs(S, noise, mean, y):
    """(truth in long double, float64 with the column recurrence, float64 in LAPACK's blocked order) for scalar noise"""
    return tuple(T.logpdf_grad(S, T.NOISE_SCALAR, noise, mean, y, dt, cholesky=ch, ops=_Ops)
                 for dt, ch in ((T.require_extended(), None), (np.float64, None), (np.float64, T.cholesky_blocked_order)))


def reference_outputs(R):
    return dict(value=R["value"], y=-R["alpha"], mean=R["alpha"], noise=R["noise"], d_coef=R["d_coef"], d_inscale=R["d_inscale"])


def units(out, R):
    """largest error of each output family against the truth R, in units of 2^-53 of grad_truth's scales"""
    n = R["n"]
    sc = T.scale_entries(R["alpha"], R["S_alpha"] / n)
    return {
        "value": T.units(out["value"], R["value"], T.scale_scalar(R["value"], R["S_value"], n)),
        "y": max(T.units(out["y"], -R["alpha"], sc), T.units(out["mean"], R["alpha"], sc)),
        "noise": T.units(out["noise"], R["noise"], T.scale_scalar(R["noise"], R["S_noise"], n)),
        "d_coef": T.units(out["d_coef"], R["d_coef"], T.scale_scalar(R["d_coef"], R["S_coef"], R["n_rows"])),
        "d_inscale": T.units(out["d_inscale"], R["d_inscale"], T.scale_scalar(R["d_inscale"], R["S_inscale"], R["n_rows"])),
    }


def yardstick(R, R64):
    figs = [units(reference_outputs(r), R) for r in R64]
    return {fam: max(f[fam] for f in figs) for fam in figs[0]}


def bound(fam, e64):
    return T.MARGIN * max(e64, FLOORS[fam])


# ---- the final case list: shared by the CPU and the GPU file ---------------------------------------------------------------
CASES = ("se_d3", "m32_d3", "m52_d3", "se_d1", "m32_d2", "m52_d1")
_KERNEL = {"se": "SEKernel", "m32": "Matern32Kernel", "m52": "Matern52Kernel"}


def build_case(name, P):
    """(FiniteGP, y) of a case: (f, d_p f, d_q f) of f ~ 0.8 base(lengthscale 1.25) + 0.3 SE, noise 0.1, blocks with points
    shared between them (coincident pairs off the diagonal) and one duplicate inside a block.  D = 3: blocks (37, 29, 64),
    130 rows -- a tile edge is crossed; D = 1, 2: blocks (20, 13, 17)"""
    base, D = name.split("_d")[0], int(name.split("_d")[1])
    sizes = (37, 29, 64) if D == 3 else (20, 13, 17)
    rng = np.random.default_rng(100 + 7 * D + len(base))
    Xs = [np.asfortranarray(rng.standard_normal((D, n)) * 0.7) for n in sizes]
    Xs[1][:, :9] = Xs[0][:, 4:13]
    Xs[2][:, 5:12] = Xs[1][:, 3:10]
    Xs[2][:, 14] = Xs[2][:, 15]
    gpc = P.GPC()
    f = P.atomic(P.GP(0.8 * P.with_lengthscale(getattr(P, _KERNEL[base])(), 1.25) + 0.3 * P.SEKernel()), gpc)
    F = P.cross([f, P.derivative(f, 0), P.derivative(f, D - 1)])
    x = P.BlockData([P.ColVecs(X) if D > 1 else X[0].copy() for X in Xs])
    y = np.cos(np.arange(sum(sizes)) * 0.37)
    return F(x, 0.1), y


_TRUTH = {}


def case_truth(name, P):
    """(spec, (R, R64a, R64b)) of a case: computed once, shared, never modified"""
    if name not in _TRUTH:
        fx, y = build_case(name, P)
        spec = P.build_spec(fx.f, fx.x)[0]
        _TRUTH[name] = (spec, runs(read_spec(spec), fx.noise, P.mean(fx), y))
    return _TRUTH[name]
