"""Extended-precision truth for the gradients with respect to a stencil's own weights and offsets
(include/sthenomi_stencil_wo.h).

TEST INFRASTRUCTURE ONLY.  A direct contraction of the header's four sums, per term and side, in the working dtype:
    W_ij = G_ij coef rs_i cs_j,   delta_pq = (x_i - a_p) - (y_j - b_q),   d2_pq = |delta_pq|^2
    grad_weights_row[p]    =  sum_ij W_ij sum_q v_q k(d2_pq)
    grad_weights_col[q]    =  sum_ij W_ij sum_p w_p k(d2_pq)
    grad_offsets_row[:, p] = -sum_ij W_ij w_p sum_q v_q 2 kappa'(d2_pq) delta_pq
    grad_offsets_col[:, q] = +sum_ij W_ij v_q sum_p w_p 2 kappa'(d2_pq) delta_pq
each returned with the sum of the absolute values of its addends (for the scale of the error unit, as tests/grad_truth.py).
grad_truth.contract forms only the row side of a symmetric spec, so expanding and folding its gx does not give the column
tables: the sums are contracted here directly.  The cotangent G comes from grad_truth's own dense / cholesky / tri_inverse on
the expanded plain spec (stencil_grad_truth.expand), through stencil_grad_truth.logpdf_truth / elbo_truth: in np.longdouble it
is the truth, in np.float64 (two orders of the factorisation) the yardstick e_float64.

The device is held as grad_truth holds it: MARGIN * max(e_float64 of the case, floor of the family); the floors are the
medians of e_float64 over WO_CASES (the diagonal: over all of them with a fixed random w), printed by
`python tests/test_stencil_wo_on_numpy.py` and recorded below.  Nothing here is taken from the device.

The cases are stencil_grad_truth.CASES unchanged, plus what the kernel of this gradient can get wrong on its own: a pair that
spans two column strips (128 columns each) and three 64-row groups with ragged ends on both, and a term whose sides have 64
points and 1 point, in both orders (the mirror pair)."""
import numpy as np

import grad_truth as T
import stencil_grad_truth as ST
import stheno_jl_amd as P

FAMILIES = ("wo.lp.weights", "wo.lp.offsets", "wo.elbo.weights", "wo.elbo.offsets", "wo.diag.weights", "wo.diag.offsets")

# e_float64 over WO_CASES (sorted), family by family, and their medians
MEASURED_FLOAT64 = {'wo.diag.offsets': [0.2, 1.0, 1.1, 1.1, 1.7, 1.8, 2.7, 2.7, 2.9, 2.9, 3.1, 3.2, 5.8, 6.1, 7.8],
 'wo.diag.weights': [0.6, 1.1, 2.0, 2.2, 2.3, 2.8, 3.4, 3.6, 4.3, 4.7, 6.1, 6.2, 7.3, 10.7, 14.5],
 'wo.elbo.offsets': [21.0, 32.9, 46.4, 321.0],
 'wo.elbo.weights': [2.8, 6.5, 34.6, 221.0],
 'wo.lp.offsets': [17.2, 26.0, 146.0, 159.9, 266.9, 291.6, 359.8, 578.6, 1270.4, 2661.2, 3266.0],
 'wo.lp.weights': [0.7, 13.0, 15.6, 47.1, 61.4, 80.9, 95.2, 139.3, 141.3, 602.9, 2210.2]}
FLOORS = {'wo.diag.offsets': 2.7,
 'wo.diag.weights': 3.6,
 'wo.elbo.offsets': 39.65,
 'wo.elbo.weights': 20.55,
 'wo.lp.offsets': 291.6,
 'wo.lp.weights': 80.9}


# ---- the sums ------------------------------------------------------------------------------------------------------------
def _or_unit(st, D):
    return (np.zeros((D, 1)), np.ones(1)) if st is None else st


def term_sums(kind, param, X, Y, rst, cst, Wm, dt, diagonal=False, shift_dt=np.float64):
    """(value, sides): value = sum_ij W_ij sum_pq w_p v_q k(d2_pq) and sides = [row, column], each None (a plain side) or
    dict(w, S_w (Q), o, S_o (D x Q)).  Wm: nr x nc (diagonal: the n weights of the entries (i, i)).  shift_dt: the dtype the
    shifted points x - a are formed in -- float64 as on the device, or dt for the derivative of the formula itself"""
    D = X.shape[0]
    (A, w), (B, v) = _or_unit(rst, D), _or_unit(cst, D)
    Qr, Qc = len(w), len(v)
    w, v = np.asarray(w).astype(dt), np.asarray(v).astype(dt)
    z = lambda *sh: np.zeros(sh, dtype=dt)      # noqa: E731
    gwr, Swr, gwc, Swc = z(Qr), z(Qr), z(Qc), z(Qc)
    gor, Sor, goc, Soc = z(D, Qr), z(D, Qr), z(D, Qc), z(D, Qc)
    value = dt(0)
    Xs = [(X.astype(shift_dt) - A[:, p:p + 1].astype(shift_dt)).astype(dt) for p in range(Qr)]
    Ys = [(Y.astype(shift_dt) - B[:, q:q + 1].astype(shift_dt)).astype(dt) for q in range(Qc)]
    diff = (lambda a, b: a - b) if diagonal else (lambda a, b: a[:, None] - b[None, :])
    for p in range(Qr):
        for q in range(Qc):
            d2 = np.zeros(Wm.shape, dtype=dt)
            for d in range(D):
                df = diff(Xs[p][d], Ys[q][d])
                d2 += df * df
            k, kp, _ = T.kappa(kind, d2, param, dt)
            wk = Wm * k
            s, a = wk.sum(), np.abs(wk).sum()
            value += w[p] * v[q] * s
            gwr[p] += v[q] * s
            Swr[p] += abs(v[q]) * a
            gwc[q] += w[p] * s
            Swc[q] += abs(w[p]) * a
            core = (dt(2) * w[p] * v[q]) * (Wm * kp)
            for d in range(D):
                c = core * diff(Xs[p][d], Ys[q][d])
                s, a = c.sum(), np.abs(c).sum()
                gor[d, p] -= s
                goc[d, q] += s
                Sor[d, p] += a
                Soc[d, q] += a
    return value, [None if rst is None else dict(w=gwr, S_w=Swr, o=gor, S_o=Sor),
                   None if cst is None else dict(w=gwc, S_w=Swc, o=goc, S_o=Soc)]


def _weights(g, coef, rs, cs, dt):
    Wm = g * dt(coef)
    if rs is not None:
        Wm = Wm * rs.astype(dt)[:, None]
    if cs is not None:
        Wm = Wm * cs.astype(dt)[None, :]
    return Wm


def contract(S, G, dt):
    """per term of S (stencil_grad_truth.read_spec): None (no stencil) or dict(n_rows, sides) against the cotangent G (the
    whole matrix, in dt)"""
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    coff = np.concatenate([[0], np.cumsum(S["col_len"])]).astype(int)
    out = []
    for (I, J, kind, ri, ci, coef, param, rs, cs), (rst, cst) in zip(S["terms"], S["stencils"]):
        if rst is None and cst is None:
            out.append(None)
            continue
        Wm = _weights(G[roff[I]:roff[I + 1], coff[J]:coff[J + 1]], coef, rs, cs, dt)
        _, sides = term_sums(kind, param, S["inputs"][ri], S["inputs"][ci], rst, cst, Wm, dt)
        out.append(dict(n_rows=max(1, int(S["row_len"][I])), sides=sides))
    return out


def contract_diag(S, w, dt):
    """the same for sgp_kernelmatrix_diag_grad_stencil_wo: entries (i, i) of the diagonal pairs with the weights w; the
    terms of other pairs: exact zeros"""
    roff = np.concatenate([[0], np.cumsum(S["row_len"])]).astype(int)
    w = np.asarray(w, np.float64).astype(dt)
    out = []
    for (I, J, kind, ri, ci, coef, param, rs, cs), (rst, cst) in zip(S["terms"], S["stencils"]):
        if rst is None and cst is None:
            out.append(None)
            continue
        n = int(S["row_len"][I])
        if I != J:
            D = S["inputs"][ri].shape[0]
            zero = lambda st: None if st is None else {k: np.zeros((len(st[1]),) if k[-1] == "w" else (D, len(st[1])), dtype=dt)   # noqa: E731
                                                       for k in ("w", "S_w", "o", "S_o")}
            out.append(dict(n_rows=max(1, n), sides=[zero(rst), zero(cst)]))
            continue
        Wm = w[roff[I]:roff[I + 1]] * dt(coef) * (1 if rs is None else rs.astype(dt)) * (1 if cs is None else cs.astype(dt))
        _, sides = term_sums(kind, param, S["inputs"][ri], S["inputs"][ci], rst, cst, Wm, dt, diagonal=True)
        out.append(dict(n_rows=max(1, n), sides=sides))
    return out


# ---- units -----------------------------------------------------------------------------------------------------------------
def scales(term, side):
    """(scale of the weights Q, scale of the offsets D x Q) of one table pair: grad_truth.scale_entries with S / n_rows"""
    r = term["sides"][side]
    return T.scale_entries(r["w"], r["S_w"] / term["n_rows"]), T.scale_entries(r["o"], r["S_o"] / term["n_rows"])


def units(gw, go, R):
    """(weights, offsets): the largest error of the tables gw[t][side] (Q) / go[t][side] (D x Q) in eps * scale, over every
    term and side of the truth R; a table the truth has and the caller lacks (or the reverse) is an error"""
    uw = uo = 0.0
    assert len(gw) == len(go) == len(R)
    for t, term in enumerate(R):
        for side in (0, 1):
            r = None if term is None else term["sides"][side]
            assert (r is None) == (gw[t][side] is None) == (go[t][side] is None), (t, side)
            if r is None:
                continue
            assert np.shape(gw[t][side]) == r["w"].shape and np.shape(go[t][side]) == r["o"].shape
            sw, so = scales(term, side)
            uw, uo = max(uw, T.units(gw[t][side], r["w"], sw)), max(uo, T.units(go[t][side], r["o"], so))
    return uw, uo


def tables_of(R):
    """the tables of a reference run, in the layout `units` takes"""
    pick = lambda key: [[None if (term is None or s is None) else s[key] for s in (term["sides"] if term else (None, None))]   # noqa: E731
                        for term in R]
    return pick("w"), pick("o")


def host_tables(raw):
    """(gw, go) of `_raw_stencils` with the offsets as D x Q"""
    gw, go = raw
    return gw, [[None if a is None else a.T for a in row] for row in go]


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Case(ST.Case):
    """an "lp" case of this file's own list (stencil_grad_truth.Case seeds by the position in ITS list)"""

    def build(self):
        rng = np.random.default_rng(9500 + EXTRA.index(self))
        F = ST.model(self.kernel, self.D, *self.stencils())
        xs = [P.GPPPInput(name, P.ColVecs(self.points(rng, n))) for name, n in self.blocks]
        n = sum(k for _, k in self.blocks)
        return F, F(P.BlockData(xs), float(0.1 + 0.2 * rng.random())), rng.standard_normal(n)


EXTRA = [
    # (g, g): 150 x 150 -- three 64-row groups and two 128-column strips, ragged on both; (g, h) and (h, g): 150 x 70 and back
    Case("wo-strips-150-70", "lp", "m52", 3, "quad:5", "fd", [("g", 150), ("h", 70)]),
    # 64 points against the one-point stencil, and (the mirror pair) 1 against 64
    Case("wo-64x1", "lp", "se", 2, "cloud:64", "unit", [("g", 20), ("h", 15)]),
]
WO_CASES = ST.CASES + EXTRA
LP_CASES = [c for c in WO_CASES if c.family == "lp"]
ELBO_CASES = [c for c in WO_CASES if c.family == "elbo"]

_RUNS = {}


def _dtype_of(R):
    return np.asarray(R["value"]).dtype.type


def logpdf_runs(case, spec, fx, y):
    """(truth, float64 run, float64 run in the blocked order) of an "lp" case: the tables against each run's own G"""
    if ("lp", case.id) not in _RUNS:
        S = ST.read_spec(spec)
        _RUNS[("lp", case.id)] = tuple(contract(S, R["G"], _dtype_of(R)) for R in ST.logpdf_truth(case, spec, fx, y))
    return _RUNS[("lp", case.id)]


def elbo_runs(case, specs, fz, fx, y, var_x):
    """the same for an "elbo" case: dict(zz, xz) per run"""
    if ("elbo", case.id) not in _RUNS:
        Sz, Sx = ST.read_spec(specs["zz"]), ST.read_spec(specs["xz"])
        _RUNS[("elbo", case.id)] = tuple(dict(zz=contract(Sz, R["dKzz"], _dtype_of(R)), xz=contract(Sx, R["dKxz"], _dtype_of(R)))
                                         for R in ST.elbo_truth(case, specs, fz, fx, y, var_x))
    return _RUNS[("elbo", case.id)]


def diag_weights(case, n):
    """the w of the diagonal check of a case: fixed, of both signs"""
    return np.random.default_rng(7700 + WO_CASES.index(case)).standard_normal(n)


def diag_runs(case, spec, w):
    """(truth, float64 run) of sgp_kernelmatrix_diag_grad_stencil_wo on `spec` with the weights w"""
    if ("diag", case.id) not in _RUNS:
        S = ST.read_spec(spec)
        _RUNS[("diag", case.id)] = (contract_diag(S, w, T.require_extended()), contract_diag(S, w, np.float64))
    return _RUNS[("diag", case.id)]


def yardstick(R, R64s):
    """(weights, offsets): the larger figure of the float64 runs against the truth"""
    figs = [units(*tables_of(r), R) for r in R64s]
    return max(f[0] for f in figs), max(f[1] for f in figs)


def bound_of(fam, e64):
    return T.MARGIN * max(e64, FLOORS[fam])


def hold(case, fam, dev, e64):
    print(f"{case.id:22s} {fam:18s} device {dev:10.1f}  float64 {e64:10.1f}  floor {FLOORS[fam]:8.1f}")
    assert dev <= bound_of(fam, e64), (case.id, fam, dev, e64)
