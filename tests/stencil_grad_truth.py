"""Extended-precision truth for the gradients through stencil terms (include/sthenomi_stencil_grad.h).

TEST INFRASTRUCTURE ONLY.  A stencil term coef sum_p w_p sum_q v_q k(x - a_p, y - b_q) is exactly the sum of Q_r Q_c plain
terms on shifted inputs: `expand` turns the description of a spec with stencil terms into the spec dictionary of
tests/grad_truth.py -- every (input, stencil) becomes Q inputs X - a_q, every stencil term Q_r Q_c plain terms with the
coefficient coef w_p v_q (kept in long double: the weights are part of the coefficient) -- the functions of grad_truth run
on it unchanged, and `fold_terms` / `fold_inputs` add their results back onto the owning term and input:
    d_coef of the owner    = sum_e w_p v_q d_coef_e      (the expanded coefficient carries the weights)
    d_inscale of the owner = sum_e d_inscale_e
    gx of the owner input  = the sum over its shifted views (shifting is a translation).
np.longdouble is the truth; the float64 run of the same code is the yardstick e_float64.

The device is held as grad_truth holds it: MARGIN * max(e_float64 of the case, floor of the family).  The per-term and
input families of a spec with stencil terms have floors of their own (FLOORS below: the medians of e_float64 over this file's
case list, printed by `python tests/test_stencil_grad_on_numpy.py`); value, y, mean, noise and z_noise use grad_truth's
families and floors.

The finite-difference stencils have a moderate step (h = 0.1: weights of order 10, not 10^3), so that the float64 yardstick
is not pure cancellation noise.  The case list lives here so that the CPU file can run the yardstick on it and the GPU file
the device."""
import numpy as np

import grad_truth as T
import stheno_jl_amd as P

# e_float64 over CASES (sorted), family by family, and their medians
MEASURED_FLOAT64 = {'st.elbo.d_coef': [2.5, 2.5, 8.4, 9.6],
 'st.elbo.d_inscale': [10.3, 25.2, 25.7, 82.8],
 'st.elbo.inputs': [42.2, 209.8, 1199.5, 4461.6],
 'st.lp.d_coef': [0.1, 2.7, 9.9, 10.7, 32.7, 35.1, 62.9, 120.7, 812.2],
 'st.lp.d_inscale': [3.2, 4.0, 5.3, 14.8, 17.1, 25.1, 294.5, 616.5, 974.5],
 'st.lp.inputs': [13.8, 24.8, 25.7, 27.7, 38.7, 129.7, 229.8, 368.3, 2665.3]}
FLOORS = {'st.elbo.d_coef': 5.45,
 'st.elbo.d_inscale': 25.45,
 'st.elbo.inputs': 704.65,
 'st.lp.d_coef': 32.7,
 'st.lp.d_inscale': 17.1,
 'st.lp.inputs': 38.7}

LD = np.longdouble


# ---- the expansion -----------------------------------------------------------------------------------------------------
def read_spec(spec):
    """grad_truth.read_spec plus `stencils`: per term (row stencil, column stencil), each None (a plain side) or
    (offsets D x Q, weights Q)"""
    S = T.read_spec(spec)
    S["stencils"] = [tuple(None if st is None else (np.asarray(st[0], dtype=np.float64), np.asarray(st[1], dtype=np.float64))
                           for st in sts) for sts in spec.term_stencils]
    return S


def _key(st):
    return None if st is None else (st[0].shape, st[0].tobytes())


def expand(S):
    """(Sx, owner, weight, in_map): the plain spec dictionary with the same matrix; owner[e] = the term of S that expanded
    term e belongs to and weight[e] = w_p v_q (long double); in_map[(k, offsets key)] = the expanded inputs that hold input k
    shifted by each offset (None: as it is).  The shifted points are the float64 differences the device forms."""
    inputs, in_map = [], {}

    def views(k, st):
        if (k, _key(st)) not in in_map:
            X = S["inputs"][k]
            vs = [X] if st is None else [np.asfortranarray(X - st[0][:, q:q + 1]) for q in range(st[0].shape[1])]
            in_map[(k, _key(st))] = list(range(len(inputs), len(inputs) + len(vs)))
            inputs.extend(vs)
        return in_map[(k, _key(st))]

    terms, owner, weight = [], [], []
    for t, ((I, J, kind, ri, ci, coef, param, rs, cs), (rst, cst)) in enumerate(zip(S["terms"], S["stencils"])):
        wr = np.ones(1) if rst is None else rst[1]
        wc = np.ones(1) if cst is None else cst[1]
        for p, a in enumerate(views(ri, rst)):
            for q, b in enumerate(views(ci, cst)):
                w = LD(wr[p]) * LD(wc[q])
                terms.append((I, J, kind, a, b, LD(coef) * w, param, rs, cs))
                owner.append(t)
                weight.append(w)
    Sx = dict(terms=terms, inputs=inputs, row_len=S["row_len"], col_len=S["col_len"], symmetric=S["symmetric"])
    return Sx, np.asarray(owner, dtype=int), np.asarray(weight, dtype=LD), in_map


def fold_terms(R, owner, weight, nt):
    """d_coef, S_coef, d_inscale, S_inscale of the expanded terms added onto their owners (n_rows: the owner's)"""
    dt = R["d_coef"].dtype
    w = weight.astype(dt)
    out = {}
    for key, fac in (("d_coef", w), ("S_coef", np.abs(w)), ("d_inscale", 1), ("S_inscale", 1)):
        v = np.zeros(nt, dtype=dt)
        np.add.at(v, owner, R[key] * fac)
        out[key] = v
    if "n_rows" in R:
        out["n_rows"] = np.ones(nt, dtype=R["n_rows"].dtype)
        out["n_rows"][owner] = R["n_rows"]
    if "diagonal" in R:
        out["diagonal"] = np.zeros(nt, bool)
        out["diagonal"][owner] = R["diagonal"]
    return out


def fold_inputs(R, in_map, n_inputs, S_key="Sn_gx"):
    """gx and its absolute sums added over the shifted views of every input"""
    gx, Sn = [None] * n_inputs, [None] * n_inputs
    for (k, _), idx in in_map.items():
        for e in idx:
            gx[k] = R["gx"][e].copy() if gx[k] is None else gx[k] + R["gx"][e]
            Sn[k] = R[S_key][e].copy() if Sn[k] is None else Sn[k] + R[S_key][e]
    return gx, Sn


def var_spec(var_x):
    """a spec dictionary whose diagonal is the given vector: sgp_elbo* take var_x as data"""
    n = len(var_x)
    return dict(terms=[(0, 0, T.CONST, 0, 0, 1.0, 1.0, np.asarray(var_x, dtype=np.float64), None)],
                inputs=[np.zeros((1, n))], row_len=[n], col_len=[n], symmetric=True)


# ---- stencils, models and cases ----------------------------------------------------------------------------------------
def fd_stencil(D, seed=0, h=0.1):
    """a forward difference along a direction: two points, weights -1 / h and 1 / h (order 10)"""
    u = np.random.default_rng(100 + seed).standard_normal(D)
    u /= np.sqrt(u @ u)
    return np.stack([np.zeros(D), -h * u], axis=1), np.array([-1.0 / h, 1.0 / h])


def quad_stencil(D, Q=15, seed=0, width=0.6):
    """a Q-point quadrature of a smoothing window along a direction: positive weights that add up to 1"""
    u = np.random.default_rng(200 + seed).standard_normal(D)
    u /= np.sqrt(u @ u)
    s = np.linspace(-1.0, 1.0, Q)
    w = np.exp(-2.0 * s * s)
    return np.outer(u, width * s), w / w.sum()


def cloud_stencil(D, Q, seed=0, width=0.5):
    """Q points scattered in D dimensions with weights of both signs, sum |w| = 4"""
    rng = np.random.default_rng(300 + seed)
    w = rng.standard_normal(Q)
    return width * rng.standard_normal((D, Q)), 4.0 * w / np.abs(w).sum()


def unit_stencil(D):
    return np.zeros((D, 1)), np.ones(1)


def dyadic_stencil(D):
    """offsets that are multiples of 0.25: on a grid of that spacing shifted pairs coincide"""
    A = np.zeros((D, 3))
    A[0] = [0.0, 0.25, -0.5]
    return A, np.array([1.0, -2.0, 1.5])


def make_stencil(tag, D, seed):
    kind, _, q = tag.partition(":")
    return {"fd": lambda: fd_stencil(D, seed), "quad": lambda: quad_stencil(D, int(q or 15), seed),
            "cloud": lambda: cloud_stencil(D, int(q or 64), seed), "unit": lambda: unit_stencil(D),
            "dyadic": lambda: dyadic_stencil(D)}[kind]()


BASE = {"se": P.SEKernel, "m12": P.Matern12Kernel, "m32": P.Matern32Kernel, "m52": P.Matern52Kernel}


def kernel_of(name, D, ls=None):
    """lengthscale 0.8 sqrt(D): the points are standard normal, so squared distances are of order 2 D"""
    return P.with_lengthscale(BASE[name](), 0.8 * np.sqrt(D) if ls is None else ls)


def model(kernel, D, st_g, st_h, variance=1.3, ls=None):
    """f = GP(variance * kernel), u = GP(0.4 Matern32); g = stencil(f, st_g), h = stencil(f, st_h); gu = g + u (the stencil
    term precedes the plain one in its pair), ug = u + g"""
    def build(GP):
        f = GP(variance * kernel_of(kernel, D, ls))
        u = GP(0.4 * P.with_lengthscale(P.Matern32Kernel(), np.sqrt(D)))
        g = P.stencil(f, *st_g)
        h = P.stencil(f, *st_h)
        return {"f": f, "u": u, "g": g, "h": h, "gu": g + u, "ug": u + g}
    return P.gppp(build)


class Case:
    """family "lp": logpdf of the joint model over `blocks` [(process, n), ...]; "elbo": `blocks` are the data, `z` =
    (process, m) the inducing points.  st_g / st_h: the stencil tags of g and h (make_stencil); grid: the points lie on a
    dyadic grid of spacing 0.25 (coincident shifted pairs)"""

    def __init__(self, id, family, kernel, D, st_g, st_h, blocks, z=None, noise="scalar", grid=False):
        self.id, self.family, self.kernel, self.D, self.st_g, self.st_h = id, family, kernel, D, st_g, st_h
        self.blocks, self.z, self.noise, self.grid = blocks, z, noise, grid

    def __repr__(self):
        return self.id

    def stencils(self):
        return make_stencil(self.st_g, self.D, 1), make_stencil(self.st_h, self.D, 2)

    def points(self, rng, n):
        if self.grid:
            return np.asfortranarray(0.25 * rng.integers(-6, 7, size=(self.D, n)).astype(np.float64))
        return np.asfortranarray(rng.standard_normal((self.D, n)))

    def build(self):
        """(F, fx, y) or (F, fz, fx, y): the same numbers on every call"""
        rng = np.random.default_rng(9000 + CASES.index(self))
        # (on the grid the lengthscale is 1: the scaled points and offsets stay dyadic, shifted pairs coincide exactly)
        F = model(self.kernel, self.D, *self.stencils(), ls=1.0 if self.grid else None)
        xs = [P.GPPPInput(name, P.ColVecs(self.points(rng, n))) for name, n in self.blocks]
        x = xs[0] if len(xs) == 1 else P.BlockData(xs)
        n = sum(k for _, k in self.blocks)
        noise = float(0.1 + 0.2 * rng.random()) if self.noise == "scalar" else 0.1 + 0.2 * rng.random(n)
        y = rng.standard_normal(n)
        if self.family == "lp":
            return F, F(x, noise), y
        z = P.GPPPInput(self.z[0], P.ColVecs(self.points(rng, self.z[1])))
        return F, F(z, 1e-2), F(x, noise), y


CASES = [
    # D = 1 (the narrowest instantiation, CC = 4): cov(g, h) with 15 x 2 points, different stencils on the two sides
    Case("d1-se-15x2", "lp", "se", 1, "quad:15", "fd", [("g", 40), ("h", 30)]),
    # D = 3 padded to 4: a two-point stencil, the one-point stencil and the plain process -- one-sided terms both ways
    Case("d3-m12-2x1", "lp", "m12", 3, "fd", "unit", [("g", 33), ("h", 20), ("f", 10)], noise="diag"),
    # D = 5 padded to 8 (CC = 2), D = 9 padded to 16 (CC = 1)
    Case("d5-m32-15x2", "lp", "m32", 5, "quad:15", "fd", [("g", 21), ("h", 13)]),
    Case("d9-m52-2x15", "lp", "m52", 9, "fd", "quad:15", [("g", 17), ("h", 9)], noise="diag"),
    # the registration limits: 64 points in 16 dimensions, n = 3
    Case("d16-se-64x2", "lp", "se", 16, "cloud:64", "fd", [("g", 3), ("h", 3)]),
    # idle lanes, one workgroup
    Case("n5", "lp", "m52", 2, "fd", "quad:15", [("g", 5)]),
    # 37 points of f and 150 of g: block pairs that start off the 64-row and 4 CC-column alignment and cross a 128 tile
    Case("joint-37-150", "lp", "m32", 2, "fd", "unit", [("f", 37), ("g", 150)]),
    # a stencil term in front of a plain term of the same pair, and behind it: the outputs are in the caller's order
    Case("order-gu", "lp", "se", 2, "quad:15", "fd", [("gu", 30), ("ug", 25)], noise="diag"),
    # coincident shifted points: Matern-1/2 on a dyadic grid, offsets that are multiples of the spacing (subgradient 0)
    Case("coincident-m12", "lp", "m12", 2, "dyadic", "fd", [("g", 40), ("f", 20)], grid=True),
    # the ELBO: 150 points of g against 20 inducing points of f, then of g itself; both noise kinds
    Case("elbo-150x20f-scalar", "elbo", "se", 2, "quad:15", "fd", [("g", 150)], z=("f", 20)),
    Case("elbo-150x20f-diag", "elbo", "m32", 3, "fd", "unit", [("g", 150)], z=("f", 20), noise="diag"),
    Case("elbo-150x20g-scalar", "elbo", "m52", 2, "fd", "unit", [("g", 150)], z=("g", 20)),
    Case("elbo-150x20g-diag", "elbo", "m12", 5, "quad:15", "fd", [("g", 150)], z=("h", 20), noise="diag"),
]
LP_CASES = [c for c in CASES if c.family == "lp"]
ELBO_CASES = [c for c in CASES if c.family == "elbo"]


def case(id):
    return next(c for c in CASES if c.id == id)


_NOISE_TAG = {"scalar": T.NOISE_SCALAR, "diag": T.NOISE_DIAG}
_TRUTH = {}          # case id -> (truth, float64 run, float64 run in the blocked order): computed once, shared, never modified


def _runs():
    return ((T.require_extended(), None), (np.float64, None), (np.float64, T.cholesky_blocked_order))


def logpdf_truth(case, spec, fx, y):
    """the three reference runs of an "lp" case on `spec` (the spec of the call under test)"""
    if case.id not in _TRUTH:
        S = read_spec(spec)
        Sx, owner, weight, in_map = expand(S)
        runs = []
        for dt, ch in _runs():
            R = T.logpdf_grad(Sx, _NOISE_TAG[case.noise], fx.noise, P.mean(fx), y, dt, inputs=True, cholesky=ch)
            R.update(fold_terms(R, owner, weight, len(S["terms"])))
            R["gx"], R["Sn_gx"] = fold_inputs(R, in_map, len(S["inputs"]))
            runs.append(R)
        _TRUTH[case.id] = tuple(runs)
    return _TRUTH[case.id]


def logpdf_outputs(g):
    gc, gs = g["_raw"]
    nt = g["_spec"].n_terms
    return dict(value=g["logpdf"], y=g["y"], mean=g["mean"], noise=g["noise"], d_coef=gc[:nt], d_inscale=gs[:nt],
                gx=g["inputs"])


def logpdf_reference_outputs(R):
    return dict(value=R["value"], y=-R["alpha"], mean=R["alpha"], noise=R["noise"], d_coef=R["d_coef"], d_inscale=R["d_inscale"],
                gx=R["gx"])


def _input_units(got, R):
    assert len(got) == len(R["gx"])
    u = 0.0
    for a, e, s in zip(got, R["gx"], R["Sn_gx"]):
        assert np.shape(a) == e.shape
        u = max(u, T.units(a, e, T.scale_entries(e, s)))
    return u


def logpdf_units(out, R):
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
    u["st.lp.d_coef"] = T.units(out["d_coef"], R["d_coef"], T.scale_scalar(R["d_coef"], R["S_coef"], R["n_rows"]))
    u["st.lp.d_inscale"] = T.units(out["d_inscale"], R["d_inscale"], T.scale_scalar(R["d_inscale"], R["S_inscale"], R["n_rows"]))
    u["st.lp.inputs"] = _input_units(out["gx"], R)
    return u


def elbo_truth(case, specs, fz, fx, y, var_x):
    """the three reference runs of an "elbo" case; var_x: what the call under test was given (sgp_elbo* take it as data).
    R["xx"]: the expanded diag_grad with w = d elbo / d var_x"""
    if case.id not in _TRUTH:
        Sp = {k: read_spec(v) for k, v in specs.items()}
        ex = {k: expand(Sp[k]) for k in ("zz", "xz", "xx")}
        runs = []
        for dt, ch in _runs():
            R = T.elbo_grad(ex["zz"][0], ex["xz"][0], var_spec(var_x), _NOISE_TAG[case.noise], fx.noise, T.NOISE_SCALAR, fz.noise,
                            P.mean(fx), y, dt, inputs=True, cholesky=ch)
            for key in ("zz", "xz"):
                _, owner, weight, in_map = ex[key]
                gx, Sn = fold_inputs(R[key], in_map, len(Sp[key]["inputs"]))
                R[key] = dict(fold_terms(R[key], owner, weight, len(Sp[key]["terms"])), gx=gx, Sn_gx=Sn)
            Sxx, owner, weight, in_map = ex["xx"]
            Rd = T.diag_grad(Sxx, np.asarray(R["var"], dtype=np.float64), dt)
            gx, Sg = fold_inputs(Rd, in_map, len(Sp["xx"]["inputs"]), S_key="S_gx")
            R["xx"] = dict(fold_terms(Rd, owner, weight, len(Sp["xx"]["terms"])), gx=gx, S_gx=Sg)
            runs.append(R)
        _TRUTH[case.id] = tuple(runs)
    return _TRUTH[case.id]


def elbo_outputs(g, gdx=None):
    nt = {k: g["_specs"][k].n_terms for k in ("zz", "xz", "xx")}
    return dict(value=g["elbo"], y=g["y"], mean=g["mean"], noise=g["noise"], z_noise=g["z_noise"], var=g["var"],
                zz=dict(d_coef=g["_raw"]["zz"][0][:nt["zz"]], d_inscale=g["_raw"]["zz"][1][:nt["zz"]], gx=g["zz_inputs"]),
                xz=dict(d_coef=g["_raw"]["xz"][0][:nt["xz"]], d_inscale=g["_raw"]["xz"][1][:nt["xz"]], gx=g["xz_inputs"]),
                xx=dict(d_coef=g["_raw"]["xx"][0][:nt["xx"]], d_inscale=g["_raw"]["xx"][1][:nt["xx"]], gx=gdx))


def elbo_reference_outputs(R):
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
    u["elbo.z_noise"] = T.units(out["z_noise"], R["z_noise"], T.scale_scalar(R["z_noise"], R["S_z_noise"], m))
    u["st.elbo.d_coef"] = u["st.elbo.d_inscale"] = u["st.elbo.inputs"] = 0.0
    for key in ("zz", "xz"):
        o, r = out[key], R[key]
        assert len(o["d_coef"]) == len(r["d_coef"])
        u["st.elbo.d_coef"] = max(u["st.elbo.d_coef"],
                                  T.units(o["d_coef"], r["d_coef"], T.scale_scalar(r["d_coef"], r["S_coef"], r["n_rows"])))
        u["st.elbo.d_inscale"] = max(u["st.elbo.d_inscale"],
                                     T.units(o["d_inscale"], r["d_inscale"],
                                             T.scale_scalar(r["d_inscale"], r["S_inscale"], r["n_rows"])))
        u["st.elbo.inputs"] = max(u["st.elbo.inputs"], _input_units(o["gx"], r))
    return u


def yardstick(runs):
    """e_float64 of a case: family by family the larger figure of the float64 runs"""
    runs = list(runs)
    return {fam: max(r[fam] for r in runs) for fam in runs[0]}


def floor_of(fam):
    return FLOORS[fam] if fam.startswith("st.") else T.FLOORS[fam]


def bound_of(fam, f64):
    return T.MARGIN * max(f64[fam], floor_of(fam))


def hold(case, dev, f64):
    """the verdict: every family's figure inside MARGIN * max(float64 figure, floor); figures printed first"""
    for fam in sorted(dev):
        print(f"{case.id:22s} {fam:20s} device {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {floor_of(fam):8.1f}")
    bad = {fam: (dev[fam], f64[fam]) for fam in dev if not dev[fam] <= bound_of(fam, f64)}
    assert not bad, (case.id, bad)


def diag_depth(case, n):
    """the longest chain of roundings an addend of sgp_kernelmatrix_diag_grad_stencil's sums goes through, for the model bound
    depth * eps * S: 2 D subtractions and D fused steps of the squared distance, 8 for the kernel and its derivative
    (grad_truth's model of a plain diagonal term), 2 products with the stencil weights and the Q_r Q_c fused additions of an
    entry, 2 products with the entry's weight, and the reduction over the n entries: ceil(n / 256) strided additions and 8
    tree steps"""
    (Ag, _), (Ah, _) = case.stencils()
    Q = max(Ag.shape[1], Ah.shape[1])
    return 3 * case.D + 8 + 2 + Q * Q + 2 + -(-n // 256) + 8
