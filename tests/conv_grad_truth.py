"""Extended-precision truth for the gradients through patch (convolutional) terms (include/sthenomi_conv_grad.h).

TEST INFRASTRUCTURE ONLY.  A patch term is exactly the sum, over patch positions, of plain terms on patch-extracted inputs:
`expand` turns the description of a spec with patch terms into the spec dictionary of tests/grad_truth.py -- every patched
input becomes P inputs (np_patches), every patch term P_r P_c plain terms with the same coef, param and scales -- the
functions of grad_truth run on it unchanged, and `fold_terms` / `fold_inputs` add their results back onto the owning term
and input.  np.longdouble is the truth; the float64 run of the same code is the yardstick e_float64.

The device is held as grad_truth holds it: MARGIN * max(e_float64 of the case, floor of the family).  The per-term families
of a spec with patch terms have floors of their own (FLOORS below: the medians of e_float64 over this file's case list,
printed by `python tests/test_conv_grad_on_numpy.py`); value, y, mean, noise and z_noise use grad_truth's families and floors.

The case list lives here so that the CPU file can run the yardstick on it and the GPU file the device."""
import numpy as np

import grad_truth as T
import stheno_jl_amd as P
from test_conv_on_numpy import np_patches

# e_float64 over CASES (sorted), family by family, and their medians
MEASURED_FLOAT64 = {'conv.elbo.d_coef': [0.9, 1.9, 2.2, 5.1, 6.5],
 'conv.elbo.d_inscale': [2.1, 2.5, 2.7, 2.9, 11.0],
 'conv.elbo.inputs': [16.2, 18.4, 77.2, 222.8, 229.1],
 'conv.lp.d_coef': [9.8, 10.3, 16.4, 26.3, 28.4, 65.1, 153.3, 462.3, 5846.3],
 'conv.lp.d_inscale': [9.7, 12.0, 16.4, 18.5, 36.4, 40.8, 271.2, 2069.8, 3690.9]}
FLOORS = {'conv.elbo.d_coef': 2.2,
 'conv.elbo.d_inscale': 2.7,
 'conv.elbo.inputs': 77.2,
 'conv.lp.d_coef': 28.4,
 'conv.lp.d_inscale': 36.4}


# ---- the expansion -----------------------------------------------------------------------------------------------------
def read_spec(spec):
    """grad_truth.read_spec plus `geoms`: per term (row geometry, column geometry), None for a plain side"""
    S = T.read_spec(spec)
    S["geoms"] = [tuple(g) for g in spec.term_geoms]
    return S


def expand(S):
    """(Sx, owner, in_map): the plain spec dictionary with the same matrix; owner[e] = the term of S that expanded term e
    belongs to; in_map[(k, geom)] = the expanded inputs that hold input k as read through geom (None: as it is)."""
    inputs, in_map = [], {}

    def views(k, geom):
        if (k, geom) not in in_map:
            X = S["inputs"][k]
            vs = [X] if geom is None else [np.asfortranarray(p.T) for p in np_patches(X, geom)]
            in_map[(k, geom)] = list(range(len(inputs), len(inputs) + len(vs)))
            inputs.extend(vs)
        return in_map[(k, geom)]

    terms, owner = [], []
    for t, ((I, J, kind, ri, ci, coef, param, rs, cs), (rg, cg)) in enumerate(zip(S["terms"], S["geoms"])):
        for a in views(ri, rg):
            for b in views(ci, cg):
                terms.append((I, J, kind, a, b, coef, param, rs, cs))
                owner.append(t)
    Sx = dict(terms=terms, inputs=inputs, row_len=S["row_len"], col_len=S["col_len"], symmetric=S["symmetric"])
    return Sx, np.asarray(owner, dtype=int), in_map


def fold_terms(R, owner, nt):
    """d_coef, S_coef, d_inscale, S_inscale of the expanded terms summed onto their owners (n_rows: the owner's)"""
    out = {}
    for key in ("d_coef", "S_coef", "d_inscale", "S_inscale"):
        v = np.zeros(nt, dtype=R[key].dtype)
        np.add.at(v, owner, R[key])
        out[key] = v
    if "n_rows" in R:
        out["n_rows"] = np.ones(nt, dtype=R["n_rows"].dtype)
        out["n_rows"][owner] = R["n_rows"]
    if "diagonal" in R:
        out["diagonal"] = np.zeros(nt, bool)
        out["diagonal"][owner] = R["diagonal"]
    return out


def fold_inputs(R, in_map, n_inputs):
    """gx / Sn_gx of the inputs that are read as they are; None for an input that holds images"""
    gx, Sn = [None] * n_inputs, [None] * n_inputs
    for (k, geom), idx in in_map.items():
        if geom is None:
            gx[k], Sn[k] = R["gx"][idx[0]], R["Sn_gx"][idx[0]]
    return gx, Sn


def var_spec(var_x):
    """a spec dictionary whose diagonal is the given vector: sgp_elbo* take var_x as data"""
    n = len(var_x)
    return dict(terms=[(0, 0, T.CONST, 0, 0, 1.0, 1.0, np.asarray(var_x, dtype=np.float64), None)],
                inputs=[np.zeros((1, n))], row_len=[n], col_len=[n], symmetric=True)


# ---- models and cases -----------------------------------------------------------------------------------------------------
KERNELS = {"se": lambda: P.with_lengthscale(P.SEKernel(), 2.5), "m12": lambda: P.with_lengthscale(P.Matern12Kernel(), 4.0),
           "m32": lambda: P.with_lengthscale(P.Matern32Kernel(), 3.5), "m52": lambda: P.with_lengthscale(P.Matern52Kernel(), 3.0)}


def model(kernel, patch, n_patches):
    """g = GP(variance * kernel), f = patch_convolve(g), fh = f + h, f2 = 2 f - 0.5 + f; the variance keeps var(f) = O(1)"""
    def build(GP):
        g = GP((1.7 / n_patches) * KERNELS[kernel]())
        h = GP(0.5 * P.Matern32Kernel())
        f = P.patch_convolve(g, patch_shape=patch)
        return {"g": g, "h": h, "f": f, "fh": f + h, "f2": 2.0 * f - 0.5 + f}
    return P.gppp(build)


class Case:
    """family "lp": logpdf of `process` at n images (jointly with n_plain points of g); "elbo": n images of f, m inducing
    patches in g"""

    def __init__(self, id, family, kernel, image, patch, n, process="f", n_plain=0, m=0, noise="scalar", truth_xx=True):
        self.id, self.family, self.kernel, self.image, self.patch, self.n = id, family, kernel, image, patch, n
        self.process, self.n_plain, self.m, self.noise, self.truth_xx = process, n_plain, m, noise, truth_xx

    def __repr__(self):
        return self.id

    @property
    def n_patches(self):
        return (self.image[0] - self.patch[0] + 1) * (self.image[1] - self.patch[1] + 1)

    def build(self):
        """(F, fx, y) or (F, fz, fx, y): the same numbers on every call"""
        rng = np.random.default_rng(7000 + CASES.index(self))
        F = model(self.kernel, self.patch, self.n_patches)
        x = P.GPPPInput(self.process, P.ImageVector(rng.standard_normal(self.image + (self.n,))))
        D = self.patch[0] * self.patch[1]
        n = self.n + self.n_plain
        noise = float(0.1 + 0.2 * rng.random()) if self.noise == "scalar" else 0.1 + 0.2 * rng.random(n)
        y = rng.standard_normal(n)
        if self.family == "lp":
            if self.n_plain:
                x = P.BlockData([x, P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((D, self.n_plain)))))])
            return F, F(x, noise), y
        z = P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((D, self.m)))))
        return F, F(z, 1e-2), F(x, noise), y


CASES = [
    # lanes idle: P = 36 < 64, D = 9 the exact instantiation; a patch term alone and with a plain term in one pair
    Case("lanes-se-f", "lp", "se", (8, 8), (3, 3), 20),
    Case("lanes-se-fh", "lp", "se", (8, 8), (3, 3), 20, process="fh"),
    Case("lanes-m52-f", "lp", "m52", (8, 8), (3, 3), 20, noise="diag"),
    Case("lanes-m52-fh", "lp", "m52", (8, 8), (3, 3), 20, process="fh"),
    # the lane loop's second trip: P = 72 > 64
    Case("trip2", "lp", "se", (11, 10), (3, 3), 12),
    # zero-padded patch dimension (D = 6 in the 8-wide instantiation), two row tiles with a partial last one; jointly with 7
    # plain points: the two-sided pair, both one-sided orientations and a plain pair in one symmetric spec
    Case("joint", "lp", "m32", (5, 5), (2, 3), 130, n_plain=7),
    Case("coef9", "lp", "se", (5, 5), (2, 3), 130, process="f2", noise="diag"),
    # the one-sided kernel's second chunk of plain points (513 > 256 * 2)
    Case("chunk2", "lp", "m12", (5, 5), (3, 3), 12, n_plain=513),
    # the whole image as one patch
    Case("whole", "lp", "m52", (3, 3), (3, 3), 150),
    Case("elbo-130x7-scalar", "elbo", "se", (5, 5), (2, 3), 130, m=7),
    Case("elbo-130x7-diag", "elbo", "m32", (5, 5), (2, 3), 130, m=7, noise="diag"),
    Case("elbo-40x130-scalar", "elbo", "m12", (8, 8), (3, 3), 40, m=130),
    Case("elbo-40x130-diag", "elbo", "m52", (8, 8), (3, 3), 40, m=130, noise="diag"),
    # the staging limit, one side patched: 64 x 48 = 3072 pixels, 8 x 8 patches (D = 64), 3 images against 5 points
    Case("staging-1sided", "elbo", "se", (64, 48), (8, 8), 3, m=5, truth_xx=False),
]
KERNELS["se-wide"] = lambda: P.with_lengthscale(P.SEKernel(), 8.0)     # 64-dimensional patches
CASES[-1].kernel = "se-wide"
LP_CASES = [c for c in CASES if c.family == "lp"]
ELBO_CASES = [c for c in CASES if c.family == "elbo"]

_NOISE_TAG = {"scalar": T.NOISE_SCALAR, "diag": T.NOISE_DIAG}
_TRUTH = {}          # case id -> (truth, float64 run, float64 run in the blocked order): computed once, shared, never modified


def _runs(case):
    """(dtype, factorisation) of the truth and of the float64 yardstick runs, as tests/test_gpu_grad_truth.py takes them.  The
    staging case factors 5 x 5 matrices, which LAPACK does not block: its second yardstick run would repeat the first (and
    leaving a run out can only lower e_float64, that is tighten the bound)"""
    runs = ((T.require_extended(), None), (np.float64, None), (np.float64, T.cholesky_blocked_order))
    return runs if case.truth_xx else runs[:2]


def logpdf_truth(case, g, fx, y):
    """the three reference runs of an "lp" case; g: the result of logpdf_and_gradient_conv (only its spec is read)"""
    if case.id not in _TRUTH:
        S = read_spec(g["_spec"])
        Sx, owner, _ = expand(S)
        runs = []
        for dt, ch in _runs(case):
            R = T.logpdf_grad(Sx, _NOISE_TAG[case.noise], fx.noise, P.mean(fx), y, dt, cholesky=ch)
            R.update(fold_terms(R, owner, len(S["terms"])))
            runs.append(R)
        _TRUTH[case.id] = tuple(runs)
    return _TRUTH[case.id]


def logpdf_outputs(g):
    gc, gs = g["_raw"]
    nt = g["_spec"].n_terms
    return dict(value=g["logpdf"], y=g["y"], mean=g["mean"], noise=g["noise"], d_coef=gc[:nt], d_inscale=gs[:nt])


def logpdf_reference_outputs(R):
    return dict(value=R["value"], y=-R["alpha"], mean=R["alpha"], noise=R["noise"], d_coef=R["d_coef"], d_inscale=R["d_inscale"])


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
    u["conv.lp.d_coef"] = T.units(out["d_coef"], R["d_coef"], T.scale_scalar(R["d_coef"], R["S_coef"], R["n_rows"]))
    u["conv.lp.d_inscale"] = T.units(out["d_inscale"], R["d_inscale"], T.scale_scalar(R["d_inscale"], R["S_inscale"], R["n_rows"]))
    return u


def elbo_truth(case, g, fz, fx, y, var_x):
    """the three reference runs of an "elbo" case; var_x: what the call under test was given (sgp_elbo* take it as data).
    R["xx"]: the expanded diag_grad with w = d elbo / d var_x (cases with truth_xx)"""
    if case.id not in _TRUTH:
        Sp = {k: read_spec(v) for k, v in g["_specs"].items()}
        (Szz, ozz, mzz), (Sxz, oxz, mxz) = expand(Sp["zz"]), expand(Sp["xz"])
        runs = []
        for dt, ch in _runs(case):
            R = T.elbo_grad(Szz, Sxz, var_spec(var_x), _NOISE_TAG[case.noise], fx.noise, T.NOISE_SCALAR, fz.noise, P.mean(fx),
                            y, dt, inputs=True, cholesky=ch)
            for key, S, owner, in_map in (("zz", Sp["zz"], ozz, mzz), ("xz", Sp["xz"], oxz, mxz)):
                gx, Sn = fold_inputs(R[key], in_map, len(S["inputs"]))
                R[key] = dict(fold_terms(R[key], owner, len(S["terms"])), gx=gx, Sn_gx=Sn)
            if case.truth_xx:
                Sxx, oxx, _ = expand(Sp["xx"])
                R["xx"] = fold_terms(T.diag_grad(Sxx, np.asarray(R["var"], dtype=np.float64), dt), oxx, len(Sp["xx"]["terms"]))
            runs.append(R)
        _TRUTH[case.id] = tuple(runs)
    return _TRUTH[case.id]


def elbo_outputs(g):
    nt = {k: g["_specs"][k].n_terms for k in ("zz", "xz", "xx")}
    return dict(value=g["elbo"], y=g["y"], mean=g["mean"], noise=g["noise"], z_noise=g["z_noise"], var=g["var"],
                zz=dict(d_coef=g["_raw"]["zz"][0][:nt["zz"]], d_inscale=g["_raw"]["zz"][1][:nt["zz"]], gx=g["zz_inputs"]),
                xz=dict(d_coef=g["_raw"]["xz"][0][:nt["xz"]], d_inscale=g["_raw"]["xz"][1][:nt["xz"]], gx=g["xz_inputs"]),
                xx=dict(d_coef=g["_raw"]["xx"][0][:nt["xx"]], d_inscale=g["_raw"]["xx"][1][:nt["xx"]]))


def elbo_reference_outputs(R):
    return dict(value=R["value"], y=R["y"], mean=-R["y"], noise=R["noise"], z_noise=R["z_noise"], var=R["var"],
                zz=R["zz"], xz=R["xz"], xx=R.get("xx"))


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
    u["conv.elbo.d_coef"] = u["conv.elbo.d_inscale"] = u["conv.elbo.inputs"] = 0.0
    for key in ("zz", "xz"):
        o, r = out[key], R[key]
        assert len(o["d_coef"]) == len(r["d_coef"]) and len(o["gx"]) == len(r["gx"])
        u["conv.elbo.d_coef"] = max(u["conv.elbo.d_coef"],
                                    T.units(o["d_coef"], r["d_coef"], T.scale_scalar(r["d_coef"], r["S_coef"], r["n_rows"])))
        u["conv.elbo.d_inscale"] = max(u["conv.elbo.d_inscale"],
                                       T.units(o["d_inscale"], r["d_inscale"],
                                               T.scale_scalar(r["d_inscale"], r["S_inscale"], r["n_rows"])))
        for a, e, s in zip(o["gx"], r["gx"], r["Sn_gx"]):
            assert (a is None) == (e is None)           # an input that holds images has no gradient on either side
            if e is not None:
                assert np.shape(a) == e.shape
                u["conv.elbo.inputs"] = max(u["conv.elbo.inputs"], T.units(a, e, T.scale_entries(e, s)))
    return u


def yardstick(runs):
    """e_float64 of a case: family by family the larger figure of the float64 runs"""
    runs = list(runs)
    return {fam: max(r[fam] for r in runs) for fam in runs[0]}


def floor_of(fam):
    return FLOORS[fam] if fam.startswith("conv.") else T.FLOORS[fam]


def hold(case, dev, f64):
    """the verdict: every family's figure inside MARGIN * max(float64 figure, floor); figures printed first"""
    for fam in sorted(dev):
        print(f"{case.id:20s} {fam:20s} device {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {floor_of(fam):8.1f}")
    bad = {fam: (dev[fam], f64[fam]) for fam in dev if not dev[fam] <= T.MARGIN * max(f64[fam], floor_of(fam))}
    assert not bad, (case.id, bad)


def diag_depth(case, n):
    """the longest chain of roundings an addend of sgp_kernelmatrix_diag_grad_conv's sums goes through, for the model bound
    depth * eps * S: D fused steps of the squared distance and 8 for the kernel and its derivative (grad_truth's model of a
    plain diagonal term), then the additions -- a lane's own run of ceil(P_r / 64) P_c of them, 6 butterfly steps over the
    wave, 2 products with the weight, and the reduction over the n entries: ceil(n / 256) strided additions and 8 tree
    steps"""
    D, Pn = case.patch[0] * case.patch[1], case.n_patches
    return D + 8 + -(-Pn // 64) * Pn + 6 + 2 + -(-n // 256) + 8
