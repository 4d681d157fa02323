"""The problems tests/kprod_grad_truth.py is pinned on, and their values at 40 digits (mpmath), written independently of that
module: scalar formulas from include/sthenomi_kprod.h applied entry by entry, mpmath.besselk for kind 20, C^-1 by mpmath's
inverse.  TEST INFRASTRUCTURE ONLY.  tests/golden/make_kprod_grad_truth.py writes what `bessel_table` and `pin_values` return
into tests/golden/kprod_grad_truth.json (25 significant digits: more than a long double's 64 bits);
tests/test_kprod_grad_truth_on_numpy.py reads that file and, where mpmath imports, derives the values again."""
import math

import numpy as np

import kprod_grad_truth as KT

DIGITS = 40
# nu: the grid of tests/matern_nu_truth.py, plus both sides of the half-integers (mu -> -+1/2, where the series' constants
# and the fraction's a1 = (1/2 - mu)(1/2 + mu) change character) and of the integers (mu -> 0)
BESSEL_NUS = (0.1, 0.3, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 2.5, 3.7, 7.5, 12.0, 25.0, 32.0,
              0.4999, 0.5001, 1.4999, 1.5001, 2.4999, 0.9999, 1.0001, 3.0001)
# x: small arguments, both sides of the truth's series / fraction split at 1 (where the fraction takes its most steps) and of
# the device's at 2, both sides of the e^-600 split, and up to 1000
BESSEL_XS = (1e-30, 1e-8, 1e-3, 0.05, 0.3, 1.0 * (1 - 2.0 ** -20), 1.0, 1.0 * (1 + 2.0 ** -20), 1.02, 1.4, 1.9,
             2.0 * (1 - 2.0 ** -20), 2.0, 2.0 * (1 + 2.0 ** -20), 2.1, 2.5, 3.0, 6.0, 10.0, 20.0, 50.0, 100.0, 400.0, 599.0,
             600.5, 750.0, 900.0, 999.0)


def bessel_points(nu):
    """the squared distances (doubles) at which x = sqrt(2 nu) sqrt(d2) is (a rounding of) BESSEL_XS"""
    return np.array([(x / math.sqrt(2.0 * nu)) ** 2 for x in BESSEL_XS])


def _mp():
    import mpmath as mp
    mp.mp.dps = DIGITS
    return mp


def _str(mp, v):
    return mp.nstr(v, 25, min_fixed=0, max_fixed=0)


def mn_truth(mp, nu, d2):
    """(k, d k / d (d^2)) of kind 20 at the doubles nu and d2 > 0"""
    v, s = mp.mpf(nu), mp.mpf(d2)
    x = mp.sqrt(2 * v * s)
    c = mp.power(2, 1 - v) / mp.gamma(v) * mp.power(x, v)
    return c * mp.besselk(v, x), -(v / x) * c * mp.besselk(v - 1, x)


def bessel_table():
    """{repr(nu): {"k": [...], "kx": [...]}} as decimal strings"""
    mp = _mp()
    out = {}
    for nu in BESSEL_NUS:
        vals = [mn_truth(mp, nu, float(d2)) for d2 in bessel_points(nu)]
        out[repr(nu)] = {"k": [_str(mp, a) for a, _ in vals], "kx": [_str(mp, b) for _, b in vals]}
    return out


# ---- the pin case: N = 24, D = 3, M = 6 ----------------------------------------------------------------------------------------
N, D, M = 24, 3, 6
NOISE, Z_NOISE = 0.15, 1e-2


def _chains(row0, col0, rs, cs):
    """one chain per kind pair, so that every kind of a chain appears; views: 0 the points, 1 the points x 0.7, 2 their first
    coordinate x 0.5 (row0 / col0: the index of view 0 on either side); the first head is function-scaled"""
    r, c = (lambda v: row0 + v), (lambda v: col0 + v)
    spec = [(0.5, rs, cs, [(KT.SE, 0, 0.0), (KT.RQ, 1, 0.9)]),
            (0.3, None, None, [(KT.MATERN32, 1, 0.0), (KT.COSINE, 2, 0.0)]),
            (0.4, None, None, [(KT.MATERN52, 0, 0.0), (KT.GAMMAEXP, 1, 1.3)]),
            (0.3, None, None, [(KT.MATERN_NU, 0, 1.25), (KT.LINEAR, 1, 0.4)]),
            (0.2, None, None, [(KT.MATERN_NU, 1, 0.3), (KT.MATERN12, 0, 0.0), (KT.LINEAR, 2, 0.6)]),
            (0.15, None, None, [(KT.MATERN_NU, 0, 3.7), (KT.CONST, 0, 0.8)])]
    chains, t = [], 0
    for coef, a, b, fac in spec:
        chains.append(dict(I=0, J=0, head=t, coef=coef, rs=a, cs=b,
                           factors=[(t + i, kind, r(v), c(v), param) for i, (kind, v, param) in enumerate(fac)]))
        t += len(fac)
    return chains


def _views(X):
    return [X, 0.7 * X, 0.5 * X[:1]]


def pin_problem():
    rng = np.random.default_rng(79)
    X, Z = (rng.standard_normal((D, k)) / np.sqrt(D) * 1.5 for k in (N, M))
    y, mean = rng.standard_normal(N), 0.1 * rng.standard_normal(N)
    sx, sz = 1.0 + 0.3 * np.sin(X.sum(0)), 1.0 + 0.3 * np.sin(Z.sum(0))
    w = rng.standard_normal(N)
    xx = KT.hand_spec(_chains(0, 0, sx, sx), _views(X), [N], [N], True)
    zz = KT.hand_spec(_chains(0, 0, sz, sz), _views(Z), [M], [M], True)
    xz = KT.hand_spec(_chains(0, 3, sx, sz), _views(X) + _views(Z), [N], [M], False)
    # the diagonal between two views that differ: rows read the views of X, columns those of 1.2 X
    dg = KT.hand_spec(_chains(0, 3, sx, sx), _views(X) + _views(1.2 * X), [N], [N], True)
    return dict(xx=xx, zz=zz, xz=xz, dg=dg, y=y, mean=mean, w=w)


def long_double_run(dt=None):
    """{family key: (values, scales)} of kprod_grad_truth on the pin problem"""
    dt = dt or KT.require_extended()
    P = pin_problem()
    out = {}

    def put(key, v, s):
        v = np.asarray(v)
        out[key] = (np.atleast_1d(v).ravel(), np.atleast_1d(np.broadcast_to(np.asarray(s), v.shape)).ravel())

    def put_terms(prefix, r, scales):
        for key in ("coef", "inscale", "param"):
            put(f"{prefix}.d_{key}", r["d_" + key], KT.scale_scalar(r["d_" + key], r["S_" + key], r["n_rows"]))
        for k, (g, s) in enumerate(zip(r["gx"], r["Sn_gx"])):
            put(f"{prefix}.inputs.{k}", g, KT.scale_entries(g, s))
        for side in scales:
            put(f"{prefix}.{side}", r[side][0], KT.scale_entries(r[side][0], r["Sn_" + side][0]))

    R = KT.logpdf_grad(P["xx"], KT.NOISE_SCALAR, NOISE, P["mean"], P["y"], dt, inputs=True, scales=True)
    put("kp.value", R["value"], KT.scale_scalar(R["value"], R["S_value"], N))
    put("kp.y", R["alpha"], KT.scale_entries(R["alpha"], R["S_alpha"] / N))
    put("kp.noise", R["noise"], KT.scale_scalar(R["noise"], R["S_noise"], N))
    put_terms("kp", R, ("rowscale",))
    E = KT.elbo_grad(P["zz"], P["xz"], P["xx"], KT.NOISE_SCALAR, NOISE, KT.NOISE_SCALAR, Z_NOISE, P["mean"], P["y"], dt,
                     inputs=True)
    put("kpelbo.value", E["value"], KT.scale_scalar(E["value"], E["S_value"], N))
    put("kpelbo.y", E["y"], KT.scale_entries(E["y"], E["S_y"] / M))
    put("kpelbo.noise", E["noise"], KT.scale_scalar(E["noise"], E["S_noise"], N))
    put("kpelbo.z_noise", E["z_noise"], KT.scale_scalar(E["z_noise"], E["S_z_noise"], M))
    put_terms("kpelbo.zz", E["zz"], ("rowscale",))
    put_terms("kpelbo.xz", E["xz"], ("rowscale", "colscale"))
    for tag, S in (("kpdiag.same", P["xx"]), ("kpdiag.views", P["dg"])):
        Dg = KT.diag_grad(S, P["w"], dt)
        for key in ("coef", "inscale", "param"):
            put(f"{tag}.d_{key}", Dg["d_" + key], np.maximum(np.abs(Dg["d_" + key]), Dg["S_" + key] / N))
        for k, (g, s) in enumerate(zip(Dg["gx"], Dg["S_gx"])):
            put(f"{tag}.inputs.{k}", g, KT.scale_entries(g, s))
        for side in ("rowscale", "colscale"):
            put(f"{tag}.{side}", Dg[side][0], KT.scale_entries(Dg[side][0], np.abs(Dg[side][0])))
    return out


# ---- the same in mpmath --------------------------------------------------------------------------------------------------------------
def _mp_factor(mp, kind, param, xr, xc):
    """(k, d k / d (d^2) or None, d k / d g, d k / d param) between two points (lists of mpf)"""
    if kind == KT.LINEAR:
        s = sum(a * b for a, b in zip(xr, xc))
        return s + mp.mpf(param), None, 2 * s, mp.mpf(1)
    d2 = sum((a - b) ** 2 for a, b in zip(xr, xc))
    d = mp.sqrt(d2)
    zero = mp.mpf(0)
    if kind == KT.CONST:
        return mp.mpf(param), zero, zero, mp.mpf(1)
    if kind == KT.WHITE:
        return mp.mpf(1 if d2 == 0 else 0), zero, zero, zero
    if kind == KT.SE:
        k = mp.exp(-d2 / 2)
        return k, -k / 2, -d2 * k, zero
    if kind == KT.MATERN12:
        k = mp.exp(-d)
        return k, (-k / (2 * d) if d2 > 0 else zero), -d * k, zero
    if kind == KT.MATERN32:
        s = mp.sqrt(3) * d
        return (1 + s) * mp.exp(-s), -mp.mpf(3) / 2 * mp.exp(-s), -3 * d2 * mp.exp(-s), zero
    if kind == KT.MATERN52:
        s = mp.sqrt(5) * d
        kp = -mp.mpf(5) / 6 * (1 + s) * mp.exp(-s)
        return (1 + s + s * s / 3) * mp.exp(-s), kp, 2 * d2 * kp, zero
    if kind == KT.RQ:
        al = mp.mpf(param)
        u = d2 / (2 * al)
        k = mp.power(1 + u, -al)
        return k, -mp.power(1 + u, -al - 1) / 2, -d2 * mp.power(1 + u, -al - 1), k * (u / (1 + u) - mp.log(1 + u))
    if kind == KT.COSINE:
        if d2 == 0:
            return mp.mpf(1), -mp.pi ** 2 / 2, zero, zero
        return mp.cos(mp.pi * d), -mp.pi * mp.sin(mp.pi * d) / (2 * d), -mp.pi * d * mp.sin(mp.pi * d), zero
    if kind == KT.GAMMAEXP:
        if d2 == 0:
            return mp.mpf(1), zero, zero, zero
        gm = mp.mpf(param)
        a = mp.power(d, gm)
        k = mp.exp(-a)
        return k, -(gm / 2) * a * k / d2, -gm * a * k, -k * a * mp.log(d2) / 2
    if kind == KT.MATERN_NU:
        v = mp.mpf(param)
        if d2 == 0:
            return mp.mpf(1), (-v / (2 * (v - 1)) if param > 1.0 else zero), zero, zero
        x = mp.sqrt(2 * v) * d
        c = mp.power(2, 1 - v) / mp.gamma(v) * mp.power(x, v)
        kx = -(v / x) * c * mp.besselk(v - 1, x)
        return c * mp.besselk(v, x), kx, 2 * d2 * kx, zero
    raise ValueError(kind)


class _MpSpec:
    """a hand spec evaluated entry by entry: F[c][f][i][j] = the factor's four numbers (diag: pairs (i, i) only)"""

    def __init__(self, mp, S, diag=False):
        self.mp, self.S, self.diag = mp, S, diag
        self.X = [[[mp.mpf(float(a[d, i])) for d in range(a.shape[0])] for i in range(a.shape[1])] for a in S["inputs"]]
        self.nr, self.nc = S["row_len"][0], S["col_len"][0]
        self.F = []
        for ch in S["chains"]:
            per = []
            for (_, kind, ri, ci, param) in ch["factors"]:
                per.append([[(_mp_factor(mp, kind, param, self.X[ri][i], self.X[ci][j]) if (not diag or i == j) else None)
                             for j in range(self.nc)] for i in range(self.nr)])
            self.F.append(per)

    def weights(self, c, i, j):
        ch, m = self.S["chains"][c], self.mp.mpf
        return (m(ch["coef"]), m(1) if ch["rs"] is None else m(float(ch["rs"][i])), m(1) if ch["cs"] is None else m(float(ch["cs"][j])))

    def prod(self, c, i, j, skip=None):
        p = self.mp.mpf(1)
        for f, per in enumerate(self.F[c]):
            if f != skip:
                p *= per[i][j][0]
        return p

    def matrix(self):
        K = self.mp.matrix(self.nr, self.nc)
        for c in range(len(self.F)):
            for i in range(self.nr):
                for j in range(self.nc):
                    coef, r, s = self.weights(c, i, j)
                    K[i, j] += coef * r * s * self.prod(c, i, j)
        return K

    def diagonal(self):
        return [sum(self.weights(c, i, i)[0] * self.weights(c, i, i)[1] * self.weights(c, i, i)[2] * self.prod(c, i, i)
                    for c in range(len(self.F))) for i in range(self.nr)]

    def contract(self, G, out, prefix, scales):
        """the documented sums for the cotangent G (a function (i, j) -> mpf; diag: (i, i) only)"""
        mp, S = self.mp, self.S
        sym = S["symmetric"] and not self.diag
        side = 2 if sym else 1
        nt = S["n_terms"]
        dc, ds, dp = [mp.mpf(0)] * nt, [mp.mpf(0)] * nt, [mp.mpf(0)] * nt
        gx = [[[mp.mpf(0)] * len(pts) for _ in range(len(pts[0]))] for pts in self.X]
        pairs = [(i, i) for i in range(self.nr)] if self.diag else [(i, j) for i in range(self.nr) for j in range(self.nc)]
        rsum, csum = [mp.mpf(0)] * self.nr, [mp.mpf(0)] * self.nc
        for c, ch in enumerate(S["chains"]):
            for (i, j) in pairs:
                coef, r, s = self.weights(c, i, j)
                g = G(i, j)
                full = self.prod(c, i, j)
                dc[ch["head"]] += g * r * s * full
                if c == 0:
                    rsum[i] += side * g * coef * s * full
                    csum[j] += g * coef * r * full
                for f, (t, kind, ri, ci, param) in enumerate(ch["factors"]):
                    k, kp, dk, dpar = self.F[c][f][i][j]
                    A = g * coef * r * s * self.prod(c, i, j, skip=f)
                    ds[t] += A * dk
                    dp[t] += A * dpar
                    xr, xc = self.X[ri][i], self.X[ci][j]
                    for d in range(len(xr)):
                        if kind == KT.LINEAR:
                            gx[ri][d][i] += side * A * xc[d]
                            if not sym:
                                gx[ci][d][j] += A * xr[d]
                        else:
                            v = 2 * A * kp * (xr[d] - xc[d])
                            gx[ri][d][i] += side * v
                            if not sym:
                                gx[ci][d][j] -= v
        out[prefix + ".d_coef"], out[prefix + ".d_inscale"], out[prefix + ".d_param"] = dc, ds, dp
        for k, g in enumerate(gx):
            out[f"{prefix}.inputs.{k}"] = [v for row in g for v in row]
        if "rowscale" in scales:
            out[prefix + ".rowscale"] = rsum
        if "colscale" in scales:
            out[prefix + ".colscale"] = csum


def pin_values():
    """{family key: [decimal strings]} of the pin problem at 40 digits, in the layout of long_double_run"""
    mp = _mp()
    P = pin_problem()
    m = lambda v: mp.mpf(float(v))      # noqa: E731
    out = {}
    xx, zz, xz = _MpSpec(mp, P["xx"]), _MpSpec(mp, P["zz"]), _MpSpec(mp, P["xz"])
    delta = mp.matrix([m(P["y"][i]) - m(P["mean"][i]) for i in range(N)])
    log2pi = mp.log(2 * mp.pi)
    # logpdf
    Cm = xx.matrix()
    for i in range(N):
        Cm[i, i] += m(NOISE)
    Ci = mp.inverse(Cm)
    alpha = Ci * delta
    out["kp.value"] = [-(N * log2pi + mp.log(mp.det(Cm)) + (delta.T * alpha)[0]) / 2]
    out["kp.y"] = list(alpha)
    out["kp.noise"] = [sum((alpha[i] * alpha[i] - Ci[i, i]) / 2 for i in range(N))]
    xx.contract(lambda i, j: (alpha[i] * alpha[j] - Ci[i, j]) / 2, out, "kp", ("rowscale",))
    # the ELBO in the dense Titsias form: Q = Kxz Kzz^-1 Kzx, elbo = log N(y; m, Q + s I) - tr(Kxx - Q) / (2 s); its
    # cotangents through S = Q + s I: T = (beta beta' - S^-1) / 2 + I / (2 s), beta = S^-1 delta
    s2 = m(NOISE)
    Kzz = zz.matrix()
    for i in range(M):
        Kzz[i, i] += m(Z_NOISE)
    Kxz = xz.matrix()
    var = xx.diagonal()
    Kzzi = mp.inverse(Kzz)
    W = Kxz * Kzzi
    Q = W * Kxz.T
    Sm = Q.copy()
    for i in range(N):
        Sm[i, i] += s2
    Si = mp.inverse(Sm)
    beta = Si * delta
    trace = sum(var[i] - Q[i, i] for i in range(N))
    out["kpelbo.value"] = [-(N * log2pi + mp.log(mp.det(Sm)) + (delta.T * beta)[0]) / 2 - trace / (2 * s2)]
    out["kpelbo.y"] = [-b for b in beta]
    Tm = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            Tm[i, j] = (beta[i] * beta[j] - Si[i, j]) / 2 + (1 / (2 * s2) if i == j else 0)
    out["kpelbo.noise"] = [sum((beta[i] * beta[i] - Si[i, i]) / 2 for i in range(N)) + trace / (2 * s2 * s2)]
    dKxz = 2 * Tm * W                       # d / d Kxz of sum(T * (Kxz Kzz^-1 Kzx))
    dKzz = -(W.T * Tm * W)                  # d / d Kzz of the same
    out["kpelbo.z_noise"] = [sum(dKzz[i, i] for i in range(M))]
    zz.contract(lambda i, j: dKzz[i, j], out, "kpelbo.zz", ("rowscale",))
    xz.contract(lambda i, j: dKxz[i, j], out, "kpelbo.xz", ("rowscale", "colscale"))
    for tag, S in (("kpdiag.same", P["xx"]), ("kpdiag.views", P["dg"])):
        sp = _MpSpec(mp, S, diag=True)
        sp.contract(lambda i, j: m(P["w"][i]), out, tag, ("rowscale", "colscale"))
    return {k: [_str(mp, v) for v in vals] for k, vals in out.items()}
