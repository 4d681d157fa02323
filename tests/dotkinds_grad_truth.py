"""Extended-precision truth for the gradients through chains that hold the NeuralNetwork, FBM and Exponentiated kinds
(include/sthenomi_kprod.h: codes 24, 25, 26).  TEST INFRASTRUCTURE ONLY.

A dtype-generic restatement of the three kinds on top of tests/kprod_grad_truth.py (imported as KT, not edited): every other
kind, the chain product, the factorisation, the ELBO's cotangents and the units are that module's and grad_truth's; what is
written here are the three kinds straight from the header's definitions in the working dtype -- k, d k / d g, d k / d param
and the point derivatives d k / d x = c1 x + c2 (x - y) + c3 y, d k / d y = c1y y + c2 (y - x) + c3 x -- and `dense`,
`diag_of` and `contract` over chains that may hold them (KT's own contract knows LINEAR and the distance kinds only).  Run in
np.longdouble it is the truth, twice in np.float64 (the column recurrence and LAPACK's blocked order) the yardstick.

The cases (CASES below; about ten, as small as the kernels' paths allow: blocks (129, 1, 70), N = 200; ELBO: inducing blocks
(33, 1)): each kind alone, each times SE, NEURALNET x FBM x LINEAR, NEURALNET x general-nu Matern x FBM, scalar and diagonal
noise, one ELBO case per kind.  The device's kp.* / kpelbo.* families are held to MARGIN * max(e_float64 of the case, the
family's floor) (tests/test_gpu_dotkinds_grad_truth.py), MARGIN from tests/grad_truth.py.  FLOORS: the medians of this
reference's own float64 figures over CASES, printed by `python tests/dotkinds_grad_truth.py` and written down below.
Nothing is taken from a device."""
import os
import sys

import numpy as np

import grad_truth as T
import kprod_grad_truth as KT
from kprod_grad_truth import EPS, MARGIN, NOISE_DIAG, NOISE_SCALAR  # noqa: F401

NEURALNET, FBM, EXPONENTIATED = 24, 25, 26
DOT = (NEURALNET, FBM, EXPONENTIATED)


def _outer(X, Y, diag):
    """(x, y) broadcast so that x[d] op y[d] is n (diag) or n x m"""
    return (X, Y) if diag else (X[:, :, None], Y[:, None, :])


def factor(kind, X, Y, param, dt, diag=False):
    """KT.factor with the three kinds: dict(k, kp, dk, dp) plus, for them, c1, c1y, c2, c3 (kp None)"""
    if kind not in DOT:
        return KT.factor(kind, X, Y, param, dt, diag)
    x, y = _outer(X, Y, diag)
    zero, one, two, half = dt(0), dt(1), dt(2), dt(1) / dt(2)
    s, a, b = (x * y).sum(0), (x * x).sum(0) + zero * (y * y).sum(0), zero * (x * x).sum(0) + (y * y).sum(0)
    z = zero * s
    if kind == EXPONENTIATED:
        k = np.exp(s)
        return dict(k=k, kp=None, dk=two * s * k, dp=z, c1=z, c1y=z, c2=z, c3=k)
    if kind == FBM:
        h = dt(param)
        d2 = ((x - y) ** 2).sum(0)

        def pw(v):
            safe = np.where(v > 0, v, one)
            p = np.where(v > 0, np.power(safe, h), zero)
            return p, p * np.where(v > 0, np.log(safe), zero), np.where(v > 0, h * np.power(safe, h - one), zero)
        (pa, la, ma), (pb, lb, mb), (pd, ld, md) = pw(a), pw(b), pw(d2)
        k = half * (pa + pb - pd)
        return dict(k=k, kp=None, dk=two * h * k, dp=half * (la + lb - ld), c1=ma, c1y=mb, c2=-md, c3=z)
    D = X.shape[0]
    lag = z
    for i in range(D):
        for j in range(i + 1, D):
            c = x[i] * y[j] - x[j] * y[i]
            lag = lag + c * c
    R = np.sqrt(one + a + b + lag)
    ia, ib = one / (one + a), one / (one + b)
    return dict(k=np.arctan2(s, R), kp=None, dk=s * (ia + ib) / R, dp=z, c1=-(s * ia) / R, c1y=-(s * ib) / R, c2=z, c3=one / R)


def dense(S, dt):
    X_in = [a.astype(dt) for a in S["inputs"]]
    roff, coff = KT._offsets(S)
    K = np.zeros((roff[-1], coff[-1]), dtype=dt)
    for ch in S["chains"]:
        ks = [factor(kind, X_in[ri], X_in[ci], param, dt)["k"] for (_, kind, ri, ci, param) in ch["factors"]]
        blk = dt(ch["coef"]) * KT._product(ks, ks[0])
        rs, cs = KT._scale_vectors(ch, dt)
        if rs is not None:
            blk = rs[:, None] * blk
        if cs is not None:
            blk = blk * cs[None, :]
        K[roff[ch["I"]]:roff[ch["I"] + 1], coff[ch["J"]]:coff[ch["J"] + 1]] += blk
    return K


def diag_of(S, dt):
    X_in = [a.astype(dt) for a in S["inputs"]]
    roff, _ = KT._offsets(S)
    v = np.zeros(roff[-1], dtype=dt)
    for ch in S["chains"]:
        if ch["I"] != ch["J"]:
            continue
        ks = [factor(kind, X_in[ri], X_in[ci], param, dt, diag=True)["k"] for (_, kind, ri, ci, param) in ch["factors"]]
        rs, cs = KT._scale_vectors(ch, dt)
        v[roff[ch["I"]]:roff[ch["I"] + 1]] += dt(ch["coef"]) * KT._product(ks, ks[0]) * (1 if rs is None else rs) * (1 if cs is None else cs)
    return v


def contract(S, G, dt, inputs=False, scales=False):
    """KT.contract (same outputs, same conventions: a symmetric spec's row side carries the factor 2 of the mirror block) over
    chains that may hold the three kinds"""
    X_in = [a.astype(dt) for a in S["inputs"]]
    sym = S["symmetric"]
    roff, coff = KT._offsets(S)
    nt = S["n_terms"]
    out = dict(n_rows=np.ones(nt, dt))
    for key in ("coef", "inscale", "param"):
        out["d_" + key], out["S_" + key] = np.zeros(nt, dt), np.zeros(nt, dt)
    if inputs:
        out["gx"] = [np.zeros(a.shape, dt) for a in X_in]
        out["Sn_gx"] = [np.zeros(a.shape, dt) for a in X_in]
    if scales:
        out["rowscale"], out["Sn_rowscale"] = [None] * nt, [None] * nt
        out["colscale"], out["Sn_colscale"] = [None] * nt, [None] * nt
    two = dt(2)
    side = two if sym else dt(1)
    for ch in S["chains"]:
        I, J, h, coef = ch["I"], ch["J"], ch["head"], dt(ch["coef"])
        rs, cs = KT._scale_vectors(ch, dt)
        fs = [factor(kind, X_in[ri], X_in[ci], param, dt) for (_, kind, ri, ci, param) in ch["factors"]]
        g = G[roff[I]:roff[I + 1], coff[J]:coff[J + 1]]
        nr, nc = g.shape
        w = g
        if rs is not None:
            w = w * rs[:, None]
        if cs is not None:
            w = w * cs[None, :]
        full = KT._product([f["k"] for f in fs], fs[0]["k"])
        a = w * full
        out["d_coef"][h], out["S_coef"][h] = a.sum(), np.abs(a).sum()
        wc = coef * w
        for ia, (t, kind, ri, ci, param) in enumerate(ch["factors"]):
            out["n_rows"][t] = max(nr, 1)
            A = wc * KT._product([f["k"] for ib, f in enumerate(fs) if ib != ia], fs[0]["k"])
            for key, q in (("inscale", fs[ia]["dk"]), ("param", fs[ia]["dp"])):
                a = A * q
                out["d_" + key][t], out["S_" + key][t] = a.sum(), np.abs(a).sum()
            if not inputs:
                continue
            X, Y = X_in[ri], X_in[ci]
            f, absA = fs[ia], np.abs(A)
            for d in range(X.shape[0]):
                xd, yd = X[d][:, None], Y[d][None, :]
                if kind in DOT:         # (c1, c2, c3) on (x, x - y, y); the column point's: (c1y, c2, c3) on (y, y - x, x)
                    rows = (f["c1"] * xd, f["c2"] * (xd - yd), f["c3"] * yd)
                    cols = (f["c1y"] * yd, f["c2"] * (yd - xd), f["c3"] * xd)
                elif kind == KT.LINEAR:
                    rows, cols = (yd + 0 * xd,), (xd + 0 * yd,)
                else:
                    rows = (two * f["kp"] * (xd - yd),)
                    cols = (-rows[0],)
                out["gx"][ri][d] += (side * A * sum(rows)).sum(1)
                out["Sn_gx"][ri][d] += (side * absA * sum(np.abs(r) for r in rows)).sum(1) / max(nc, 1)
                if not sym:
                    out["gx"][ci][d] += (A * sum(cols)).sum(0)
                    out["Sn_gx"][ci][d] += (absA * sum(np.abs(c) for c in cols)).sum(0) / max(nr, 1)
        if scales:
            base = coef * g * full
            if rs is not None:
                wcs = base if cs is None else base * cs[None, :]
                out["rowscale"][h] = side * wcs.sum(1)
                out["Sn_rowscale"][h] = side * np.abs(wcs).sum(1) / max(nc, 1)
            if cs is not None and not sym:
                wrs = base if rs is None else base * rs[:, None]
                out["colscale"][h] = wrs.sum(0)
                out["Sn_colscale"][h] = np.abs(wrs).sum(0) / max(nr, 1)
    return out


class _Ops:
    dense, diag_of = staticmethod(dense), staticmethod(diag_of)

    @staticmethod
    def contract(S, G, dt, inputs=False, scales=True):
        return contract(S, G, dt, inputs=inputs, scales=scales)


def logpdf_grad(S, noise_kind, noise, mean, y, dt, inputs=False, scales=False, cholesky=None):
    return T.logpdf_grad(S, noise_kind, noise, mean, y, dt, inputs=inputs, scales=scales, cholesky=cholesky, ops=_Ops)


def elbo_grad(Szz, Sxz, Sxx, noise_kind, noise, z_noise_kind, z_noise, mean, y, dt, inputs=False, cholesky=None):
    """sgp_elbo_grad_param's zz and xz sides (the diagonal's own outputs are not part of the kp.* / kpelbo.* families)"""
    return T.elbo_grad(Szz, Sxz, Sxx, noise_kind, noise, z_noise_kind, z_noise, mean, y, dt, inputs=inputs, cholesky=cholesky, ops=_Ops)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
LAYOUT, Z_LAYOUT = (129, 1, 70), (33, 1)


def _kernels():
    import stheno_jl_amd as P
    wl = P.with_lengthscale
    NN, FB, EX, SE = P.NeuralNetworkKernel, P.FBMKernel, P.ExponentiatedKernel, P.SEKernel
    return {"nn": lambda: 0.6 * wl(NN(), 0.8), "fbm": lambda: 0.5 * FB(0.7), "exp": lambda: 0.3 * wl(EX(), 2.0),
            "nn-se": lambda: 0.8 * wl(SE(), 1.3) * wl(NN(), 0.7) + 0.2 * wl(P.Matern32Kernel(), 1.5),
            "fbm-se": lambda: 0.7 * wl(SE(), 1.4) * FB(0.4) + 0.2 * wl(P.Matern52Kernel(), 1.2),
            "exp-se": lambda: 0.5 * wl(SE(), 1.2) * wl(EX(), 2.5) + 0.2 * P.RationalQuadraticKernel(0.9),
            "nn-fbm-lin": lambda: 0.5 * wl(NN(), 0.9) * FB(0.6) * P.LinearKernel(0.4) + 0.3 * wl(SE(), 1.5),
            "nn-mn-fbm": lambda: 0.7 * wl(NN(), 1.1) * wl(P.GeneralMaternKernel(0.8), 1.2) * FB(0.6) + 0.2 * wl(SE(), 1.3)}


# (id, kind of case, kernel, D, noise): "diag" noise is a vector; every case asks for inputs
CASES = [("dk-nn-D1", "lp", "nn", 1, "scalar"), ("dk-fbm-D3", "lp", "fbm", 3, "diag"), ("dk-exp-D8", "lp", "exp", 8, "scalar"),
         ("dk-nn-se-D16", "lp", "nn-se", 16, "diag"), ("dk-fbm-se-D2", "lp", "fbm-se", 2, "scalar"),
         ("dk-exp-se-D3", "lp", "exp-se", 3, "scalar"), ("dk-nn-fbm-lin-D8", "lp", "nn-fbm-lin", 8, "scalar"),
         ("dk-nn-mn-fbm-D2", "lp", "nn-mn-fbm", 2, "diag"),
         ("dkelbo-nn-D2", "elbo", "nn-se", 2, "scalar"), ("dkelbo-fbm-D1", "elbo", "fbm-se", 1, "scalar"),
         ("dkelbo-exp-D8", "elbo", "exp-se", 8, "scalar")]


def problem(case):
    """(F, x, z or None, noise, y) of a case; points standard_normal / sqrt(D) * 1.5, one exact duplicate and a point at the
    origin in the first block"""
    import stheno_jl_amd as P
    cid, what, kname, D, noise_kind = case
    rng = np.random.default_rng(9000 + [c[0] for c in CASES].index(cid))
    F = P.gppp(lambda GP: {"f": GP(_kernels()[kname]())})

    def blocks(layout):
        X = rng.standard_normal((D, sum(layout))) / np.sqrt(D) * 1.5
        X[:, 5], X[:, 11] = X[:, 3], 0.0
        off = np.concatenate([[0], np.cumsum(layout)])
        return P.BlockData([P.GPPPInput("f", P.ColVecs(np.asfortranarray(X[:, off[i]:off[i + 1]]))) for i in range(len(layout))])
    x = blocks(LAYOUT)
    z = blocks(Z_LAYOUT) if what == "elbo" else None
    n = sum(LAYOUT)
    noise = 0.05 + 0.25 * rng.random(n) if noise_kind == "diag" else float(0.05 + 0.25 * rng.random())
    return F, x, z, noise, rng.standard_normal(n)


def _runs():
    return ((KT.require_extended(), None), (np.float64, None), (np.float64, KT.cholesky_blocked_order))


_TRUTH = {}


def truth(case):
    """(long double, float64, float64 in the blocked order): computed once per case, shared, never modified"""
    import stheno_jl_amd as P
    if case[0] not in _TRUTH:
        F, x, z, noise, y = problem(case)
        mean = P.mean(F(x, noise))
        nk = NOISE_DIAG if np.ndim(noise) else NOISE_SCALAR
        if z is None:
            S = KT.read_spec(P.build_spec(F, x)[0])
            _TRUTH[case[0]] = tuple(logpdf_grad(S, nk, noise, mean, y, dt, inputs=True, scales=True, cholesky=ch) for dt, ch in _runs())
        else:
            Ss = [KT.read_spec(sp) for sp in (P.build_spec(F, z)[0], P.build_spec(F, x, None, z)[0], P.build_spec(F, x)[0])]
            _TRUTH[case[0]] = tuple(elbo_grad(*Ss, nk, noise, NOISE_SCALAR, 1e-2, mean, y, dt, inputs=True, cholesky=ch)
                                    for dt, ch in _runs())
    return _TRUTH[case[0]]


def logpdf_units(out, R):
    """KT.logpdf_units; with a diagonal Sigma_y the noise gradient is a vector of sums, scaled entry by entry as KT.elbo_units
    scales it: max(the largest entry, the entry's own absolute addends) -- an entry that cancels to nothing is not held to
    its own size"""
    u = KT.logpdf_units(out, R)
    if np.ndim(R["noise"]):
        u["kp.noise"] = T.units(out["noise"], R["noise"], T.scale_entries(R["noise"], R["S_noise"]))
    return u


def reference_figures(case):
    """e_float64 of a case: family by family the larger figure of the two float64 runs against the long-double run"""
    R, *R64 = truth(case)
    if case[1] == "lp":
        runs = [logpdf_units(KT.logpdf_reference_outputs(r), R) for r in R64]
    else:
        runs = [KT.elbo_units(dict(KT.elbo_reference_outputs(dict(r, xx=None))), R) for r in R64]
    return {fam: max(r[fam] for r in runs) for fam in runs[0]}


# the medians of reference_figures over CASES (sorted lists first), printed by `python tests/dotkinds_grad_truth.py`
MEASURED_FLOAT64 = {'kp.d_coef': [116.0, 118.9, 231.3, 491.8, 750.0, 1821.9, 2533.3, 4371.3],
                    'kp.d_inscale': [75.3, 172.0, 232.4, 492.5, 584.6, 707.5, 2292.7, 4374.7],
                    'kp.d_param': [0.0, 0.0, 0.0, 134.9, 230.8, 347.1, 491.4, 16583.8],
                    'kp.inputs': [29.5, 38.1, 94.9, 103.5, 108.0, 200.0, 620.7, 815.3],
                    'kp.noise': [5.9, 8.4, 11.1, 17.0, 18.9, 43.8, 62.8, 110.5],
                    'kp.value': [1.2, 1.6, 2.4, 3.0, 3.8, 7.0, 10.6, 16.1],
                    'kp.y': [9.4, 11.1, 31.0, 39.9, 56.1, 62.3, 117.1, 162.6],
                    'kpelbo.d_coef': [760.9, 797.8, 1557.1], 'kpelbo.d_inscale': [427.6, 842.7, 2799.7],
                    'kpelbo.d_param': [0.0, 229.0, 398.4], 'kpelbo.inputs': [120.0, 584.2, 932.0],
                    'kpelbo.noise': [1.2, 2.8, 3.0], 'kpelbo.value': [1.9, 2.0, 4.5], 'kpelbo.y': [12.1, 15.7, 32.4],
                    'kpelbo.z_noise': [3.1, 32.6, 38.8]}
FLOORS = {fam: float(np.median(v)) for fam, v in MEASURED_FLOAT64.items()}


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    entry.load_package()
    figs = {}
    for case in CASES:
        for fam, v in reference_figures(case).items():
            figs.setdefault(fam, []).append(round(float(v), 1))
    print("MEASURED_FLOAT64 =", {k: sorted(v) for k, v in sorted(figs.items())})
    print("FLOORS =", {k: float(np.median(v)) for k, v in sorted(figs.items())})


if __name__ == "__main__":
    main()
