"""NumPy (float64) formulas of the NeuralNetwork, FBM and Exponentiated kinds (csrc/kprod.hip: dotkind_eval / dotkind_derivs)
in the library's own formulation, and the evaluators of tests/kprod_np.py and tests/kprod_grad_np.py extended to them.  TEST
INFRASTRUCTURE ONLY (tests/test_dotkinds_truth_on_numpy.py holds the formulas to the 60-digit table;
tests/test_gpu_dotkinds.py holds the library to them).

The three kinds are functions of s = x'y, a = x'x, b = y'y and of one more scalar formed from the points directly:
    FBM         d2 = |x - y|^2 from direct differences (never a + b - 2 s)
    NEURALNET   L = sum_{i<j} (x_i y_j - x_j y_i)^2 = a b - s^2 (Lagrange's identity), R^2 = ((a + b) + 1) + L
Point derivatives come as three coefficients: d k / d x = c1 x + c2 (x - y) + c3 y, d k / d y = c1y y + c2 (y - x) + c3 x.

install(monkeypatch) makes kprod_np.factor, kprod_grad_np.np_input_grads and kprod_grad_np.np_diag_grads know kinds 24 .. 26;
every other kind is passed on to the definition that was there (kinds_np's, matern_nu_np's if installed before)."""
import numpy as np

import kinds_np  # noqa: F401  (COSINE / GAMMAEXP in kprod_np.factor and kprod_grad_np.kappa_prime)
import kprod_grad_np as kg
import kprod_np as kn
from stheno_jl_amd import lib as L

DOT_KINDS = (L.NEURALNET, L.FBM, L.EXPONENTIATED)


def is_dot(kind):
    return (int(kind) & L.KIND_MASK) in DOT_KINDS


def scalars(Xr, Xc):
    """(s, a, b, d2, L) between the columns of Xr (D x n) and Xc (D x m); a is n x 1, b is 1 x m"""
    Xr, Xc = np.asarray(Xr, dtype=np.float64), np.asarray(Xc, dtype=np.float64)
    D = Xr.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.zeros((Xr.shape[1], Xc.shape[1]))
        a, b = np.zeros((Xr.shape[1], 1)), np.zeros((1, Xc.shape[1]))
        d2, lag = np.zeros_like(s), np.zeros_like(s)
        for d in range(D):
            s = s + Xr[d][:, None] * Xc[d][None, :]
            a = a + (Xr[d] * Xr[d])[:, None]
            b = b + (Xc[d] * Xc[d])[None, :]
            df = Xr[d][:, None] - Xc[d][None, :]
            d2 = d2 + df * df
        for i in range(D):
            for j in range(i + 1, D):
                c = Xr[i][:, None] * Xc[j][None, :] - Xr[j][:, None] * Xc[i][None, :]
                lag = lag + c * c
    return s, a, b, d2, lag


def _pow0(v, h):
    """v^h with 0^h = 0"""
    with np.errstate(over="ignore"):
        return np.where(v > 0.0, np.power(np.where(v > 0.0, v, 1.0), h), 0.0)


def _powlog0(v, h):
    """v^h log v with 0^h log 0 := 0"""
    w = np.where(v > 0.0, v, 1.0)
    return np.where(v > 0.0, np.power(w, h) * np.log(w), 0.0)


def _powm1(v, h):
    """h v^h / v, the library's h v^(h - 1); 0 at v = 0"""
    w = np.where(v > 0.0, v, 1.0)
    return np.where(v > 0.0, h * np.power(w, h) / w, 0.0)


def derivs(kind, Xr, Xc, param):
    """dict(k, dk, dp, c1, c1y, c2, c3) of n x m arrays (broadcastable), the library's formulas"""
    code = int(kind) & L.KIND_MASK
    s, a, b, d2, lag = scalars(Xr, Xc)
    z = np.zeros_like(s)
    with np.errstate(over="ignore", invalid="ignore"):
        if code == L.EXPONENTIATED:
            k = np.exp(s)
            return dict(k=k, dk=2.0 * s * k, dp=z, c1=z, c1y=z, c2=z, c3=k)
        if code == L.FBM:
            h = float(param)
            pa, pb, pd = _pow0(a, h), _pow0(b, h), _pow0(d2, h)
            k = 0.5 * ((pa + pb) - pd)
            dp = 0.5 * ((_powlog0(a, h) + _powlog0(b, h)) - _powlog0(d2, h))
            return dict(k=k, dk=2.0 * h * k, dp=dp, c1=_powm1(a, h) + z, c1y=_powm1(b, h) + z, c2=-_powm1(d2, h), c3=z)
        if code == L.NEURALNET:
            R = np.sqrt(((a + b) + 1.0) + lag)
            ia, ib = 1.0 / (1.0 + a), 1.0 / (1.0 + b)
            return dict(k=np.arctan2(s, R), dk=s * (ia + ib) / R, dp=z, c1=-(s * ia) / R, c1y=-(s * ib) / R, c2=z, c3=1.0 / R + z)
    raise ValueError(kind)


def neuralnet_textbook(Xr, Xc):
    """asin(s / sqrt((1 + a)(1 + b))): the form the library does NOT use (it loses everything near |u| = 1)"""
    s, a, b, _, _ = scalars(Xr, Xc)
    return np.arcsin(np.clip(s / np.sqrt((1.0 + a) * (1.0 + b)), -1.0, 1.0))


def point_derivs(kind, Xr, Xc, param):
    """(d k / d x, d k / d y), each D x n x m, of ANY kind the evaluators know: the three kinds' coefficient form, LINEAR's
    (x', x), a distance kind's +- 2 kappa'(d2) (x - x') from direct differences"""
    Xr, Xc = np.asarray(Xr, dtype=np.float64), np.asarray(Xc, dtype=np.float64)
    xv, yv = Xr[:, :, None], Xc[:, None, :]
    code = int(kind) & L.KIND_MASK
    if code in DOT_KINDS:
        r = derivs(kind, Xr, Xc, param)
        with np.errstate(over="ignore", invalid="ignore"):
            return (r["c1"][None] * xv + r["c2"][None] * (xv - yv) + r["c3"][None] * yv,
                    r["c1y"][None] * yv + r["c2"][None] * (yv - xv) + r["c3"][None] * xv)
    if code == L.LINEAR:
        return yv + 0.0 * xv, xv + 0.0 * yv
    d2 = ((xv - yv) ** 2).sum(0)
    E = (2.0 * kg.kappa_prime(kind, d2, param))[None] * (xv - yv)
    return E, -E


def extended_factor(before):
    def factor(kind, Xr, Xc, param):
        if is_dot(kind):
            r = derivs(kind, Xr, Xc, param)
            return r["k"], r["dk"], r["dp"]
        return before(kind, Xr, Xc, param)
    return factor


def _has_dot(spec):
    return any(is_dot(t.kind) for t in spec._terms[:spec.n_terms])


def extended_input_grads(before):
    def np_input_grads(spec, G, pairs=None):
        """kprod_grad_np.np_input_grads for specs with the three kinds (point_derivs per factor); others: untouched"""
        if not _has_dot(spec):
            return before(spec, G, pairs)
        roff, coff = kg._offsets(spec)
        row = [np.zeros(np.asarray(a).shape) for a in spec.inputs]
        col = [np.zeros(np.asarray(a).shape) for a in spec.inputs]
        rs, cs = [None] * spec.n_terms, [None] * spec.n_terms
        for I, J, ts in kn.chains(spec):
            if pairs is not None and (I, J) not in pairs:
                continue
            Gb = G[roff[I]:roff[I + 1], coff[J]:coff[J + 1]]
            T = [spec._terms[t] for t in ts]
            X = [(np.asarray(spec.inputs[t.row_input], dtype=float), np.asarray(spec.inputs[t.col_input], dtype=float)) for t in T]
            ks = [kn.factor(t.kind, xr, xc, t.param)[0] for t, (xr, xc) in zip(T, X)]
            coef, rsv, csv = kn._weights(spec, ts[0])
            full = 1.0
            for k in ks:
                full = full * k
            if spec.term_row_scale[ts[0]] is not None:
                rs[ts[0]] = np.sum(Gb * coef * csv * full, axis=1)
            if spec.term_col_scale[ts[0]] is not None:
                cs[ts[0]] = np.sum(Gb * coef * rsv * full, axis=0)
            W = coef * Gb * rsv * csv
            for a, t in enumerate(T):
                others = 1.0
                for b, k in enumerate(ks):
                    if b != a:
                        others = others * k
                A = W * others
                dX, dY = point_derivs(t.kind, X[a][0], X[a][1], t.param)
                row[t.row_input] += (A[None] * dX).sum(2)
                col[t.col_input] += (A[None] * dY).sum(1)
        return dict(row=row, col=col, rs=rs, cs=cs)
    return np_input_grads


def extended_diag_grads(before):
    def np_diag_grads(spec, w):
        """kprod_grad_np.np_diag_grads for specs with the three kinds.  They follow LINEAR's convention: the row input
        receives d k / d x, the column input d k / d y, both added when they are one array"""
        if not _has_dot(spec):
            return before(spec, w)
        roff, _ = kg._offsets(spec)
        n = spec.n_terms
        gc, gs, gp = np.zeros(n), np.zeros(n), np.zeros(n)
        gx = [np.zeros(np.asarray(a).shape) for a in spec.inputs]
        rs, cs = [None] * n, [None] * n
        for I, J, ts in kn.chains(spec):
            if I != J:
                continue
            wb = w[roff[I]:roff[I + 1]]
            T = [spec._terms[t] for t in ts]
            X = [(np.asarray(spec.inputs[t.row_input], dtype=float), np.asarray(spec.inputs[t.col_input], dtype=float)) for t in T]
            m = len(wb)
            fs, pd = [], []
            for t, (xr, xc) in zip(T, X):
                # pair i with itself: one 1 x 1 evaluation per point
                vals = [kn.factor(t.kind, xr[:, i:i + 1], xc[:, i:i + 1], t.param) for i in range(m)]
                fs.append(tuple(np.array([np.asarray(v[q]).reshape(-1)[0] for v in vals]) for q in range(3)))
                ders = [point_derivs(t.kind, xr[:, i:i + 1], xc[:, i:i + 1], t.param) for i in range(m)]
                pd.append((np.hstack([d[0][:, :, 0] for d in ders]), np.hstack([d[1][:, :, 0] for d in ders])))
            head = ts[0]
            rv, cv = spec.term_row_scale[head], spec.term_col_scale[head]
            rsv = 1.0 if rv is None else np.asarray(rv)
            csv = 1.0 if cv is None else np.asarray(cv)
            coef = spec._terms[head].coef
            full = 1.0
            for f in fs:
                full = full * f[0]
            gc[head] = np.sum(wb * rsv * csv * full)
            if rv is not None:
                rs[head] = wb * coef * csv * full
            if cv is not None:
                cs[head] = wb * coef * rsv * full
            for a, t in enumerate(T):
                others = 1.0
                for b, f in enumerate(fs):
                    if b != a:
                        others = others * f[0]
                A = wb * rsv * csv * coef * others
                gs[ts[a]] = np.sum(A * fs[a][1])
                gp[ts[a]] = np.sum(A * fs[a][2])
                code = int(t.kind) & L.KIND_MASK
                if code in DOT_KINDS or code == L.LINEAR or t.row_input != t.col_input:
                    gx[t.row_input] += A[None, :] * pd[a][0]
                    gx[t.col_input] += A[None, :] * pd[a][1]
        return dict(gc=gc, gs=gs, gp=gp, gx=gx, rs=rs, cs=cs)
    return np_diag_grads


def extended_abs_bound(before):
    def factor_abs_bound(kind, Xr, Xc, param):
        """kinds_np.factor_abs_bound with the three kinds: (|k|, e), e the value bound of tests/dotkinds_truth.py per entry"""
        if not is_dot(kind):
            return before(kind, Xr, Xc, param)
        import dotkinds_truth as dt
        code = int(kind) & L.KIND_MASK
        Xr, Xc = np.asarray(Xr, dtype=np.float64), np.asarray(Xc, dtype=np.float64)
        D = Xr.shape[0]
        s, a, b, d2, lag = scalars(Xr, Xc)
        k = np.abs(derivs(kind, Xr, Xc, param)["k"])
        ds = (D + 1) * dt.EPS * (np.abs(Xr).T @ np.abs(Xc))
        if code == L.EXPONENTIATED:
            return k, k * (ds + 7.0 * dt.EPS)
        if code == L.FBM:
            return k, (50.0 + param * (1.5 * D + 3.5)) * dt.EPS * (_pow0(a, param) + _pow0(b, param)) + dt.EPS * k
        dl = np.zeros_like(s)
        for i in range(D):
            for j in range(i + 1, D):
                p, q = Xr[i][:, None] * Xc[j][None, :], Xr[j][:, None] * Xc[i][None, :]
                dl = dl + 2.0 * np.abs(p - q) * (np.abs(p) + np.abs(q) + np.abs(p - q))
        dl = dt.EPS * (dl + (D * (D - 1) / 2 + 1) * lag)
        R2 = ((a + b) + 1.0) + lag
        R = np.sqrt(R2)
        dR = ((D + 1) * dt.EPS * (a + b) + 3.0 * dt.EPS * R2 + dl) / (2.0 * R) + dt.EPS * R
        return k, (R * ds + np.abs(s) * dR) / ((1.0 + a) * (1.0 + b)) + 13.0 * dt.EPS * k
    return factor_abs_bound


def install(monkeypatch):
    """teach the two evaluators the three kinds for the duration of a test"""
    monkeypatch.setattr(kinds_np, "factor_abs_bound", extended_abs_bound(kinds_np.factor_abs_bound))
    monkeypatch.setattr(kn, "factor", extended_factor(kn.factor))
    monkeypatch.setattr(kg, "np_input_grads", extended_input_grads(kg.np_input_grads))
    monkeypatch.setattr(kg, "np_diag_grads", extended_diag_grads(kg.np_diag_grads))
