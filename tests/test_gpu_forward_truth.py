"""Posterior moments, samples and updates against an extended-precision truth (tests/forward_truth.py), through the public
host calls: P.posterior (alpha, mean_and_var, cov), sgp_posterior_predict_explicit through the C boundary, P.rand with the
caller's Z, P.posterior(P.VFE(..)) with P.elbo, and P.update_posterior of both kinds of posterior.

Errors are counted in eps = 2^-53 times a scale taken from the truth; the bound of a case and family is
MARGIN * max(the same reference run in float64 on this case, the family's floor) -- from the reference, never from the
device (docs/04_oracle_and_parity.md, "Posterior moments, samples and updates against the same kind of truth").  Models,
points, noises and the four kernels in rotation are those of tests/test_gpu_grad_truth.py.

Shapes, the smallest that reach each branch of the row solve (capi.hip: row_trsm / row_trsm_block / panel_solve_kernel) and
of the back substitution: 70 training points (one panel step, one diagonal back-solve), (129, 1, 128, 70) (three tiles:
halving of an odd tile count), one block of 513 (a second 512-column block behind a deep product with K = 512) and
(600, 500) (a third block, K = 1024); test layouts (1,), (128,), (129, 1, 70), (257,); D in {1, 3, 17}; scalar, diagonal
and dense noise.  Sparse: Z layouts (33, 1, 70) and (129,), Sigma_z = 1e-2 I and once 1e-6 I, each created plainly and
row-chunked (SGP_VFE_CHUNK=128).  Extensions (N, n_new) in (70, 40), (128, 1), (129, 127), (200, 400) and a chain of three
with and without a reservation; VFE updates of 200 points by 1, 128 and 300, one row-chunked, and a chain of three.
The bodies re-run on the NumPy double of the C-ABI in tests/test_forward_truth_on_numpy.py."""
import numpy as np
import pytest

import forward_truth as FT
import grad_truth as T
import stheno_jl_amd as P
import test_gpu_grad_truth as GT

pytestmark = pytest.mark.gpu

LAYOUT, X_LAYOUT = GT.LAYOUT, GT.X_LAYOUT            # (129, 1, 128, 70) and (129, 70, 131)
Z_LAYOUTS = ((33, 1, 70), (129,))
_MODELS = (lambda q: GT._two_atoms(q), lambda q: GT._three_atoms(q), lambda q: GT._kernel_sum(3, q), lambda q: GT._two_views(q))
_NOISE_TAG = GT._NOISE_TAG


class Case:
    def __init__(self, id, kind, D, model, layout, noise="scalar", test_layout=(129, 1, 70), **kw):
        self.id, self.kind, self.D, self.model, self.layout = id, kind, D, model, layout
        self.noise, self.test_layout = noise, test_layout
        self.explicit, self.z_layout, self.sigma_z, self.S = False, None, 1e-2, 1
        self.steps, self.reserve, self.noise_new = (), None, None
        self.__dict__.update(kw)

    def __repr__(self):
        return self.id


def _m(q):
    return lambda: _MODELS[q % 4](q)


POST_CASES = [
    Case("post-N70-D1", "post", 1, _m(0), (70,), "scalar", (1,)),
    Case("post-N328-D3", "post", 3, _m(1), LAYOUT, "diag", (129, 1, 70)),
    Case("post-N513-D17", "post", 17, _m(2), (513,), "scalar", (128,)),
    Case("post-N1100-D3", "post", 3, _m(3), (600, 500), "diag", (257,)),
    Case("post-N328-D1-dense", "post", 1, _m(4), LAYOUT, "dense", (257,)),
    Case("post-N513-D1", "post", 1, _m(5), (513,), "diag", (129, 1, 70)),
    Case("post-N328-D3-mean", "post", 3, _m(8), LAYOUT, "scalar", (128,)),                 # two atoms: means 0.2 and -0.1
    Case("post-N328-D17-explicit", "post", 17, _m(7), LAYOUT, "scalar", (129, 1, 70), explicit=True),
]
SPARSE_CASES = [
    Case("spost-Z104-D2", "spost", 2, _m(0), X_LAYOUT, "scalar", (129, 1, 70), z_layout=Z_LAYOUTS[0]),
    Case("spost-Z129-D8", "spost", 8, _m(1), X_LAYOUT, "diag", (257,), z_layout=Z_LAYOUTS[1]),
    Case("spost-Z104-D3-sz1e-6", "spost", 3, _m(3), X_LAYOUT, "diag", (128,), z_layout=Z_LAYOUTS[0], sigma_z=1e-6),
    Case("spost-Z129-D3", "spost", 3, _m(2), X_LAYOUT, "scalar", (1,), z_layout=Z_LAYOUTS[1]),
]
RAND_CASES = [
    Case("rand-N328-S1", "rand", 3, _m(0), LAYOUT, "scalar", S=1),
    Case("rand-N328-S3", "rand", 2, _m(1), LAYOUT, "diag", S=3),
    Case("rand-N513-S3", "rand", 3, _m(2), (513,), "scalar", S=3),
    Case("rand-N513-S1", "rand", 1, _m(3), (513,), "diag", S=1),
]
EXT_CASES = [
    Case("ext-70+40", "ext", 1, _m(1), (70,), "scalar", (1,), steps=(40,), noise_new="other"),
    Case("ext-128+1", "ext", 3, _m(2), (128,), "scalar", (128,), steps=(1,)),
    Case("ext-129+127", "ext", 3, _m(5), (129,), "diag", (129, 1, 70), steps=(127,)),
    Case("ext-200+400", "ext", 17, _m(6), (200,), "scalar", (257,), steps=(400,), noise_new="other"),
    Case("ext-chain-reserve", "ext", 3, _m(9), (70,), "scalar", (129, 1, 70), steps=(40, 19, 130), reserve=259),
    Case("ext-chain-realloc", "ext", 3, _m(9), (70,), "scalar", (129, 1, 70), steps=(40, 19, 130)),
]
VUPD_CASES = [
    Case("vupd-Z104-200+1", "vupd", 2, _m(1), (200,), "diag", (129, 1, 70), z_layout=Z_LAYOUTS[0], steps=(1,)),
    Case("vupd-Z129-200+128", "vupd", 3, _m(2), (200,), "scalar", (128,), z_layout=Z_LAYOUTS[1], steps=(128,)),
    Case("vupd-Z104-200+300", "vupd", 8, _m(5), (200,), "diag", (257,), z_layout=Z_LAYOUTS[0], steps=(300,)),
    Case("vupd-Z129-200+300-chunked", "vupd", 3, _m(0), (200,), "diag", (1,), z_layout=Z_LAYOUTS[1], steps=(300,), chunk=128),
    Case("vupd-Z104-chain", "vupd", 3, _m(6), (200,), "scalar", (129, 1, 70), z_layout=Z_LAYOUTS[0], steps=(1, 128, 300)),
]
ALL_CASES = POST_CASES + SPARSE_CASES + RAND_CASES + EXT_CASES + VUPD_CASES   # a case's seed is its position: additions at the end

_TRUTH = {}          # case id -> (truth in long double, two float64 runs): computed once, shared, never modified


def _names(names, k):
    return tuple(names[i % len(names)] for i in range(k))


def _rng(case):
    return np.random.default_rng(8100 + ALL_CASES.index(case))


def _runs(case, fn):
    """the truth and the two float64 runs of a case, cached by its id"""
    if case.id not in _TRUTH:
        _TRUTH[case.id] = tuple(fn(dt, ch) for dt, ch in GT._RUNS())
    return _TRUTH[case.id]


def yardstick(unit_fn, R, R64):
    return GT.yardstick(unit_fn(FT.reference_outputs(r), R) for r in R64)


def hold(case, dev, f64):
    """every family's device figure inside MARGIN * max(float64 figure, floor); figures printed first"""
    for fam in sorted(dev):
        print(f"{case.id:26s} {fam:13s} device {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {FT.FLOORS[fam]:8.1f}")
    bad = {fam: (dev[fam], f64[fam]) for fam in dev if not dev[fam] <= FT.MARGIN * max(f64[fam], FT.FLOORS[fam])}
    assert not bad, (case.id, bad)


def _test_points(case, rng, F, names):
    ts = [GT._points(rng, case.D, k) for k in case.test_layout]
    return GT._blocks(F, _names(names, len(ts)), ts)


def _predict(post, xt):
    m, v = post.mean_and_var(xt)
    return dict(mean=m, var=v, cov=post.cov(xt))


# ---- dense posterior -----------------------------------------------------------------------------------------------------
def run_post(case):
    rng = _rng(case)
    F, names = case.model()
    x = GT._blocks(F, _names(names, len(case.layout)), [GT._points(rng, case.D, n) for n in case.layout])
    n = sum(case.layout)
    noise = GT._noise(rng, case.noise, n)
    y = rng.standard_normal(n)
    xt = _test_points(case, rng, F, names)
    post = P.posterior(F(x, noise), y)
    St = T.read_spec(P.build_spec(F, x)[0])
    Sc, Sp = T.read_spec(P.build_spec(F, xt, F, x)[0]), T.read_spec(P.build_spec(F, xt)[0])
    mx, ms = P.mean_vector(F, x), P.mean_vector(F, xt)
    if case.explicit:
        # the cross matrix, prior variance and prior covariance as matrices, from the truth's float64 K
        ns = len(ms)
        Ks = np.asfortranarray(T.dense(Sc, np.float64))
        Kss = T.dense(Sp, np.float64)
        Kss = np.asfortranarray(np.tril(Kss) + np.tril(Kss, -1).T)
        pv = np.ascontiguousarray(np.diag(Kss))
        msb = np.ascontiguousarray(ms, dtype=np.float64)
        mo, vo, co = np.zeros(ns), np.zeros(ns), np.zeros((ns, ns), order="F")
        L = P.lib
        rc = L.default_context().lib.sgp_posterior_predict_explicit(post._ensure(), L.dptr(Ks), ns, ns, L.dptr(pv), L.dptr(Kss), ns,
                                                                    L.dptr(msb), L.dptr(mo), L.dptr(vo), L.dptr(co), ns)
        L.check(rc, "sgp_posterior_predict_explicit")
        out = dict(alpha=post.alpha, mean=mo, var=vo, cov=co)
        extra = dict(Ks=Ks, prior_var=pv, Kss=Kss)
    else:
        out = dict(alpha=post.alpha, **_predict(post, xt))
        extra = {}
    runs = _runs(case, lambda dt, ch: FT.posterior(St, _NOISE_TAG[case.noise], noise, mx, y, Sc, Sp, ms, dt, cholesky=ch, **extra))
    return out, runs, dict(mx=mx, ms=ms)


@pytest.mark.parametrize("case", POST_CASES, ids=repr)
def test_dense_posterior_against_truth(case):
    out, (R, *R64), s = run_post(case)
    assert not any(np.any(np.isnan(v)) for v in out.values())
    if "mean" in case.id:
        assert np.min(np.abs(s["mx"])) > 0.05 and np.min(np.abs(s["ms"])) > 0.05          # a prior mean on both sides
    fn = lambda o, r: FT.posterior_units("post", {k: o[k] for k in ("alpha", "mean", "var", "cov")}, r)   # noqa: E731
    hold(case, fn(out, R), yardstick(fn, R, R64))


# ---- sparse posterior ----------------------------------------------------------------------------------------------------
def _sparse_truth(case, F, z, x_all, noise_kind, noise_all, y_all, xt):
    Szz = T.read_spec(P.build_spec(F, z)[0])
    Sxz = T.read_spec(P.build_spec(F, x_all, F, z)[0])
    Sxx = T.read_spec(P.build_spec(F, x_all)[0])
    Sc, Sp = T.read_spec(P.build_spec(F, xt, F, z)[0]), T.read_spec(P.build_spec(F, xt)[0])
    mx, ms = P.mean_vector(F, x_all), P.mean_vector(F, xt)
    return _runs(case, lambda dt, ch: FT.sparse_posterior(Szz, T.NOISE_SCALAR, case.sigma_z, Sxz, noise_kind, noise_all, mx, y_all,
                                                          Sxx, Sc, Sp, ms, dt, cholesky=ch))


def run_sparse(case, chunk, monkeypatch):
    rng = _rng(case)
    F, names = case.model()
    x = GT._blocks(F, _names(names, len(case.layout)), [GT._points(rng, case.D, n) for n in case.layout])
    z = GT._blocks(F, _names(names, len(case.z_layout)), [GT._points(rng, case.D, k) for k in case.z_layout])
    n = sum(case.layout)
    noise = GT._noise(rng, case.noise, n)
    y = rng.standard_normal(n)
    xt = _test_points(case, rng, F, names)
    if chunk:
        monkeypatch.setenv("SGP_VFE_CHUNK", str(chunk))
    vfe = P.VFE(F(z, case.sigma_z))
    post = P.posterior(vfe, F(x, noise), y)
    out = dict(elbo=P.elbo(vfe, F(x, noise), y), **_predict(post, xt))
    return out, _sparse_truth(case, F, z, x, _NOISE_TAG[case.noise], noise, y, xt)


@pytest.mark.parametrize("chunk", [None, 128], ids=["plain", "chunk128"])
@pytest.mark.parametrize("case", SPARSE_CASES, ids=repr)
def test_sparse_posterior_against_truth(case, chunk, monkeypatch):
    out, (R, *R64) = run_sparse(case, chunk, monkeypatch)
    assert not any(np.any(np.isnan(v)) for v in out.values())
    fn = lambda o, r: FT.sparse_units("spost", o, r)   # noqa: E731
    hold(case, fn(out, R), yardstick(fn, R, R64))


# ---- rand ------------------------------------------------------------------------------------------------------------------
def run_rand(case):
    rng = _rng(case)
    F, names = case.model()
    x = GT._blocks(F, _names(names, len(case.layout)), [GT._points(rng, case.D, n) for n in case.layout])
    n = sum(case.layout)
    noise = GT._noise(rng, case.noise, n)
    Z = np.asfortranarray(rng.standard_normal((n, case.S)))
    fx = F(x, noise)
    out = np.asarray(P.rand(None, fx, case.S, Z=Z)).reshape(n, case.S)
    S = T.read_spec(P.build_spec(F, x)[0])
    mx = P.mean_vector(F, x)
    return out, _runs(case, lambda dt, ch: FT.rand(S, _NOISE_TAG[case.noise], noise, mx, Z, dt, cholesky=ch))


@pytest.mark.parametrize("case", RAND_CASES, ids=repr)
def test_rand_with_the_callers_z_against_truth(case):
    out, (R, *R64) = run_rand(case)
    assert not np.any(np.isnan(out))
    hold(case, FT.rand_units(out, R), GT.yardstick(FT.rand_units(r["rand"], R) for r in R64))


# ---- extension of a kept factor --------------------------------------------------------------------------------------------
def _batch_noise(case, rng, n, first):
    if case.noise_new == "other" and not first:
        return float(0.05 + 0.25 * rng.random())          # another scalar: the stacked noise becomes a diagonal
    return GT._noise(rng, case.noise, n) if (first or case.noise == "diag") else None


def _stack_noise(noises, sizes):
    if all(np.ndim(s) == 0 and float(s) == float(noises[0]) for s in noises):
        return T.NOISE_SCALAR, float(noises[0])
    return T.NOISE_DIAG, np.concatenate([np.broadcast_to(np.asarray(s, dtype=np.float64), (k,)) for s, k in zip(noises, sizes)])


def _batches(case, rng, F, names):
    """the data a case starts from and the batches it adds: (input, noise, y) each; a scalar noise repeats the first one's
    unless the case asks for another"""
    sizes = (sum(case.layout),) + tuple(case.steps)
    out = []
    for i, k in enumerate(sizes):
        xin = P.GPPPInput(names[i % len(names)], P.ColVecs(GT._points(rng, case.D, k)))
        s = _batch_noise(case, rng, k, i == 0)
        out.append((xin, out[0][1] if s is None else s, rng.standard_normal(k)))
    return out, sizes


def run_ext(case):
    rng = _rng(case)
    F, names = case.model()
    batches, sizes = _batches(case, rng, F, names)
    xt = _test_points(case, rng, F, names)
    post = P.posterior(F(batches[0][0], batches[0][1]), batches[0][2])
    for xin, s, yb in batches[1:]:
        post = P.update_posterior(post, F(xin, s), yb, reserve=case.reserve)
    assert len(post.y) == sum(sizes)
    out = dict(alpha=post.alpha, logpdf_y=post.logpdf_y, **_predict(post, xt))
    x_all = P.BlockData([b[0] for b in batches])
    kind, noise_all = _stack_noise([b[1] for b in batches], sizes)
    y_all = np.concatenate([b[2] for b in batches])
    St = T.read_spec(P.build_spec(F, x_all)[0])
    Sc, Sp = T.read_spec(P.build_spec(F, xt, F, x_all)[0]), T.read_spec(P.build_spec(F, xt)[0])
    mx, ms = P.mean_vector(F, x_all), P.mean_vector(F, xt)
    return out, _runs(case, lambda dt, ch: FT.posterior(St, kind, noise_all, mx, y_all, Sc, Sp, ms, dt, cholesky=ch)), kind


@pytest.mark.parametrize("case", EXT_CASES, ids=repr)
def test_extended_posterior_against_truth_of_the_stacked_data(case):
    out, (R, *R64), kind = run_ext(case)
    assert not any(np.any(np.isnan(v)) for v in out.values())
    if case.noise_new == "other":
        assert kind == T.NOISE_DIAG                        # different noise on old and new data
    fn = lambda o, r: FT.posterior_units("ext", o, r)   # noqa: E731
    hold(case, fn(out, R), yardstick(fn, R, R64))


# ---- VFE update ------------------------------------------------------------------------------------------------------------
def run_vupd(case, monkeypatch):
    rng = _rng(case)
    F, names = case.model()
    batches, sizes = _batches(case, rng, F, names)
    z = GT._blocks(F, _names(names, len(case.z_layout)), [GT._points(rng, case.D, k) for k in case.z_layout])
    xt = _test_points(case, rng, F, names)
    if getattr(case, "chunk", None):
        monkeypatch.setenv("SGP_VFE_CHUNK", str(case.chunk))
    post = P.posterior(P.VFE(F(z, case.sigma_z)), F(batches[0][0], batches[0][1]), batches[0][2])
    for xin, s, yb in batches[1:]:
        post = P.update_posterior(post, F(xin, s), yb)
    out = dict(elbo=post.elbo_y, **_predict(post, xt))        # elbo_y: elbo_out less half the create call's trace term
    x_all = P.BlockData([b[0] for b in batches])
    kind, noise_all = _stack_noise([b[1] for b in batches], sizes)
    y_all = np.concatenate([b[2] for b in batches])
    return out, _sparse_truth(case, F, z, x_all, kind, noise_all, y_all, xt)


@pytest.mark.parametrize("case", VUPD_CASES, ids=repr)
def test_updated_vfe_posterior_against_truth_of_the_stacked_data(case, monkeypatch):
    out, (R, *R64) = run_vupd(case, monkeypatch)
    assert not any(np.any(np.isnan(v)) for v in out.values())
    fn = lambda o, r: FT.sparse_units("vupd", o, r)   # noqa: E731
    hold(case, fn(out, R), yardstick(fn, R, R64))
