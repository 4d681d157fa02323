"""update_posterior for a sparse (VFE) posterior on the device (include/sthenomi_vfe_update.h: sgp_sparse_posterior_update /
sgp_sparse_posterior_count), run with -m gpu on an MI355X.

A batch of new observations joins the sums a kept sparse posterior holds; the inducing points stay.  The reference is
oracle.abstractgps (elbo / posterior_vfe) on the STACKED data, and the bounds are those the one-shot create is held to in
tests/test_gpu_parity.py::test_elbo_and_sparse_posterior_row_chunked_path: ELBO 1e-9 relative, mean at 50 test points 1e-7
relative, variance (and covariance) 1e-8 absolute.  The recursion itself loses nothing against them (NumPy, the same batches:
2e-15 / 4e-13 / 2e-14), so what the bounds leave is the device's own rounding.

The model, where none is named: Matern-5/2, mean 0.2, D = 2, M = 150 inducing points (two tile columns, identity padding),
sigma_z^2 = 1e-6, observation noise 0.1 + rng.random(n).

elbo_out and the create call: sgp_sparse_posterior_create takes no var_x, so of the ELBO's terms the kept sum of var / s2
cannot cover the points the posterior was created on; the header defines elbo_out as the ELBO of all the points plus
1/2 sum var_n / s2_n over those points, a constant the caller subtracts.  `trace0` below is that constant, from the prior
variances sgp_elbo is given; what is held to the oracle's ELBO of the stacked data, at 1e-9, is elbo_out - trace0 / 2."""
import ctypes as C
import os

import numpy as np
import pytest

import models
import oracle.abstractgps as oagp
import oracle.kernelfunctions as okf
import oracle.stheno as ost
import stheno_jl_amd as P

pytestmark = pytest.mark.gpu

L = P.lib
FG = P.finite_gp
ELBO_REL, MEAN_REL, VAR_ABS = 1e-9, 1e-7, 1e-8
SZ = 1e-6
BATCHES = (700, 300, 37, 1)


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _fo():
    return ost.atomic(oagp.GP(0.2, okf.Matern52Kernel()), ost.GPC())


def _fp():
    return P.atomic(P.GP(0.2, P.Matern52Kernel()), P.GPC())


def _full(noise, n):
    return np.full(n, float(noise)) if np.ndim(noise) == 0 else np.asarray(noise, dtype=np.float64)


class _Case:
    """the default model's data in four batches -- diagonal noise, diagonal, a scalar different from anything before,
    diagonal -- and the oracle's answers on every prefix of them, computed once"""

    def __init__(self, M=150, seed=41):
        rng = np.random.default_rng(seed)
        N, D = sum(BATCHES), 2
        self.X = np.asfortranarray(rng.standard_normal((D, N)))
        self.Z = np.asfortranarray(rng.standard_normal((D, M)))
        self.Xs = np.asfortranarray(rng.standard_normal((D, 50)))
        self.y = rng.standard_normal(N)
        self.noises = [0.1 + rng.random(700), 0.1 + rng.random(300), 0.37, 0.1 + rng.random(1)]
        self.fo, self.fp = _fo(), _fp()
        self.offs = np.concatenate([[0], np.cumsum(BATCHES)])
        self._ref = {}

    def batch(self, k):
        a, b = self.offs[k], self.offs[k + 1]
        return np.asfortranarray(self.X[:, a:b]), self.noises[k], self.y[a:b]

    def rows(self, a, b):
        nz = np.concatenate([_full(s, n) for s, n in zip(self.noises, BATCHES)])
        return np.asfortranarray(self.X[:, a:b]), nz[a:b], self.y[a:b]

    def ref(self, a, b):
        """oracle (elbo, mean, var, cov) at Xs given the rows [a, b)"""
        if (a, b) not in self._ref:
            X, nz, y = self.rows(a, b)
            vfe = oagp.VFE(self.fo(okf.ColVecs(self.Z), SZ))
            fx = self.fo(okf.ColVecs(X), nz)
            po = oagp.posterior_vfe(vfe, fx, y)
            xs = okf.ColVecs(self.Xs)
            self._ref[(a, b)] = (oagp.elbo(vfe, fx, y), po.mean(xs), po.var(xs), po.cov(xs))
        return self._ref[(a, b)]

    def create(self, a, b):
        X, nz, y = self.rows(a, b)
        return P.posterior(P.VFE(self.fp(P.ColVecs(self.Z), SZ)), self.fp(P.ColVecs(X), nz), y)

    def trace0(self, a, b):
        X, nz, _ = self.rows(a, b)
        return trace0(self.fp, P.ColVecs(X), nz)


@pytest.fixture(scope="module")
def case():
    return _Case()


def raw_update(post, f, x2, noise2, y2, want_elbo=True, y_null=False, kind=None, z=None):
    """sgp_sparse_posterior_update on post's handle through the ABI signature -> (rc, elbo, last error)"""
    n2 = len(x2)
    xz, _, _ = P.build_spec(f, x2, f, post.z if z is None else z)
    if n2 == 0:      # (no rows: one-element vectors, so that every pointer is a real one and only the row count is wrong)
        k, nbuf, mean2, var2, y2 = L.NOISE_DIAG, np.array([0.1]), np.zeros(1), np.ones(1), np.zeros(1)
    else:
        k, nbuf = L._noise_args(noise2, n2)
        mean2 = np.ascontiguousarray(FG.mean_vector(f, x2), dtype=np.float64)
        var2 = np.ascontiguousarray(FG.prior_var(f, x2), dtype=np.float64)
        y2 = np.ascontiguousarray(y2, dtype=np.float64)
    out = np.full(1, np.nan)
    rc = L.vfe_update_lib().sgp_sparse_posterior_update(post._h, xz.ref(), L.dptr(var2), L.dptr(mean2), k if kind is None else kind,
                                                        L.dptr(nbuf), None if y_null else L.dptr(y2), L.dptr(out) if want_elbo else None)
    return rc, float(out[0]), L.last_error()


def trace0(f, x, noise):
    """sum_n var(f, x_n) / s2_n over the points a posterior was created on (see the module docstring)"""
    return float(np.sum(np.asarray(FG.prior_var(f, x), dtype=np.float64) / FG._noise_diag(noise, len(x))))


def count(post):
    n = C.c_int64(-1)
    assert L.vfe_update_lib().sgp_sparse_posterior_count(post._h, C.byref(n)) == 0
    return n.value


def predict(post, Xs):
    xs = Xs if not isinstance(Xs, np.ndarray) else P.ColVecs(Xs)
    m, v = P.mean_and_var(post(xs, 0.0))
    return m, v, P.cov(post(xs, 0.0))


def within_bounds(post, elbo, ref, Xs, what=""):
    eo, mo, vo, co = ref
    m, v, c = predict(post, Xs)
    figs = (abs(elbo - eo) / abs(eo) if elbo is not None else 0.0, rel(m, mo), np.abs(v - vo).max(), np.abs(c - co).max())
    print(f"\n{what}: elbo rel {figs[0]:.3e}  mean rel {figs[1]:.3e}  var abs {figs[2]:.3e}  cov abs {figs[3]:.3e}")
    assert figs[0] <= ELBO_REL and figs[1] < MEAN_REL and figs[2] < VAR_ABS and figs[3] < VAR_ABS, (what, figs)


def bit_equal(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


class _chunk:
    """SGP_VFE_CHUNK, set as tests/test_gpu_parity.py::test_elbo_and_sparse_posterior_row_chunked_path sets it"""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        os.environ["SGP_VFE_CHUNK"] = str(self.rows)

    def __exit__(self, *a):
        del os.environ["SGP_VFE_CHUNK"]


# ---- 1. successive updates ------------------------------------------------------------------------------------------------
def test_successive_updates(case):
    pp = case.create(0, 700)
    assert count(pp) == 700
    within_bounds(pp, None, case.ref(0, 700), case.Xs, "create 700")
    t0 = case.trace0(0, 700)
    for k in (1, 2, 3):
        X2, s2, y2 = case.batch(k)
        rc, e, err = raw_update(pp, case.fp, P.ColVecs(X2), s2, y2)
        assert rc == 0, err
        n = int(case.offs[k + 1])
        assert count(pp) == n
        within_bounds(pp, e - 0.5 * t0, case.ref(0, n), case.Xs, f"after batch {k} ({n} points)")


# ---- 2. chunked create, chunked update ---------------------------------------------------------------------------------
def test_chunked_create_chunked_update(case):
    with _chunk(256):
        pp = case.create(0, 700)                           # 768 padded rows > 256: vfe_pipeline_chunked
        X2, s2, y2 = case.batch(1)
        rc, e, err = raw_update(pp, case.fp, P.ColVecs(X2), s2, y2)     # 384 padded rows: two chunks
        assert rc == 0, err
        assert count(pp) == 1000
        within_bounds(pp, e - 0.5 * case.trace0(0, 700), case.ref(0, 1000), case.Xs, "chunked 700 + 300")


# ---- 3. aligned chunks give the same bits ------------------------------------------------------------------------------
def test_aligned_chunks_give_the_same_bits(case):
    """create on 512 + update with 200 and create on the stacked 712 both accumulate the chunks [256, 256, 200 (+ 56 padded)]
    in that order through the same launches: mean, var and cov must be bit-equal.  The ELBO's four scalar sums are grouped
    differently (per call, not per chunk), so it is held to 1e-9 relative."""
    with _chunk(256):
        pp = case.create(0, 512)
        X2, s2, y2 = case.rows(512, 712)
        rc, e, err = raw_update(pp, case.fp, P.ColVecs(X2), s2, y2)
        assert rc == 0, err
        one = case.create(0, 712)
        X, nz, y = case.rows(0, 712)
        e_one = P.elbo(P.VFE(case.fp(P.ColVecs(case.Z), SZ)), case.fp(P.ColVecs(X), nz), y)
        a, b = predict(pp, case.Xs), predict(one, case.Xs)
    print(f"\nelbo update {e!r} one-shot {e_one!r}; max |d mean| {np.abs(a[0] - b[0]).max():.3e} |d var| {np.abs(a[1] - b[1]).max():.3e}")
    assert bit_equal(a, b)
    assert abs(e - 0.5 * case.trace0(0, 512) - e_one) <= ELBO_REL * abs(e_one)


# ---- 4. GPPP blocks -------------------------------------------------------------------------------------------------------
def test_gppp_blocks():
    """the @gppp docstring model (f3 = f1 + f2): inducing points in the two independent processes f1 and f2 -- K(z, z) has
    structural zeros -- data observed at the sum, the update batch a BlockData of two blocks"""
    rng = np.random.default_rng(5)
    fo, go = models.gppp_docstring(models.oracle_api())
    fp, gp = models.gppp_docstring(models.product_api())
    Fo, Fp = ost.GPPP(fo, go), P.GPPP(fp, gp)

    def blocks(names, xs):
        return (ost.BlockData([ost.GPPPInput(k, x) for k, x in zip(names, xs)]),
                P.BlockData([P.GPPPInput(k, x) for k, x in zip(names, xs)]))
    zs = [np.linspace(-4, 4, 20), np.linspace(-3.9, 3.9, 17)]
    x1, x2a, x2b = rng.uniform(-4, 4, 170), rng.uniform(-4, 4, 90), rng.uniform(-4, 4, 45)
    zo, zp = blocks(("f1", "f2"), zs)
    _, xp1 = blocks(("f3",), [x1])
    _, xp2 = blocks(("f3", "f1"), [x2a, x2b])
    xo_all, _ = blocks(("f3", "f3", "f1"), [x1, x2a, x2b])
    so, sp = blocks(("f2", "f3"), [rng.uniform(-4, 4, 30), rng.uniform(-4, 4, 20)])
    y = rng.standard_normal(305)
    nz = 0.1 + rng.random(305)
    pp = P.posterior(P.VFE(Fp(zp, SZ)), Fp(xp1, nz[:170]), y[:170])
    rc, e, err = raw_update(pp, Fp, xp2, nz[170:], y[170:])
    assert rc == 0, err
    assert count(pp) == 305
    vfe = oagp.VFE(Fo(zo, SZ))
    po = oagp.posterior_vfe(vfe, Fo(xo_all, nz), y)
    ref = (oagp.elbo(vfe, Fo(xo_all, nz), y), po.mean(so), po.var(so), po.cov(so))
    within_bounds(pp, e - 0.5 * trace0(Fp, xp1, nz[:170]), ref, sp, "gppp blocks 170 + (90, 45)")


# ---- 5. edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [128, 1])
def test_edge_numbers_of_inducing_points_with_an_update_of_one_point(M):
    c = _Case(M=M, seed=100 + M)
    pp = c.create(0, 300)
    X2, nz2, y2 = c.rows(300, 301)
    rc, e, err = raw_update(pp, c.fp, P.ColVecs(X2), nz2, y2)
    assert rc == 0, err
    assert count(pp) == 301
    within_bounds(pp, e - 0.5 * c.trace0(0, 300), c.ref(0, 301), c.Xs, f"M = {M}: 300 + 1")


def test_an_update_larger_than_the_data_it_started_from(case):
    pp = case.create(0, 130)
    X2, nz2, y2 = case.rows(130, 830)
    rc, e, err = raw_update(pp, case.fp, P.ColVecs(X2), nz2, y2)
    assert rc == 0, err
    assert count(pp) == 830
    within_bounds(pp, e - 0.5 * case.trace0(0, 130), case.ref(0, 830), case.Xs, "130 + 700")


# ---- 6. downstream calls --------------------------------------------------------------------------------------------------
def test_logpdf_and_rand_on_the_handle_agree_with_a_stacked_create(case):
    """sgp_sparse_posterior_logpdf / _rand (S = 2, fixed Z) after an update against the same calls on a create of the stacked
    data: the bounds of this file with the scaling of tests/test_gpu_postfx.py::test_vfe_parity_with_the_oracle -- every
    logpdf column relative to itself at the ELBO's 1e-9 (both are log-densities of the whole vector), the draws by
    max |difference| / max |value| at the mean's 1e-7 (a draw is the mean plus a factor of the covariance times Z)."""
    pp = case.create(0, 700)
    X2, s2, y2 = case.batch(1)
    rc, _, err = raw_update(pp, case.fp, P.ColVecs(X2), s2, y2, want_elbo=False)
    assert rc == 0, err
    one = case.create(0, 1000)
    rng = np.random.default_rng(7)
    xs, noise = P.ColVecs(case.Xs), 0.1 + rng.random(50)
    Y, Z = rng.standard_normal((50, 2)), rng.standard_normal((50, 2))
    la, lb = P.logpdf(pp(xs, noise), Y), P.logpdf(one(xs, noise), Y)
    ra, rb = P.rand(None, pp(xs, noise), 2, Z=Z), P.rand(None, one(xs, noise), 2, Z=Z)
    print(f"\nlogpdf rel {np.max(np.abs(la - lb) / np.abs(lb)):.3e}  rand rel {rel(ra, rb):.3e}")
    assert np.all(np.abs(la - lb) <= ELBO_REL * np.abs(lb))
    assert rel(ra, rb) < MEAN_REL


# ---- 7. refusals leave the posterior alone --------------------------------------------------------------------------------
def test_refusals_leave_the_posterior_alone(case):
    pp = case.create(0, 700)
    before = predict(pp, case.Xs)
    X2, s2, y2 = case.batch(1)
    x2 = P.ColVecs(X2)
    other_z = P.ColVecs(np.asfortranarray(case.Z[:, :149]))
    dense = 0.2 * np.eye(300)
    x0 = P.ColVecs(np.asfortranarray(X2[:, :0]))
    refused = [raw_update(pp, case.fp, x2, s2, y2, z=other_z),                                  # a wrong column count
               raw_update(pp, case.fp, x2, dense, y2),                                          # dense noise kind
               raw_update(pp, case.fp, x2, s2, y2, kind=L.NOISE_DENSE),
               raw_update(pp, case.fp, x2, s2, y2, y_null=True),                                # NULL y_new
               raw_update(pp, case.fp, x0, np.zeros(0) + 0.1, np.zeros(0))]                     # n_new = 0
    for rc, _, err in refused:
        assert rc < 0 and err.startswith("sgp_sparse_posterior_update:"), (rc, err)
        assert bit_equal(predict(pp, case.Xs), before) and count(pp) == 700
    rc = L.vfe_update_lib().sgp_sparse_posterior_update(None, None, None, None, 0, None, None, None)
    assert rc < 0 and L.last_error().startswith("sgp_sparse_posterior_update:")
    # a handle whose context was destroyed
    ctx = L.Context(0)
    prev = L.set_default_context(ctx)
    try:
        gone = case.create(0, 700)
    finally:
        L.set_default_context(prev)
    ctx.close()
    rc, _, err = raw_update(gone, case.fp, x2, s2, y2)
    assert rc < 0 and err.startswith("sgp_sparse_posterior_update:") and "destroyed" in err
    del gone
    # a sharded posterior (a multi-GPU context: one device listed twice)
    mctx = L.Context(devices=[0, 0])
    prev = L.set_default_context(mctx)
    try:
        sh = case.create(0, 700)
        m_before = sh.mean(P.ColVecs(case.Xs))
        rc, _, err = raw_update(sh, case.fp, x2, s2, y2)
        assert rc < 0 and err.startswith("sgp_sparse_posterior_update:") and "multi-GPU" in err
        assert np.array_equal(sh.mean(P.ColVecs(case.Xs)), m_before)
        del sh
    finally:
        L.set_default_context(prev)
        mctx.close()
    # and a valid call after all of them
    rc, e, err = raw_update(pp, case.fp, x2, s2, y2)
    assert rc == 0, err
    within_bounds(pp, e - 0.5 * case.trace0(0, 700), case.ref(0, 1000), case.Xs, "after the refusals")


def test_a_nan_coordinate_is_reported_as_create_reports_it(case):
    """one NaN coordinate in x_new: the update reports what sgp_sparse_posterior_create on the same stacked data reports.
    Where that is rc > 0 (A A' + I not positive definite) the posterior must be bit for bit what it was; where create
    returns 0 with NaNs the update does the same, and the handle then answers NaN like the created one."""
    pp = case.create(0, 700)
    before = predict(pp, case.Xs)
    X2, s2, y2 = case.batch(1)
    X2 = X2.copy(order="F")
    X2[1, 17] = np.nan
    Xall = np.asfortranarray(np.concatenate([case.rows(0, 700)[0], X2], axis=1))
    _, nz, y = case.rows(0, 1000)
    vfe, fx = P.VFE(case.fp(P.ColVecs(case.Z), SZ)), case.fp(P.ColVecs(Xall), nz)
    zz, xz, mean_x, nk, nbuf, zk, zbuf = FG._vfe_args(vfe, fx)
    h = C.c_void_p()
    ctx = L.default_context()
    rc_create = ctx.lib.sgp_sparse_posterior_create(ctx.handle, zz.ref(), xz.ref(), L.dptr(mean_x), nk, L.dptr(nbuf), zk,
                                                    L.dptr(zbuf), L.dptr(np.ascontiguousarray(y)), C.byref(h))
    rc, _, err = raw_update(pp, case.fp, P.ColVecs(X2), s2, y2)
    print(f"\ncreate rc {rc_create}, update rc {rc} ({err if rc else 'ok'})")
    assert (rc > 0) == (rc_create > 0) and (rc == 0) == (rc_create == 0)
    if rc_create == 0:
        # create returns 0 for this input (the kernels answer a NaN distance with a number or with NaN, they do not fail):
        # so does the update, and both handles are finite or not at the same test points
        made = P.ApproxPosteriorGP(case.fp, pp.z, h)
        a, b = predict(pp, case.Xs), predict(made, case.Xs)
        assert count(pp) == 1000
        assert all(np.array_equal(np.isfinite(u), np.isfinite(v)) for u, v in zip(a, b))
    else:
        assert rc == rc_create
        assert bit_equal(predict(pp, case.Xs), before) and count(pp) == 700


# ---- 8. determinism ---------------------------------------------------------------------------------------------------------
def test_the_same_updates_twice_give_equal_bits(case):
    runs = []
    for _ in range(2):
        pp = case.create(0, 700)
        es = []
        for k in (1, 2):
            X2, s2, y2 = case.batch(k)
            rc, e, err = raw_update(pp, case.fp, P.ColVecs(X2), s2, y2)
            assert rc == 0, err
            es.append(e)
        runs.append((np.array(es),) + predict(pp, case.Xs))
    assert bit_equal(runs[0], runs[1])


# ---- 9. the host mirror -----------------------------------------------------------------------------------------------------
def test_host_mirror(case):
    pp = case.create(0, 700)
    old = predict(pp, case.Xs)
    X2, s2, y2 = case.batch(1)
    new = P.update_posterior(pp, case.fp(P.ColVecs(X2), s2), y2)
    assert isinstance(new, P.ApproxPosteriorGP) and pp._h is None
    assert count(new) == 1000
    within_bounds(new, new.elbo_y, case.ref(0, 1000), case.Xs, "update_posterior 700 + 300")
    # elbo_y is elbo_out less the create call's trace term: the same call on a second handle gives the same bits
    twin = case.create(0, 700)
    rc, e, err = raw_update(twin, case.fp, P.ColVecs(X2), s2, y2)
    assert rc == 0 and e - 0.5 * case.trace0(0, 700) == new.elbo_y, err
    # the old object still predicts as before (it rebuilds factors of its own)
    assert bit_equal(predict(pp, case.Xs), old) and pp._h is not None
    # new inducing points: the stacked one-shot posterior, and that very call
    z2 = P.ColVecs(np.asfortranarray(np.random.default_rng(9).standard_normal((2, 90))))
    X, nz, y = case.rows(0, 1000)
    moved = P.update_posterior(new, case.fp(z2, SZ))
    x_all = P.BlockData([P.ColVecs(case.batch(0)[0]), P.ColVecs(X2)])        # the kept batches, block by block
    want = P.posterior(P.VFE(case.fp(z2, SZ)), case.fp(x_all, nz), y)
    assert isinstance(moved, P.ApproxPosteriorGP) and len(moved.z) == 90
    assert bit_equal(predict(moved, case.Xs), predict(want, case.Xs))


def test_host_mirror_on_a_multi_gpu_context_takes_the_stacked_route(case):
    """a multi-GPU context (one device listed twice): the sharded posterior keeps no sums, so the mirror conditions on the
    stacked data; the new object carries elbo_y (sgp_elbo on the stacked data) and meets the bounds"""
    X2, s2, y2 = case.batch(1)
    mctx = L.Context(devices=[0, 0])
    prev = L.set_default_context(mctx)
    try:
        pp = case.create(0, 700)
        new = P.update_posterior(pp, case.fp(P.ColVecs(X2), s2), y2)
        assert isinstance(new, P.ApproxPosteriorGP) and pp._h is not None and len(new.batches) == 2
        within_bounds(new, new.elbo_y, case.ref(0, 1000), case.Xs, "multi-GPU context 700 + 300")
        del pp, new
    finally:
        L.set_default_context(prev)
        mctx.close()
