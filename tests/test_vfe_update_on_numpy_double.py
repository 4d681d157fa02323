"""`update_posterior` of a sparse (VFE) posterior -> sgp_sparse_posterior_update WITHOUT a GPU: the host mirror's marshalling
(the rows and columns of the xz_new spec, the choice between a scalar and a diagonal noise, var_x_new, the mean), the
hand-over of the handle, the rebuild of the old object, the ValueError for dense noise, the multi-GPU fallback and the
fz_new method, against the NumPy double of the C-ABI (tests/np_capi.py).  The double learns the two entry points here from
the words of include/sthenomi_vfe_update.h: a posterior keeps the sums over its data points (A A', A delta, sum log s2,
delta' delta, sum var / s2 -- zero for the create call's points, which has no var_x -- and |A|_F^2) and Lz; an update adds
the new rows' terms and finishes afresh (Le, alpha, the ELBO on the kept scalars), rc < 0 is a refusal that leaves the
posterior alone.  The device's own arithmetic is tests/test_gpu_vfe_update.py's business."""
import numpy as np
import pytest
import scipy.linalg as sla

import np_capi
import stheno_jl_amd as P

L = P.lib
LOG2PI = float(np.log(2.0 * np.pi))
WHO = "sgp_sparse_posterior_update"


def _create(self, ctx, zz, xz, mean_x, nk, noise_x, zk, z_noise, y, out):
    rc = np_capi.FakeLib._screate0(self, ctx, zz, xz, mean_x, nk, noise_x, zk, z_noise, y, out)
    if rc == 0:
        (Lz, A, Le, delta, sy), _ = self._vfe_parts(zz, xz, mean_x, nk, noise_x, zk, z_noise, y)
        self.sums[id(np_capi._struct(out))] = {"Lz": Lz, "G": A @ A.T, "Ad": A @ delta, "logs": np.log(sy).sum(),
                                               "dd": delta @ delta, "trace": 0.0, "AA": (A * A).sum(), "n": len(delta)}
    return rc


def _update(self, post, xz_new, var_x_new, mean_x_new, kind, noise_new, y_new, elbo_out):
    if not (xz_new and var_x_new and noise_new and y_new):      # (the double's handles are empty c_void_p objects)
        return self._fail(WHO + ": NULL argument")
    if id(post) not in self.sums:
        return self._fail(WHO + ": this posterior keeps no sums (it was created on a multi-GPU context)")
    if kind not in (L.NOISE_SCALAR, L.NOISE_DIAG):
        return self._fail(WHO + ": Sigma_y must be isotropic or diagonal (as in AbstractGPs.elbo)")
    S = self.sums[id(post)]
    sx = np_capi._Spec(xz_new)
    n, M = sx.N, S["Lz"].shape[0]
    self.update_calls.append({"rows": [int(v) for v in sx.row_len], "cols": [int(v) for v in sx.col_len], "kind": kind,
                              "var": np_capi._vec(var_x_new, n).copy(), "mean": None if not mean_x_new else np_capi._vec(mean_x_new, n).copy()})
    if sx.M != M:
        return self._fail(WHO + ": the columns of xz_new are not the inducing points the posterior was created with")
    if n < 1:
        return self._fail(WHO + ": no new data points")
    sy = np.full(n, float(noise_new[0])) if kind == L.NOISE_SCALAR else np_capi._vec(noise_new, n).copy()
    A = sla.solve_triangular(S["Lz"], sx.dense().T, lower=True, check_finite=False) / np.sqrt(sy)[None, :]
    m = np.zeros(n) if not mean_x_new else np_capi._vec(mean_x_new, n)
    delta = (np_capi._vec(y_new, n) - m) / np.sqrt(sy)
    new = {"Lz": S["Lz"], "G": S["G"] + A @ A.T, "Ad": S["Ad"] + A @ delta, "logs": S["logs"] + np.log(sy).sum(),
           "dd": S["dd"] + delta @ delta, "trace": S["trace"] + (np_capi._vec(var_x_new, n) / sy).sum(),
           "AA": S["AA"] + (A * A).sum(), "n": S["n"] + n}
    Le, info = np_capi._chol(new["G"] + np.eye(M))
    if info:
        return self._fail("matrix is not positive definite", info)       # the posterior is left exactly as it was
    b = sla.solve_triangular(Le, new["Ad"], lower=True, check_finite=False)
    alpha = sla.solve_triangular(S["Lz"], sla.solve_triangular(Le, b, lower=True, trans="T", check_finite=False), lower=True,
                                 trans="T", check_finite=False)
    self.sums[id(post)] = new
    self.sposts[id(post)] = (S["Lz"], Le, alpha)
    if elbo_out:
        tmp = new["logs"] + 2.0 * np.log(np.diag(Le)).sum() + new["dd"] - b @ b
        elbo_out[0] = -0.5 * (new["n"] * LOG2PI + tmp) - 0.5 * (new["trace"] - new["AA"])
    return 0


def _count(self, post, n_out):
    if id(post) not in self.sums:
        return self._fail("sgp_sparse_posterior_count: this posterior keeps no sums")
    n_out[0] = self.sums[id(post)]["n"]
    return 0


@pytest.fixture(autouse=True)
def _numpy_double(monkeypatch):
    ctx = np_capi.install(monkeypatch)
    monkeypatch.setattr(np_capi.FakeLib, "_screate0", np_capi.FakeLib.sgp_sparse_posterior_create, raising=False)
    monkeypatch.setattr(np_capi.FakeLib, "sgp_sparse_posterior_create", _create)
    monkeypatch.setattr(np_capi.FakeLib, "sgp_sparse_posterior_update", _update, raising=False)
    monkeypatch.setattr(np_capi.FakeLib, "sgp_sparse_posterior_count", _count, raising=False)
    ctx.lib.update_calls, ctx.lib.sums = [], {}
    ctx.vfe_update = ctx.lib          # (Context.vfe_update: libsthenomi_vfe_update.so; the double serves both libraries)
    return ctx


def _data(rng, n1=60, n2=(14, 11), D=2):
    F = P.gppp_sum_model()
    inp = lambda name, n: P.GPPPInput(name, P.ColVecs(np.asfortranarray(rng.standard_normal((D, n)))))
    z = P.BlockData([inp("f1", 9), inp("f2", 8)])
    x1 = inp("f3", n1)
    x2 = P.BlockData([inp("f3", n2[0]), inp("f1", n2[1])])
    xs = inp("f2", 11)
    return F, z, x1, x2, xs, rng.standard_normal(n1), rng.standard_normal(sum(n2))


def _same(a, b, xs, exact=False):
    cmp = np.array_equal if exact else (lambda u, v: np.allclose(u, v, rtol=0, atol=1e-9))
    assert cmp(a.mean(xs), b.mean(xs)) and cmp(a.var(xs), b.var(xs)) and cmp(a.cov(xs), b.cov(xs))


def test_marshalling_rows_columns_noise_var_and_mean(_numpy_double):
    rng = np.random.default_rng(1)
    F, z, x1, x2, xs, y1, y2 = _data(rng)
    calls = _numpy_double.lib.update_calls
    post = P.posterior(P.VFE(F(z, 1e-6)), F(x1, 0.1), y1)
    assert calls == [] and len(post.batches) == 1 and post.vfe.fz.x is z
    new = P.update_posterior(post, F(x2, 0.3), y2)                      # a scalar noise other than the old one: SCALAR
    c = calls[-1]
    assert c["rows"] == [14, 11] and c["cols"] == [9, 8] and c["kind"] == L.NOISE_SCALAR
    assert np.array_equal(c["var"], P.prior_var(F, x2)) and np.array_equal(c["mean"], P.prior_mean(F, x2))
    assert isinstance(new, P.ApproxPosteriorGP) and new.z is z and len(new.batches) == 2
    x_all = P.BlockData([x1] + list(x2.X))
    nz_all, y_all = np.r_[np.full(60, 0.1), np.full(25, 0.3)], np.concatenate([y1, y2])
    ref = P.posterior(P.VFE(F(z, 1e-6)), F(x_all, nz_all), y_all)
    _same(new, ref, xs)
    e = P.elbo(P.VFE(F(z, 1e-6)), F(x_all, nz_all), y_all)
    assert abs(new.elbo_y - e) <= 1e-10 * abs(e)                        # the create call's trace term is the mirror's to add
    n = np.zeros(1, dtype=np.int64)
    assert _numpy_double.lib.sgp_sparse_posterior_count(new._h, n) == 0 and n[0] == 85
    # a vector noise: DIAG with n_new values; a second update on the updated posterior
    x3 = P.GPPPInput("f2", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 7)))))
    v3, y3 = 0.05 + rng.random(7), rng.standard_normal(7)
    newer = P.update_posterior(new, F(x3, v3), y3)
    assert calls[-1]["rows"] == [7] and calls[-1]["kind"] == L.NOISE_DIAG and len(newer.batches) == 3
    x_all3 = P.BlockData(list(x_all.X) + [x3])
    e3 = P.elbo(P.VFE(F(z, 1e-6)), F(x_all3, np.r_[nz_all, v3]), np.concatenate([y_all, y3]))
    assert abs(newer.elbo_y - e3) <= 1e-10 * abs(e3)
    _same(newer, P.posterior(P.VFE(F(z, 1e-6)), F(x_all3, np.r_[nz_all, v3]), np.concatenate([y_all, y3])), xs)


def test_the_new_object_takes_the_handle_over_and_the_old_one_rebuilds(_numpy_double):
    rng = np.random.default_rng(2)
    F, z, x1, x2, xs, y1, y2 = _data(rng)
    post = P.posterior(P.VFE(F(z, 1e-6)), F(x1, 0.2), y1)
    h, m_old = post._h, post.mean(xs)
    new = P.update_posterior(post, F(x2, 0.2), y2)
    assert new._h is h and post._h is None
    assert not np.allclose(new.mean(xs), m_old)
    assert np.array_equal(post.mean(xs), m_old) and post._h is not None and post._h is not h
    # the rebuilt old object can be updated again and gives the same posterior
    again = P.update_posterior(post, F(x2, 0.2), y2)
    _same(again, new, xs, exact=True)
    assert again.elbo_y == new.elbo_y


def test_dense_noise_other_processes_and_lengths_are_errors(_numpy_double):
    rng = np.random.default_rng(3)
    F, z, x1, x2, xs, y1, y2 = _data(rng)
    post = P.posterior(P.VFE(F(z, 1e-6)), F(x1, 0.1), y1)
    h = post._h
    with pytest.raises(ValueError, match="isotropic or diagonal"):
        P.update_posterior(post, F(x2, 0.2 * np.eye(25)), y2)
    with pytest.raises(ValueError):
        P.update_posterior(post, P.gppp_sum_model()(x2, 0.1), y2)       # another programme's process
    with pytest.raises(ValueError):
        P.update_posterior(post, F(x2, 0.1), y2[:-1])
    with pytest.raises(ValueError):
        P.update_posterior(post, P.gppp_sum_model()(z, 1e-6))           # fz_new of another programme
    assert post._h is h and _numpy_double.lib.update_calls == []
    # a refusal of the entry point becomes an error and leaves the handle with the old object
    del _numpy_double.lib.sums[id(h)]
    with pytest.raises(P.SthenoMIError, match="multi-GPU"):
        P.update_posterior(post, F(x2, 0.1), y2)
    assert post._h is h


def test_multi_gpu_context_takes_the_stacked_route(_numpy_double):
    rng = np.random.default_rng(4)
    F, z, x1, x2, xs, y1, y2 = _data(rng)
    post = P.posterior(P.VFE(F(z, 1e-6)), F(x1, 0.1), y1)
    _numpy_double.is_multi = True
    via = P.update_posterior(post, F(x2, 0.1), y2)
    _numpy_double.is_multi = False
    assert _numpy_double.lib.update_calls == [] and post._h is not None and len(via.batches) == 2
    ref = P.posterior(P.VFE(F(z, 1e-6)), F(P.BlockData([x1] + list(x2.X)), 0.1), np.concatenate([y1, y2]))
    _same(via, ref, xs, exact=True)
    # the new object carries elbo_y on this route too (sgp_elbo on the stacked data), and a further update on a single-GPU
    # context subtracts the trace term of BOTH batches: both went through its handle's create call
    x_all = P.BlockData([x1] + list(x2.X))
    assert via.elbo_y == P.elbo(P.VFE(F(z, 1e-6)), F(x_all, 0.1), np.concatenate([y1, y2]))
    x3 = P.GPPPInput("f2", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 7)))))
    y3 = rng.standard_normal(7)
    more = P.update_posterior(via, F(x3, 0.1), y3)
    e3 = P.elbo(P.VFE(F(z, 1e-6)), F(P.BlockData(list(x_all.X) + [x3]), 0.1), np.concatenate([y1, y2, y3]))
    assert len(_numpy_double.lib.update_calls) == 1 and abs(more.elbo_y - e3) <= 1e-10 * abs(e3)


def test_new_inducing_points_are_the_stacked_one_shot_posterior(_numpy_double):
    rng = np.random.default_rng(5)
    F, z, x1, x2, xs, y1, y2 = _data(rng)
    new = P.update_posterior(P.posterior(P.VFE(F(z, 1e-6)), F(x1, 0.1), y1), F(x2, 0.3), y2)
    z2 = P.GPPPInput("f3", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 12)))))
    moved = P.update_posterior(new, F(z2, 1e-6))
    ref = P.posterior(P.VFE(F(z2, 1e-6)), F(P.BlockData([x1] + list(x2.X)), np.r_[np.full(60, 0.1), np.full(25, 0.3)]),
                      np.concatenate([y1, y2]))
    assert isinstance(moved, P.ApproxPosteriorGP) and moved.z is z2 and len(moved.batches) == 2 and new._h is not None
    _same(moved, ref, xs, exact=True)


def test_new_inducing_points_then_new_data_keeps_the_elbo_right(_numpy_double):
    """create 60, update 25, re-induce on 12 points, update 7: the re-induced handle's create call saw BOTH kept batches, so
    the trace term of both is subtracted from elbo_out; the rebuilt old objects do the same with their own batches"""
    rng = np.random.default_rng(6)
    F, z, x1, x2, xs, y1, y2 = _data(rng)
    new = P.update_posterior(P.posterior(P.VFE(F(z, 1e-6)), F(x1, 0.1), y1), F(x2, 0.3), y2)
    z2 = P.GPPPInput("f3", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 12)))))
    moved = P.update_posterior(new, F(z2, 1e-6))
    x3 = P.GPPPInput("f2", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 7)))))
    v3, y3 = 0.05 + rng.random(7), rng.standard_normal(7)
    x_all = P.BlockData([x1] + list(x2.X) + [x3])
    nz_all, y_all = np.r_[np.full(60, 0.1), np.full(25, 0.3), v3], np.concatenate([y1, y2, y3])
    last = P.update_posterior(moved, F(x3, v3), y3)
    e = P.elbo(P.VFE(F(z2, 1e-6)), F(x_all, nz_all), y_all)
    assert abs(last.elbo_y - e) <= 1e-10 * abs(e)
    _same(last, P.posterior(P.VFE(F(z2, 1e-6)), F(x_all, nz_all), y_all), xs)
    # `moved` gave its handle away: rebuilt from its two batches, updated again, it answers the same
    again = P.update_posterior(moved, F(x3, v3), y3)
    assert abs(again.elbo_y - e) <= 1e-10 * abs(e)
    # `new` (two batches, the second through an update) still has its handle and its own inducing points
    e_old = P.elbo(P.VFE(F(z, 1e-6)), F(x_all, nz_all), y_all)
    assert abs(P.update_posterior(new, F(x3, v3), y3).elbo_y - e_old) <= 1e-10 * abs(e_old)


def test_a_missing_y2_on_an_exact_posterior_is_a_type_error(_numpy_double):
    rng = np.random.default_rng(7)
    F, z, x1, x2, xs, y1, y2 = _data(rng)
    with pytest.raises(TypeError, match="y2"):
        P.update_posterior(P.posterior(F(x1, 0.1), y1), F(x2, 0.1))
