"""sgp_logpdf_grad_batch: logpdf AND its gradient for B independent models in one call -- the step of several hyper-parameter
chains at once (restarts, folds, candidates) around /root/reference/examples/getting_started/script.jl:154-213.  Equally sized
members are factored ([K + Sigma_y ; (y - m)' ; I]) by ONE launch of the dataflow kernel with the dense gradient-border
pattern, and their C^-1 = inv(L)' inv(L) by ONE launch.  The contract: every member's dict is BIT-EQUAL to its own
`logpdf_and_gradient` call and agrees with the CPU oracle; a member that is not positive definite does not lose the others."""
import json
import os

import numpy as np
import pytest

import bench_configs
import models
import oracle.abstractgps as oagp
import stheno_jl_amd as P
from test_gpu_parity import _oracle_term_grads, blockdata, both, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _members(B, N, D=8, seed=5):
    """Matern-5/2 members with their own lengthscale, variance and noise (what an optimiser's restarts look like)"""
    rng = np.random.default_rng(seed)
    fxs, ys = [], []
    for b in range(B):
        ell, v, s2 = 0.7 + rng.random(), 0.5 + rng.random(), 0.05 + 0.2 * rng.random()
        f = v * P.stretch(P.atomic(P.GP(P.Matern52Kernel()), P.GPC()), 1.0 / ell)
        fxs.append(f(P.ColVecs(np.asfortranarray(rng.standard_normal((D, N)))), s2))
        ys.append(rng.standard_normal(N))
    return fxs, ys


def _assert_bit_equal(got, ref):
    assert set(got) == set(ref)
    assert got["logpdf"] == ref["logpdf"], (got["logpdf"], ref["logpdf"])
    assert np.array_equal(got["y"], ref["y"]) and np.array_equal(got["mean"], ref["mean"])
    assert np.array_equal(np.asarray(got["noise"]), np.asarray(ref["noise"]))
    assert type(got["noise"]) is type(ref["noise"])
    assert len(got["terms"]) == len(ref["terms"])
    for a, b in zip(got["terms"], ref["terms"]):
        assert (a["I"], a["J"], a["kind"], a["t"], a["mirror_t"]) == (b["I"], b["J"], b["kind"], b["t"], b["mirror_t"])
        assert np.array_equal(a["d_coef"], b["d_coef"]) and np.array_equal(a["d_inscale"], b["d_inscale"])
    assert np.array_equal(got["_raw"][0], ref["_raw"][0]) and np.array_equal(got["_raw"][1], ref["_raw"][1])


@pytest.mark.parametrize("B,N", [(2, 300), (3, 1000), (8, 1536), (16, 640), (5, 4096), (19, 512)])
def test_batch_members_are_bit_equal_to_their_own_calls(B, N):
    fxs, ys = _members(B, N)
    single = [P.logpdf_and_gradient(fx, y) for fx, y in zip(fxs, ys)]
    got = P.logpdf_and_gradient_batch(fxs, ys)
    assert len(got) == B
    for g, r in zip(got, single):
        _assert_bit_equal(g, r)
    for g, r in zip(P.logpdf_and_gradient_batch(fxs, ys), single):      # repeated call: the pool is reused
        _assert_bit_equal(g, r)


def test_structured_members_with_diagonal_noise_and_means_against_the_oracle():
    """Three processes, two of them independent (zero blocks in K: the member's own call skips them, the batch computes them
    as the exact zeros they are), non-zero means, diagonal noise: the oracle's cotangents at 1e-10, the own call's bits."""
    rng = np.random.default_rng(21)
    Fo, Fp, fo, _ = both(models.toy_gppp)
    names = list(fo)[:3]
    fxs, ys, cases = [], [], []
    for b in range(4):
        xs = [rng.standard_normal(n) * (1.0 + 0.2 * b) for n in (400, 300, 331)]
        xo, xp = blockdata(names, xs, False)
        N = sum(len(x) for x in xs)
        noise = 0.05 + 0.2 * rng.random(N)
        y = rng.standard_normal(N)
        fxs.append(Fp(xp, noise))
        ys.append(y)
        cases.append((Fo(xo, noise), y))
    got = P.logpdf_and_gradient_batch(fxs, ys)
    for g, fx, y, (fo_, yo) in zip(got, fxs, ys, cases):
        _assert_bit_equal(g, P.logpdf_and_gradient(fx, y))
        lp_o, alpha, G = oagp.logpdf_gradient_wrt_cov(fo_, yo)
        assert abs(g["logpdf"] - lp_o) <= 1e-10 * abs(lp_o)
        assert rel(g["y"], -alpha) < 1e-10 and rel(g["mean"], alpha) < 1e-10
        assert rel(g["noise"], np.diag(G)) < 1e-10
        gc, gs = g["_raw"]
        for t, (ec, es) in enumerate(_oracle_term_grads(g["_spec"], G)):
            assert abs(gc[t] - ec) <= 1e-10 * max(1.0, abs(ec)), (t, gc[t], ec)
            assert abs(gs[t] - es) <= 2e-6 * max(1.0, abs(es)), (t, gs[t], es)   # FD reference for dk/dg


def test_n4k_configuration_inside_a_batch_of_eight_against_the_golden():
    w = bench_configs.build(P, "n4k")
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "grad_configs.json")))["cases"]["n4k"]
    others, oys = _members(7, w["N"], seed=8)
    got = P.logpdf_and_gradient_batch([w["fx"]] + others, [w["y"]] + oys)
    g = got[0]
    assert abs(g["logpdf"] - ref["logpdf"]) <= 1e-10 * abs(ref["logpdf"])
    assert abs(g["noise"] - ref["d_sigma2"]) <= 1e-10 * abs(ref["d_sigma2"])
    assert abs(g["terms"][0]["d_inscale"] - ref["d_inscale"]) <= 1e-10 * abs(ref["d_inscale"])
    _assert_bit_equal(g, P.logpdf_and_gradient(w["fx"], w["y"]))


@pytest.mark.parametrize("N", [640, 4096])
def test_one_bad_member_does_not_lose_the_others(N):
    fxs, ys = _members(4, N, seed=9)
    fxs[2] = fxs[2].f(fxs[2].x, -3.0)                     # K - 3 I: not positive definite
    with pytest.raises(P.PosDefException) as e:
        P.logpdf_and_gradient(fxs[2], ys[2])
    got, infos = P.logpdf_and_gradient_batch(fxs, ys, return_infos=True)
    assert np.isnan(got[2]["logpdf"]) and got[2]["info"] == e.value.info == infos[2] >= 1 and got[2]["terms"] is None
    for b in (0, 1, 3):
        assert infos[b] == 0
        _assert_bit_equal(got[b], P.logpdf_and_gradient(fxs[b], ys[b]))


def test_mixed_sizes_and_dense_noise_run_member_by_member():
    f1, y1 = _members(2, 500, seed=1)
    f2, y2 = _members(2, 700, seed=2)
    fxs, ys = f1 + f2, y1 + y2
    for g, fx, y in zip(P.logpdf_and_gradient_batch(fxs, ys), fxs, ys):
        _assert_bit_equal(g, P.logpdf_and_gradient(fx, y))
    rng = np.random.default_rng(3)
    dense = []
    for fx in f1:
        Bm = rng.standard_normal((500, 4))
        dense.append(fx.f(fx.x, 0.2 * np.eye(500) + 0.01 * Bm @ Bm.T))
    for g, fx, y in zip(P.logpdf_and_gradient_batch(dense, y1), dense, y1):
        _assert_bit_equal(g, P.logpdf_and_gradient(fx, y))
        assert g["noise"].shape == (500, 500)


def test_batch_gradient_matches_finite_differences_of_hyperparameters():
    """variance, lengthscale and noise of member 1 of a batch against central differences of the GPU logpdf (the tolerance of
    the single call's FD test, tests/test_gpu_parity.py)"""
    rng = np.random.default_rng(9)
    X = P.ColVecs(rng.standard_normal((3, 400)))
    y = rng.standard_normal(400)

    def model(v, l):
        return np.sqrt(v) * P.stretch(P.atomic(P.GP(P.Matern52Kernel()), P.GPC()), 1.0 / l)

    v, l, s2 = 1.7, 0.8, 0.25
    others, oys = _members(3, 400, D=3, seed=4)
    g = P.logpdf_and_gradient_batch([others[0], model(v, l)(X, s2)] + others[1:], [oys[0], y] + oys[1:])[1]
    (term,) = g["terms"]
    h = 1e-5
    fd_v = (P.logpdf(model(v + h, l)(X, s2), y) - P.logpdf(model(v - h, l)(X, s2), y)) / (2 * h)
    fd_l = (P.logpdf(model(v, l + h)(X, s2), y) - P.logpdf(model(v, l - h)(X, s2), y)) / (2 * h)
    fd_s = (P.logpdf(model(v, l)(X, s2 + h), y) - P.logpdf(model(v, l)(X, s2 - h), y)) / (2 * h)
    assert abs(term["d_coef"] - fd_v) <= 1e-6 * max(1.0, abs(fd_v))
    assert abs(-(1.0 / l) * term["d_inscale"] - fd_l) <= 1e-6 * max(1.0, abs(fd_l))
    assert abs(g["noise"] - fd_s) <= 1e-6 * max(1.0, abs(fd_s))


def test_batch_switched_off_and_under_a_forced_timeout(monkeypatch):
    """SGP_BATCH_MAX_N=0: member by member.  SGP_DF_TIMEOUT_S tiny: the pooled launch runs into its wait bound, the call
    reports the time-out whatever the members' own infos say and reruns on the launch-based schedule -- same bits."""
    fxs, ys = _members(6, 1024, seed=3)
    good = [P.logpdf_and_gradient(fx, y) for fx, y in zip(fxs, ys)]
    for env in ({"SGP_BATCH_MAX_N": "0"}, {"SGP_DF_TIMEOUT_S": "1e-7"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = P.lib.Context(0)
        prev = P.lib.set_default_context(ctx)
        try:
            for g, r in zip(P.logpdf_and_gradient_batch(fxs, ys), good):
                _assert_bit_equal(g, r)
        finally:
            P.lib.set_default_context(prev)
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)
