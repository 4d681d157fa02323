"""Two pins on the shared read side of a kept posterior (csrc/kept.h), on the device (run with -m gpu on an MI355X).

(a) The sparse predict call makes ONE pass over the solved cross rows whatever is asked of it: mean_and_var and mean_and_cov
    of a VFE posterior are np.array_equal to mean, var and cov asked one at a time.  (Two passes gave the same bits: this
    guards the one pass against a later change, it does not tell it from two.)
(b) The uploaded and the assembled cross side meet in one path: sgp_posterior_predict_explicit, fed sgp_kernelmatrix of the
    cross spec, sgp_kernelmatrix_diag and sgp_kernelmatrix of prior_ss and the same mean_s, is np.array_equal to
    sgp_posterior_predict for mean, var and cov.

Sizes: N in {200, 256} training points (inside a tile, on a tile edge) in two blocks, M = 130 inducing points, N* in
{1, 128, 150}, D = 2; f1 ~ SE, f2 ~ Matern32, f3 = f1 + f2."""
import numpy as np
import pytest

import stheno_jl_amd as P

pytestmark = pytest.mark.gpu

L = P.lib
D, M = 2, 130


def _blocks(rng, names, sizes):
    return P.BlockData([P.GPPPInput(k, P.ColVecs(np.asfortranarray(rng.uniform(-2, 2, (D, n))))) for k, n in zip(names, sizes)])


class _Case:
    """the model, its data and the exact and VFE posteriors at one training size, built once"""

    def __init__(self, N):
        rng = np.random.default_rng(N)
        self.F = P.gppp(lambda GP: (lambda f1, f2: {"f1": f1, "f2": f2, "f3": f1 + f2})(GP(P.SEKernel()), GP(P.Matern32Kernel())))
        self.x = _blocks(rng, ("f3", "f1"), (N - N // 3, N // 3))
        y = rng.standard_normal(N)
        self.star = {1: _blocks(rng, ("f3",), (1,)), 128: _blocks(rng, ("f2", "f3"), (70, 58)),
                     150: _blocks(rng, ("f2", "f3"), (80, 70))}
        self.exact = P.posterior(self.F(self.x, 0.1), y)
        self.vfe = P.posterior(P.VFE(self.F(_blocks(rng, ("f3",), (M,)), 1e-6)), self.F(self.x, 0.1), y)


_cases = {}


@pytest.fixture(params=[200, 256])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = _Case(request.param)
    return _cases[request.param]


@pytest.mark.parametrize("n", [1, 128, 150])
def test_sparse_moments_in_one_call_are_those_asked_one_at_a_time(case, n):
    xs = case.star[n]
    m, v, c = case.vfe.mean(xs), case.vfe.var(xs), case.vfe.cov(xs)
    mv, mc = case.vfe.mean_and_var(xs), case.vfe.mean_and_cov(xs)
    assert np.array_equal(mv[0], m) and np.array_equal(mv[1], v)
    assert np.array_equal(mc[0], m) and np.array_equal(mc[1], c)


@pytest.mark.parametrize("n", [1, 128, 150])
def test_explicit_predict_is_predict_on_the_matrices_of_its_specs(case, n):
    xs, post = case.star[n], case.exact
    cross, _, _ = P.build_spec(post.prior, xs, post.prior, post.x)
    pss = P.finite_gp._prior_spec(post.prior, xs)
    ms = np.ascontiguousarray(P.mean_vector(post.prior, xs), dtype=np.float64)
    lib, h = L.default_context().lib, post._ensure()

    def outs():
        return np.zeros(n), np.zeros(n), np.zeros((n, n), order="F")
    m0, v0, c0 = outs()
    L.check(lib.sgp_posterior_predict(h, cross.ref(), pss.ref(), L.dptr(ms), L.dptr(m0), L.dptr(v0), L.dptr(c0), n),
            "sgp_posterior_predict")
    Kc = np.asfortranarray(P.finite_gp._kernelmatrix(cross))          # N* x N
    kd = np.ascontiguousarray(P.finite_gp._kernelmatrix_diag(pss))
    Kp = np.asfortranarray(P.finite_gp._kernelmatrix(pss))
    assert Kc.shape == (n, len(post.x)) and Kc.dtype == kd.dtype == Kp.dtype == np.float64
    m1, v1, c1 = outs()
    L.check(lib.sgp_posterior_predict_explicit(h, L.dptr(Kc), n, n, L.dptr(kd), L.dptr(Kp), n, L.dptr(ms), L.dptr(m1), L.dptr(v1),
                                               L.dptr(c1), n), "sgp_posterior_predict_explicit")
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0) and np.array_equal(c1, c0)
