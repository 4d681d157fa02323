"""The entry points each of the eight gradient functions of the host mirror calls, in order, for every combination of its
flags -- over the NumPy doubles (np_capi, conv_grad_np, stencil_wo_np, the product double of test_kprod_grad_on_numpy), with a
recorder around the fake library.  The doubles depend on the order (stencil_wo_np reads the cotangents of zz, then xz; every
ELBO gradient reads var(f, x) before its gradient call and the diagonal's gradient after it), and a registration
(sgp_conv_geom, sgp_stencil_register) happens where a spec is first handed to the library."""
import numpy as np
import pytest

import conv_grad_np
import np_capi
import stencil_wo_np
import stheno_jl_amd as P
import test_kprod_grad_on_numpy as TK
from test_conv_on_numpy import images


class Recorder:
    """the fake library, with the name of every sgp_* entry point it is asked to run appended to `calls`"""

    def __init__(self, inner, calls):
        self.__dict__.update(_inner=inner, _calls=calls)

    def __getattr__(self, name):
        f = getattr(self._inner, name)
        if not name.startswith("sgp_") or not callable(f):
            return f

        def call(*args):
            self._calls.append(name)
            return f(*args)
        return call

    def __setattr__(self, name, value):
        setattr(self._inner, name, value)


def _install(double, monkeypatch):
    calls = []
    if double == "kprod":
        ctx = TK.install_fake(monkeypatch)
        fake = ctx.kprod_grad

        class Kprod:        # sgp_logpdf_grad_param is sgp_logpdf_grad_param_xs without its two tables (include/sthenomi_kprod.h)
            def sgp_logpdf_grad_param(self, *args):
                return fake.sgp_logpdf_grad_param_xs(*args, None, None)
        ctx.kprod, ctx.kprod_grad, ctx.is_multi = Recorder(Kprod(), calls), Recorder(fake, calls), False
    else:
        ctx = {"plain": np_capi, "conv": conv_grad_np, "stencil": stencil_wo_np}[double].install(monkeypatch)
    ctx.lib = Recorder(ctx.lib, calls)      # (the doubles' install() reaches ctx.lib at call time)
    return calls


def _blocks(name, seed, ns, D=2):
    rng = np.random.default_rng(seed)
    return P.BlockData([P.GPPPInput(name, P.ColVecs(np.asfortranarray(rng.standard_normal((D, n))))) for n in ns])


def _sigma(v):
    return 1.0 + 0.5 * float(np.sin(np.sum(v)))


def _plain():
    return P.gppp(lambda GP: {"f": _sigma * P.stretch(GP(1.3 * P.Matern52Kernel()), 0.7) + GP(0.4 * P.SEKernel())}), "f", "f"


def _product():
    k = 1.1 * (P.SEKernel() @ P.ARDTransform(np.array([0.7, 1.2]))) * P.Matern32Kernel() + 0.6 * P.RationalQuadraticKernel(1.3)
    return P.gppp(lambda GP: {"f": _sigma * GP(k)}), "f", "f"


def _stencil():
    A, w = np.array([[0.0, 0.1, -0.25], [0.0, -0.05, 0.1]]), np.array([-0.6, 1.0, -0.3])
    return P.gppp(lambda GP: (lambda f: {"f": f, "g": P.stencil(P.stretch(f, 0.7), A, w)})(GP(1.3 * P.Matern52Kernel()))), "g", "f"


def _pair(model, monkeypatch, double):
    """(the recorded calls, fx, VFE(fz), y) of a two-block model with 4 + 3 observations and 2 + 2 inducing points"""
    F, xname, zname = model()
    calls = _install(double, monkeypatch)
    return calls, F(_blocks(xname, 1, (4, 3)), 0.15), P.VFE(F(_blocks(zname, 2, (2, 2)), 1e-3)), np.random.default_rng(3).standard_normal(7)


def _patch_pair(monkeypatch):
    def build(GP):
        g = GP(0.002 * P.with_lengthscale(P.SEKernel(), 2.2))
        f = P.patch_convolve(P.stretch(g, 0.7))
        return {"g": g, "f": f, "fh": f + GP(0.5 * P.Matern32Kernel())}
    F = P.gppp(build)
    calls = _install("conv", monkeypatch)
    z = P.GPPPInput("g", P.ColVecs(np.asfortranarray(np.random.default_rng(7).standard_normal((9, 3)))))
    return calls, F, P.VFE(F(z, 1e-3)), np.random.default_rng(3).standard_normal(5)


FLAGS = [(False, False), (True, False), (False, True), (True, True)]
DIAG = "sgp_kernelmatrix_diag"


def _suffix(inputs, scales):
    return "_xs" if scales else "_x" if inputs else ""


@pytest.mark.parametrize("inputs,scales", FLAGS)
def test_plain_family(inputs, scales, monkeypatch):
    calls, fx, vfe, y = _pair(_plain, monkeypatch, "plain")
    P.logpdf_and_gradient(fx, y, inputs=inputs, scales=scales)
    assert calls == ["sgp_logpdf_grad" + _suffix(inputs, scales)]
    del calls[:]
    P.elbo_and_gradient(vfe, fx, y, inputs=inputs, scales=scales)
    assert calls == [DIAG, "sgp_elbo_grad" + _suffix(inputs, scales), "sgp_kernelmatrix_diag_grad" + _suffix(inputs, scales)]


@pytest.mark.parametrize("inputs,scales", FLAGS)
def test_param_family(inputs, scales, monkeypatch):
    calls, fx, vfe, y = _pair(_product, monkeypatch, "kprod")
    P.logpdf_and_gradient_param(fx, y, inputs=inputs, scales=scales)
    assert calls == ["sgp_logpdf_grad_param_xs"]
    del calls[:]
    P.elbo_and_gradient_param(vfe, fx, y, inputs=inputs, scales=scales)
    assert calls == [DIAG, "sgp_elbo_grad_param", "sgp_kernelmatrix_diag_grad_param"]


def test_a_product_model_through_the_plain_function_and_the_families_that_forward_it(monkeypatch):
    calls, fx, vfe, y = _pair(_product, monkeypatch, "kprod")
    for call, expected in ((lambda: P.logpdf_and_gradient(fx, y), "sgp_logpdf_grad_param"),
                           (lambda: P.logpdf_and_gradient_conv(fx, y), "sgp_logpdf_grad_param"),
                           (lambda: P.logpdf_and_gradient_stencil(fx, y, stencils=True), "sgp_logpdf_grad_param"),
                           (lambda: P.logpdf_and_gradient_stencil(fx, y, inputs=True), "sgp_logpdf_grad_param_xs")):
        del calls[:]
        call()
        assert calls == [expected]
    del calls[:]
    for call in (lambda: P.logpdf_and_gradient(fx, y, inputs=True), lambda: P.elbo_and_gradient(vfe, fx, y),
                 lambda: P.elbo_and_gradient_conv(vfe, fx, y), lambda: P.elbo_and_gradient_stencil(vfe, fx, y)):
        with pytest.raises(NotImplementedError, match="product"):
            call()
    assert calls == []          # refused before any library call


@pytest.mark.parametrize("inputs", [False, True])
def test_conv_family(inputs, monkeypatch):
    calls, F, vfe, y = _patch_pair(monkeypatch)
    P.logpdf_and_gradient_conv(F(P.GPPPInput("fh", images(5, seed=3)), 0.15), y)
    assert calls == ["sgp_conv_geom", "sgp_logpdf_grad_conv"]
    del calls[:]
    # xx binds its geometry for sgp_kernelmatrix_diag, xz where the gradient call takes it; zz has no patch side
    P.elbo_and_gradient_conv(vfe, F(P.GPPPInput("f", images(5, seed=3)), 0.15), y, inputs=inputs)
    assert calls == ["sgp_conv_geom", DIAG, "sgp_conv_geom", "sgp_elbo_grad_conv", "sgp_kernelmatrix_diag_grad_conv"]


def test_conv_family_on_a_plain_model(monkeypatch):
    calls, fx, vfe, y = _pair(_plain, monkeypatch, "conv")
    P.logpdf_and_gradient_conv(fx, y)
    P.elbo_and_gradient_conv(vfe, fx, y, inputs=True)
    assert calls == ["sgp_logpdf_grad_conv", DIAG, "sgp_elbo_grad_conv", "sgp_kernelmatrix_diag_grad_conv"]


@pytest.mark.parametrize("inputs,stencils", FLAGS)
def test_stencil_family(inputs, stencils, monkeypatch):
    calls, fx, vfe, y = _pair(_stencil, monkeypatch, "stencil")
    wo = "_wo" if stencils else ""
    P.logpdf_and_gradient_stencil(fx, y, inputs=inputs, stencils=stencils)
    assert calls == ["sgp_stencil_register", "sgp_logpdf_grad_stencil" + wo]
    del calls[:]
    # xx registers its stencil for sgp_kernelmatrix_diag, xz where the gradient call takes it; zz (z in f) has none
    P.elbo_and_gradient_stencil(vfe, fx, y, inputs=inputs, stencils=stencils)
    assert calls == ["sgp_stencil_register", DIAG, "sgp_stencil_register", "sgp_elbo_grad_stencil" + wo,
                     "sgp_kernelmatrix_diag_grad_stencil" + wo]
