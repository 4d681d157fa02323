"""Gradients through stencil terms without a GPU: the expansion behind the truth (tests/stencil_grad_truth.py) against
np_spec_matrix, the float64 yardstick of every case against its long-double truth and the floors recorded from it, the host
functions logpdf_and_gradient_stencil / elbo_and_gradient_stencil over the NumPy double of the three entry points
(tests/stencil_grad_np.py) against central differences of the NumPy logpdf / Titsias bound -- coefficients, lengthscale,
noise and the points, chained back through Stretch and Shift below the stencil -- the caller's term order, the refusals, and
the extension header include/sthenomi_stencil_grad.h (plain C, exactly what libsthenomi_stencil_grad.so exports and lib.py
types).

`python tests/test_stencil_grad_on_numpy.py` prints the float64 figures of every case and family: the lists recorded in
stencil_grad_truth.MEASURED_FLOAT64."""
import os
import subprocess

import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (registers the product package, as under pytest)

import grad_truth as T
import stencil_grad_np
import stencil_grad_truth as ST
import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_stencil_on_numpy import np_spec_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the expansion ---------------------------------------------------------------------------------------------------
def _specs():
    rng = np.random.default_rng(1)
    F = ST.model("m52", 2, ST.quad_stencil(2, 5), ST.fd_stencil(2))
    pts = lambda n: P.ColVecs(np.asfortranarray(rng.standard_normal((2, n))))     # noqa: E731
    yield P.build_spec(F, P.GPPPInput("g", pts(6)))[0], [25]
    yield P.build_spec(F, P.BlockData([P.GPPPInput("gu", pts(5)), P.GPPPInput("f", pts(3)), P.GPPPInput("h", pts(4))]))[0], None
    yield P.build_spec(F, P.GPPPInput("g", pts(6)), None, P.GPPPInput("h", pts(4)))[0], [10]
    yield P.build_spec(F, P.GPPPInput("f", pts(3)), None, P.GPPPInput("ug", pts(4)))[0], None


def test_expansion_reproduces_np_spec_matrix():
    for spec, counts in _specs():
        assert spec.has_stencil
        S = ST.read_spec(spec)
        Sx, owner, weight, in_map = ST.expand(S)
        assert len(owner) == len(weight) == len(Sx["terms"]) and set(owner) == set(range(spec.n_terms))
        n_exp = [(1 if r is None else len(r[1])) * (1 if c is None else len(c[1])) for r, c in S["stencils"]]
        assert [int((owner == t).sum()) for t in range(spec.n_terms)] == n_exp
        if counts is not None:
            assert n_exp == counts
        K, Ke = np_spec_matrix(spec), T.dense(Sx, np.float64)
        assert np.max(np.abs(K - Ke)) <= 1e-12 * np.max(np.abs(K))


# ---- 2. the yardstick and the floors --------------------------------------------------------------------------------------
def _figures(case, monkeypatch):
    """e_float64 of a case, family by family: the reference's float64 runs against its long-double run.  The specs come from
    the host mirror running on the NumPy double; the double's numbers are not looked at."""
    stencil_grad_np.install(monkeypatch)
    if case.family == "lp":
        F, fx, y = case.build()
        g = P.logpdf_and_gradient_stencil(fx, y, inputs=True)
        R, *R64 = ST.logpdf_truth(case, g["_spec"], fx, y)
        return ST.yardstick(ST.logpdf_units(ST.logpdf_reference_outputs(r), R) for r in R64)
    F, fz, fx, y = case.build()
    g = P.elbo_and_gradient_stencil(P.VFE(fz), fx, y, inputs=True)
    var_x = P.finite_gp._kernelmatrix_diag(g["_specs"]["xx"])
    R, *R64 = ST.elbo_truth(case, g["_specs"], fz, fx, y, var_x)
    return ST.yardstick(ST.elbo_units(ST.elbo_reference_outputs(r), R) for r in R64)


@pytest.mark.parametrize("case", ST.CASES, ids=repr)
def test_float64_run_is_inside_its_bound(case, monkeypatch):
    for fam, e in _figures(case, monkeypatch).items():
        assert np.isfinite(e)
        assert e <= T.SELF_MARGIN * max(e, ST.floor_of(fam)), (case.id, fam, e)
        if fam.startswith("st."):          # the recorded figure is this run's (to the printed digit and the last bits)
            assert any(abs(e - v) <= 0.05 + 0.25 * v for v in ST.MEASURED_FLOAT64[fam]), (case.id, fam, e)


def test_floors_are_the_medians_of_the_recorded_float64_figures():
    assert set(ST.FLOORS) == set(ST.MEASURED_FLOAT64) == {"st.lp.d_coef", "st.lp.d_inscale", "st.lp.inputs", "st.elbo.d_coef",
                                                          "st.elbo.d_inscale", "st.elbo.inputs"}
    for fam, vals in ST.MEASURED_FLOAT64.items():
        assert len(vals) == len(ST.LP_CASES if ".lp." in fam else ST.ELBO_CASES)
        assert ST.FLOORS[fam] == float(np.median(vals)), fam


def test_the_finite_difference_stencils_have_moderate_weights():
    for c in ST.CASES:
        for A, w in c.stencils():
            assert np.max(np.abs(w)) <= 10.0 + 1e-12 and A.shape == (c.D, len(w)) and len(w) <= 64


# ---- 3. the host functions over the double, against central differences ------------------------------------------------------
TH0 = dict(v=1.3, vu=0.4, l=0.9, s2=0.15)
A0, W0 = np.array([[0.0, 0.1, -0.25], [0.0, -0.05, 0.1]]), np.array([-6.0, 10.0, -3.0])
SHIFT, STRETCH = np.array([0.3, -0.2]), 0.7


def hyper_model(**th):
    """f = GP(v Matern52(l)), u = GP(vu SE); g = stencil(shift(stretch(f, 0.7), b), A, w); gu = g + u"""
    th = dict(TH0, **th)

    def build(GP):
        f = GP(th["v"] * P.with_lengthscale(P.Matern52Kernel(), th["l"]))
        u = GP(th["vu"] * P.SEKernel())
        g = P.stencil(P.shift(P.stretch(f, STRETCH), SHIFT), A0, W0)
        return {"f": f, "u": u, "g": g, "gu": g + u}
    return P.gppp(build)


def np_logpdf(K, y):
    Lc = np.linalg.cholesky(K)
    a = np.linalg.solve(Lc, y)
    return -0.5 * a @ a - np.sum(np.log(np.diag(Lc))) - 0.5 * len(y) * np.log(2 * np.pi)


def np_lp(name, X, y, **th):
    th = dict(TH0, **th)
    x = P.GPPPInput(name, P.ColVecs(np.asfortranarray(X)))
    return np_logpdf(np_spec_matrix(P.build_spec(hyper_model(**th), x)[0]) + th["s2"] * np.eye(len(y)), y)


def np_bound(xname, X, zname, Z, y, **th):
    """the Titsias bound from np_spec_matrix: logpdf under Q + s2 I minus the trace term"""
    th = dict(TH0, **th)
    F = hyper_model(**th)
    x, z = P.GPPPInput(xname, P.ColVecs(np.asfortranarray(X))), P.GPPPInput(zname, P.ColVecs(np.asfortranarray(Z)))
    Kzz = np_spec_matrix(P.build_spec(F, z)[0]) + 1e-3 * np.eye(Z.shape[1])
    Kxz = np_spec_matrix(P.build_spec(F, x, None, z)[0])
    var = np.diag(np_spec_matrix(P.build_spec(F, x)[0]))
    A = np.linalg.solve(np.linalg.cholesky(Kzz), Kxz.T)
    Q = A.T @ A
    return np_logpdf(Q + th["s2"] * np.eye(len(y)), y) - 0.5 * (np.sum(var) - np.trace(Q)) / th["s2"]


def _d_theta(records):
    """(d / dv, d / dvu, d / dl) from the term records: coef = v (or vu) times the model's scalings; the points AND the
    offsets of f's terms are read divided by l, so d / dl = -sum d_inscale / l"""
    f = [r for r in records if r["kind"] == P.lib.MATERN52]
    u = [r for r in records if r["kind"] == P.lib.SE]
    return (sum(r["d_coef"] * r["coef"] for r in f) / TH0["v"], sum(r["d_coef"] * r["coef"] for r in u) / TH0["vu"],
            -sum(r["d_inscale"] for r in f) / TH0["l"])


H = 1e-5


def _fd(f, name):
    """the central difference in log(theta), as d / d theta"""
    return (f(**{name: TH0[name] * np.exp(H)}) - f(**{name: TH0[name] * np.exp(-H)})) / (2 * H) / TH0[name]


def _fd_x(f, X, d, j):
    Xp, Xn = X.copy(), X.copy()
    Xp[d, j] += H
    Xn[d, j] -= H
    return (f(Xp) - f(Xn)) / (2 * H)


def _off(a, fd, name=None):
    th = TH0[name] if name else 1.0
    return abs(a - fd) * th / max(1.0, abs(fd) * th)


def _fd_model(value):
    """what such a central difference can be off by: the rounding of the two values, eps |f| / H, and the third-derivative
    term H^2 |f| (smooth functions of the logarithms of their parameters and of O(1) coordinates)"""
    return 2.0 ** -52 * abs(value) / H + H * H * abs(value)


def test_host_functions_match_central_differences_of_numpy(monkeypatch):
    stencil_grad_np.install(monkeypatch)
    rng = np.random.default_rng(4)
    X = rng.standard_normal((2, 9))
    y = rng.standard_normal(9)
    fx = hyper_model()(P.GPPPInput("gu", P.ColVecs(np.asfortranarray(X))), TH0["s2"])
    g = P.logpdf_and_gradient_stencil(fx, y, inputs=True)
    assert g["_spec"].has_stencil and abs(g["logpdf"] - np_lp("gu", X, y)) <= 1e-12 * abs(g["logpdf"])
    # the caller's order: the stencil term of g precedes the plain term of u in the pair, and the records follow it
    assert [r["kind"] for r in g["terms"]] == [P.lib.MATERN52, P.lib.SE]
    assert g["terms"][0]["row_stencil"] is not None and g["terms"][1]["row_stencil"] is None
    need = 0.0
    for name, a in zip(("v", "vu", "l", "s2"), _d_theta(g["terms"]) + (g["noise"],)):
        need = max(need, _off(a, _fd(lambda **th: np_lp("gu", X, y, **th), name), name))
    for (d, j) in ((0, 0), (1, 8), (0, 4)):          # the chain back through Shift and Stretch below the stencil
        need = max(need, _off(g["x"][0][d, j], _fd_x(lambda Xm: np_lp("gu", Xm, y), X, d, j)))
    model = _fd_model(g["logpdf"])
    print(f"logpdf: variances, lengthscale, noise, points need {need:.2e}; the difference's own error {model:.2e}")
    assert need <= 2 * model
    # the ELBO: data at g, inducing points at f, then at g itself
    for zname in ("f", "g"):
        Z = rng.standard_normal((2, 4))
        F = hyper_model()
        fz = F(P.GPPPInput(zname, P.ColVecs(np.asfortranarray(Z))), 1e-3)
        fg = F(P.GPPPInput("g", P.ColVecs(np.asfortranarray(X))), TH0["s2"])
        ge = P.elbo_and_gradient_stencil(P.VFE(fz), fg, y, inputs=True)
        assert abs(ge["elbo"] - np_bound("g", X, zname, Z, y)) <= 1e-10 * abs(ge["elbo"])
        assert (len(ge["zz_terms"]), len(ge["xz_terms"]), len(ge["xx_terms"])) == (1, 1, 1)
        dv, _, dl = _d_theta(ge["zz_terms"] + ge["xz_terms"] + ge["xx_terms"])
        need = 0.0
        for name, a in (("v", dv), ("l", dl), ("s2", ge["noise"])):
            need = max(need, _off(a, _fd(lambda **th: np_bound("g", X, zname, Z, y, **th), name), name))
        for (d, j) in ((0, 0), (1, 3)):
            need = max(need, _off(ge["z"][0][d, j], _fd_x(lambda Zm: np_bound("g", X, zname, Zm, y), Z, d, j)))
        for (d, j) in ((0, 1), (1, 7)):
            need = max(need, _off(ge["x"][0][d, j], _fd_x(lambda Xm: np_bound("g", Xm, zname, Z, y), X, d, j)))
        model = _fd_model(ge["elbo"])
        print(f"elbo, z in {zname}: variance, lengthscale, noise, inducing and data points need {need:.2e}; "
              f"the difference's own error {model:.2e}")
        assert need <= 2 * model


def test_models_without_stencil_terms_return_what_the_old_functions_return(monkeypatch):
    stencil_grad_np.install(monkeypatch)
    rng = np.random.default_rng(6)
    F = P.gppp(lambda GP: {"f": GP(1.3 * P.with_lengthscale(P.Matern52Kernel(), 0.8)) + GP(0.4 * P.SEKernel())})
    x = P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((3, 11)))))
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((3, 4)))))
    y = rng.standard_normal(11)
    a, b = P.logpdf_and_gradient(F(x, 0.2), y, inputs=True), P.logpdf_and_gradient_stencil(F(x, 0.2), y, inputs=True)
    assert a["logpdf"] == b["logpdf"] and a["terms"] == b["terms"] and a["noise"] == b["noise"]
    assert np.array_equal(a["y"], b["y"]) and np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["x"][0], b["x"][0])
    assert P.logpdf_and_gradient_stencil(F(x, 0.2), y)["inputs"] is None
    a = P.elbo_and_gradient(P.VFE(F(z, 1e-3)), F(x, 0.2), y, inputs=True)
    b = P.elbo_and_gradient_stencil(P.VFE(F(z, 1e-3)), F(x, 0.2), y, inputs=True)
    assert a["elbo"] == b["elbo"] and a["noise"] == b["noise"] and a["z_noise"] == b["z_noise"]
    for key in ("zz_terms", "xz_terms", "xx_terms"):
        assert a[key] == b[key]
    assert all(np.array_equal(p, q) for key in ("x", "z", "zz_inputs", "xz_inputs") for p, q in zip(a[key], b[key]))


def test_the_old_functions_still_raise_and_name_the_new_ones(monkeypatch):
    stencil_grad_np.install(monkeypatch)
    F = hyper_model()
    fx = F(P.GPPPInput("g", P.ColVecs(np.zeros((2, 4)) + np.arange(4.0))), 0.1)
    z = P.GPPPInput("f", P.ColVecs(np.ones((2, 2)) * np.arange(2.0)))
    for call in (lambda: P.logpdf_and_gradient(fx, np.zeros(4)), lambda: P.logpdf_and_gradient_batch([fx], [np.zeros(4)]),
                 lambda: P.logpdf_and_gradient_param(fx, np.zeros(4)), lambda: P.logpdf_and_gradient_conv(fx, np.zeros(4)),
                 lambda: P.elbo_and_gradient(P.VFE(F(z)), fx, np.zeros(4)),
                 lambda: P.elbo_and_gradient_conv(P.VFE(F(z)), fx, np.zeros(4)),
                 lambda: P.elbo_and_gradient_param(P.VFE(F(z)), fx, np.zeros(4))):
        with pytest.raises(NotImplementedError, match="stencil.*logpdf_and_gradient_stencil / elbo_and_gradient_stencil"):
            call()


def test_multi_gpu_contexts_and_products_below_are_refused_by_name(monkeypatch):
    ctx = stencil_grad_np.install(monkeypatch)
    F = hyper_model()
    x = P.GPPPInput("g", P.ColVecs(np.asfortranarray(np.random.default_rng(2).standard_normal((2, 5)))))
    spec = P.build_spec(F, x)[0]
    # the double, as the library: rc < 0 naming the multi-GPU context
    ctx.lib.multi_handles = {ctx.handle.value}
    d, v = P.lib.dptr, np.ones(5)
    rc = ctx.lib.sgp_logpdf_grad_stencil(ctx.handle, spec.ref(), d(v), 0, d(v), d(v), d(np.zeros(1)), None, None, None, None,
                                         None, None)
    assert rc < 0 and "multi-GPU" in ctx.lib.sgp_last_error().decode()
    assert ctx.lib.sgp_kernelmatrix_diag_grad_stencil(ctx.handle, spec.ref(), d(v), None, None, None) < 0
    assert "multi-GPU" in ctx.lib.sgp_last_error().decode()
    ctx.lib.multi_handles = set()
    plain = P.gppp(lambda GP: {"f": GP(P.SEKernel())})
    ctx.is_multi = True
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        P.logpdf_and_gradient_stencil(plain(P.GPPPInput("f", x.x), 0.1), np.zeros(5))
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        P.elbo_and_gradient_stencil(P.VFE(plain(P.GPPPInput("f", x.x), 1e-3)), plain(P.GPPPInput("f", x.x), 0.1), np.zeros(5))
    ctx.is_multi = False
    # a stencil process next to a product of kernels: the records of a product carry d_param, which these calls do not return
    mixed = P.gppp(lambda GP: (lambda f: {"g": P.stencil(f, A0, W0), "p": GP(P.SEKernel() * P.Matern32Kernel())})(
        GP(P.SEKernel())))
    xb = P.BlockData([P.GPPPInput("g", x.x), P.GPPPInput("p", x.x)])
    with pytest.raises(NotImplementedError, match="product of kernels"):
        P.logpdf_and_gradient_stencil(mixed(xb, 0.1), np.zeros(10))


# ---- 4. the extension header -------------------------------------------------------------------------------------------------
def test_stencil_grad_header_is_plain_c(tmp_path):
    src = tmp_path / "stencil_grad_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include "sthenomi_stencil_grad.h"
int main(void) {
  int (*a)(sgp_ctx*, const sgp_cov_spec*, const double*, int, const double*, const double*, double*, double*, double*,
           double*, double*, double*, double* const*) = &sgp_logpdf_grad_stencil;
  int (*b)(sgp_ctx*, const sgp_cov_spec*, const double*, double*, double*, double* const*) = &sgp_kernelmatrix_diag_grad_stencil;
  printf("%d %d %d\n", (int)sizeof(a), (int)sizeof(b), (int)sizeof(&sgp_elbo_grad_stencil));
  return 0;
}
''')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "stencil_grad_consumer.o")])


def test_stencil_grad_library_exports_exactly_its_header():
    syms = _symbols_of("sthenomi_stencil_grad.h")
    assert syms == ["sgp_elbo_grad_stencil", "sgp_kernelmatrix_diag_grad_stencil", "sgp_logpdf_grad_stencil"]
    assert syms == P.lib.stencil_grad_symbols()
    assert _c_exports(P.lib.STENCIL_GRAD_LIB_PATH) == syms
    others = [P.lib.LIB_PATH, P.lib.CONV_LIB_PATH, P.lib.CONV_GRAD_LIB_PATH, P.lib.STENCIL_LIB_PATH, P.lib.KPROD_LIB_PATH,
              P.lib.KPROD_GRAD_LIB_PATH, P.lib.BATCH_LIB_PATH, P.lib.POOL_LIB_PATH, P.lib.EXTEND_LIB_PATH,
              P.lib.POSTFX_LIB_PATH, P.lib.VFE_UPDATE_LIB_PATH, P.lib.BENCH_LIB_PATH]
    for path in others:
        assert not set(syms) & set(_c_exports(path)), path
    assert _c_exports(P.lib.STENCIL_LIB_PATH) == ["sgp_stencil_register"]
    for header in ("sthenomi.h", "sthenomi_stencil.h", "sthenomi_conv_grad.h", "sthenomi_kprod_grad.h"):
        assert not set(syms) & set(_symbols_of(header))


if __name__ == "__main__":          # the measurement behind stencil_grad_truth.FLOORS / MEASURED_FLOAT64
    import pprint
    import time

    class _MP:
        def __init__(self):
            self.undo = []

        def setattr(self, obj, name, value):
            self.undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)

        def close(self):
            for obj, name, value in reversed(self.undo):
                setattr(obj, name, value)

    lists = {}
    for c in ST.CASES:
        mp, t0 = _MP(), time.time()
        figs = _figures(c, mp)
        mp.close()
        for fam, e in figs.items():
            if fam.startswith("st."):
                lists.setdefault(fam, []).append(round(e, 1))
            print(f"{c.id:22s} {fam:20s} {e:10.1f}", flush=True)
        print(f"{c.id:22s} truth and yardstick: {time.time() - t0:.1f} s", flush=True)
    lists = {k: sorted(v) for k, v in lists.items()}
    print("MEASURED_FLOAT64 = ", end="")
    pprint.pprint(lists, width=120, compact=True)
    print("FLOORS = ", end="")
    pprint.pprint({k: float(np.median(v)) for k, v in lists.items()}, width=120)
