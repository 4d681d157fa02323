"""Gradients through patch (convolutional) terms without a GPU: the expansion behind the truth (tests/conv_grad_truth.py)
against np_spec_matrix, the float64 yardstick of every case against its long-double truth and the floors recorded from it,
the host functions logpdf_and_gradient_conv / elbo_and_gradient_conv over the NumPy double of the three entry points
(tests/conv_grad_np.py) against central differences of the NumPy logpdf / Titsias bound, the refusals, and the extension
header include/sthenomi_conv_grad.h (plain C, exactly what libsthenomi_conv_grad.so exports and lib.py types).

`python tests/test_conv_grad_on_numpy.py` prints the float64 figures of every case and family: the lists recorded in
conv_grad_truth.MEASURED_FLOAT64."""
import os
import subprocess

import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (registers the product package, as under pytest)

import conv_grad_np
import conv_grad_truth as CT
import grad_truth as T
import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_conv_on_numpy import conv_model, images, np_spec_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the expansion ---------------------------------------------------------------------------------------------------
def _specs():
    f = conv_model()
    x, z = P.GPPPInput("f", images(5)), P.GPPPInput("g", P.ColVecs(np.random.default_rng(1).standard_normal((9, 4))))
    yield P.build_spec(f, x)[0]
    yield P.build_spec(f, P.BlockData([P.GPPPInput("fh", images(5)), z]))[0]        # every mix of sides, and a plain term
    yield P.build_spec(f, x, None, z)[0]
    yield P.build_spec(f, z, None, P.GPPPInput("f2", images(3, seed=2)))[0]


def test_expansion_reproduces_np_spec_matrix():
    for spec in _specs():
        S = CT.read_spec(spec)
        Sx, owner, in_map = CT.expand(S)
        assert len(owner) == len(Sx["terms"]) and set(owner) == set(range(spec.n_terms))
        n_exp = [(36 if rg else 1) * (36 if cg else 1) for rg, cg in S["geoms"]]
        assert [int((owner == t).sum()) for t in range(spec.n_terms)] == n_exp
        K, Ke = np_spec_matrix(spec), T.dense(Sx, np.float64)
        assert np.max(np.abs(K - Ke)) <= 1e-12 * np.max(np.abs(K))


# ---- 2. the yardstick and the floors --------------------------------------------------------------------------------------
def _figures(case, monkeypatch):
    """e_float64 of a case, family by family: the reference's float64 runs against its long-double run.  The specs come from
    the host mirror running on the NumPy double; the double's numbers are not looked at."""
    conv_grad_np.install(monkeypatch)
    if case.family == "lp":
        F, fx, y = case.build()
        R, *R64 = CT.logpdf_truth(case, P.logpdf_and_gradient_conv(fx, y), fx, y)
        return CT.yardstick(CT.logpdf_units(CT.logpdf_reference_outputs(r), R) for r in R64)
    F, fz, fx, y = case.build()
    # (the staging case's diagonal has 2337^2 pairs of patches per entry: the bound takes var_x as data, any positive vector)
    var_x = P.finite_gp._kernelmatrix_diag(P.build_spec(F, fx.x)[0]) if case.truth_xx else np.full(len(fx), 1.7)
    if not case.truth_xx:
        monkeypatch.setattr(P.finite_gp, "_kernelmatrix_diag", lambda spec: var_x)
        monkeypatch.setattr(conv_grad_np.FakeLib, "sgp_kernelmatrix_diag_grad_conv", lambda self, *a: 0)
    R, *R64 = CT.elbo_truth(case, P.elbo_and_gradient_conv(P.VFE(fz), fx, y, inputs=True), fz, fx, y, var_x)
    return CT.yardstick(CT.elbo_units(CT.elbo_reference_outputs(r), R) for r in R64)


@pytest.mark.parametrize("case", CT.CASES, ids=repr)
def test_float64_run_is_inside_its_bound(case, monkeypatch):
    for fam, e in _figures(case, monkeypatch).items():
        assert np.isfinite(e)
        assert e <= T.SELF_MARGIN * max(e, CT.floor_of(fam)), (case.id, fam, e)
        if fam.startswith("conv."):          # the recorded figure is this run's (to the printed digit and the last bits)
            assert any(abs(e - v) <= 0.05 + 0.25 * v for v in CT.MEASURED_FLOAT64[fam]), (case.id, fam, e)


def test_floors_are_the_medians_of_the_recorded_float64_figures():
    assert set(CT.FLOORS) == set(CT.MEASURED_FLOAT64) == {"conv.lp.d_coef", "conv.lp.d_inscale", "conv.elbo.d_coef",
                                                          "conv.elbo.d_inscale", "conv.elbo.inputs"}
    for fam, vals in CT.MEASURED_FLOAT64.items():
        assert len(vals) == len(CT.LP_CASES if ".lp." in fam else CT.ELBO_CASES)
        assert CT.FLOORS[fam] == float(np.median(vals)), fam


# ---- 3. the host functions over the double, against central differences ------------------------------------------------------
TH0 = dict(v=0.002, l=2.2, a=0.7, s2=0.15)      # var(f) = v * 36^2 * O(0.3): O(1), next to the noise


def hyper_model(**th):
    """g = GP(v SE(l)), f = patch_convolve(stretch(g, a)), fh = f + h"""
    th = dict(TH0, **th)

    def build(GP):
        g = GP(th["v"] * P.with_lengthscale(P.SEKernel(), th["l"]))
        h = GP(0.5 * P.Matern32Kernel())
        f = P.patch_convolve(P.stretch(g, th["a"]))
        return {"g": g, "h": h, "f": f, "fh": f + h}
    return P.gppp(build)


def np_logpdf(K, y):
    Lc = np.linalg.cholesky(K)
    a = np.linalg.solve(Lc, y)
    return -0.5 * a @ a - np.sum(np.log(np.diag(Lc))) - 0.5 * len(y) * np.log(2 * np.pi)


def np_lp(x, y, **th):
    th = dict(TH0, **th)
    return np_logpdf(np_spec_matrix(P.build_spec(hyper_model(**th), x)[0]) + th["s2"] * np.eye(len(y)), y)


def np_bound(x, z, y, **th):
    """the Titsias bound from np_spec_matrix: logpdf under Q + s2 I minus the trace term"""
    th = dict(TH0, **th)
    F = hyper_model(**th)
    Kzz = np_spec_matrix(P.build_spec(F, z)[0]) + 1e-3 * np.eye(len(z))
    Kxz = np_spec_matrix(P.build_spec(F, x, None, z)[0])
    var = np.diag(np_spec_matrix(P.build_spec(F, x)[0]))
    A = np.linalg.solve(np.linalg.cholesky(Kzz), Kxz.T)
    Q = A.T @ A
    return np_logpdf(Q + th["s2"] * np.eye(len(y)), y) - 0.5 * (np.sum(var) - np.trace(Q)) / th["s2"]


def _d_theta(records, kind):
    """(d / dv, d / dl, d / da) from the records of the terms of g's kernel: coef = v (x 1), the images are read as
    (a / l) x and the plain points as z / l, so d / dl = -sum d_inscale / l; d / da needs both sides under the stretch"""
    rec = [r for r in records if r["kind"] == kind]
    dv = sum(r["d_coef"] * r["coef"] for r in rec) / TH0["v"]
    dl = -sum(r["d_inscale"] for r in rec) / TH0["l"]
    da = sum(r["d_inscale"] for r in rec if r.get("row_geom") and r.get("col_geom")) / TH0["a"]
    return dv, dl, da


H = 1e-5


def _fd(f, name):
    """the central difference in log(theta) -- the parameters are positive and of very different sizes -- as d / d theta"""
    return (f(**{name: TH0[name] * np.exp(H)}) - f(**{name: TH0[name] * np.exp(-H)})) / (2 * H) / TH0[name]


def _off(a, fd, name=None):
    """|a - fd| in units of max(1, |fd|), for a difference taken in log(theta) (name given) or in a coordinate of O(1)"""
    th = TH0[name] if name else 1.0
    return abs(a - fd) * th / max(1.0, abs(fd) * th)


def _fd_model(value):
    """what such a central difference can be off by: the rounding of the two values, eps |f| / H, and the third-derivative
    term H^2 |f| (smooth functions of the logarithms of their parameters and of O(1) coordinates)"""
    return 2.0 ** -52 * abs(value) / H + H * H * abs(value)


def test_host_functions_match_central_differences_of_numpy(monkeypatch):
    conv_grad_np.install(monkeypatch)
    rng = np.random.default_rng(4)
    x = P.GPPPInput("fh", images(9, seed=3))
    y = rng.standard_normal(9)
    g = P.logpdf_and_gradient_conv(hyper_model()(x, TH0["s2"]), y)
    assert g["_spec"].has_patch and abs(g["logpdf"] - np_lp(x, y)) <= 1e-12 * abs(g["logpdf"])
    assert len(g["terms"]) == 2 and sorted(bool(r["row_geom"]) for r in g["terms"]) == [False, True]
    got = _d_theta(g["terms"], P.lib.SE) + (g["noise"],)
    need = 0.0
    for name, a in zip(("v", "l", "a", "s2"), got):
        fd = _fd(lambda **th: np_lp(x, y, **th), name)
        need = max(need, _off(a, fd, name))
    model = _fd_model(g["logpdf"])
    print(f"logpdf: variance, lengthscale, stretch, noise need {need:.2e}; the difference's own error {model:.2e}")
    assert need <= 2 * model
    # the ELBO: f at images, inducing patches in g
    x = P.GPPPInput("f", images(9, seed=3))
    Z = np.asfortranarray(rng.standard_normal((9, 4)))
    z = lambda Zm: P.GPPPInput("g", P.ColVecs(Zm))      # noqa: E731
    F = hyper_model()
    ge = P.elbo_and_gradient_conv(P.VFE(F(z(Z), 1e-3)), F(x, TH0["s2"]), y, inputs=True)
    assert abs(ge["elbo"] - np_bound(x, z(Z), y)) <= 1e-11 * abs(ge["elbo"])
    assert (len(ge["zz_terms"]), len(ge["xz_terms"]), len(ge["xx_terms"])) == (1, 1, 1)
    assert ge["x"] is None and ge["xz_inputs"][0] is None and ge["xz_inputs"][1].shape == (9, 4)
    recs = ge["zz_terms"] + ge["xz_terms"] + ge["xx_terms"]
    dv, dl, _ = _d_theta(recs, P.lib.SE)
    # (the stretch reaches the images alone, and d_inscale of the one-sided term scales z with them: no record is d / da here)
    need = 0.0
    for name, a in (("v", dv), ("l", dl), ("s2", ge["noise"])):
        fd = _fd(lambda **th: np_bound(x, z(Z), y, **th), name)
        need = max(need, _off(a, fd, name))
    for (d, j) in ((0, 0), (8, 3), (4, 1)):
        Zp, Zn = Z.copy(), Z.copy()
        Zp[d, j] += H
        Zn[d, j] -= H
        fd = (np_bound(x, z(Zp), y) - np_bound(x, z(Zn), y)) / (2 * H)
        need = max(need, _off(ge["z"][0][d, j], fd))
    model = _fd_model(ge["elbo"])
    print(f"elbo: variance, lengthscale, noise, inducing coordinates need {need:.2e}; the difference's own error {model:.2e}")
    assert need <= 2 * model


def test_models_without_patch_terms_return_what_the_old_functions_return(monkeypatch):
    conv_grad_np.install(monkeypatch)
    rng = np.random.default_rng(6)
    F = P.gppp(lambda GP: {"f": GP(1.3 * P.with_lengthscale(P.Matern52Kernel(), 0.8)) + GP(0.4 * P.SEKernel())})
    x = P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((3, 11)))))
    z = P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.standard_normal((3, 4)))))
    y = rng.standard_normal(11)
    a, b = P.logpdf_and_gradient(F(x, 0.2), y), P.logpdf_and_gradient_conv(F(x, 0.2), y)
    assert a["logpdf"] == b["logpdf"] and a["terms"] == b["terms"] and a["noise"] == b["noise"]
    assert np.array_equal(a["y"], b["y"]) and np.array_equal(a["mean"], b["mean"])
    a = P.elbo_and_gradient(P.VFE(F(z, 1e-3)), F(x, 0.2), y, inputs=True)
    b = P.elbo_and_gradient_conv(P.VFE(F(z, 1e-3)), F(x, 0.2), y, inputs=True)
    assert a["elbo"] == b["elbo"] and a["noise"] == b["noise"] and a["z_noise"] == b["z_noise"]
    for key in ("zz_terms", "xz_terms", "xx_terms"):
        assert a[key] == b[key]
    assert all(np.array_equal(p, q) for p, q in zip(a["z"], b["z"])) and b["x"] is None
    assert all(np.array_equal(p, q) for key in ("zz_inputs", "xz_inputs") for p, q in zip(a[key], b[key]))


def test_the_old_functions_still_raise_and_name_the_new_ones(monkeypatch):
    conv_grad_np.install(monkeypatch)
    f = conv_model()
    fx = f(P.GPPPInput("f", images(4)), 0.1)
    z = P.GPPPInput("g", P.ColVecs(np.zeros((9, 2))))
    for call in (lambda: P.logpdf_and_gradient(fx, np.zeros(4)), lambda: P.logpdf_and_gradient_batch([fx], [np.zeros(4)]),
                 lambda: P.logpdf_and_gradient_param(fx, np.zeros(4)),
                 lambda: P.elbo_and_gradient(P.VFE(f(z)), fx, np.zeros(4))):
        with pytest.raises(NotImplementedError, match="patch_convolve.*logpdf_and_gradient_conv / elbo_and_gradient_conv"):
            call()


def test_stencil_terms_and_multi_gpu_contexts_are_refused_by_name(monkeypatch):
    ctx = conv_grad_np.install(monkeypatch)
    F = P.gppp(lambda GP: (lambda g: {"g": g, "d": P.stencil(g, [0.0, 0.1], [-1.0, 1.0])})(
        GP(P.SEKernel())))
    x = P.GPPPInput("d", P.ColVecs(np.asfortranarray(np.linspace(0.0, 1.0, 5)[None, :])))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.logpdf_and_gradient_conv(F(x, 0.1), np.zeros(5))
    with pytest.raises(NotImplementedError, match="stencil"):
        P.elbo_and_gradient_conv(P.VFE(F(P.GPPPInput("g", x.x), 1e-3)), F(x, 0.1), np.zeros(5))
    ctx.is_multi = True
    f = conv_model()
    fx = f(P.GPPPInput("f", images(4)), 0.1)
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        P.logpdf_and_gradient_conv(fx, np.zeros(4))
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        P.elbo_and_gradient_conv(P.VFE(f(P.GPPPInput("g", P.ColVecs(np.zeros((9, 2)))))), fx, np.zeros(4))


def test_an_image_gradient_is_refused_by_the_double_as_by_the_library(monkeypatch):
    ctx = conv_grad_np.install(monkeypatch)
    f = conv_model()
    xz = P.build_spec(f, P.GPPPInput("f", images(4)), None, P.GPPPInput("g", P.ColVecs(np.ones((9, 2)))))[0]
    zz = P.build_spec(f, P.GPPPInput("g", P.ColVecs(np.ones((9, 2)))))[0]
    import ctypes as C
    gx = [np.zeros(a.shape, order="F") for a in xz.inputs]
    px = (C.POINTER(C.c_double) * len(gx))(*[P.lib.dptr(a) for a in gx])
    d, v = P.lib.dptr, np.ones(4)
    rc = ctx.lib.sgp_elbo_grad_conv(ctx.handle, zz.ref(), xz.ref(), d(v), d(v), 0, d(v), 0, d(v), d(v), d(np.zeros(1)), None,
                                    None, None, None, None, None, None, None, None, None, px)
    assert rc < 0 and "patch" in ctx.lib.sgp_last_error().decode() and "images" in ctx.lib.sgp_last_error().decode()


# ---- 4. the extension header -------------------------------------------------------------------------------------------------
def test_conv_grad_header_is_plain_c(tmp_path):
    src = tmp_path / "conv_grad_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include "sthenomi_conv_grad.h"
int main(void) {
  int (*a)(sgp_ctx*, const sgp_cov_spec*, const double*, int, const double*, const double*, double*, double*, double*,
           double*, double*, double*) = &sgp_logpdf_grad_conv;
  int (*b)(sgp_ctx*, const sgp_cov_spec*, const double*, double*, double*) = &sgp_kernelmatrix_diag_grad_conv;
  printf("%d %d %d\n", (int)sizeof(a), (int)sizeof(b), (int)sizeof(&sgp_elbo_grad_conv));
  return 0;
}
''')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "conv_grad_consumer.o")])


def test_conv_grad_library_exports_exactly_its_header():
    syms = _symbols_of("sthenomi_conv_grad.h")
    assert syms == ["sgp_elbo_grad_conv", "sgp_kernelmatrix_diag_grad_conv", "sgp_logpdf_grad_conv"] == P.lib.conv_grad_symbols()
    assert _c_exports(P.lib.CONV_GRAD_LIB_PATH) == syms
    others = [P.lib.LIB_PATH, P.lib.CONV_LIB_PATH, P.lib.STENCIL_LIB_PATH, P.lib.KPROD_LIB_PATH, P.lib.KPROD_GRAD_LIB_PATH,
              P.lib.BATCH_LIB_PATH, P.lib.POOL_LIB_PATH, P.lib.EXTEND_LIB_PATH, P.lib.POSTFX_LIB_PATH,
              P.lib.VFE_UPDATE_LIB_PATH, P.lib.BENCH_LIB_PATH]
    for path in others:
        assert not set(syms) & set(_c_exports(path)), path
    assert _c_exports(P.lib.CONV_LIB_PATH) == ["sgp_conv_geom"]
    for header in ("sthenomi.h", "sthenomi_conv.h", "sthenomi_kprod_grad.h"):
        assert not set(syms) & set(_symbols_of(header))


if __name__ == "__main__":          # the measurement behind conv_grad_truth.FLOORS / MEASURED_FLOAT64
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
    for c in CT.CASES:
        mp, t0 = _MP(), time.time()
        figs = _figures(c, mp)
        mp.close()
        for fam, e in figs.items():
            if fam.startswith("conv."):
                lists.setdefault(fam, []).append(round(e, 1))
            print(f"{c.id:20s} {fam:20s} {e:10.1f}", flush=True)
        print(f"{c.id:20s} truth and yardstick: {time.time() - t0:.1f} s", flush=True)
    lists = {k: sorted(v) for k, v in lists.items()}
    print("MEASURED_FLOAT64 = ", end="")
    pprint.pprint(lists, width=120, compact=True)
    print("FLOORS = ", end="")
    pprint.pprint({k: float(np.median(v)) for k, v in lists.items()}, width=120)
