"""Input-point gradients through product chains (include/sthenomi_kprod_grad.h; csrc/kprod.hip: grad_kprod_inputs_kernel):
what the input pass costs beside the same call's term contraction.  One box, one process, medians after a warm-up.
  logpdf: sgp_logpdf_grad_param_xs at N = 4096 and 16 384, D = 3, for the golden model (chains of 2) and a chain of 8, called
          with (none) no term or input output, (terms) grad_coef / _inscale / _param, (inputs) grad_inputs, (both): the
          factorisation and C^-1 are in every call, so terms - none is the term contraction and inputs - none the input pass;
  ELBO:   elbo_and_gradient_param (inputs on / off) of the golden model at (N, M) = (65 536, 1024) against
          elbo_and_gradient (sgp_elbo_grad_xs) of a KernelSum with as many terms, inputs on / off.
usage: python tools/gpu_kprod_grad_time.py [--out FILE] [--quick]      -> JSON on stdout (and in FILE)"""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

P = entry.load_package()
L = P.lib
argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
QUICK = "--quick" in argv
NS, NE, ME = ((512, 1024), 4096, 256) if QUICK else ((4096, 16384), 65536, 1024)
D = 3
PD = C.POINTER(C.c_double)


def med(f, reps=5, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def model(k):
    return P.gppp(lambda GP: {"f": GP(k)})


def golden_kernel():
    return (4.0 * P.with_lengthscale(P.SEKernel(), 1.5) * (P.PeriodicKernel(0.6) @ P.ScaleTransform(1.0 / 0.9)) +
            0.7 * P.with_lengthscale(P.RationalQuadraticKernel(1.3), 0.8) + 0.1 * P.PolynomialKernel(2, 0.25))


def chain_of_8():
    wl = P.with_lengthscale
    return 0.8 * (wl(P.SEKernel(), 2.0) * wl(P.Matern12Kernel(), 3.0) * wl(P.Matern32Kernel(), 2.5) * P.Matern52Kernel() *
                  P.RationalQuadraticKernel(1.3) * P.LinearKernel(1.0) * P.ConstantKernel(1.1) * wl(P.SEKernel(), 4.0))


def sum_kernel():
    return P.KernelSum([4.0 * P.with_lengthscale(P.SEKernel(), 1.5), P.PeriodicKernel(0.6) @ P.ScaleTransform(1.0 / 0.9),
                        0.7 * P.with_lengthscale(P.Matern52Kernel(), 0.8), 0.1 * P.Matern32Kernel(), 0.1 * P.Matern12Kernel()])


def points(rng, n):
    return P.GPPPInput("f", P.ColVecs(np.asfortranarray(rng.uniform(-3.0, 3.0, (D, n)))))


def logpdf_variants(ctx, spec, y):
    d, n, nt = L.dptr, spec.N, max(1, spec.n_terms)
    m, nz, lp, gy = np.zeros(n), np.array([0.1]), np.zeros(1), np.zeros(n)
    gc, gs, gp = np.zeros(nt), np.zeros(nt), np.zeros(nt)
    gx = [np.zeros(a.shape, order="F") for a in spec.inputs]
    px = (PD * len(gx))(*[d(a) for a in gx])
    fn = L.kprod_grad_lib().sgp_logpdf_grad_param_xs

    def call(terms, inputs):
        t = (d(gc), d(gs), d(gp)) if terms else (None, None, None)
        return lambda: L.check(fn(ctx.handle, spec.ref(ctx), d(m), L.NOISE_SCALAR, d(nz), d(y), d(lp), d(gy), None, None, *t,
                                  px if inputs else None, None), "sgp_logpdf_grad_param_xs")
    r = {k: med(call(*v), reps=5) for k, v in dict(none=(0, 0), terms=(1, 0), inputs=(0, 1), both=(1, 1)).items()}
    r["term_contraction_s"] = r["terms"] - r["none"]
    r["input_pass_s"] = r["inputs"] - r["none"]
    r["input_pass / term_contraction"] = r["input_pass_s"] / r["term_contraction_s"]
    return r


def main():
    ctx = L.default_context()
    rng = np.random.default_rng(0)
    res = dict(shape=dict(D=D, N_logpdf=list(NS), N_elbo=NE, M_elbo=ME), logpdf={}, elbo={})
    for n in NS:
        x = points(rng, n)
        y = rng.standard_normal(n)
        for label, k in (("golden model (chains of 2)", golden_kernel()), ("chain of 8", chain_of_8())):
            spec = P.build_spec(model(k), x)[0]
            assert spec.has_kprod
            res["logpdf"][f"{label}, N = {n}"] = logpdf_variants(ctx, spec, y)
    x, z = points(rng, NE), points(rng, ME)
    y = rng.standard_normal(NE)
    for label, k, fn in (("product chains, elbo_and_gradient_param", golden_kernel(), P.elbo_and_gradient_param),
                         ("five-term KernelSum, elbo_and_gradient (sgp_elbo_grad_xs)", sum_kernel(), P.elbo_and_gradient)):
        F = model(k)
        vfe, fx = P.VFE(F(z, 1e-3)), F(x, 0.1)
        off = med(lambda: fn(vfe, fx, y), reps=3)
        on = med(lambda: fn(vfe, fx, y, inputs=True), reps=3)
        res["elbo"][label] = dict(without_inputs_s=off, with_inputs_s=on, input_passes_s=on - off)
    res["build"] = dict(libsthenomi_sha16=hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16],
                        kprod_hip_sha16=hashlib.sha256(open(os.path.join(ROOT, "stheno.jl_amd", "csrc", "kprod.hip"), "rb").read()).hexdigest()[:16])
    out = json.dumps(res, indent=1)
    print(out)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
