"""Product chains (include/sthenomi_kprod.h; csrc/kprod.hip): timing of the chain assembly and of the gradient through it.
Model: the scikit-learn golden's kernel (tests/golden/make_kprod_golden.py),
    4 SE o (1/1.5) * PeriodicKernel(0.6) o (1/0.9) + 0.7 RQ(1.3) o (1/0.8) + 0.1 PolynomialKernel(2, 0.25)
-- three chains, five leaf evaluations per entry -- on N = 16 384 points of a 1-D input:
  (chain) sgp_kernelmatrix of the model (wall, host copy of the N x N result included) and the assembly alone (device
          events around the assembly of the lower tiles inside sgp_dev_logpdf);
  (a)     the same two figures for a KernelSum of five plain terms (SE, SE over the periodic embedding, Matern-5/2, -3/2,
          -1/2): the plain assembly at the same number of leaf evaluations, the floor;
  (b)     what a user can do without chains: one sgp_kernelmatrix per factor (five calls of a one-term model; Matern-5/2 and a
          constant stand in for the two kinds the plain path does not have), multiplied and added on the host.
And logpdf + gradient over logpdf at N = 4096 for the model (sgp_logpdf_grad_param) against the same ratio for a four-term
KernelSum (sgp_logpdf_grad), same run.  Medians of repeats after a warm-up.
--matern-nu: instead, the general-nu Matern kind (SGP_MATERN_NU: a Bessel function per entry) -- the assembly of
GeneralMaternKernel(1.25) and GeneralMaternKernel(25) at N = 4096 and 16 384, D = 8, against plain Matern-5/2 and
GammaExponential(1.3) in the same process, and the assembly's share of logpdf at both sizes.
usage: python tools/gpu_kprod_time.py [--out FILE] [--quick] [--matern-nu]      -> JSON on stdout (and in FILE)"""
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
MATERN_NU = "--matern-nu" in argv
N_K, N_G = (2048, 1024) if QUICK else (16384, 4096)


def med(f, reps=5, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def atom(k):
    return P.atomic(P.GP(k), P.GPC())


def golden_kernel():
    return (4.0 * P.with_lengthscale(P.SEKernel(), 1.5) * (P.PeriodicKernel(0.6) @ P.ScaleTransform(1.0 / 0.9)) +
            0.7 * P.with_lengthscale(P.RationalQuadraticKernel(1.3), 0.8) + 0.1 * P.PolynomialKernel(2, 0.25))


def sum_kernel(n):
    ks = [4.0 * P.with_lengthscale(P.SEKernel(), 1.5), P.PeriodicKernel(0.6) @ P.ScaleTransform(1.0 / 0.9),
          0.7 * P.with_lengthscale(P.Matern52Kernel(), 0.8), 0.1 * P.Matern32Kernel(), 0.1 * P.Matern12Kernel()][:n]
    return P.KernelSum(ks)


def assemble_ms(ctx, spec, reps=5):
    """median device time of the assembly of K + 0.1 I (lower tiles) inside sgp_dev_logpdf"""
    import torch
    lib = ctx.lib
    N = spec.N
    ds = C.c_void_p()
    L.check(lib.sgp_dspec_create(ctx.handle, spec.ref(ctx), C.byref(ds)), "sgp_dspec_create")
    npad, mtot = C.c_int64(), C.c_int64()
    lib.sgp_geometry(N, 1, C.byref(npad), C.byref(mtot))
    A = torch.empty(npad.value * mtot.value, dtype=torch.float64, device="cuda")
    dY = torch.zeros(N, dtype=torch.float64, device="cuda")
    out, nz, tm = np.zeros(1), np.array([0.1]), np.zeros(8)
    got = []
    for r in range(reps + 1):
        L.check(lib.sgp_dev_logpdf(ctx.handle, ds, A.data_ptr(), None, L.NOISE_SCALAR, L.dptr(nz), None, dY.data_ptr(), N, 1,
                                   L.dptr(out), L.dptr(tm)), "sgp_dev_logpdf")
        if r:
            got.append(float(tm[0]))
    lib.sgp_dspec_destroy(ds)
    del A
    return float(np.median(got))


def finish(res):
    res["build"] = dict(libsthenomi_sha16=hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16],
                        kprod_hip_sha16=hashlib.sha256(open(os.path.join(ROOT, "stheno.jl_amd", "csrc", "kprod.hip"), "rb").read()).hexdigest()[:16])
    out = json.dumps(res, indent=1)
    print(out)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(out + "\n")


def main_matern_nu():
    """one term each, lengthscale 1 on points of unit variance per coordinate / sqrt(D): x = sqrt(2 nu) d spreads over both
    branches of the routine (Temme's series up to x = 2, the continued fraction beyond)"""
    ctx = L.default_context()
    rng = np.random.default_rng(0)
    kernels = (("GeneralMaternKernel(1.25)", P.GeneralMaternKernel(1.25)), ("GeneralMaternKernel(25)", P.GeneralMaternKernel(25.0)),
               ("Matern52Kernel (plain assembly)", P.Matern52Kernel()), ("GammaExponentialKernel(1.3)", P.GammaExponentialKernel(1.3)))
    res = dict(shape=dict(N=[1024, 2048] if QUICK else [4096, 16384], D=8), runs={})
    for N in res["shape"]["N"]:
        X = P.ColVecs(np.asfortranarray(rng.standard_normal((8, N)) / np.sqrt(8.0)))
        y = rng.standard_normal(N)
        for label, k in kernels:
            spec = P.build_spec(atom(k), X)[0]
            fx = atom(k)(X, 0.1)
            a_ms, lp_s = assemble_ms(ctx, spec), med(lambda: P.logpdf(fx, y), reps=3)
            res["runs"][f"{label}, N = {N}"] = dict(assemble_ms=a_ms, logpdf_s=lp_s, assembly_share_of_logpdf=a_ms / (1e3 * lp_s))
        for nu in ("1.25", "25"):
            a = res["runs"][f"GeneralMaternKernel({nu}), N = {N}"]["assemble_ms"]
            res[f"assembly ratio nu = {nu} / Matern52, N = {N}"] = a / res["runs"][f"Matern52Kernel (plain assembly), N = {N}"]["assemble_ms"]
            res[f"assembly ratio nu = {nu} / GammaExponential, N = {N}"] = a / res["runs"][f"GammaExponentialKernel(1.3), N = {N}"]["assemble_ms"]
    finish(res)


def main():
    if MATERN_NU:
        return main_matern_nu()
    ctx = L.default_context()
    rng = np.random.default_rng(0)
    x = np.sort(rng.uniform(-3.0, 3.0, N_K))
    res = dict(shape=dict(N_kernelmatrix=N_K, N_gradient=N_G, D=1, leaf_evaluations_per_entry=5, chains=3), runs={})
    K = np.zeros((N_K, N_K), order="F")

    def kernelmatrix(spec, into):
        return lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, spec.ref(ctx), L.dptr(into), spec.N), "sgp_kernelmatrix")

    chain = P.build_spec(atom(golden_kernel()), x)[0]
    plain = P.build_spec(atom(sum_kernel(5)), x)[0]
    assert chain.has_kprod and chain.n_terms == 5 and not plain.has_kprod and plain.n_terms == 5
    res["runs"]["(chain) sgp_kernelmatrix, product chains"] = dict(s=med(kernelmatrix(chain, K), reps=3),
                                                                 assemble_ms=assemble_ms(ctx, chain))
    res["runs"]["(a) sgp_kernelmatrix, KernelSum of five plain terms"] = dict(s=med(kernelmatrix(plain, K), reps=3),
                                                                            assemble_ms=assemble_ms(ctx, plain))
    factors = [P.build_spec(atom(k), x)[0] for k in
               (P.with_lengthscale(P.SEKernel(), 1.5), P.PeriodicKernel(0.6) @ P.ScaleTransform(1.0 / 0.9),
                P.with_lengthscale(P.Matern52Kernel(), 0.8), P.ConstantKernel(0.25), P.ConstantKernel(0.25))]
    Ks = [np.zeros((N_K, N_K), order="F") for _ in factors]

    def composed(K=K):
        for sp, Kf in zip(factors, Ks):
            kernelmatrix(sp, Kf)()
        np.multiply(Ks[0], Ks[1], out=K)
        K *= 4.0
        np.multiply(Ks[3], Ks[4], out=Ks[3])
        K += 0.7 * Ks[2]
        K += 0.1 * Ks[3]
    res["runs"]["(b) one sgp_kernelmatrix per factor, multiplied on the host"] = dict(s=med(composed, reps=3))
    del Ks
    r = res["runs"]
    res["ratio chain / (a), wall"] = r["(chain) sgp_kernelmatrix, product chains"]["s"] / r["(a) sgp_kernelmatrix, KernelSum of five plain terms"]["s"]
    res["ratio chain / (a), assembly"] = (r["(chain) sgp_kernelmatrix, product chains"]["assemble_ms"] /
                                          r["(a) sgp_kernelmatrix, KernelSum of five plain terms"]["assemble_ms"])
    res["ratio (b) / chain, wall"] = r["(b) one sgp_kernelmatrix per factor, multiplied on the host"]["s"] / r["(chain) sgp_kernelmatrix, product chains"]["s"]
    # gradient
    xg = np.sort(rng.uniform(-3.0, 3.0, N_G))
    yg = np.sin(2.0 * xg) + 0.3 * rng.standard_normal(N_G)
    for label, k in (("product model", golden_kernel()), ("four-term KernelSum", sum_kernel(4))):
        fx = atom(k)(xg, 0.1)
        t_lp = med(lambda: P.logpdf(fx, yg), reps=5)
        t_g = med(lambda: P.logpdf_and_gradient(fx, yg), reps=5)
        res["runs"][f"logpdf + gradient / logpdf, {label}, N = {N_G}"] = dict(logpdf_s=t_lp, logpdf_and_gradient_s=t_g, ratio=t_g / t_lp)
    finish(res)


if __name__ == "__main__":
    main()
