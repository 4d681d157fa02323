"""Stencil GPs (stencil, quadrature_convolve; include/sthenomi_stencil.h): timing of the stencil-term assembly.
  (a) the full cov(g, x) of g = quadrature_convolve(f, 15), f ~ GP(Matern-5/2, lengthscale 0.5), 1-D, N = 8192
      (symmetric: the lower triangle's 128 x 128 tiles, mirrored; 225 kernel evaluations per entry);
  (b) the same matrix through the composed sum of 15 `shift` views of f (what a user could write without stencils: 225
      plain terms per block pair through the existing assembly);
  (c) var(g, x) at N = 65 536;
  (d) the full cov(g, x) of a central-difference stencil of 2D + 1 points (the discrete Laplacian) in D = 8, SE, N = 4096.
Kernel evaluations per second for each, the (b) / (a) ratio, and the fp64 VALU instructions per evaluation of the stencil
kernel's inner loop read from the device assembly of csrc/stencil.hip (hipcc -S, 1-D Matern-5/2 instantiation).  Timed
around the calls with prebuilt specs, median of repeats after a warm-up.
usage: python tools/gpu_stencil_time.py [--out FILE] [--quick]      -> JSON on stdout (and in FILE)"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
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
N_A, N_C, N_D = (1024, 8192, 512) if QUICK else (8192, 65536, 4096)


def med(f, reps=5, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def lower_entries(n):
    """entries of the lower triangle's 128 x 128 tiles (what a symmetric assembly computes before mirroring)"""
    tiles = -(-n // 128)
    full = [min(128, n - 128 * k) for k in range(tiles)]
    return sum(full[i] * full[j] for i in range(tiles) for j in range(i + 1))


def kernelmatrix(ctx, spec, K):
    return lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, spec.ref(ctx), L.dptr(K), spec.N), "sgp_kernelmatrix")


def inner_loop(asm, symbol):
    """the innermost loop of `symbol` that reads LDS and evaluates the kernel: instructions per kernel evaluation"""
    lines = asm.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    labels = {ln.split(":")[0]: i for i, ln in enumerate(body) if re.match(r"^\.LBB\w+:", ln)}
    best = None
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_(?:cbranch_\w+|branch)\s+(\.LBB\w+)", ln)
        if not (m and m.group(1) in labels and labels[m.group(1)] < i):
            continue
        ops = [s.split()[0] for s in body[labels[m.group(1)]:i + 1]
               if s.strip() and not s.strip().startswith((";", ".")) and not s.strip().endswith(":")]
        nexp = ops.count("v_ldexp_f64")          # one per kernel evaluation (exp_nonpos)
        if nexp and any(o.startswith("ds_read") for o in ops) and (best is None or len(ops) < len(best[0])):
            best = (ops, nexp)
    ops, nexp = best
    return dict(evaluations_per_iteration=nexp,
                valu_f64_per_eval=sum(1 for o in ops if o.startswith("v_") and "f64" in o) / nexp,
                valu_per_eval=sum(1 for o in ops if o.startswith("v_")) / nexp,
                lds_reads_per_eval=sum(1 for o in ops if o.startswith("ds_read")) / nexp)


def isa_figures():
    src = os.path.join(ROOT, "stheno.jl_amd", "csrc", "stencil.hip")
    with tempfile.TemporaryDirectory() as td:
        s = os.path.join(td, "stencil.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                               "--cuda-device-only", "-S", "-o", s, src], stderr=subprocess.DEVNULL)
        asm = open(s).read()
    return {"stencil_kernel, D = 1, Matern-5/2 (4 entries per thread)":
            inner_loop(asm, "_ZN3sgp14stencil_kernelILi1ELi3EEEvPdlllllllPKNS_7DevTermEiiidPKd"),
            "stencil_kernel, D = 8, SE (2 entries per thread)":
            inner_loop(asm, "_ZN3sgp14stencil_kernelILi8ELi0EEEvPdlllllllPKNS_7DevTermEiiidPKd")}


def main():
    ctx = L.default_context()
    rng = np.random.default_rng(0)
    t_nodes, w_nodes = np.polynomial.hermite.hermgauss(15)

    def build(GP):
        f = GP(P.with_lengthscale(P.Matern52Kernel(), 0.5))
        fs = w_nodes[0] * P.shift(f, t_nodes[0])
        for q in range(1, 15):
            fs = fs + w_nodes[q] * P.shift(f, t_nodes[q])
        return {"f": f, "g": P.quadrature_convolve(f, 15), "fs": fs}
    F = P.gppp(build)
    res = dict(shape=dict(N_a=N_A, N_c=N_C, N_d=N_D, Q_quadrature=15, D_laplacian=8, Q_laplacian=17), runs={})
    # (a) / (b)
    x = rng.uniform(-5.0, 5.0, N_A)
    sg = P.build_spec(F, P.GPPPInput("g", x))[0]
    ss = P.build_spec(F, P.GPPPInput("fs", x))[0]
    Kg, Ks = np.zeros((N_A, N_A), order="F"), np.zeros((N_A, N_A), order="F")
    ta = med(kernelmatrix(ctx, sg, Kg), reps=3)
    tb = med(kernelmatrix(ctx, ss, Ks), reps=3)
    ev = float(lower_entries(N_A)) * 225
    res["runs"]["(a) cov(g, x) quadrature_convolve(f, 15), stencil terms"] = dict(
        s=ta, evaluations_computed=ev, evals_per_s=ev / ta, terms=sg.n_terms,
        note="symmetric: the lower triangle's 128 x 128 tiles are computed, then mirrored; includes the host copy of the "
             "N x N result")
    res["runs"]["(b) the same matrix as the composed sum of 15 shift views"] = dict(
        s=tb, evaluations_computed=ev, evals_per_s=ev / tb, terms=ss.n_terms)
    res["ratio (b) / (a)"] = tb / ta
    res["max_rel_diff (a) vs (b)"] = float(np.max(np.abs(Kg - Ks)) / np.max(np.abs(Ks)))
    del Kg, Ks
    # (c)
    xc = rng.uniform(-5.0, 5.0, N_C)
    sc = P.build_spec(F, P.GPPPInput("g", xc))[0]
    out = np.zeros(N_C)
    tc = med(lambda: L.check(ctx.lib.sgp_kernelmatrix_diag(ctx.handle, sc.ref(ctx), L.dptr(out)), "diag"), reps=5)
    ev = float(N_C) * 225
    res["runs"]["(c) var(g, x)"] = dict(s=tc, evaluations=ev, evals_per_s=ev / tc)
    # (d)
    D, h = 8, 1e-2
    A = np.zeros((D, 2 * D + 1))
    wl = np.zeros(2 * D + 1)
    wl[0] = -2.0 * D / h ** 2
    for d in range(D):
        A[d, 1 + 2 * d], A[d, 2 + 2 * d] = h, -h
        wl[1 + 2 * d] = wl[2 + 2 * d] = 1.0 / h ** 2

    def build_d(GP):
        f = GP(P.with_lengthscale(P.SEKernel(), 2.0))
        return {"f": f, "g": P.stencil(f, A, wl)}
    Fd = P.gppp(build_d)
    xd = P.ColVecs(rng.standard_normal((D, N_D)))
    sd = P.build_spec(Fd, P.GPPPInput("g", xd))[0]
    Kd = np.zeros((N_D, N_D), order="F")
    td = med(kernelmatrix(ctx, sd, Kd), reps=3)
    ev = float(lower_entries(N_D)) * (2 * D + 1) ** 2
    res["runs"]["(d) cov(g, x) central-difference stencil, D = 8, Q = 17"] = dict(
        s=td, evaluations_computed=ev, evals_per_s=ev / td)
    res["isa"] = isa_figures()
    res["build"] = dict(libsthenomi_sha16=hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16],
                        stencil_hip_sha16=hashlib.sha256(open(os.path.join(ROOT, "stheno.jl_amd", "csrc", "stencil.hip"), "rb").read()).hexdigest()[:16])
    out = json.dumps(res, indent=1)
    print(out)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
