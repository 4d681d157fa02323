"""Convolutional GPs (patch_convolve, include/sthenomi_conv.h): timing of the patch-term assembly.
  (a) cov(f, x, z) and var(f, x) at the reference example's shape scaled up: N = 8192 images of 28 x 28, 3 x 3 patches
      (P = 676), M = 512 pseudo-points in g;
  (b) the whole elbo(VFE(f(z)), f(x, 0.1), y) at that shape (host side included: specs, means, the call);
  (c) the full cov(f, x) at N = 1024 (symmetric: the lower triangle's tiles, mirrored);
  (d) the same 8 x 8 / P = 36 matrix through patch_convolve and through the composed sum of 36 `select` views of g (what a
      user could write without patch terms: 1296 plain terms per block pair).
Kernel evaluations per second for each, and the fp64 VALU instructions per evaluation of the two inner loops read from the
device assembly of csrc/conv.hip (hipcc -S, the instantiations of 3 x 3 patches and the SE kernel).  Timed around the
calls with prebuilt specs, median of repeats after a warm-up.
usage: python tools/gpu_conv_time.py [--out FILE] [--quick]      -> JSON on stdout (and in FILE)"""
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
N_BIG, M_BIG, N_FULL = (1024, 128, 256) if QUICK else (8192, 512, 1024)


def med(f, reps=5, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def model():
    def build(GP):
        g = GP(1.0 * P.with_lengthscale(P.SEKernel(), 1.0))
        return {"g": g, "f": P.patch_convolve(g)}
    return P.gppp(build)


def kernelmatrix(ctx, spec):
    K = np.zeros((spec.N, spec.M), order="F")
    return lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, spec.ref(ctx), L.dptr(K), spec.N), "sgp_kernelmatrix")


def diag(ctx, spec):
    out = np.zeros(spec.N)
    return lambda: L.check(ctx.lib.sgp_kernelmatrix_diag(ctx.handle, spec.ref(ctx), L.dptr(out)), "sgp_kernelmatrix_diag")


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
    src = os.path.join(ROOT, "stheno.jl_amd", "csrc", "conv.hip")
    with tempfile.TemporaryDirectory() as td:
        s = os.path.join(td, "conv.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                               "--cuda-device-only", "-S", "-o", s, src], stderr=subprocess.DEVNULL)
        asm = open(s).read()
    return {"conv2 (both sides patched), 3x3, SE": inner_loop(asm, "_ZN3sgp12conv2_kernelILi9ELb1ELi0EEEvPdlllllllPKNS_7DevTermEiiidPKd"),
            "conv1 (one side patched), 3x3, SE": inner_loop(asm, "_ZN3sgp12conv1_kernelILi9ELb1ELi0EEEvPdlllllllPKNS_7DevTermEiiidPKd")}


def main():
    ctx = L.default_context()
    rng = np.random.default_rng(0)
    f = model()
    Pn = 26 * 26
    res = dict(shape=dict(N=N_BIG, M=M_BIG, image=[28, 28], patch=[3, 3], P=Pn, N_full=N_FULL), runs={})
    x = P.GPPPInput("f", P.ImageVector(rng.uniform(0.0, 1.0, (28, 28, N_BIG))))
    z = P.GPPPInput("g", P.ColVecs(rng.standard_normal((9, M_BIG))))
    sxz = P.build_spec(f, x, None, z)[0]
    sxx = P.build_spec(f, x)[0]
    t = med(kernelmatrix(ctx, sxz), reps=3)
    ev = float(N_BIG) * M_BIG * Pn
    res["runs"]["cov(f, x, z)"] = dict(s=t, evaluations=ev, evals_per_s=ev / t)
    t = med(diag(ctx, sxx), reps=3)
    ev = float(N_BIG) * Pn * Pn
    res["runs"]["var(f, x)"] = dict(s=t, evaluations=ev, evals_per_s=ev / t)
    y = rng.standard_normal(N_BIG)
    vfe, fx = P.VFE(f(z)), f(x, 0.1)
    val = [None]

    def run_elbo():
        val[0] = P.elbo(vfe, fx, y)
    t = med(run_elbo, reps=3)
    ev = float(N_BIG) * M_BIG * Pn + float(N_BIG) * Pn * Pn + float(M_BIG) * M_BIG
    res["runs"]["elbo"] = dict(s=t, evaluations=ev, evals_per_s=ev / t, value=val[0])
    xf = P.GPPPInput("f", P.ImageVector(rng.uniform(0.0, 1.0, (28, 28, N_FULL))))
    sff = P.build_spec(f, xf)[0]
    t = med(kernelmatrix(ctx, sff), reps=3)
    tiles = -(-N_FULL // 128)
    live = min(N_FULL, 128) ** 2 * tiles * (tiles + 1) // 2 if N_FULL > 128 else N_FULL ** 2   # entries of the lower tiles
    ev = float(live) * Pn * Pn
    res["runs"]["cov(f, x) full"] = dict(s=t, evaluations_computed=ev, evals_per_s=ev / t,
                                         note="symmetric: the lower triangle's 128 x 128 tiles are computed, then mirrored")
    # (d) patch terms vs the composed sum of selects, 8 x 8 images, P = 36
    H = 8
    idx = [[(pr + a) + (pc + b) * H for b in range(3) for a in range(3)] for pc in range(H - 2) for pr in range(H - 2)]

    def build(GP):
        g = GP(1.0 * P.with_lengthscale(P.SEKernel(), 1.0))
        fs = P.select(g, idx[0])
        for ix in idx[1:]:
            fs = fs + P.select(g, ix)
        return {"g": g, "f": P.patch_convolve(g), "fs": fs}
    f8 = P.gppp(build)
    n8 = 512
    im = P.ImageVector(rng.uniform(0.0, 1.0, (8, 8, n8)))
    sc = P.build_spec(f8, P.GPPPInput("f", im))[0]
    ss = P.build_spec(f8, P.GPPPInput("fs", P.ColVecs(im.X)))[0]
    Kc, Ks = np.zeros((n8, n8), order="F"), np.zeros((n8, n8), order="F")
    tc = med(lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, sc.ref(ctx), L.dptr(Kc), n8), "conv"), reps=3)
    ts = med(lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, ss.ref(ctx), L.dptr(Ks), n8), "selects"), reps=3)
    res["runs"]["8x8 P=36 N=512: patch terms vs 36 selects"] = dict(
        patch_s=tc, selects_s=ts, speedup=ts / tc, selects_terms=ss.n_terms, patch_terms=sc.n_terms,
        max_rel_diff=float(np.max(np.abs(Kc - Ks)) / np.max(np.abs(Ks))))
    res["isa"] = isa_figures()
    res["build"] = dict(libsthenomi_sha16=hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16],
                        conv_hip_sha16=hashlib.sha256(open(os.path.join(ROOT, "stheno.jl_amd", "csrc", "conv.hip"), "rb").read()).hexdigest()[:16],
                        parent_commit=os.environ.get("SGP_PARENT_COMMIT", ""))
    out = json.dumps(res, indent=1)
    print(out)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
