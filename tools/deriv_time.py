"""What derivative(f) costs (include/sthenomi.h: SGP_DERIV_*; csrc/deriv.hip), beside the stencil central-difference
composition of the same models (stencil(f, [-h, h] e_d, [1/2h, -1/2h]), docs/03 section 3.2d) and the two yardstick models of
tools/wienerpp_time.py.  Method as there: one box, one process, medians of 7 calls after a warm-up, with min and max; wall
time around host calls that end in a copy back to the host.  N = 4096 rows in all, noise 0.1, points standard normal.
  models:      (f, d0 f) at D in {1, 8} (2048 points each), (f, d0 f, d1 f, d2 f) at D = 3 (1024 points each), f ~ GP(SE);
               each as derivative(f, d) and as the stencil composition with h = 1e-2
  per model:   cov (sgp_kernelmatrix into a kept host buffer), logpdf, logpdf_and_gradient (the stencil composition:
               logpdf_and_gradient_stencil)
  yardsticks:  LinearKernel, SEKernel * Matern32Kernel at D in {1, 8}: cov, logpdf, logpdf_and_gradient
usage: python tools/deriv_time.py [--out FILE] [--quick] [--yardsticks] [--root DIR] [--merge FILE]
  --yardsticks   the yardstick models only
  --root DIR     time the package of another checkout (its stheno.jl_amd/ with built libraries), e.g. a build of the parent
                 commit: the criterion is that this build's yardstick medians lie inside that build's min - max
  --merge FILE   put FILE (the JSON of such a run) under "parent" in the output and record the criterion's outcome
-> JSON on stdout (and in FILE)"""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]


def _opt(name):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return None


out_path, root, merge = _opt("--out"), _opt("--root") or ROOT, _opt("--merge")
QUICK, YARD = "--quick" in argv, "--yardsticks" in argv
REPS = 3 if QUICK else 7
N = 512 if QUICK else 4096
H = 1e-2

pkg_dir = os.path.join(os.path.abspath(root), "stheno.jl_amd")
spec = importlib.util.spec_from_file_location("stheno_jl_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
P = importlib.util.module_from_spec(spec)
sys.modules["stheno_jl_amd"] = P
spec.loader.exec_module(P)


def stat(f, reps=REPS, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))


def joint(D, dims, how):
    gpc = P.GPC()
    f = P.atomic(P.GP(P.SEKernel()), gpc)

    def d(k):
        if how == "derivative":
            return P.derivative(f, k)
        A = np.zeros((D, 2))
        A[k] = (-H, H)
        return P.stencil(f, A, [0.5 / H, -0.5 / H])
    X = np.asfortranarray(np.random.default_rng(D).standard_normal((D, N // (1 + len(dims)))))
    x = P.ColVecs(X) if D > 1 else X[0].copy()
    return P.cross([f] + [d(k) for k in dims])(P.BlockData([x] * (1 + len(dims))), 0.1)


def yardstick(D, name):
    k = P.LinearKernel() if name == "Linear" else P.SEKernel() * P.Matern32Kernel()
    f = P.atomic(P.GP(k), P.GPC())
    X = np.asfortranarray(np.random.default_rng(D).standard_normal((D, N)) / np.sqrt(D))
    return f(P.ColVecs(X) if D > 1 else X[0].copy(), 0.1)


def measure(fx, grad):
    """cov: sgp_kernelmatrix into a kept host buffer (the assembly kernels and the copy back, no host arithmetic)"""
    L = P.lib
    y = np.sin(np.arange(len(fx)) * 0.1)
    sp = P.build_spec(fx.f, fx.x)[0]
    n = sp.N
    K = np.zeros((n, n), order="F")
    ctx = L.default_context()
    r = dict(cov=stat(lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, sp.ref(ctx), L.dptr(K), n), "sgp_kernelmatrix")))
    del K
    r["logpdf"] = stat(lambda: P.logpdf(fx, y))
    r["logpdf_and_gradient"] = stat(lambda: grad(fx, y))
    return r


res = dict(N=N, reps=REPS, h=H, root=os.path.abspath(root), models={}, yardsticks={})
for D in (1, 8):
    for name in ("Linear", "SE * Matern32"):
        res["yardsticks"][f"{name}, D = {D}"] = measure(yardstick(D, name), P.logpdf_and_gradient)
if not YARD:
    for label, D, dims in (("(f, d0 f), D = 1", 1, (0,)), ("(f, d0 f), D = 8", 8, (0,)), ("(f, d0 f, d1 f, d2 f), D = 3", 3, (0, 1, 2))):
        exact = measure(joint(D, dims, "derivative"), P.logpdf_and_gradient)
        fd = measure(joint(D, dims, "stencil"), P.logpdf_and_gradient_stencil)
        res["models"][label] = dict(derivative=exact, stencil=fd,
                                    stencil_over_derivative={k: fd[k]["median_ms"] / exact[k]["median_ms"] for k in exact})
if merge:
    parent = json.load(open(merge))
    res["parent"] = parent
    res["inside_parent_min_max"] = {
        m: {k: parent["yardsticks"][m][k]["min_ms"] <= v["median_ms"] <= parent["yardsticks"][m][k]["max_ms"] for k, v in r.items()}
        for m, r in res["yardsticks"].items()}
text = json.dumps(res, indent=1)
print(text)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
