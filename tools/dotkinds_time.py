"""What the NeuralNetwork, FBM and Exponentiated kinds cost (include/sthenomi_kprod.h; csrc/kprod.hip: dotkind_eval /
dotkind_derivs and the mode-2 instantiations of the product kernels), beside LinearKernel -- the one older kind of x'y -- and
SEKernel * Matern32Kernel, a chain of the instantiations every older chain runs.
One box, one process, medians of 7 calls after a warm-up, with min and max; wall time around host calls that end in a copy
back to the host (so every call is complete when the clock stops).  N = 4096, D in {1, 8}, points uniform in [-1, 1]^D,
noise 0.1.  Per model: cov (sgp_kernelmatrix into a kept host buffer), logpdf, logpdf_and_gradient_param(inputs=True).
  models:      NeuralNetwork, FBM(0.5), Exponentiated (lone terms), SE * NeuralNetwork
  yardsticks:  Linear, SE * Matern32
`vs Linear` = the model's median over LinearKernel's median in the same run.
usage: python tools/dotkinds_time.py [--out FILE] [--quick] [--yardsticks] [--root DIR] [--merge FILE]
  --yardsticks   the two yardstick models only
  --root DIR     time the package of another checkout (its stheno.jl_amd/ with built libraries), e.g. a build of the parent
                 commit: the regression criterion is that this build's yardstick medians lie inside that build's min - max
  --merge FILE   put FILE (the JSON of such a run) under "parent" in the output and record the criterion's outcome
-> JSON on stdout (and in FILE)"""
import hashlib
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

pkg_dir = os.path.join(os.path.abspath(root), "stheno.jl_amd")
spec = importlib.util.spec_from_file_location("stheno_jl_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
P = importlib.util.module_from_spec(spec)
sys.modules["stheno_jl_amd"] = P
spec.loader.exec_module(P)
L = P.lib


def stat(f, reps=REPS, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)))


def kernels():
    ks = {"Linear": lambda: P.LinearKernel(0.0), "SE * Matern32": lambda: P.SEKernel() * P.Matern32Kernel()}
    if not YARD:
        ks.update({"NeuralNetwork": lambda: P.NeuralNetworkKernel(), "FBM(0.5)": lambda: P.FBMKernel(0.5),
                   "Exponentiated": lambda: P.ExponentiatedKernel(), "SE * NeuralNetwork": lambda: P.SEKernel() * P.NeuralNetworkKernel()})
    return ks


def measure(kernel, X, y, noise=0.1):
    n = X.shape[1]
    F = P.gppp(lambda GP: {"f": GP(kernel())})
    x = P.GPPPInput("f", X[0].copy() if X.shape[0] == 1 else P.ColVecs(X))
    fx = F(x, noise)
    sp = P.build_spec(F, fx.x)[0]
    K = np.zeros((n, n), order="F")
    ctx = L.default_context()
    r = dict(cov=stat(lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, sp.ref(ctx), L.dptr(K), n), "sgp_kernelmatrix")))
    del K
    r["logpdf"] = stat(lambda: P.logpdf(fx, y))
    r["logpdf_and_gradient_param, inputs"] = stat(lambda: P.logpdf_and_gradient_param(fx, y, inputs=True))
    return r


OPS = ("cov", "logpdf", "logpdf_and_gradient_param, inputs")


def main():
    rng = np.random.default_rng(0)
    res = dict(shape=dict(N=N, reps=REPS), root=os.path.relpath(os.path.abspath(root), ROOT))
    for D in (1, 8):
        X = np.asfortranarray(rng.uniform(-1.0, 1.0, (D, N)))
        y = rng.standard_normal(N)
        cell = {name: measure(k, X, y) for name, k in kernels().items()}
        for name, r in cell.items():
            r["vs Linear"] = {op: r[op]["median_s"] / cell["Linear"][op]["median_s"] for op in OPS}
        res[f"D = {D}"] = cell
        print(f"D = {D}: done", file=sys.stderr, flush=True)
    src = os.path.join(pkg_dir, "csrc", "kprod.hip")
    res["build"] = dict(libsthenomi_sha16=hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16],
                        kprod_hip_sha16=hashlib.sha256(open(src, "rb").read()).hexdigest()[:16])
    if merge:
        parent = json.load(open(merge))
        res["parent"] = parent
        inside = {}
        for D in ("D = 1", "D = 8"):
            for name in ("Linear", "SE * Matern32"):
                for op in OPS:
                    p, m = parent[D][name][op], res[D][name][op]["median_s"]
                    inside[f"{D}, {name}, {op}"] = dict(median_s=m, parent_min_s=p["min_s"], parent_max_s=p["max_s"],
                                                        inside=bool(p["min_s"] <= m <= p["max_s"]), not_slower=bool(m <= p["max_s"]))
        res["yardsticks against the parent build"] = inside
    out = json.dumps(res, indent=1)
    print(out)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
