"""What the Wiener and PiecewisePolynomial kinds cost (include/sthenomi_kprod.h; csrc/kprod.hip: wiener_eval / wiener_derivs /
pp_derivs and the mode-3 instantiations of the product kernels), beside LinearKernel and SEKernel * Matern32Kernel, a chain of
the instantiations every older chain runs.
One box, one process, medians of 7 calls after a warm-up, with min and max; wall time around host calls that end in a copy
back to the host (so every call is complete when the clock stops).  N = 4096, D in {1, 8}, points uniform in [0, 1]^D / sqrt(D)
(the half line at D = 1: WIENER with i >= 1 is not known to be positive definite beyond it), noise 0.1.  Per model: cov
(sgp_kernelmatrix into a kept host buffer), logpdf, logpdf_and_gradient_param(inputs=True).
  models:      Wiener(1), Wiener(3), PiecewisePolynomial(0), PiecewisePolynomial(3) (lone terms; beyond D = 1 the WIENER
               factors read coordinate 0), SE * PiecewisePolynomial(2)
  yardsticks:  Linear, SE * Matern32
`vs Linear` / `vs SE * Matern32` = the model's median over the yardstick's median in the same run.
usage: python tools/wienerpp_time.py [--out FILE] [--quick] [--yardsticks] [--root DIR] [--merge FILE]
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
YARDSTICKS = ("Linear", "SE * Matern32")


def stat(f, reps=REPS, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)))


def kernels(D):
    ks = {"Linear": lambda: P.LinearKernel(0.0), "SE * Matern32": lambda: P.SEKernel() * P.Matern32Kernel()}
    if not YARD:
        w = (lambda i: P.WienerKernel(i)) if D == 1 else (lambda i: P.WienerKernel(i) @ P.SelectTransform([0]))
        ks.update({"Wiener(1)": lambda: w(1), "Wiener(3)": lambda: w(3),
                   "PiecewisePolynomial(0)": lambda: P.PiecewisePolynomialKernel(0, dim=D),
                   "PiecewisePolynomial(3)": lambda: P.PiecewisePolynomialKernel(3, dim=D),
                   "SE * PiecewisePolynomial(2)": lambda: P.SEKernel() * P.PiecewisePolynomialKernel(2, dim=D)})
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
        X = np.asfortranarray(rng.uniform(0.0, 1.0, (D, N)) / np.sqrt(D))
        y = rng.standard_normal(N)
        cell = {name: measure(k, X, y) for name, k in kernels(D).items()}
        for name, r in cell.items():
            for yard in YARDSTICKS:
                r[f"vs {yard}"] = {op: r[op]["median_s"] / cell[yard][op]["median_s"] for op in OPS}
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
            for name in YARDSTICKS:
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
