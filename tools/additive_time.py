#!/usr/bin/env python3
"""Time an additive model (additive_kernel(SEKernel(), R variances) behind an ARDTransform) beside an SE model of the same shape
on one MI355X (docs/05_measurement.md: one process, a warm-up call, the median of --reps timed calls with min and max):
`logpdf` and logpdf_and_gradient(inputs=True) at N = 4096 and 16 384 for (D, R) = (4, 2), (8, 4), (16, 8).  At (4, 2) the same
model is also written as its 10 product chains (4 + 6 products of SEKernel @ SelectTransform) and timed through logpdf and
logpdf_and_gradient_param.  The assembly kernels' own durations come from running this tool under
`rocprofv3 --kernel-trace --stats`, one size per run.  Not a test, not part of bench.py; no threshold.

    python tools/additive_time.py [--out profiles/NAME.json] [--reps 5] [--sizes 4096,16384]
"""
import argparse
import importlib.util
import itertools
import json
import os
import sys
import time

import numpy as np

pkg_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stheno.jl_amd")
spec = importlib.util.spec_from_file_location("stheno_jl_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
P = importlib.util.module_from_spec(spec)
sys.modules["stheno_jl_amd"] = P
spec.loader.exec_module(P)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts))


def chains(D, R, variances):
    """the additive model as a sum of C(D, r) products per order"""
    one = [P.SEKernel() @ P.SelectTransform([d]) for d in range(D)]
    terms = []
    for r in range(1, R + 1):
        for c in itertools.combinations(range(D), r):
            k = one[c[0]]
            for d in c[1:]:
                k = k * one[d]
            terms.append(variances[r - 1] * k)
    return P.KernelSum(terms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--shapes", default="4:2,8:4,16:8")
    a = ap.parse_args()
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        for D, R in [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]:
            rng = np.random.default_rng(n + D)
            x, y = P.ColVecs(np.asfortranarray(rng.uniform(-1.0, 1.0, (D, n)))), rng.standard_normal(n)
            var = [1.0 / (r + 1) for r in range(R)]
            ard = P.ARDTransform(np.linspace(0.8, 1.6, D))
            kernels = {"additive": P.additive_kernel(P.SEKernel(), var) @ ard, "se": P.SEKernel() @ ard}
            row = dict(N=n, D=D, R=R)
            for name, k in kernels.items():
                f = P.atomic(P.GP(k), P.GPC())
                row[name] = dict(logpdf=timed(lambda: P.logpdf(f(x, 0.1), y), a.reps),
                                 logpdf_and_gradient_inputs=timed(lambda: P.logpdf_and_gradient(f(x, 0.1), y, inputs=True), a.reps))
            if (D, R) == (4, 2):
                f = P.atomic(P.GP(chains(D, R, var) @ ard), P.GPC())
                row["chains"] = dict(logpdf=timed(lambda: P.logpdf(f(x, 0.1), y), a.reps),
                                     logpdf_and_gradient_param=timed(lambda: P.logpdf_and_gradient_param(f(x, 0.1), y, inputs=True), a.reps))
            for what in ("logpdf", "logpdf_and_gradient_inputs"):
                row[f"ratio_{what}"] = row["additive"][what]["median_ms"] / row["se"][what]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/additive_time.py", reps=a.reps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
