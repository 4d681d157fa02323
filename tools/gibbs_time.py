#!/usr/bin/env python3
"""Time a GibbsKernel model beside an SE model of the same shape on one MI355X (docs/05_measurement.md: one process, a warm-up
call, the median of --reps timed calls with min and max): `cov` (sgp_kernelmatrix, with its copy to the host), `logpdf` (the
matrix stays on the device) and logpdf_and_gradient(inputs=True) at N = 4096 and 16 384, D = 2.  The assembly kernels' own
durations come from running this tool under `rocprofv3 --kernel-trace --stats`, one size per run.  Not a test, not part of
bench.py; no threshold.

    python tools/gibbs_time.py [--out profiles/NAME.json] [--reps 5] [--sizes 4096,16384]
"""
import argparse
import importlib.util
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4096,16384")
    a = ap.parse_args()
    kernels = {"gibbs_p2": P.GibbsKernel(lambda X: 0.3 + 0.2 * (X * X).sum(0), power=2), "se": P.with_lengthscale(P.SEKernel(), 0.4)}
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        rng = np.random.default_rng(n)
        x, y = P.ColVecs(np.asfortranarray(rng.uniform(-1.0, 1.0, (2, n)))), rng.standard_normal(n)
        row = dict(N=n, D=2)
        for name, k in kernels.items():
            f = P.atomic(P.GP(k), P.GPC())
            row[name] = dict(cov=timed(lambda: P.prior_cov(f, x), a.reps), logpdf=timed(lambda: P.logpdf(f(x, 0.1), y), a.reps),
                             logpdf_and_gradient_inputs=timed(lambda: P.logpdf_and_gradient(f(x, 0.1), y, inputs=True), a.reps))
        for what in ("cov", "logpdf", "logpdf_and_gradient_inputs"):
            row[f"ratio_{what}"] = row["gibbs_p2"][what]["median_ms"] / row["se"][what]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(tool="tools/gibbs_time.py", reps=a.reps, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
