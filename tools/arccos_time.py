#!/usr/bin/env python3
"""Time the arc-cosine kinds on one MI355X (docs/05_measurement.md: one process, a warm-up call, the median of --reps timed
calls with min and max).  Not a test, not part of bench.py; no threshold.

    python tools/arccos_time.py [--out profiles/NAME.json] [--reps 5] [--sizes 4096,16384]
        `logpdf` and logpdf_and_gradient(inputs=True) of an NNGP + NTK model of depth L = 1, 4, 16 (D = 8, bias 1) beside an SE
        model of the same shape
    python tools/arccos_time.py --trace N
        --reps + 1 sgp_kernelmatrix calls each of an N x N SE block and of an NTK block at L = 1, 4, 16 (D = 8): run under
        `rocprofv3 --kernel-trace --stats` for the assembly kernels' own durations
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stheno.jl_amd")
_spec = importlib.util.spec_from_file_location("stheno_jl_amd", os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
P = importlib.util.module_from_spec(_spec)
sys.modules["stheno_jl_amd"] = P
_spec.loader.exec_module(P)

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="4096,16384")
ap.add_argument("--trace", type=int)
A = ap.parse_args()
DEPTHS, D = (1, 4, 16), 8


def timed(fn):
    fn()
    ts = []
    for _ in range(A.reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts))


def two(k, x, y):
    f = P.atomic(P.GP(k), P.GPC())
    return dict(logpdf=timed(lambda: P.logpdf(f(x, 0.1), y)),
                logpdf_and_gradient_inputs=timed(lambda: P.logpdf_and_gradient(f(x, 0.1), y, inputs=True)))


def models():
    rows = []
    for n in [int(v) for v in A.sizes.split(",")]:
        rng = np.random.default_rng(n)
        x, y = P.ColVecs(np.asfortranarray(rng.uniform(-1.0, 1.0, (D, n)))), rng.standard_normal(n)
        se = two(P.with_lengthscale(P.SEKernel(), 0.7), x, y)
        for depth in DEPTHS:
            row = dict(N=n, D=D, L=depth, se=se,
                       arccos=two(0.5 * P.NNGPKernel(depth, bias=1.0) + 0.5 * P.NTKKernel(depth, bias=1.0), x, y))
            for what in ("logpdf", "logpdf_and_gradient_inputs"):
                row[f"ratio_to_se_{what}"] = row["arccos"][what]["median_ms"] / se[what]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def trace(n):
    L = P.lib
    ctx, rng = L.default_context(), np.random.default_rng(n)
    K, X = np.zeros((n, n), order="F"), np.asfortranarray(rng.uniform(-1.0, 1.0, (D, n)))
    rows = []
    for name, kind, depth in [("se", L.SE, 0)] + [(f"ntk_L{d}", L.NTK, d) for d in DEPTHS]:
        sp = L.Spec([n], [n], [X, X], {(0, 0): [(kind, 0, 1, 1.0, float(depth), None, None)]}, False)
        rows.append(dict(N=n, D=D, block=name,
                         call=timed(lambda: L.check(L.load().sgp_kernelmatrix(ctx.handle, sp.ref(ctx), L.dptr(K), n), name))))
        print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    rows = trace(A.trace) if A.trace else models()
    if A.out:
        with open(A.out, "w") as fh:
            json.dump(dict(tool="tools/arccos_time.py", reps=A.reps, rows=rows), fh, indent=1)
