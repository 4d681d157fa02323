#!/usr/bin/env python3
"""Time the blur kind on one MI355X (docs/05_measurement.md: one process, a warm-up call, the median of --reps timed calls
with min and max).  Not a test, not part of bench.py; no threshold.

    python tools/blur_time.py [--out profiles/NAME.json] [--reps 7] [--sizes 4096,16384]
        `cov` (with its copy to the host), `logpdf` and logpdf_and_gradient(inputs=True) of (f, blur f), N / 2 points each,
        at D = 1 and 8, beside an SE model of N points and -- at D = 1 -- beside quadrature_convolve with the smallest
        Gauss-Hermite rule whose covariance agrees with the exact kind to 1e-10 (that count is searched first and stated)
    python tools/blur_time.py --trace N
        one sgp_kernelmatrix each of an N x N SE, one-sided blur and two-sided blur block (D = 8 and D = 1): run under
        `rocprofv3 --kernel-trace --stats` for the assembly kernels' own durations
    python tools/blur_time.py --yardstick [--pkg OTHER/stheno.jl_amd]
        logpdf of the LinearKernel and SEKernel * Matern32Kernel yardstick models (N = 4096, D = 4); --pkg: another build's
        package (the parent commit's), to be run alternately with this one
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sizes", default="4096,16384")
ap.add_argument("--trace", type=int)
ap.add_argument("--yardstick", action="store_true")
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stheno.jl_amd"))
A = ap.parse_args()
spec = importlib.util.spec_from_file_location("stheno_jl_amd", os.path.join(A.pkg, "__init__.py"), submodule_search_locations=[A.pkg])
P = importlib.util.module_from_spec(spec)
sys.modules["stheno_jl_amd"] = P
spec.loader.exec_module(P)


def timed(fn):
    fn()
    ts = []
    for _ in range(A.reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts))


def three(F, x, y):
    return dict(cov=timed(lambda: P.prior_cov(F, x)), logpdf=timed(lambda: P.logpdf(F(x, 0.1), y)),
                logpdf_and_gradient_inputs=timed(lambda: P.logpdf_and_gradient(F(x, 0.1), y, inputs=True)))


def quadrature_nodes():
    """the smallest Gauss-Hermite rule whose cov of (f, quadrature_convolve f) agrees with (f, sqrt(pi) blur(f, 1/2)) to 1e-10
    at D = 1: quadrature_convolve is int exp(-t^2) f(x - t) dt, i.e. sqrt(pi) times the N(0, 1/2) footprint"""
    x = np.linspace(-2.0, 2.0, 64)
    f = P.atomic(P.GP(P.SEKernel()), P.GPC())
    xx = P.BlockData([x, x])
    exact = P.prior_cov(P.cross([f, np.sqrt(np.pi) * P.blur(f, 0.5)]), xx)
    for q in range(2, 65):
        err = float(np.max(np.abs(P.prior_cov(P.cross([f, P.quadrature_convolve(f, q)]), xx) - exact)))
        if err <= 1e-10:
            return q, err
    return None, err


def models():
    q, err = quadrature_nodes()
    rows = [dict(quadrature_nodes_for_1e_10=q, error_at_that_count=err)]
    print(json.dumps(rows[0]), flush=True)
    for n in [int(v) for v in A.sizes.split(",")]:
        for D in (1, 8):
            rng = np.random.default_rng(n + D)
            X, y = np.asfortranarray(rng.uniform(-1.0, 1.0, (D, n))), rng.standard_normal(n)
            h = n // 2
            halves = P.BlockData([P.ColVecs(np.asfortranarray(X[:, :h])), P.ColVecs(np.asfortranarray(X[:, h:]))])
            f = P.atomic(P.GP(P.with_lengthscale(P.SEKernel(), 0.4)), P.GPC())
            row = dict(N=n, D=D, blur=three(P.cross([f, P.blur(f, 0.05)]), halves, y), se=three(f, P.ColVecs(X), y))
            if D == 1 and q is not None:
                x1 = P.BlockData([X[0, :h].copy(), X[0, h:].copy()])
                row["quadrature"] = dict(nodes=q, cov=timed(lambda: P.prior_cov(P.cross([f, P.quadrature_convolve(f, q)]), x1)),
                                         logpdf=timed(lambda: P.logpdf(P.cross([f, P.quadrature_convolve(f, q)])(x1, 0.1), y)))
            for what in ("cov", "logpdf", "logpdf_and_gradient_inputs"):
                row[f"ratio_to_se_{what}"] = row["blur"][what]["median_ms"] / row["se"][what]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def trace(n):
    L = P.lib
    ctx, rng = L.default_context(), np.random.default_rng(n)
    K = np.zeros((n, n), order="F")
    for D in (8, 1):
        X = rng.uniform(-1.0, 1.0, (D, n))
        plain, wide = np.asfortranarray(np.vstack([X, 0 * X])), np.asfortranarray(np.vstack([X, 0.05 + 0 * X]))
        for name, kind, Zr, Zc in (("se", L.SE, np.asfortranarray(X), np.asfortranarray(X)), ("blur_one_sided", L.BLUR_SE, wide, plain),
                                   ("blur_two_sided", L.BLUR_SE, wide, wide)):
            sp = L.Spec([n], [n], [Zr, Zc], {(0, 0): [(kind, 0, 1, 1.0, 0.0, None, None)]}, False)
            t0 = time.perf_counter()
            assert L.load().sgp_kernelmatrix(ctx.handle, sp.ref(ctx), L.dptr(K), n) == 0, L.last_error()
            print(json.dumps(dict(N=n, D=D, block=name, call_ms=(time.perf_counter() - t0) * 1e3)), flush=True)


def yardstick():
    n, D = 4096, 4
    rng = np.random.default_rng(1)
    x, y = P.ColVecs(np.asfortranarray(rng.uniform(-1.0, 1.0, (D, n)))), rng.standard_normal(n)
    rows = []
    for name, k in (("linear", P.LinearKernel()), ("se_times_matern32", P.SEKernel() * P.Matern32Kernel())):
        f = P.atomic(P.GP(k), P.GPC())
        rows.append(dict(model=name, N=n, D=D, pkg=A.pkg, logpdf=timed(lambda: P.logpdf(f(x, 0.1), y))))
        print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    rows = trace(A.trace) if A.trace else yardstick() if A.yardstick else models()
    if A.out:
        with open(A.out, "w") as fh:
            json.dump(dict(tool="tools/blur_time.py", reps=A.reps, rows=rows), fh, indent=1)
