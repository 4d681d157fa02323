"""logpdf + gradient of B independent models (Matern-5/2, D = 8, different hyper-parameters and inputs per member)
  (a) one sgp_logpdf_grad after the other on one context  -- the loop a host runs today,
  (b) ONE sgp_logpdf_grad_batch call (one dataflow task pool for the factorisations, one launch for every C^-1).
ms per call, aggregate TFLOP/s on B N^3 (the flop convention of bench.py's `grad` block: factorisation N^3 / 3 + inverse
2 N^3 / 3) and its fraction of the 78.6 TFLOP/s fp64 MFMA peak, a per-member bit-equality flag (logpdf and every gradient
output of (b) against (a)), and the context's dataflow time-out fallbacks.  Timed around the C-ABI calls with prebuilt specs.
usage: python tools/gpu_grad_batch_time.py [--out FILE] [--batches B,B,...] [N ...]      -> JSON on stdout (and in FILE)
(--batches 8: one batch size only -- what a kernel trace of N = 4096, B = 8 runs)"""
import ctypes as C
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
PEAK = 78.6
argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
Bs = (1, 4, 8, 16)
if "--batches" in argv:
    i = argv.index("--batches")
    Bs = tuple(int(b) for b in argv[i + 1].split(","))
    del argv[i:i + 2]
Ns = [int(a) for a in argv] or [2048, 4096, 8192]
D = 8


def members(N, B, seed=0):
    rng = np.random.default_rng(seed + N)
    out = []
    for b in range(B):
        ell, v, s2 = 0.8 + 0.4 * rng.random(), 0.5 + rng.random(), 0.05 + 0.1 * rng.random()
        f = v * P.stretch(P.atomic(P.GP(P.Matern52Kernel()), P.GPC()), 1.0 / ell)
        x = np.asfortranarray(rng.standard_normal((D, N)))
        spec = P.build_spec(f, P.ColVecs(x))[0]
        nt = max(1, spec.n_terms)
        out.append(dict(spec=spec, y=np.ascontiguousarray(rng.standard_normal(N)), nz=np.array([s2]),
                        outs=[np.zeros(1), np.zeros(N), np.zeros(N), np.zeros(1), np.zeros(nt), np.zeros(nt)]))
    return out


def single(ctx, m, outs):
    L.check(ctx.lib.sgp_logpdf_grad(ctx.handle, m["spec"].ref(), None, L.NOISE_SCALAR, L.dptr(m["nz"]), L.dptr(m["y"]),
                                    *[L.dptr(o) for o in outs]), "sgp_logpdf_grad")


def med(f, reps=5, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def fallbacks(ctx):
    n = C.c_int64(0)
    L.check(ctx.bench.sgp_bench_df_fallbacks(ctx.handle, C.byref(n)))
    return int(n.value)


res = {}
for N in Ns:
    fl = float(N) ** 3
    ms = members(N, max(Bs))
    ctx = L.Context(0)
    r = dict(schedule_single=ctx.factor_schedule(N), B={})
    for B in Bs:
        mb = ms[:B]
        # (a) the member-by-member loop; its outputs are the reference bits
        ta = med(lambda: [single(ctx, m, m["outs"]) for m in mb])
        ref = [[o.copy() for o in m["outs"]] for m in mb]
        # (b) one batch call into fresh buffers
        nb = B
        specs = (C.POINTER(L.sgp_cov_spec) * nb)(*[C.pointer(m["spec"].c) for m in mb])
        noises = (C.POINTER(C.c_double) * nb)(*[L.dptr(m["nz"]) for m in mb])
        ys = (C.POINTER(C.c_double) * nb)(*[L.dptr(m["y"]) for m in mb])
        lp = np.zeros(nb)
        bufs = [[np.zeros_like(o) for o in m["outs"][1:]] for m in mb]
        arrs = [(C.POINTER(C.c_double) * nb)(*[L.dptr(bufs[b][q]) for b in range(nb)]) for q in range(5)]
        infos = np.zeros(nb, dtype=np.int32)
        fb0 = fallbacks(ctx)

        def call():
            L.check(ctx.batch.sgp_logpdf_grad_batch(ctx.handle, nb, specs, None, L.NOISE_SCALAR, noises, ys, L.dptr(lp), *arrs,
                                                    infos.ctypes.data_as(C.POINTER(C.c_int))), "sgp_logpdf_grad_batch")
        tb = med(call)
        eq = [bool(lp[b] == ref[b][0][0] and all(np.array_equal(bufs[b][q], ref[b][q + 1]) for q in range(5)))
              for b in range(nb)]
        r["B"][B] = dict(loop_ms=ta, loop_tflops=B * fl / (ta * 1e-3) / 1e12, loop_frac=B * fl / (ta * 1e-3) / 1e12 / PEAK,
                         batch_ms=tb, batch_tflops=B * fl / (tb * 1e-3) / 1e12, batch_frac=B * fl / (tb * 1e-3) / 1e12 / PEAK,
                         speedup=ta / tb, bit_equal=eq, all_bit_equal=all(eq), infos=[int(i) for i in infos],
                         df_fallbacks=fallbacks(ctx) - fb0)
        print(N, B, json.dumps(r["B"][B]), file=sys.stderr, flush=True)
    ctx.close()
    res[N] = r
txt = json.dumps(res, indent=1)
print(txt)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(txt + "\n")
