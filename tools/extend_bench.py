"""update_posterior (include/sthenomi_extend.h: sgp_posterior_extend) against the stacked re-factorisation, on one box in one run.

For N in {4096, 16384, 32768} x n_new in {16, 128, 1024}, each configuration in a fresh child process under its own time
limit (a configuration that fails or overruns ends the run: nothing more is started on the GPU):
  * sgp_posterior_extend reallocating: a posterior of N points extended by n_new, the buffer reserved for N + 2 n_new;
  * sgp_posterior_extend reserved (in place): that posterior extended by n_new MORE points (so its base is N + n_new points:
    a little more work than the configuration's name says, never less);
  * the row solve of the extension by both of its schedules (sgp_bench_extend_row_solve: deep products as single launches /
    split over K), on the tile rows the first extension solves;
  * sgp_posterior_create on the stacked N + n_new points -- the only route without the extension;
  * the largest difference of mean_and_var at 256 test points between the extended and the stacked posterior;
  * the stages of one more reserved extension (sgp_ctx_stage_timing).
Method as docs/05_measurement.md: wall time around the C call with prebuilt specs, a warm-up, then the median of the repeats.
usage: python tools/extend_bench.py [--out FILE] [--quick] [--reps K]   -> profiles/r08_extend.json + a line in profiles/INDEX.md"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(n, k) for n in (4096, 16384, 32768) for k in (16, 128, 1024)]
QUICK_SIZES = [(1024, 16), (2048, 128)]
STAGES = ["buffer (reallocation, tile copy, save)", "assembly of the row window", "row solve", "trailing update",
          "factorisation of the trailing block", "scalars and alpha"]
INDEX_LINE = ("| **update_posterior**: sgp_posterior_extend (reallocating / reserved) against sgp_posterior_create on the stacked "
              "data, both row-solve schedules, per-stage times; N = 4096 / 16 384 / 32 768 x n_new = 16 / 128 / 1024 "
              "(`tools/extend_bench.py`) | `r08_extend.json` |")


def child(N, k, reps):
    import __graft_entry__ as entry
    P = entry.load_package()
    L = P.lib
    ctx = L.default_context()
    lib, ext = ctx.lib, ctx.extend
    rng = np.random.default_rng(N + k)
    D, s2 = 4, 0.1
    F = P.gppp_sum_model()
    X = np.asfortranarray(rng.standard_normal((D, N + 2 * k)))
    y = rng.standard_normal(N + 2 * k)
    Xs = P.GPPPInput("f3", P.ColVecs(np.asfortranarray(rng.standard_normal((D, 256)))))

    def inp(a, b):
        return P.GPPPInput("f3", P.ColVecs(np.asfortranarray(X[:, a:b])))
    blocks = [inp(0, N), inp(N, N + k), inp(N + k, N + 2 * k)]
    spec0 = P.finite_gp._prior_spec(F, blocks[0])
    spec1 = P.finite_gp._prior_spec(F, P.BlockData(blocks[:2]))
    spec2 = P.finite_gp._prior_spec(F, P.BlockData(blocks))
    noise = np.array([s2])
    m2 = np.asfortranarray(P.mean_vector(F, P.BlockData(blocks)), dtype=np.float64)

    def create(spec, n):
        h = C.c_void_p()
        t0 = time.perf_counter()
        L.check(lib.sgp_posterior_create(ctx.handle, spec.ref(), L.dptr(m2[:n].copy()), L.NOISE_SCALAR, L.dptr(noise), L.dptr(y[:n].copy()), None,
                                         C.byref(h)), "sgp_posterior_create")
        return h, time.perf_counter() - t0

    def extend(h, spec, n, n_new, reserve):
        yy = y[:n].copy()
        t0 = time.perf_counter()
        L.check(ext.sgp_posterior_extend(h, spec.ref(), L.dptr(m2[:n].copy()), L.NOISE_SCALAR, L.dptr(noise), L.dptr(yy), n_new, reserve, None, None),
                "sgp_posterior_extend")
        return time.perf_counter() - t0

    def predict(h, x_train, n):
        post = P.PosteriorGP(F, x_train, h, None, None, s2, y[:n].copy(), mean_x=m2[:n].copy())
        out = post.mean_and_var(Xs)
        post._h = None                   # (the handle stays ours)
        return out

    t_stack, t_realloc, t_inplace = [], [], []
    diff = None
    for r in range(reps + 1):            # (the first repeat is the warm-up)
        h1, t = create(spec1, N + k)
        t_stack.append(t)
        h, _ = create(spec0, N)
        t_realloc.append(extend(h, spec1, N + k, k, N + 2 * k))
        if diff is None:
            a, b = predict(h, P.BlockData(blocks[:2]), N + k), predict(h1, P.BlockData(blocks[:2]), N + k)
            diff = dict(mean=float(np.max(np.abs(a[0] - b[0]))), var=float(np.max(np.abs(a[1] - b[1]))))
        lib.sgp_posterior_destroy(h1)
        t_inplace.append(extend(h, spec2, N + 2 * k, k, 0))
        lib.sgp_posterior_destroy(h)
    # the stages of one more reserved extension, and the row solve by both schedules on the kept factor of N points
    h, _ = create(spec0, N)
    extend(h, spec1, N + k, k, N + 2 * k)
    L.check(lib.sgp_ctx_stage_timing(ctx.handle, 1), "stage_timing")
    extend(h, spec2, N + 2 * k, k, 0)
    ms = np.zeros(16)
    L.check(lib.sgp_ctx_stage_ms(ctx.handle, L.dptr(ms)), "stage_ms")
    L.check(lib.sgp_ctx_stage_timing(ctx.handle, 0), "stage_timing")
    lib.sgp_posterior_destroy(h)
    h, _ = create(spec0, N)
    tile_rows = (-(-(N + k) // 128) * 128 - N // 128 * 128) // 128 + 1
    rs = {}
    for sched, name in ((0, "single launches (drv_row_trsm)"), (1, "split over K")):
        out = np.zeros(reps + 1)
        L.check(L.extend_bench_lib().sgp_bench_extend_row_solve(h, tile_rows, sched, reps + 1, L.dptr(out)), "sgp_bench_extend_row_solve")
        rs[name] = float(np.median(out[1:]))
    lib.sgp_posterior_destroy(h)
    med = lambda v: float(np.median(v[1:]) * 1e3)   # noqa: E731
    res = dict(N=N, n_new=k, reps=reps, extend_reallocating_ms=med(t_realloc), extend_reserved_ms=med(t_inplace),
               stacked_create_ms=med(t_stack), reserved_over_stacked=med(t_inplace) / med(t_stack),
               row_solve_tile_rows=int(tile_rows), row_solve_ms=rs, max_abs_diff_mean_and_var_256=diff,
               stages_of_one_reserved_extension_ms={STAGES[i]: float(ms[i]) for i in range(len(STAGES))})
    print("RESULT " + json.dumps(res))


def ensure_index_line():
    path = os.path.join(ROOT, "profiles", "INDEX.md")
    txt = open(path).read()
    if "r08_extend.json" not in txt:
        with open(path, "a") as fh:
            fh.write(("" if txt.endswith("\n") else "\n") + INDEX_LINE + "\n")


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--child":
        return child(int(argv[1]), int(argv[2]), int(argv[3]))
    out_path = os.path.join(ROOT, "profiles", "r08_extend.json")
    reps = 5
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
    sizes = QUICK_SIZES if "--quick" in argv else SIZES
    res = dict(what="sgp_posterior_extend against sgp_posterior_create on the stacked data; see tools/extend_bench.py",
               method="wall time around the C call, prebuilt specs, one warm-up, median of the repeats; one fresh process per "
                      "configuration", configs=[])
    for N, k in sizes:
        limit = 120 + N // 128
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N), str(k), str(reps)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"N={N} n_new={k}: no result within {limit} s; nothing further was started"
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            res["stopped"] = f"N={N} n_new={k}: exit status {p.returncode}; nothing further was started: {p.stderr[-600:]}"
            break
        res["configs"].append(json.loads(line[-1][7:]))
        print(line[-1], flush=True)
    for c in res["configs"]:
        if (c["N"], c["n_new"]) == (16384, 128):
            res["condition"] = dict(text="N = 16384, n_new = 128: reserved extension <= 1/3 of the stacked re-factorisation",
                                    ratio=c["reserved_over_stacked"], met=bool(c["reserved_over_stacked"] <= 1.0 / 3.0))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    if os.path.abspath(out_path) == os.path.join(ROOT, "profiles", "r08_extend.json"):
        ensure_index_line()
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
