"""update_posterior of a sparse posterior (include/sthenomi_vfe_update.h: sgp_sparse_posterior_update) against
sgp_sparse_posterior_create on the stacked data, on one box in one run.

The claim under test: the time of one update does not depend on the number of points absorbed before.  For M = 4096,
N in {65 536, 262 144} x n_new in {128, 1024, 8192}, each configuration in a fresh child process under its own time limit (a
configuration that fails or overruns ends the run: nothing more is started on the GPU):
  * sgp_sparse_posterior_update of n_new points on a posterior of N (the repeats go on absorbing batches of n_new: the
    posterior grows, the work per call does not): median, minimum and maximum of the repeats;
  * sgp_sparse_posterior_create on the stacked N + n_new points in the same process -- the only route without the update;
  * the stages of one more update (sgp_ctx_stage_timing; slots as vfe_rows_partial);
  * the largest difference of mean_and_var at 256 test points between the updated and the stacked posterior.
The two N are reported side by side for each n_new; no ratio is asserted.
The create-time cost of keeping the sums: `--create-only [--root DIR]` times sgp_sparse_posterior_create at N = 65 536 with
the libraries of the tree at DIR (default: this one) -- run once on this commit and once with DIR = a built checkout of the
parent, on the same box; `--parent-root DIR` makes the full run do both and record them.
Method as docs/05_measurement.md: wall time around the C call with prebuilt specs, a warm-up, then the median of the repeats.
usage: python tools/vfe_update_bench.py [--out FILE] [--quick] [--reps K] [--parent-root DIR]
       -> profiles/r15_vfe_update.json + a line in profiles/INDEX.md"""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M_IND = 4096
SIZES = [(M_IND, n, k) for k in (128, 1024, 8192) for n in (65536, 262144)]
QUICK_SIZES = [(256, 2048, 128), (256, 8192, 128)]
STAGES = ["buffers (uploads, scratch copy of the sums)", "assembly", "row solve", "transpose + column sums", "Gram",
          "prepare + factor + scalars + copies back"]
OUT_NAME = "r15_vfe_update.json"
INDEX_LINE = ("| **update_posterior, VFE**: sgp_sparse_posterior_update against sgp_sparse_posterior_create on the stacked data, "
              "per-stage times, the two N side by side; M = 4096, N = 65 536 / 262 144 x n_new = 128 / 1024 / 8192; the create "
              "call with and without the kept sums (`tools/vfe_update_bench.py`) | `" + OUT_NAME + "` |")


def _package(root):
    spec = importlib.util.spec_from_file_location("graft_entry_of_" + str(abs(hash(root))), os.path.join(root, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


def _model(P, rng, M, N, D=4):
    f = P.atomic(P.GP(0.2, P.Matern52Kernel()), P.GPC())
    Z = P.ColVecs(np.asfortranarray(rng.standard_normal((D, M))))
    X = np.asfortranarray(rng.standard_normal((D, N)))
    return f, Z, X


def _create(P, ctx, f, Z, x, noise, y):
    """(handle, seconds) of sgp_sparse_posterior_create with prebuilt specs"""
    L = P.lib
    zz, xz, mean_x, nk, nbuf, zk, zbuf = P.finite_gp._vfe_args(P.VFE(f(Z, 1e-6)), f(x, noise))
    y = np.ascontiguousarray(y, dtype=np.float64)
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = ctx.lib.sgp_sparse_posterior_create(ctx.handle, zz.ref(), xz.ref(), L.dptr(mean_x), nk, L.dptr(nbuf), zk, L.dptr(zbuf),
                                             L.dptr(y), C.byref(h))
    dt = time.perf_counter() - t0
    L.check(rc, "sgp_sparse_posterior_create")
    return h, dt


def child_create_only(root, M, N, reps):
    P = _package(root)
    ctx = P.lib.default_context()
    rng = np.random.default_rng(M + N)
    f, Z, X = _model(P, rng, M, N)
    noise, y = 0.1 + rng.random(N), rng.standard_normal(N)
    x = P.ColVecs(X)
    ts = []
    for _ in range(reps + 1):           # (the first repeat is the warm-up)
        h, t = _create(P, ctx, f, Z, x, noise, y)
        ctx.lib.sgp_sparse_posterior_destroy(h)
        ts.append(t * 1e3)
    print("RESULT " + json.dumps(dict(M=M, N=N, reps=reps, create_ms=float(np.median(ts[1:])), min_ms=float(min(ts[1:])),
                                      max_ms=float(max(ts[1:])))))


def child(M, N, k, reps):
    P = _package(ROOT)
    L = P.lib
    ctx = L.default_context()
    upd = ctx.vfe_update
    rng = np.random.default_rng(N + k)
    n_batches = reps + 2                 # warm-up, the repeats, the staged one
    f, Z, X = _model(P, rng, M, N + n_batches * k)
    noise, y = 0.1 + rng.random(X.shape[1]), rng.standard_normal(X.shape[1])
    Xs = P.ColVecs(np.asfortranarray(rng.standard_normal((4, 256))))
    col = lambda a, b: P.ColVecs(np.asfortranarray(X[:, a:b]))   # noqa: E731

    def update(h, a, b):
        x2 = col(a, b)
        xz, _, _ = P.build_spec(f, x2, f, Z)
        var2 = np.ascontiguousarray(P.prior_var(f, x2), dtype=np.float64)
        mean2 = np.ascontiguousarray(P.mean_vector(f, x2), dtype=np.float64)
        nz, yy, out = noise[a:b].copy(), y[a:b].copy(), np.zeros(1)
        t0 = time.perf_counter()
        rc = upd.sgp_sparse_posterior_update(h, xz.ref(), L.dptr(var2), L.dptr(mean2), L.NOISE_DIAG, L.dptr(nz), L.dptr(yy), L.dptr(out))
        dt = time.perf_counter() - t0
        L.check(rc, "sgp_sparse_posterior_update")
        return dt * 1e3

    def predict(h):
        post = P.ApproxPosteriorGP(f, Z, h)
        out = post.mean_and_var(Xs)
        post._h = None                   # (the handle stays ours)
        return out

    h, t_create = _create(P, ctx, f, Z, col(0, N), noise[:N], y[:N])
    t_upd = [update(h, N + r * k, N + (r + 1) * k) for r in range(reps + 1)]
    t_stack = []
    for r in range(3):                   # (the stacked route is the slow one: a warm-up and two repeats)
        h1, t = _create(P, ctx, f, Z, col(0, N + k), noise[:N + k], y[:N + k])
        t_stack.append(t * 1e3)
        if r < 2:
            ctx.lib.sgp_sparse_posterior_destroy(h1)
    # the difference to the stacked posterior: a fresh posterior of N points updated once against h1 (N + k points)
    h2, _ = _create(P, ctx, f, Z, col(0, N), noise[:N], y[:N])
    update(h2, N, N + k)
    a, b = predict(h2), predict(h1)
    diff = dict(mean=float(np.max(np.abs(a[0] - b[0]))), var=float(np.max(np.abs(a[1] - b[1]))))
    ctx.lib.sgp_sparse_posterior_destroy(h1)
    ctx.lib.sgp_sparse_posterior_destroy(h2)
    L.check(ctx.lib.sgp_ctx_stage_timing(ctx.handle, 1), "stage_timing")
    update(h, N + (reps + 1) * k, N + (reps + 2) * k)
    ms = np.zeros(16)
    L.check(ctx.lib.sgp_ctx_stage_ms(ctx.handle, L.dptr(ms)), "stage_ms")
    L.check(ctx.lib.sgp_ctx_stage_timing(ctx.handle, 0), "stage_timing")
    n = C.c_int64(0)
    L.check(upd.sgp_sparse_posterior_count(h, C.byref(n)), "sgp_sparse_posterior_count")
    assert n.value == N + n_batches * k, n.value
    ctx.lib.sgp_sparse_posterior_destroy(h)
    res = dict(M=M, N=N, n_new=k, reps=reps, update_ms=float(np.median(t_upd[1:])), update_min_ms=float(min(t_upd[1:])),
               update_max_ms=float(max(t_upd[1:])), first_create_ms=t_create * 1e3, stacked_create_ms=float(np.median(t_stack[1:])),
               update_over_stacked=float(np.median(t_upd[1:]) / np.median(t_stack[1:])),
               max_abs_diff_mean_and_var_256=diff, stages_of_one_update_ms={STAGES[i]: float(ms[i]) for i in range(len(STAGES))})
    print("RESULT " + json.dumps(res))


def ensure_index_line():
    path = os.path.join(ROOT, "profiles", "INDEX.md")
    txt = open(path).read()
    if OUT_NAME not in txt:
        with open(path, "a") as fh:
            fh.write(("" if txt.endswith("\n") else "\n") + INDEX_LINE + "\n")


def _run_child(args, limit):
    """the child's RESULT record, or a string saying why there is none"""
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], capture_output=True, text=True,
                           timeout=limit)
    except subprocess.TimeoutExpired:
        return f"no result within {limit} s"
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        return f"exit status {p.returncode}: {p.stderr[-600:]}"
    print(line[-1], flush=True)
    return json.loads(line[-1][7:])


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--child":
        return child(int(argv[1]), int(argv[2]), int(argv[3]), int(argv[4]))
    if argv and argv[0] == "--child-create":
        return child_create_only(argv[1], int(argv[2]), int(argv[3]), int(argv[4]))
    out_path = os.path.join(ROOT, "profiles", OUT_NAME)
    reps = 7
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
    quick = "--quick" in argv
    m_c, n_c = (256, 8192) if quick else (M_IND, 65536)
    if "--create-only" in argv:
        root = argv[argv.index("--root") + 1] if "--root" in argv else ROOT
        r = _run_child(["--child-create", os.path.abspath(root), m_c, n_c, reps], 300)
        return 0 if isinstance(r, dict) else 1
    res = dict(what="sgp_sparse_posterior_update against sgp_sparse_posterior_create on the stacked data; see tools/vfe_update_bench.py",
               method="wall time around the C call, prebuilt specs, one warm-up, median (and minimum / maximum) of the repeats; one "
                      "fresh process per configuration", configs=[])
    for M, N, k in (QUICK_SIZES if quick else SIZES):
        limit = 180 + N // 2048
        r = _run_child(["--child", M, N, k, reps], limit)
        if not isinstance(r, dict):
            res["stopped"] = f"M={M} N={N} n_new={k}: {r}; nothing further was started"
            break
        res["configs"].append(r)
    # the two N side by side for each n_new
    side = {}
    for c in res["configs"]:
        side.setdefault(str(c["n_new"]), {})[str(c["N"])] = dict(update_ms=c["update_ms"], min_ms=c["update_min_ms"],
                                                                 max_ms=c["update_max_ms"], stacked_create_ms=c["stacked_create_ms"])
    res["update_ms_by_n_new_then_N"] = side
    if "stopped" not in res:
        keep = dict(text=f"sgp_sparse_posterior_create at M = {m_c}, N = {n_c}: this commit (keeps the sums) and the parent")
        for name, root in (("this_commit", ROOT), ("parent", argv[argv.index("--parent-root") + 1] if "--parent-root" in argv else None)):
            if root is None:
                keep[name] = "not measured (no --parent-root)"
                continue
            r = _run_child(["--child-create", os.path.abspath(root), m_c, n_c, reps], 300)
            keep[name] = r
            if not isinstance(r, dict):
                res["stopped"] = f"create-only ({name}): {r}; nothing further was started"
                break
        res["create_cost_of_keeping_the_sums"] = keep
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    if os.path.abspath(out_path) == os.path.join(ROOT, "profiles", OUT_NAME):
        ensure_index_line()
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
