"""rand / logpdf of a posterior FiniteGP: the device route (include/sthenomi_postfx.h) against the host round trip it replaces,
on one box in one run.

For (N, N*) in {(4096, 2048), (16384, 8192)} -- N training points of the 3-process @gppp sum model, N* test points in two
blocks of two processes, S* a scalar -- each size in a fresh child process under its own time limit (a size that fails or
overruns ends the run: nothing more is started on the GPU):
  * host route, spelled out through public calls: post.cov(x*), post.mean(x*), S* added in NumPy, the zero-term spec with the
    sum as dense noise, sgp_logpdf / sgp_rand;
  * device route: P.logpdf(post(x*, s), y*) / P.rand(rng, post(x*, s), 4), which reach sgp_posterior_logpdf / _rand;
  * both for logpdf of one y* and for rand at S = 4, alternating, one warm-up, then the median of the repeats;
  * whether the two routes gave the same bits at that size (np.array_equal).
Method as docs/05_measurement.md: wall time around calls that end in a device synchronise, profiler off.

The bytes of host <-> device copies come from runs of their own under `rocprofv3 --memory-copy-trace` (no counters, no other
tracing; the program after `--`, the whole under `timeout`): per size one run that only builds the posterior, one that adds one
logpdf and one rand by the host route, one that adds them by the device route; a route's bytes are its run's minus the first's, per direction
as the profiler labels it (it files the host route's download of the covariance into pageable memory under device_to_device:
compare with the 8 N*^2 bytes of that matrix, recorded next to the figures).

usage: python tools/postfx_time.py [--out FILE] [--quick] [--reps K] [--no-copies] [--trace-dir DIR]
       python tools/postfx_time.py --parse RESULTS.json        (bytes per direction of one trace file)
-> profiles/r11_postfx.json + a line in profiles/INDEX.md"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(4096, 2048), (16384, 8192)]
QUICK_SIZES = [(512, 300)]
S_RAND, NOISE_STAR = 4, 0.05
INDEX_LINE = ("| **rand / logpdf of a posterior FiniteGP**: the device route (sgp_posterior_logpdf / _rand) against the host round "
              "trip through post.cov + dense noise, medians and host <-> device bytes (rocprofv3 --memory-copy-trace); (N, N*) = "
              "(4096, 2048) / (16 384, 8192), logpdf and rand at S = 4 (`tools/postfx_time.py`) | `r11_postfx.json` |")


def setup(N, NS):
    import __graft_entry__ as entry
    P = entry.load_package()
    rng = np.random.default_rng(N + NS)
    D = 4
    F = P.gppp_sum_model()

    def inp(name, n):
        return P.GPPPInput(name, P.ColVecs(np.asfortranarray(rng.standard_normal((D, n)))))
    x = inp("f3", N)
    xs = P.BlockData([inp("f1", NS // 2), inp("f3", NS - NS // 2)])
    y = rng.standard_normal(N)
    ys = rng.standard_normal(NS)
    Z = np.asfortranarray(rng.standard_normal((NS, S_RAND)))
    post = P.posterior(F(x, 0.1), y)
    return P, post, xs, ys, Z


def host_route(P, post, xs, ys, Z, what):
    """today's route through public calls"""
    from stheno_jl_amd.flatten import zero_spec
    L = P.lib
    ctx = L.default_context()
    n = len(xs)
    Cm = np.asfortranarray(post.cov(xs) + P.finite_gp._noise_dense(NOISE_STAR, n))
    m = np.ascontiguousarray(post.mean(xs), dtype=np.float64)
    spec = zero_spec(n)
    if what == "logpdf":
        Y = np.asfortranarray(ys.reshape(n, 1))
        out = np.zeros(1)
        L.check(ctx.lib.sgp_logpdf(ctx.handle, spec.ref(), L.dptr(m), L.NOISE_DENSE, L.dptr(Cm), L.dptr(Y), n, 1, L.dptr(out)),
                "sgp_logpdf")
        return out
    out = np.zeros(Z.shape, order="F")
    L.check(ctx.lib.sgp_rand(ctx.handle, spec.ref(), L.dptr(m), L.NOISE_DENSE, L.dptr(Cm), L.dptr(Z), n, Z.shape[1], L.dptr(out), n),
            "sgp_rand")
    return out


def device_route(P, post, xs, ys, Z, what):
    if what == "logpdf":
        return np.array([P.logpdf(post(xs, NOISE_STAR), ys)])
    return P.rand(None, post(xs, NOISE_STAR), Z.shape[1], Z=Z)


def child(N, NS, reps):
    P, post, xs, ys, Z = setup(N, NS)
    assert P.finite_gp._postfx_route(post(xs, NOISE_STAR)) is not None
    res = dict(N=N, N_star=NS, reps=reps, S=S_RAND)
    for what in ("logpdf", "rand"):
        t = {"host": [], "device": []}
        same = True
        for r in range(reps + 1):            # (the first repeat is the warm-up)
            outs = {}
            for route, fn in (("host", host_route), ("device", device_route)):
                t0 = time.perf_counter()
                outs[route] = fn(P, post, xs, ys, Z, what)
                t[route].append(time.perf_counter() - t0)
            same = same and bool(np.array_equal(outs["host"], outs["device"]))
        key = what if what == "logpdf" else f"rand_S{S_RAND}"
        res[key] = dict(host_route_ms=float(np.median(t["host"][1:]) * 1e3), device_route_ms=float(np.median(t["device"][1:]) * 1e3),
                        host_route_ms_all=[round(v * 1e3, 3) for v in t["host"][1:]],
                        device_route_ms_all=[round(v * 1e3, 3) for v in t["device"][1:]], bit_equal=same)
        res[key]["device_over_host"] = res[key]["device_route_ms"] / res[key]["host_route_ms"]
    print("RESULT " + json.dumps(res))


def copies_child(kind, N, NS):
    """what one traced run does: the posterior, then (host / device) one logpdf and one rand by that route"""
    P, post, xs, ys, Z = setup(N, NS)
    fn = {"base": None, "host": host_route, "device": device_route}[kind]
    if fn is not None:
        fn(P, post, xs, ys, Z, "logpdf")
        fn(P, post, xs, ys, Z, "rand")
    print("COPIES_DONE " + kind)


# rocprofiler_memory_copy_operation_t
COPY_OPS = {0: "none", 1: "host_to_host", 2: "host_to_device", 3: "device_to_host", 4: "device_to_device"}


def _find_lists(node, key, found):
    if isinstance(node, dict):
        for k, v in node.items():
            if k == key and isinstance(v, list):
                found.append(v)
            else:
                _find_lists(v, key, found)
    elif isinstance(node, list):
        for v in node:
            _find_lists(v, key, found)


def parse_trace(path):
    """bytes and copies per direction of a rocprofv3 --memory-copy-trace JSON result"""
    doc = json.load(open(path))
    lists = []
    _find_lists(doc, "memory_copy", lists)
    recs = [r for lst in lists for r in lst if isinstance(r, dict) and "bytes" in r]
    names = []
    _find_lists(doc, "operations", names)
    table = next((ops for ops in names if any("HOST_TO_DEVICE" in str(o) for o in ops)), None)
    out = {}
    for r in recs:
        op = r.get("operation", -1)
        name = COPY_OPS.get(op, str(op))
        if table is not None and isinstance(op, int) and 0 <= op < len(table):
            name = str(table[op]).lower().replace("memory_copy_", "")
        d = out.setdefault(name, dict(bytes=0, copies=0))
        d["bytes"] += int(r["bytes"])
        d["copies"] += 1
    return out


def trace_one(kind, N, NS, trace_dir, limit):
    name = f"postfx_{kind}_{N}_{NS}"
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--memory-copy-trace", "-f", "json", "-d", trace_dir, "-o", name, "--",
           sys.executable, os.path.abspath(__file__), "--copies-child", kind, str(N), str(NS)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0 or f"COPIES_DONE {kind}" not in p.stdout:
        return None, f"{name}: exit status {p.returncode}: {(p.stderr or p.stdout)[-600:]}"
    hits = [os.path.join(d, f) for d, _, fs in os.walk(trace_dir) for f in fs if f.startswith(name) and f.endswith("_results.json")]
    if not hits:
        return None, f"{name}: no *_results.json under {trace_dir}"
    try:
        return parse_trace(hits[0]), None
    except Exception as e:   # the trace stays on disk for --parse
        return None, f"{name}: {hits[0]} could not be read: {e!r}"


def route_bytes(runs):
    """per route and direction (the profiler's labels), its traced run minus the run that only builds the posterior"""
    out = {}
    for kind in ("host", "device"):
        dirs = sorted(set(runs[kind]) | set(runs["base"]))
        d = {k: runs[kind].get(k, {}).get("bytes", 0) - runs["base"].get(k, {}).get("bytes", 0) for k in dirs}
        d["all_directions"] = sum(d.values())
        out[kind + "_route"] = d
    return out


def copies(N, NS, trace_dir):
    limit = 240 + N // 64
    runs = {}
    for kind in ("base", "host", "device"):
        runs[kind], err = trace_one(kind, N, NS, trace_dir, limit)
        if err:
            return dict(error=err + "; nothing further was started")
    out = dict(traced_runs=runs, one_logpdf_and_one_rand=route_bytes(runs))
    # what the host route must move for one logpdf and one rand: cov down and cov + S* up, twice
    out["n_star_squared_matrix_bytes"] = 8 * NS * NS
    return out


def ensure_index_line():
    path = os.path.join(ROOT, "profiles", "INDEX.md")
    txt = open(path).read()
    if "r11_postfx.json" not in txt:
        with open(path, "a") as fh:
            fh.write(("" if txt.endswith("\n") else "\n") + INDEX_LINE + "\n")


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--child":
        return child(int(argv[1]), int(argv[2]), int(argv[3]))
    if argv and argv[0] == "--copies-child":
        return copies_child(argv[1], int(argv[2]), int(argv[3]))
    if argv and argv[0] == "--parse":
        print(json.dumps(parse_trace(argv[1]), indent=1))
        return 0
    out_path = os.path.join(ROOT, "profiles", "r11_postfx.json")
    trace_dir = None
    reps = 5
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    if "--reps" in argv:
        reps = int(argv[argv.index("--reps") + 1])
    if "--trace-dir" in argv:
        trace_dir = argv[argv.index("--trace-dir") + 1]
    if trace_dir is None and "--no-copies" not in argv:
        trace_dir = tempfile.mkdtemp(prefix="postfx_trace_")
    sizes = QUICK_SIZES if "--quick" in argv else SIZES
    res = dict(what="rand / logpdf of a posterior FiniteGP: sgp_posterior_logpdf / _rand against the host round trip; see "
                    "tools/postfx_time.py",
               method="wall time around the calls (they end in a device synchronise), routes alternating in one process, one "
                      "warm-up, median of the repeats; one fresh process per size; copy bytes from rocprofv3 --memory-copy-trace "
                      "runs of their own, a route's run minus a run that only builds the posterior",
               noise_star=NOISE_STAR, configs=[])
    for N, NS in sizes:
        limit = 240 + N // 64
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N), str(NS), str(reps)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"N={N} N*={NS}: no result within {limit} s; nothing further was started"
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            res["stopped"] = f"N={N} N*={NS}: exit status {p.returncode}; nothing further was started: {p.stderr[-600:]}"
            break
        cfg = json.loads(line[-1][7:])
        print(line[-1], flush=True)
        if "--no-copies" not in argv:
            cfg["copied_bytes"] = copies(N, NS, trace_dir)
            print("COPIES " + json.dumps(cfg["copied_bytes"]), flush=True)
            if "error" in cfg["copied_bytes"]:
                res["configs"].append(cfg)
                res["stopped"] = cfg["copied_bytes"]["error"]
                break
        res["configs"].append(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    if os.path.abspath(out_path) == os.path.join(ROOT, "profiles", "r11_postfx.json"):
        ensure_index_line()
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
