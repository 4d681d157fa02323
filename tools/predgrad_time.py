"""mean_and_var of a posterior with its gradients in x* (include/sthenomi_predgrad.h) against the predict call it extends and
against the route there was before it: central differences through 2 D calls of mean_and_var.

Per size, in ONE process, after a warm-up of every call, REPS = 7 rounds that alternate the three routes; medians:
  predict_ms      P.mean_and_var(post(x*))                       -- sgp_posterior_predict / sgp_sparse_posterior_predict
  predgrad_ms     P.mean_and_var_and_gradient(post(x*))          -- sgp_posterior_predict_grad_x / its sparse form
  extra_over_predict = (predgrad - predict) / predict            -- the expectation to check: about one more row solve
  central_differences_ms   2 D calls of P.mean_and_var at x* +- h e_d
Wall time around the calls; every one ends in a device synchronise.  The gradients are compared with the central differences
on the way (largest difference over the largest gradient entry) -- a sanity figure, not the test.

Sizes (N, N*, D): (4096, 128, 2), (16 384, 128, 8), (16 384, 1024, 8) on the exact posterior, and the VFE posterior with M = 4096
inducing points (N = 16 384 data points, N* = 128, D = 8).  One SE atom of lengthscale sqrt(D) / 2, noise 0.1.

usage: python tools/predgrad_time.py [--out FILE] [--quick]
-> profiles/r19_predgrad.json + a line in profiles/INDEX.md"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 7
SIZES = [("exact", 4096, 128, 2, 0), ("exact", 16384, 128, 8, 0), ("exact", 16384, 1024, 8, 0), ("sparse", 16384, 128, 8, 4096)]
QUICK_SIZES = [("exact", 512, 128, 2, 0), ("sparse", 1024, 64, 3, 256)]
FD_H = 2.0 ** -17
INDEX_LINE = ("| **gradients of posterior mean and variance in x\\***: sgp_posterior_predict_grad_x / its sparse form against the "
              "predict call and against central differences through 2 D predict calls, medians of 7 in one process; (N, N\\*, D) = "
              "(4096, 128, 2) / (16 384, 128, 8) / (16 384, 1024, 8) exact, M = 4096 sparse (`tools/predgrad_time.py`) | "
              "`r19_predgrad.json` |")


def setup(P, kind, N, NS, D, M):
    rng = np.random.default_rng(N + NS + D + M)
    gpc = P.GPC()
    F = P.GPPP({"f": P.atomic(P.GP(P.with_lengthscale(P.SEKernel(), np.sqrt(D) / 2.0)), gpc)}, gpc)

    def inp(X):
        return P.GPPPInput("f", P.ColVecs(np.asfortranarray(X)))
    X = rng.standard_normal((D, N))
    y = rng.standard_normal(N)
    Xs = rng.standard_normal((D, NS))
    if kind == "sparse":
        post = P.posterior(P.VFE(F(inp(X[:, :M] + 0.01 * rng.standard_normal((D, M))), 1e-4)), F(inp(X), 0.1), y)
    else:
        post = P.posterior(F(inp(X), 0.1), y)
    return post, inp, Xs


def central_differences(P, post, inp, Xs):
    D = Xs.shape[0]
    dm, dv = np.zeros(Xs.shape), np.zeros(Xs.shape)
    for d in range(D):
        Xp, Xm = Xs.copy(), Xs.copy()
        Xp[d] += FD_H
        Xm[d] -= FD_H
        mp, vp = P.mean_and_var(post(inp(Xp)))
        mm, vm = P.mean_and_var(post(inp(Xm)))
        dm[d], dv[d] = (mp - mm) / (2 * FD_H), (vp - vm) / (2 * FD_H)
    return dm, dv


def measure(P, kind, N, NS, D, M):
    post, inp, Xs = setup(P, kind, N, NS, D, M)
    fxs = post(inp(Xs))
    routes = {"predict": lambda: P.mean_and_var(fxs), "predgrad": lambda: P.mean_and_var_and_gradient(fxs),
              "central_differences": lambda: central_differences(P, post, inp, Xs)}
    t = {k: [] for k in routes}
    outs = {}
    for r in range(REPS + 1):                    # (the first round is the warm-up)
        for name, fn in routes.items():
            t0 = time.perf_counter()
            outs[name] = fn()
            t[name].append(time.perf_counter() - t0)
    g, (dm, dv) = outs["predgrad"], outs["central_differences"]
    res = dict(posterior=kind, N=N, N_star=NS, D=D, reps=REPS)
    if M:
        res["M"] = M
    for name in routes:
        res[name + "_ms"] = float(np.median(t[name][1:]) * 1e3)
        res[name + "_ms_all"] = [round(v * 1e3, 3) for v in t[name][1:]]
    res["extra_over_predict"] = (res["predgrad_ms"] - res["predict_ms"]) / res["predict_ms"]
    res["central_differences_over_predgrad"] = res["central_differences_ms"] / res["predgrad_ms"]
    res["values_bit_equal_to_predict"] = bool(np.array_equal(g["mean"], outs["predict"][0]) and
                                              np.array_equal(g["var"], outs["predict"][1]))
    res["d_mean_vs_central_differences"] = float(np.abs(g["d_mean"][0] - dm).max() / np.abs(g["d_mean"][0]).max())
    res["d_var_vs_central_differences"] = float(np.abs(g["d_var"][0] - dv).max() / np.abs(g["d_var"][0]).max())
    return res


def ensure_index_line():
    path = os.path.join(ROOT, "profiles", "INDEX.md")
    txt = open(path).read()
    if "r19_predgrad.json" not in txt:
        with open(path, "a") as fh:
            fh.write(("" if txt.endswith("\n") else "\n") + INDEX_LINE + "\n")


def main():
    argv = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "r19_predgrad.json")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    import torch
    if not torch.cuda.is_available():
        print("predgrad_time: no GPU here; nothing was measured", file=sys.stderr)
        return 2
    import __graft_entry__ as entry
    P = entry.load_package()
    res = dict(what="mean_and_var with gradients in x* (sgp_posterior_predict_grad_x / sparse) against predict and against central "
                    "differences through 2 D predict calls; see tools/predgrad_time.py",
               method="wall time around the calls (they end in a device synchronise), the three routes alternating in one process, "
                      "one warm-up round, median of 7", configs=[])
    for cfg in (QUICK_SIZES if "--quick" in argv else SIZES):
        r = measure(P, *cfg)
        print("RESULT " + json.dumps(r), flush=True)
        res["configs"].append(r)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:          # (after every size: a later one that runs out of time loses nothing)
            fh.write(json.dumps(res, indent=1) + "\n")
    if os.path.abspath(out_path) == os.path.join(ROOT, "profiles", "r19_predgrad.json"):
        ensure_index_line()
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
