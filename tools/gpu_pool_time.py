"""Ragged pools against their alternatives: independent logpdf evaluations of DIFFERENT sizes (Matern-5/2, D = 8, different
hyper-parameters and inputs per member), three ways
  loop     one sgp_logpdf call per member,
  grouped  members grouped by padded size, each group of two or more through sgp_logpdf_batch (the rest on their own),
  pool     ONE sgp_logpdf_pool call (include/sthenomi_pool.h: one ragged launch of the dataflow kernel per 16 members)
on four workloads
  equal8   8 members at N = 4096 (sanity: the pool must match sgp_logpdf_batch on the same members)
  curve    a learning curve N = 512, 1024, 2048, 4096, 8192
  series16 16 series with sizes drawn from [1000, 6000] (fixed seed)
  folds8   8 folds at N = 3968 of which one has one tile more (N = 3969)
and, for `curve` and `series16`, value plus gradient (sgp_logpdf_grad / sgp_logpdf_grad_batch / sgp_logpdf_grad_pool).
Specs are prebuilt (host-side spec construction is not in the timed region); after a warm-up pass the variants are timed in
turn, pass after pass, and the medians reported.  Every variant's values are compared bit for bit with the loop's.
usage: python tools/gpu_pool_time.py [--out profiles/r09_pool.json] [--passes 7] [workload ...]
The output file's `headline_guard` entry, if it has one, is kept."""
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
D = 8
_DP = C.POINTER(C.c_double)

args = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "r09_pool.json")
PASSES = 7
while args and args[0].startswith("--"):
    if args[0] == "--out":
        OUT = args[1]
    elif args[0] == "--passes":
        PASSES = int(args[1])
    else:
        raise SystemExit(__doc__)
    args = args[2:]

WORKLOADS = {
    "equal8": [4096] * 8,
    "curve": [512, 1024, 2048, 4096, 8192],
    "series16": [int(n) for n in np.random.default_rng(2024).integers(1000, 6001, size=16)],
    "folds8": [3968] * 7 + [3969],
}
WITH_GRADIENT = ("curve", "series16")
names = args or list(WORKLOADS)


def members(sizes, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for N in sizes:
        ell, s2 = 0.8 + 0.4 * rng.random(), 0.05 + 0.1 * rng.random()
        f = P.atomic(P.GP(P.with_lengthscale(P.Matern52Kernel(), ell)), P.GPC())
        x = np.asfortranarray(rng.standard_normal((D, N)))
        spec = P.build_spec(f, P.ColVecs(x))[0]
        spec.ref()
        nt = max(1, spec.n_terms)
        out.append(dict(spec=spec, N=N, y=np.ascontiguousarray(rng.standard_normal(N)), nz=np.array([s2]),
                        g=[np.zeros(N), np.zeros(N), np.zeros(1), np.zeros(nt), np.zeros(nt)]))
    return out


def ptrs(arrs):
    return (_DP * len(arrs))(*[L.dptr(a) for a in arrs])


class Call:
    """one library call over the members `ids` of `ms`, writing values into out[ids]"""

    def __init__(self, ctx, ms, ids, out, how, grad):
        self.ctx, self.ids, self.out, self.how, self.grad = ctx, ids, out, how, grad
        sub = [ms[i] for i in ids]
        self.sub = sub
        nb = len(sub)
        self.nb = nb
        self.specs = (C.POINTER(L.sgp_cov_spec) * nb)(*[C.pointer(m["spec"].c) for m in sub])
        self.means = ptrs([None] * nb)
        self.noises = ptrs([m["nz"] for m in sub])
        self.ys = ptrs([m["y"] for m in sub])
        self.kinds = (C.c_int * nb)(*[L.NOISE_SCALAR] * nb)
        self.vals = np.zeros(nb)
        self.infos = np.zeros(nb, dtype=np.int32)
        self.g = [ptrs([m["g"][q] for m in sub]) for q in range(5)]
        self.rep = L.sgp_pool_report()

    def __call__(self):
        ctx, ip = self.ctx, self.infos.ctypes.data_as(C.POINTER(C.c_int))
        if self.how == "single":
            m = self.sub[0]
            if self.grad:
                L.check(ctx.lib.sgp_logpdf_grad(ctx.handle, m["spec"].ref(), None, L.NOISE_SCALAR, L.dptr(m["nz"]), L.dptr(m["y"]),
                                                L.dptr(self.vals), *[L.dptr(a) for a in m["g"]]))
            else:
                L.check(ctx.lib.sgp_logpdf(ctx.handle, m["spec"].ref(), None, L.NOISE_SCALAR, L.dptr(m["nz"]), L.dptr(m["y"]),
                                           m["N"], 1, L.dptr(self.vals)))
        elif self.how == "batch":
            if self.grad:
                L.check(ctx.batch.sgp_logpdf_grad_batch(ctx.handle, self.nb, self.specs, self.means, L.NOISE_SCALAR, self.noises,
                                                        self.ys, L.dptr(self.vals), *self.g, ip))
            else:
                L.check(ctx.lib.sgp_logpdf_batch(ctx.handle, self.nb, self.specs, self.means, L.NOISE_SCALAR, self.noises, self.ys,
                                                 L.dptr(self.vals), ip))
        else:
            if self.grad:
                L.check(ctx.pool.sgp_logpdf_grad_pool(ctx.handle, self.nb, self.specs, self.means, self.kinds, self.noises, self.ys,
                                                      L.dptr(self.vals), *self.g, ip, C.byref(self.rep)))
            else:
                L.check(ctx.pool.sgp_logpdf_pool(ctx.handle, self.nb, self.specs, self.means, self.kinds, self.noises, self.ys,
                                                 L.dptr(self.vals), ip, C.byref(self.rep)))
        self.out[self.ids] = self.vals


def variants(ctx, ms, grad):
    n = len(ms)
    outs = {k: np.zeros(n) for k in ("loop", "grouped", "pool")}
    loop = [Call(ctx, ms, [i], outs["loop"], "single", grad) for i in range(n)]
    groups = {}
    for i, m in enumerate(ms):
        groups.setdefault(-(-m["N"] // 128), []).append(i)
    grouped = [Call(ctx, ms, ids, outs["grouped"], "batch" if len(ids) > 1 else "single", grad) for ids in groups.values()]
    pool = [Call(ctx, ms, list(range(n)), outs["pool"], "pool", grad)]
    return {"loop": loop, "grouped": grouped, "pool": pool}, outs, len(groups)


def measure(ctx, ms, grad):
    calls, outs, ngroups = variants(ctx, ms, grad)
    ts = {k: [] for k in calls}
    for p in range(PASSES + 1):          # pass 0: warm-up (allocations, first launches)
        for k, cs in calls.items():
            t0 = time.perf_counter()
            for c in cs:
                c()
            if p:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    rep = calls["pool"][0].rep
    r = {k: dict(ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v))) for k, v in ts.items()}
    r["grouped"]["groups"] = ngroups
    r["pool"]["report"] = dict(pool_launches=rep.pool_launches, pooled_members=rep.pooled_members,
                               single_members=rep.single_members, distinct_sizes=rep.distinct_sizes)
    r["bit_equal_to_loop"] = {k: bool(np.array_equal(outs[k], outs["loop"])) for k in ("grouped", "pool")}
    r["pool_over_loop"] = r["loop"]["ms"] / r["pool"]["ms"]
    r["pool_over_grouped"] = r["grouped"]["ms"] / r["pool"]["ms"]
    return r


res = {"tool": "tools/gpu_pool_time.py", "passes": PASSES, "kernel": "Matern52, D = 8, scalar noise", "workloads": {}}
ctx = L.Context(0)
for name in names:
    sizes = WORKLOADS[name]
    ms = members(sizes, seed=len(name))
    w = dict(sizes=sizes, logpdf=measure(ctx, ms, False))
    if name in WITH_GRADIENT:
        w["logpdf_and_gradient"] = measure(ctx, ms, True)
    res["workloads"][name] = w
    print(name, json.dumps(w), file=sys.stderr)
ctx.close()
if os.path.exists(OUT):
    try:
        old = json.load(open(OUT))
        if "headline_guard" in old:
            res["headline_guard"] = old["headline_guard"]
    except ValueError:
        pass
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
