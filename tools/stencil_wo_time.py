"""Gradients with respect to a stencil's own weights and offsets (include/sthenomi_stencil_wo.h; csrc/stencil.hip:
stencil_wo_kernel, stencil_wo_reduce_kernel): what the two side passes cost beside the assembly and the gradient call they
ride on, and against the only route that existed before -- the same model rebuilt as a sum of `shift` views, Q_r Q_c plain
terms with Q copies of the inputs, through logpdf_and_gradient(inputs=True), whose input gradients per view add up to
-d / d offset.
One box, one process, medians of 7 calls after a warm-up, with min and max; wall time around host calls that end in a copy
back to the host (so every call is complete when the clock stops).  The two configurations of profiles/r17_stencil_grad.json:
  the 15-point quadrature stencil (quadrature_convolve, Matern-5/2), N = 4096, D = 1;
  the 17-point central-difference stencil (SE), N = 4096, D = 8.
At each: cov (sgp_kernelmatrix into a kept host buffer), logpdf_and_gradient_stencil without and with stencils=True,
`ratio` = (with - without) / cov -- the two side passes of the one diagonal pair (row side, column side at the mirrored
address), their reductions and the chain back to the node, in units of one assembly -- and the composed route.
usage: python tools/stencil_wo_time.py [--out FILE] [--quick]      -> JSON on stdout (and in FILE)"""
import hashlib
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
argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
QUICK = "--quick" in argv
REPS = 3 if QUICK else 7
N = 512 if QUICK else 4096


def stat(f, reps=REPS, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)))


def models(kernel, A, w):
    """g = stencil(f, A, w) and fs = sum_q w_q shift(f, a_q): the same process"""
    A = np.atleast_2d(A)

    def build(GP):
        f = GP(kernel())
        fs = w[0] * P.shift(f, A[:, 0])
        for q in range(1, len(w)):
            fs = fs + w[q] * P.shift(f, A[:, q])
        return {"f": f, "g": P.stencil(f, A, w), "fs": fs}
    return P.gppp(build)


def composed_d_offsets(b, A):
    """d logpdf / d a_q from the composed route: minus the sum over the points of the gradient of the view shifted by a_q,
    through that view's kernel input scale (the views are the spec inputs whose warp chain is one Shift)"""
    spec, out = b["_spec"], np.zeros(A.shape)
    cols = {A[:, q].tobytes(): q for q in range(A.shape[1])}
    for k, gk in enumerate(b["inputs"]):
        _, _, chain, kchain, X_raw = spec.input_origin[k]
        (warp, _), = chain
        q = cols[np.asarray(warp.a, dtype=np.float64).tobytes()]
        out[:, q] -= P.kernels.chain_vjp(kchain, X_raw, gk).sum(axis=1) if kchain else gk.sum(axis=1)
    return out


def measure(F, A, X, rng, noise):
    n = X.shape[1]
    y = rng.standard_normal(n)
    fg, fs = F(P.GPPPInput("g", P.ColVecs(X)), noise), F(P.GPPPInput("fs", P.ColVecs(X)), noise)
    r = dict(shape=dict(N=n, D=X.shape[0], Q=int(A.shape[1])))
    sg = P.build_spec(F, fg.x)[0]
    K = np.zeros((n, n), order="F")
    ctx = L.default_context()
    r["cov"] = stat(lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, sg.ref(ctx), L.dptr(K), n), "sgp_kernelmatrix"))
    del K
    r["logpdf_and_gradient_stencil"] = stat(lambda: P.logpdf_and_gradient_stencil(fg, y))
    r["logpdf_and_gradient_stencil, stencils"] = stat(lambda: P.logpdf_and_gradient_stencil(fg, y, stencils=True))
    r["logpdf_and_gradient_stencil, inputs"] = stat(lambda: P.logpdf_and_gradient_stencil(fg, y, inputs=True))
    r["ratio"] = ((r["logpdf_and_gradient_stencil, stencils"]["median_s"] - r["logpdf_and_gradient_stencil"]["median_s"]) /
                  r["cov"]["median_s"])
    r["ratio, inputs (one row-side pass, for comparison)"] = (
        (r["logpdf_and_gradient_stencil, inputs"]["median_s"] - r["logpdf_and_gradient_stencil"]["median_s"]) / r["cov"]["median_s"])
    a, b = P.logpdf_and_gradient_stencil(fg, y, stencils=True), P.logpdf_and_gradient(fs, y, inputs=True)
    (node,) = a["stencils"]
    ref = composed_d_offsets(b, np.atleast_2d(A))
    r["composed_agrees"] = dict(logpdf_rel=abs(a["logpdf"] - b["logpdf"]) / abs(b["logpdf"]),
                                d_offsets_rel=float(np.max(np.abs(node["d_offsets"] - ref)) / np.max(np.abs(ref))),
                                stencil_terms=len(a["terms"]), composed_terms=len(b["terms"]))
    r["composed logpdf_and_gradient, inputs"] = stat(lambda: P.logpdf_and_gradient(fs, y, inputs=True))
    r["composed / stencil"] = (r["composed logpdf_and_gradient, inputs"]["median_s"] /
                               r["logpdf_and_gradient_stencil, stencils"]["median_s"])
    return r


def main():
    rng = np.random.default_rng(0)
    res = dict(note="`ratio`: the row-side and the column-side pass over all N^2 entries of the diagonal pair, Q (1 + D) sums "
                    "each, in units of the assembly of its lower 128 x 128 tiles")
    t_nodes, w_nodes = np.polynomial.hermite.hermgauss(15)
    F = models(lambda: P.with_lengthscale(P.Matern52Kernel(), 0.5), t_nodes[None, :], w_nodes)
    X = np.asfortranarray(rng.uniform(-5.0, 5.0, (1, N)))
    res["15-point quadrature stencil, D = 1"] = measure(F, t_nodes[None, :], X, rng, 0.1)
    print("quadrature: done", file=sys.stderr, flush=True)
    D, h = 8, 1e-2
    A = np.zeros((D, 2 * D + 1))
    wl = np.zeros(2 * D + 1)
    wl[0] = -2.0 * D / h ** 2
    for d in range(D):
        A[d, 1 + 2 * d], A[d, 2 + 2 * d] = h, -h
        wl[1 + 2 * d] = wl[2 + 2 * d] = 1.0 / h ** 2
    F = models(lambda: P.with_lengthscale(P.SEKernel(), 2.0), A, wl)
    X = np.asfortranarray(rng.standard_normal((D, N)))
    res["17-point central-difference stencil, D = 8"] = measure(F, A, X, rng, 0.1)
    res["17-point central-difference stencil, D = 8"]["note"] = (
        "h = 1e-2: weights of 1e4 with alternating signs, so both routes carry the cancellation of a second difference in "
        "float64 and `composed_agrees` shows it; the timings do not depend on it")
    print("central difference: done", file=sys.stderr, flush=True)
    src = os.path.join(ROOT, "stheno.jl_amd", "csrc", "stencil.hip")
    res["build"] = dict(libsthenomi_sha16=hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16],
                        stencil_hip_sha16=hashlib.sha256(open(src, "rb").read()).hexdigest()[:16])
    out = json.dumps(res, indent=1)
    print(out)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
