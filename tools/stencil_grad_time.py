"""Gradients through stencil terms (include/sthenomi_stencil_grad.h; csrc/stencil.hip: stencil_grad_kernel,
stencil_points_kernel, stencil_diag_grad_kernel): what the contraction and the input-point pass cost beside the assembly they
mirror, and against the only route that existed before -- the same model rebuilt as a sum of `shift` views, Q_r Q_c plain
terms with Q copies of the inputs, through logpdf_and_gradient(inputs=True).
One box, one process, medians of 7 calls after a warm-up, with min and max; wall time around host calls that end in a copy
back to the host (so every call is complete when the clock stops).  The two configurations of profiles/stencil_time.json:
  the 15-point quadrature stencil (quadrature_convolve, Matern-5/2), N = 4096, D = 1;
  the 17-point central-difference stencil (SE), N = 4096, D = 8.
At each: cov (sgp_kernelmatrix into a kept host buffer), logpdf, logpdf_and_gradient_stencil with and without inputs,
`ratio` = (gradient - logpdf) / cov -- the contraction (with C^-1, the bordered rows and the copies that the gradient call
adds) in units of one assembly -- and the composed route.  The contraction walks all N^2 entries of the diagonal pair where
the assembly walks its lower tiles only.
usage: python tools/stencil_grad_time.py [--out FILE] [--quick]      -> JSON on stdout (and in FILE)"""
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


def host_gradients(g, v0=1.0):
    """(d / d variance, sum of d_inscale, d / d noise, d / d x) from a gradient record"""
    return (sum(r["d_coef"] * r["coef"] for r in g["terms"]) / v0, sum(r["d_inscale"] for r in g["terms"]), g["noise"], g["x"][0])


def measure(F, X, rng, noise):
    n = X.shape[1]
    y = rng.standard_normal(n)
    fg, fs = F(P.GPPPInput("g", P.ColVecs(X)), noise), F(P.GPPPInput("fs", P.ColVecs(X)), noise)
    r = dict(shape=dict(N=n, D=X.shape[0]))
    # cov: sgp_kernelmatrix into a kept host buffer (the figure of profiles/stencil_time.json: the assembly of the lower tiles,
    # the mirror and the copy of the N x N result); the host function P.cov, which also allocates the result, beside it
    sg = P.build_spec(F, fg.x)[0]
    K = np.zeros((n, n), order="F")
    ctx = L.default_context()
    r["cov"] = stat(lambda: L.check(ctx.lib.sgp_kernelmatrix(ctx.handle, sg.ref(ctx), L.dptr(K), n), "sgp_kernelmatrix"))
    del K
    r["cov, host function"] = stat(lambda: P.cov(fg))
    r["logpdf"] = stat(lambda: P.logpdf(fg, y))
    r["logpdf_and_gradient_stencil"] = stat(lambda: P.logpdf_and_gradient_stencil(fg, y))
    r["logpdf_and_gradient_stencil, inputs"] = stat(lambda: P.logpdf_and_gradient_stencil(fg, y, inputs=True))
    r["ratio"] = (r["logpdf_and_gradient_stencil"]["median_s"] - r["logpdf"]["median_s"]) / r["cov"]["median_s"]
    r["ratio, inputs"] = (r["logpdf_and_gradient_stencil, inputs"]["median_s"] - r["logpdf"]["median_s"]) / r["cov"]["median_s"]
    a, b = P.logpdf_and_gradient_stencil(fg, y, inputs=True), P.logpdf_and_gradient(fs, y, inputs=True)
    ha, hb = host_gradients(a), host_gradients(b)
    rel = lambda p, q: float(np.max(np.abs(np.asarray(p) - np.asarray(q))) / np.max(np.abs(q)))      # noqa: E731
    r["composed_agrees"] = dict(logpdf_rel=abs(a["logpdf"] - b["logpdf"]) / abs(b["logpdf"]), d_variance_rel=rel(ha[0], hb[0]),
                                d_inscale_rel=rel(ha[1], hb[1]), d_noise_rel=rel(ha[2], hb[2]), d_x_rel=rel(ha[3], hb[3]),
                                stencil_terms=len(a["terms"]), composed_terms=len(b["terms"]))
    r["composed logpdf_and_gradient, inputs"] = stat(lambda: P.logpdf_and_gradient(fs, y, inputs=True), reps=3 if QUICK else REPS)
    r["composed logpdf_and_gradient"] = stat(lambda: P.logpdf_and_gradient(fs, y), reps=3 if QUICK else REPS)
    r["composed / stencil, inputs"] = (r["composed logpdf_and_gradient, inputs"]["median_s"] /
                                       r["logpdf_and_gradient_stencil, inputs"]["median_s"])
    r["composed / stencil"] = r["composed logpdf_and_gradient"]["median_s"] / r["logpdf_and_gradient_stencil"]["median_s"]
    return r


def main():
    rng = np.random.default_rng(0)
    res = dict(note="the contraction walks all N^2 entries of the diagonal pair; the assembly (cov, logpdf) walks its lower "
                    "128 x 128 tiles and mirrors them: `ratio` carries that factor of about two")
    # the 15-point quadrature stencil: the nodes and weights of quadrature_convolve(f, 15)
    t_nodes, w_nodes = np.polynomial.hermite.hermgauss(15)
    F = models(lambda: P.with_lengthscale(P.Matern52Kernel(), 0.5), t_nodes[None, :], w_nodes)
    X = np.asfortranarray(rng.uniform(-5.0, 5.0, (1, N)))
    res["15-point quadrature stencil, D = 1"] = measure(F, X, rng, 0.1)
    print("quadrature: done", file=sys.stderr, flush=True)
    # the 17-point central-difference (Laplacian) stencil in 8 dimensions
    D, h = 8, 1e-2
    A = np.zeros((D, 2 * D + 1))
    wl = np.zeros(2 * D + 1)
    wl[0] = -2.0 * D / h ** 2
    for d in range(D):
        A[d, 1 + 2 * d], A[d, 2 + 2 * d] = h, -h
        wl[1 + 2 * d] = wl[2 + 2 * d] = 1.0 / h ** 2
    F = models(lambda: P.with_lengthscale(P.SEKernel(), 2.0), A, wl)
    X = np.asfortranarray(rng.standard_normal((D, N)))
    res["17-point central-difference stencil, D = 8"] = measure(F, X, rng, 0.1)
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
