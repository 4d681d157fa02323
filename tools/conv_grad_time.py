"""Gradients through patch (convolutional) terms (include/sthenomi_conv_grad.h; csrc/conv.hip: conv2_grad_kernel,
conv1_grad_kernel, conv_diag_grad_kernel, conv1_points_kernel): what the contraction costs beside the assembly it mirrors.
One box, one process, medians of 7 calls after a warm-up, with min and max; wall time around host calls that end in a copy
back to the host (so every call is complete when the clock stops).
  28 x 28 images, 3 x 3 patches (P = 676), N = 512 and 1024, M = 256 inducing patches: cov, logpdf,
      logpdf_and_gradient_conv, elbo, elbo_and_gradient_conv (inputs=True);
  8 x 8 images (P = 36), N = 512: the same, and logpdf_and_gradient of the composed model f = sum_p select(g, idx_p) --
      1296 plain terms in the one block pair -- the only route to these derivatives before.
`ratio` = (logpdf_and_gradient_conv - logpdf) / cov: the contraction (with C^-1, the bordered rows and the copies that the
gradient call adds) in units of one assembly of the same entries.
usage: python tools/conv_grad_time.py [--out FILE] [--quick]      -> JSON on stdout (and in FILE)"""
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


def stat(f, reps=REPS, warm=1):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)))


def conv_model(n_patches):
    def build(GP):
        g = GP((1.0 / n_patches) * P.with_lengthscale(P.SEKernel(), 2.0))
        return {"g": g, "f": P.patch_convolve(g)}
    return P.gppp(build)


def composed_model(H, W):
    """the same f as a sum of select views: one plain term per pair of patches"""
    idx = [[(pr + a) + (pc + b) * H for b in range(3) for a in range(3)] for pc in range(W - 2) for pr in range(H - 2)]

    def build(GP):
        g = GP((1.0 / len(idx)) * P.with_lengthscale(P.SEKernel(), 2.0))
        fs = P.select(g, idx[0])
        for ix in idx[1:]:
            fs = fs + P.select(g, ix)
        return {"g": g, "fs": fs}
    return P.gppp(build)


def measure(H, W, n, m, rng, composed):
    Pn = (H - 2) * (W - 2)
    F = conv_model(Pn)
    X = rng.standard_normal((H, W, n))
    x = P.GPPPInput("f", P.ImageVector(X))
    z = P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((9, m)))))
    y = rng.standard_normal(n)
    fx, vfe = F(x, 0.1), P.VFE(F(z, 1e-2))
    r = dict(shape=dict(H=H, W=W, patches=Pn, N=n, M=m))
    r["cov"] = stat(lambda: P.cov(fx))
    r["logpdf"] = stat(lambda: P.logpdf(fx, y))
    r["logpdf_and_gradient_conv"] = stat(lambda: P.logpdf_and_gradient_conv(fx, y))
    r["elbo"] = stat(lambda: P.elbo(vfe, fx, y))
    r["elbo_and_gradient_conv"] = stat(lambda: P.elbo_and_gradient_conv(vfe, fx, y, inputs=True))
    r["ratio"] = (r["logpdf_and_gradient_conv"]["median_s"] - r["logpdf"]["median_s"]) / r["cov"]["median_s"]
    if composed:
        Fc = composed_model(H, W)
        fc = Fc(P.GPPPInput("fs", P.ColVecs(X.reshape(H * W, n, order="F"))), 0.1)
        a, b = P.logpdf_and_gradient_conv(fx, y), P.logpdf_and_gradient(fc, y)
        r["composed_agrees"] = dict(logpdf_rel=abs(a["logpdf"] - b["logpdf"]) / abs(b["logpdf"]),
                                    d_coef_rel=abs(a["terms"][0]["d_coef"] * a["terms"][0]["coef"] -
                                                   sum(t["d_coef"] * t["coef"] for t in b["terms"])) /
                                    abs(a["terms"][0]["d_coef"] * a["terms"][0]["coef"]),
                                    composed_terms=len(b["terms"]))
        r["composed_logpdf_and_gradient"] = stat(lambda: P.logpdf_and_gradient(fc, y), reps=3 if QUICK else REPS)
        r["composed / conv"] = r["composed_logpdf_and_gradient"]["median_s"] / r["logpdf_and_gradient_conv"]["median_s"]
    return r


def main():
    rng = np.random.default_rng(0)
    res = {}
    for (H, W, n, m, composed) in ((8, 8, 512, 256, True), (28, 28, 512, 256, False), (28, 28, 1024, 256, False)):
        if QUICK and H == 28:
            n = 64
        res[f"{H} x {W}, N = {n}"] = measure(H, W, n, m, rng, composed)
        print(f"{H} x {W}, N = {n}: done", file=sys.stderr, flush=True)
    src = os.path.join(ROOT, "stheno.jl_amd", "csrc", "conv.hip")
    res["build"] = dict(libsthenomi_sha16=hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()[:16],
                        conv_hip_sha16=hashlib.sha256(open(src, "rb").read()).hexdigest()[:16])
    out = json.dumps(res, indent=1)
    print(out)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
