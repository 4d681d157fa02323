"""The bits of every way of asking a kept posterior something: one line per call with a SHA-256 over that call's outputs.

Two builds answer alike exactly when their lists are equal line for line -- run it on this checkout and with --root on a built
checkout of another commit (profiles/r24_kept_bits.txt: this commit and its parent).

Model: f1 ~ SE, f2 ~ Matern32, f3 = f1 + f2 on D = 2 inputs; training data in two blocks (f3, f1) of N points in all,
N in {200, 256} (inside a tile, on a tile edge); M = 130 inducing points of f3; test points in two blocks (f2, f3), N* in
{1, 128, 150}.  Per N, for the exact and the VFE posterior, and again after one update_posterior with 20 new points:
  mean, var, cov, mean_and_var, mean_and_cov, cov(xs, zs)
  rand with a fixed Z (3 columns) and logpdf of post(x*, noise) for a scalar, a diagonal and a dense noise
  mean_and_var_and_gradient
and the first six for an ExplicitPosteriorGP conditioned on the VFE posterior, before and after that update.

usage: python tools/posterior_bits.py [--root DIR]"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
root = os.path.abspath(argv[argv.index("--root") + 1]) if "--root" in argv else ROOT

pkg_dir = os.path.join(root, "stheno.jl_amd")
spec = importlib.util.spec_from_file_location("stheno_jl_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
P = importlib.util.module_from_spec(spec)
sys.modules["stheno_jl_amd"] = P
spec.loader.exec_module(P)

D, M, N_NEW = 2, 130, 20
N_TRAIN, N_STAR = (200, 256), (1, 128, 150)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float64)
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def blocks(rng, names, sizes):
    return P.BlockData([P.GPPPInput(k, P.ColVecs(np.asfortranarray(rng.uniform(-2, 2, (D, n))))) for k, n in zip(names, sizes)])


def noises(n):
    rng = np.random.default_rng(n + 7)
    B = rng.standard_normal((n, 3))
    return {"scalar": 0.3, "diag": 0.1 + rng.random(n), "dense": 0.2 * np.eye(n) + 0.05 * B @ B.T}


def moments(tag, post, xs, zs):
    print(tag, "mean", sha(post.mean(xs)))
    print(tag, "var", sha(post.var(xs)))
    print(tag, "cov", sha(post.cov(xs)))
    print(tag, "mean_and_var", sha(*post.mean_and_var(xs)))
    print(tag, "mean_and_cov", sha(*post.mean_and_cov(xs)))
    print(tag, "cov_xs_zs", sha(post.cov(xs, zs)))


def reads(tag, post, xs, zs):
    moments(tag, post, xs, zs)
    n = len(xs)
    rng = np.random.default_rng(n)
    Z, y = rng.standard_normal((n, 3)), rng.standard_normal(n)
    for kind, s in noises(n).items():
        print(tag, "rand", kind, sha(P.rand(None, post(xs, s), 3, Z=Z)))
        print(tag, "logpdf", kind, sha(P.logpdf(post(xs, s), y)))
    g = P.mean_and_var_and_gradient(post(xs, 0.3))
    print(tag, "mean_and_var_and_gradient", sha(g["mean"], g["var"], *g["d_mean"], *g["d_var"]))


def main():
    F = P.gppp(lambda GP: (lambda f1, f2: {"f1": f1, "f2": f2, "f3": f1 + f2})(GP(P.SEKernel()), GP(P.Matern32Kernel())))
    for N in N_TRAIN:
        rng = np.random.default_rng(N)
        x = blocks(rng, ("f3", "f1"), (N - N // 3, N // 3))
        y = rng.standard_normal(N)
        z = blocks(rng, ("f3",), (M,))
        x_new = blocks(rng, ("f3",), (N_NEW,))
        y_new = rng.standard_normal(N_NEW)
        star = {n: ((blocks(rng, ("f2", "f3"), (n // 2, n - n // 2)) if n > 1 else blocks(rng, ("f3",), (1,))), blocks(rng, ("f1",), (5,))) for n in N_STAR}
        posts = {"dense": P.posterior(F(x, 0.1), y), "vfe": P.posterior(P.VFE(F(z, 1e-6)), F(x, 0.1), y)}
        for kind, post in posts.items():
            for n, (xs, zs) in star.items():
                reads(f"N={N} {kind} N*={n}", post, xs, zs)
        ex = P.posterior(posts["vfe"](x_new, 0.1), y_new)
        for n, (xs, zs) in star.items():
            moments(f"N={N} explicit-on-vfe N*={n}", ex, xs, zs)
        x2 = blocks(rng, ("f1",), (N_NEW,))
        for kind, post in posts.items():
            new = P.update_posterior(post, F(x_new, 0.1), y_new)
            for n, (xs, zs) in star.items():
                reads(f"N={N} {kind} updated N*={n}", new, xs, zs)
            if kind == "vfe":
                ex = P.posterior(new(x2, 0.1), y_new)
                for n, (xs, zs) in star.items():
                    moments(f"N={N} explicit-on-vfe updated N*={n}", ex, xs, zs)


if __name__ == "__main__":
    main()
