"""The bits of the covariance assembly: one line per call with a SHA-256 over that call's output.

Two builds assemble alike exactly when their lists are equal line for line -- run it on this checkout and with --root on a built
checkout of another commit (profiles/r25_asm_frame_bits.txt: this commit and its parent).

Per term class (classes(): plain at D = 1, 3, 17, 70, plain then chain, chain first, stencil, one- and two-sided patch,
derivative, derivative after plain, a pair without terms -- for each class a pair whose FIRST launch is of that class, so that
Sigma_y enters through each kernel) and per layout of blocks
  (70,)              one partial tile
  (128,)             the aligned 16-byte store; with noise, that store with Sigma_y
  (256,)             the triangular launch of a square window on the diagonal
  (129, 1, 128, 70)  pairs that begin at rows 129, 130 and 258: shared tiles, odd and even offsets, never the aligned store
the calls
  prior_cov(F, x)                        the full matrix, no noise
  prior_cov(F, x_I, x_J) for every I, J  rectangular windows (and whether it equals block [I, J] of the full matrix)
  logpdf with a scalar and a diagonal noise, rand with a fixed Z: lower tiles only, Sigma_y, padding

usage: python tools/assembly_bits.py [--root DIR]"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ((70,), (128,), (256,), (129, 1, 128, 70))


def load(root):
    pkg_dir = os.path.join(root, "stheno.jl_amd")
    spec = importlib.util.spec_from_file_location("stheno_jl_amd", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    P = importlib.util.module_from_spec(spec)
    sys.modules["stheno_jl_amd"] = P
    spec.loader.exec_module(P)
    return P


def classes(P):
    """name -> (gppp model, the processes its blocks cycle through, input dimension or "images", launches of a diagonal pair)"""
    wl, SE, M32, M52 = P.with_lengthscale, P.SEKernel, P.Matern32Kernel, P.Matern52Kernel
    rng = np.random.default_rng(1)
    A, w = 0.5 * rng.standard_normal((3, 5)), rng.standard_normal(5)
    one = lambda k: P.gppp(lambda GP: {"f": GP(k)})
    derived = lambda make: P.gppp(lambda GP: (lambda f: {"f": f, "g": make(f)})(GP(1.7 * wl(SE(), 0.9))))
    return {
        "plain D=1": (one(1.7 * wl(SE(), 0.9)), ("f",), 1, 1),
        "plain D=3": (one(1.7 * wl(SE(), 0.9) + 0.4 * M52()), ("f",), 3, 1),
        "plain D=17 three terms": (one(SE() + 0.5 * M32() + 0.3 * wl(M52(), 0.7)), ("f",), 17, 2),   # two terms per launch
        "plain D=70 two terms": (one(SE() + 0.5 * M32()), ("f",), 70, 2),                               # one term per launch
        "plain then chain": (one(0.4 * M52() + 1.3 * wl(SE(), 1.3) * M32()), ("f",), 3, 2),
        "chain first": (one(1.3 * wl(SE(), 1.3) * M32() + 0.2 * P.RationalQuadraticKernel(0.7)), ("f",), 3, 1),
        "stencil": (derived(lambda f: P.stencil(f, A, w)), ("g",), 3, 1),
        "patch": (derived(lambda f: P.patch_convolve(f, patch_shape=(2, 2))), ("g", "f"), "images", 1),
        "derivative": (derived(lambda f: P.derivative(f, 1)), ("g",), 3, 1),
        "derivative after plain": (derived(lambda f: f + P.derivative(f, 1)), ("g",), 3, 2),
        "no terms": (P.gppp(lambda GP: {"f": GP(SE()), "u": GP(M32())}), ("f", "u"), 3, 1),
    }


def blocks(P, procs, D, layout, seed):
    """one GPPPInput per block: the processes in turn; "images": 4 x 4 images for the patched process g (2 x 2 patches), points
    of the patch dimension 4 for f"""
    rng = np.random.default_rng(seed)
    out = []
    for b, n in enumerate(layout):
        name = procs[b % len(procs)]
        if D == "images":
            x = P.ImageVector(rng.standard_normal((4, 4, n))) if name == "g" else P.ColVecs(np.asfortranarray(rng.standard_normal((4, n))))
        else:
            X = np.asfortranarray(rng.uniform(-2.0, 2.0, (D, n)) / np.sqrt(D))
            x = X[0].copy() if D == 1 else P.ColVecs(X)
        out.append(P.GPPPInput(name, x))
    return out


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float64)
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    argv = sys.argv[1:]
    P = load(os.path.abspath(argv[argv.index("--root") + 1]) if "--root" in argv else ROOT)
    for name, (F, procs, D, _) in classes(P).items():
        for layout in LAYOUTS:
            tag = f"{name} {layout}"
            ins = blocks(P, procs, D, layout, seed=len(layout) + layout[0])
            x = P.BlockData(ins)
            N = len(x)
            K = P.prior_cov(F, x)
            print(tag, "prior_cov", sha(K))
            off = np.concatenate([[0], np.cumsum(layout)])
            for I in range(len(layout)):
                for J in range(len(layout)):
                    Kc = P.prior_cov(F, ins[I], ins[J])
                    same = np.array_equal(Kc, K[off[I]:off[I + 1], off[J]:off[J + 1]])
                    print(tag, f"prior_cov[{I},{J}]", sha(Kc), "== its block of the full matrix" if same else "!= its block of the full matrix")
            rng = np.random.default_rng(N)
            y, Z = rng.standard_normal(N), rng.standard_normal((N, 3))
            for kind, s in (("scalar", 0.3), ("diag", 0.1 + rng.random(N))):
                print(tag, "logpdf", kind, sha(P.logpdf(F(x, s), y)))
                print(tag, "rand", kind, sha(P.rand(None, F(x, s), 3, Z=Z)))


if __name__ == "__main__":
    main()
