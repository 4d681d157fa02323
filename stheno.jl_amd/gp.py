"""GP node types and affine transformations of the drop-in surface (host side).

Same names and semantics as the reference's Julia surface:
  GP(mean, kernel)                [EXT] AbstractGPs.GP
  GPC, atomic, AtomicGP            /root/reference/src/gp/util.jl:18-25, gp/atomic_gp.jl:11-22
  DerivedGP                        src/gp/derived_gp.jl:7-29
  +, -, *                          src/affine_transformations/addition.jl, product.jl
  compose (the Julia `∘`), stretch, select, periodic, shift   compose.jl:8-127
  additive_gp                      additive_gp.jl:10-29
  cross                            cross.jl:37-45
  stencil, quadrature_convolve     weighted sums of shifted views (the reference's examples/quadrature-convolution,
                                   custom_affine_transformations, differentiation)

Nothing here touches a covariance matrix: the tree is only *described* on the host.  Means are
evaluated on the host (O(N), as SURVEY.md Appendix B prescribes); covariances are flattened
into kernel terms (flatten.py) and evaluated by the HIP library.
"""
from __future__ import annotations

import numpy as np

from .inputs import BlockData, ColVecs, GPPPInput, ImageVector, as_matrix, blocks, is_pair_vector, regroup_pairs
from .kernels import Kernel


# ---- leaf GP ([EXT] AbstractGPs.GP) -----------------------------------------------------------
class GP:
    """GP(kernel) | GP(c::Real, kernel) | GP(meanfunction, kernel)."""

    def __init__(self, *args):
        if len(args) == 1:
            self.mean_spec, self.kernel = None, args[0]
        elif len(args) == 2:
            self.mean_spec, self.kernel = args
        else:
            raise TypeError("GP(kernel) or GP(mean, kernel)")
        if not isinstance(self.kernel, Kernel):
            raise TypeError("GP needs a Kernel")

    def mean_vector(self, x):
        n = len(x)
        m = self.mean_spec
        if m is None:
            return np.zeros(n)
        if isinstance(m, (int, float, np.integer, np.floating)):
            return np.full(n, float(m))
        return _map_points(m, x)


def _map_points(g, x):
    """g.(x): g maps one input (a float, or a D-vector for ColVecs) to a float."""
    if isinstance(x, ColVecs):
        return np.array([float(g(x.X[:, i])) for i in range(len(x))], dtype=np.float64)
    return np.array([float(g(float(v))) for v in np.asarray(x)], dtype=np.float64)


def _is_real(s):
    return isinstance(s, (int, float, np.integer, np.floating))


# ---- bookkeeping (gp/util.jl:18-25) -------------------------------------------------------------
class GPC:
    """GP collection: hands out creation indices; all nodes of one model share one GPC."""

    def __init__(self):
        self.n = 0


class SthenoAbstractGP:
    gpc: GPC
    n: int

    def __call__(self, x, noise=1e-18):
        from .finite_gp import FiniteGP
        return FiniteGP(self, x, noise)

    def __add__(self, other):
        if isinstance(other, SthenoAbstractGP):
            assert self.gpc is other.gpc, "GPs must share a GPC"
            return DerivedGP(("+", self, other), self.gpc)
        return DerivedGP(("+known", other, self), self.gpc)

    def __radd__(self, other):
        return DerivedGP(("+known", other, self), self.gpc)

    def __neg__(self):
        return DerivedGP(("*", -1.0, self), self.gpc)       # product.jl:73

    def __sub__(self, other):
        return self + (-other)

    def __rsub__(self, other):
        return other + (-self)

    def __mul__(self, s):
        if isinstance(s, SthenoAbstractGP):
            raise ValueError("Cannot multiply two GPs together.")  # product.jl:13
        return DerivedGP(("*", s, self), self.gpc)

    __rmul__ = __mul__


class AtomicGP(SthenoAbstractGP):
    def __init__(self, gp, gpc):
        self.gp, self.gpc = gp, gpc
        self.n = gpc.n + 1
        gpc.n += 1


def atomic(gp, gpc):
    return AtomicGP(gp, gpc)


class DerivedGP(SthenoAbstractGP):
    def __init__(self, args, gpc):
        self.args, self.gpc = args, gpc
        self.n = gpc.n + 1
        gpc.n += 1


# ---- input warps (compose.jl:36-127) -----------------------------------------------------------
class Stretch:
    def __init__(self, l):
        self.l = l

    def __call__(self, x):
        if isinstance(x, ColVecs):
            if np.ndim(self.l) == 0:
                return ColVecs(self.l * x.X)
            return ColVecs(np.asarray(self.l, dtype=np.float64) @ x.X)
        return self.l * np.asarray(x, dtype=np.float64)


class Select:
    def __init__(self, idx):
        self.idx = idx

    def __call__(self, x):
        if isinstance(self.idx, (int, np.integer)):
            return np.array(x.X[self.idx, :], dtype=np.float64)
        return ColVecs(x.X[np.asarray(self.idx), :])


class Periodic:
    def __init__(self, f):
        self.f = float(f)

    def __call__(self, x):
        t = (2.0 * np.pi * self.f) * np.asarray(x, dtype=np.float64)
        return ColVecs(np.vstack([np.cos(t), np.sin(t)]))


class Shift:
    def __init__(self, a):
        self.a = a

    def __call__(self, x):
        if isinstance(x, ColVecs):
            a = np.asarray(self.a, dtype=np.float64)
            return ColVecs(x.X - (a[:, None] if a.ndim == 1 else a))
        return np.asarray(x, dtype=np.float64) - self.a


def warp(g, x):
    """g.(x) for the structured warps (fast broadcasts) or any point-wise function."""
    if isinstance(g, (Stretch, Select, Periodic, Shift)):
        return g(x)
    if isinstance(x, ColVecs):
        vals = [g(x.X[:, i]) for i in range(len(x))]
    else:
        vals = [g(float(v)) for v in np.asarray(x)]
    if np.ndim(vals[0]) == 0:
        return np.array(vals, dtype=np.float64)
    return ColVecs(np.stack([np.asarray(v, dtype=np.float64) for v in vals], axis=1))


def compose(f, g):
    """f ∘ g : the DerivedGP f'(x) := f(g(x))."""
    return DerivedGP(("o", f, g), f.gpc)


def stretch(f, l):
    if np.ndim(l) == 1:
        l = np.diag(np.asarray(l, dtype=np.float64))
    return compose(f, Stretch(l))


def select(f, idx):
    return compose(f, Select(idx))


def periodic(f, freq):
    return compose(f, Periodic(freq))


def shift(f, a):
    return compose(f, Shift(a))


def additive_gp(fs, indices=None):
    if indices is None:
        indices = list(range(len(fs)))
    proj = [compose(f, Select(idx)) for f, idx in zip(fs, indices)]
    out = proj[0]
    for p in proj[1:]:
        out = out + p
    return out


def cross(fs):
    fs = list(fs)
    assert len(fs) >= 1 and all(f.gpc is fs[0].gpc for f in fs)
    return DerivedGP(("cross", fs), fs[0].gpc)


# ---- convolutional GPs (the reference's examples/convolutional_gp/script.jl) ----------------------------------------
def patch_convolve(g, image_shape=None, patch_shape=(3, 3)):
    """f = patch_convolve(g): the process f(x) = sum_p g(patch_p(x)) over every patch_shape patch, stride 1, of an image x
    (the convolutional GP, van der Wilk et al. 2017).  Its inputs are images: an ImageVector, or a ColVecs of column-major
    flattened images (then image_shape = (H, W) is required).  Below f, g may carry sums, scalar scales, `+ known` and
    scalar Stretch warps; the kernel's ScaleTransform / with_lengthscale commutes with patch extraction too.  Any other
    warp under f raises NotImplementedError."""
    ph, pw = (int(patch_shape[0]), int(patch_shape[1]))
    if ph < 1 or pw < 1:
        raise ValueError("patch_convolve: patch_shape must be positive")
    shape = None if image_shape is None else (int(image_shape[0]), int(image_shape[1]))
    return DerivedGP(("conv", g, shape, (ph, pw)), g.gpc)


def conv_geometry(f, x):
    """(H, W, ph, pw) of the patch_convolve node f evaluated at the images x"""
    _, _, shape, (ph, pw) = f.args
    if isinstance(x, ImageVector):
        if shape is not None and shape != x.image_shape:
            raise ValueError(f"patch_convolve: images of {x.image_shape} given to a process of {shape} images")
        shape = x.image_shape
    elif not isinstance(x, ColVecs):
        raise TypeError("patch_convolve: the inputs must be an ImageVector or a ColVecs of flattened images")
    if shape is None:
        raise ValueError("patch_convolve: pass image_shape=(H, W) to read flattened images from a ColVecs")
    H, W = shape
    if as_matrix(x).shape[0] != H * W:
        raise ValueError(f"patch_convolve: inputs of dimension {as_matrix(x).shape[0]} are not {H} x {W} images")
    if ph > H or pw > W:
        raise ValueError("patch_convolve: the patch is larger than the image")
    return (H, W, ph, pw)


def extract_patches(x, patch_shape=(3, 3), image_shape=None):
    """[ColVecs of patch (p, q) of every image]: patch (p, q) of image n is X[p:p+ph, q:q+pw, n] flattened column-major,
    listed p-major as the reference example's comprehension `for p in ... for q in ...` lists them."""
    ph, pw = patch_shape
    if isinstance(x, ImageVector):
        H, W = x.image_shape
    elif image_shape is not None:
        H, W = image_shape
    else:
        raise ValueError("extract_patches: pass image_shape=(H, W) for a ColVecs of flattened images")
    X = as_matrix(x).reshape(H, W, -1, order="F")
    n = X.shape[2]
    return [ColVecs(X[p:p + ph, q:q + pw, :].reshape(ph * pw, n, order="F"))
            for p in range(H - ph + 1) for q in range(W - pw + 1)]


# ---- stencils: weighted sums of shifted views ----------------------------------------------------------------------
def stencil(f, offsets, weights):
    """g = stencil(f, A, w): the process g(x) = sum_q w[q] f(x - A[:, q]) (the sign of `shift`).  `offsets` is a length-Q
    vector for scalar inputs or a D x Q matrix for ColVecs; `weights` a finite length-Q vector, Q >= 1.  The reference's
    examples/quadrature-convolution (`quadrature_convolve`), custom_affine_transformations (f(x) + f(x + 3):
    stencil(f, [0, -3], [1, 1])) and differentiation (central differences) are such sums.  The library assembles one
    term per pair of paths (include/sthenomi_stencil.h) instead of Q^2 terms of shifted copies."""
    w = np.array(weights, dtype=np.float64)
    if w.ndim != 1 or w.shape[0] < 1:
        raise ValueError("stencil: weights must be a vector of length Q >= 1")
    A = np.array(offsets, dtype=np.float64)
    if A.ndim == 1:
        A = A.reshape(1, -1)
    if A.ndim != 2 or A.shape[1] != w.shape[0]:
        raise ValueError("stencil: offsets must be a length-Q vector or a D x Q matrix, Q = length(weights)")
    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(A))):
        raise ValueError("stencil: offsets and weights must be finite")
    return DerivedGP(("stencil", f, A, w), f.gpc)


def quadrature_convolve(f, num_points=15):
    """the reference example's `convolve(f)` (examples/quadrature-convolution/script.jl): Gauss-Hermite quadrature of
    int exp(-t^2) f(x - t) dt with num_points nodes, on 1-D inputs -- stencil(f, t, w) with t, w = hermgauss(num_points)"""
    t, w = np.polynomial.hermite.hermgauss(int(num_points))
    return stencil(f, t, w)


# ---- derivative processes -------------------------------------------------------------------------------------------
def derivative(f, dim=0):
    """g = derivative(f, dim): the process g(x) = d f(x) / d x[dim], exactly -- the covariances of f and g are kappa' and
    kappa'' of f's kernel times coordinate differences, one closed-form evaluation per entry (include/sthenomi.h: the
    SGP_DERIV kinds), where the reference's examples/differentiation/script.jl takes a finite difference.  `dim` counts
    the coordinates of the inputs g is evaluated at (0 for scalar inputs).

    Below g, f may carry sums, scalar scales, `+ constant`, Shift, Stretch and Select warps (a direction that is no longer
    axis-aligned in the kernel's coordinates expands into one term per coordinate; a coordinate a Select drops removes
    the term), and kernels that are SE, Matern-3/2 or Matern-5/2, sums and scalings of these, under ScaleTransform /
    ARDTransform / LinearTransform / SelectTransform / with_lengthscale.  Everything else raises NotImplementedError that
    names the derivative: a function-valued scale, Periodic, a second derivative on one side, patch_convolve or stencil
    above or below, a nested GPPP, products of kernels and every other kernel, and a callable prior mean (a constant mean
    differentiates to 0)."""
    if not isinstance(dim, (int, np.integer)) or dim < 0:
        raise ValueError("derivative: dim must be a non-negative integer")
    return DerivedGP(("deriv", f, int(dim)), f.gpc)


def _deriv_mean(f, x):
    """mean(derivative(f), x): 0 where every mean below the node is a constant; a callable one is refused"""
    from .gppp import GPPP
    if isinstance(f, GPPP):
        raise NotImplementedError("derivative of a nested GPPP is not supported")
    if isinstance(f, AtomicGP):
        if not isinstance(f.gp, GP):
            raise NotImplementedError("derivative of a nested GPPP is not supported")
        m = f.gp.mean_spec
        if m is not None and not _is_real(m):
            raise NotImplementedError("derivative: a callable prior mean below the node cannot be differentiated (a constant "
                                      "mean differentiates to 0)")
        return np.zeros(len(x))
    op = f.args[0]
    if op == "+":
        return _deriv_mean(f.args[1], x) + _deriv_mean(f.args[2], x)
    if op == "+known":
        if not _is_real(f.args[1]):
            raise NotImplementedError("derivative: a known function added below the node cannot be differentiated (a "
                                      "constant differentiates to 0)")
        return _deriv_mean(f.args[2], x)
    if op == "*":
        if not _is_real(f.args[1]):
            raise NotImplementedError("derivative: a function-valued scale below the node is not supported")
        return _deriv_mean(f.args[2], x)
    if op == "o":
        if not isinstance(f.args[2], (Stretch, Select, Shift)):
            raise NotImplementedError("derivative: only Shift, Stretch and Select warps are supported below the node")
        return _deriv_mean(f.args[1], x)
    raise NotImplementedError(f"derivative over `{op}` is not supported")


# ---- prior mean (host, O(N) per node) ----------------------------------------------------------
def mean_vector(f, x):
    """mean(f, x) by the reference's recursion (addition.jl:26,73-74; product.jl:25,54;
    compose.jl:16; cross.jl:54-57; atomic_gp.jl:28)."""
    from .gppp import GPPP, extract_components
    if isinstance(f, GPPP):
        node, v = extract_components(f, x)
        return mean_vector(node, v)
    if is_pair_vector(x):     # pairs on their way to a nested programme: regrouped by key (gppp.jl:32-43), as flatten.block_list does
        x = regroup_pairs(x)
    if isinstance(x, BlockData) and not (isinstance(f, DerivedGP) and f.args[0] == "cross"):
        # BlockData is an ordinary AbstractVector for any GP: the same process on each block
        return np.concatenate([mean_vector(f, b) for b in blocks(x)]) if len(blocks(x)) else np.zeros(0)
    if isinstance(f, AtomicGP):
        if isinstance(f.gp, GP):
            return f.gp.mean_vector(x)
        return mean_vector(f.gp, x)          # a wrapped GPPP / other Stheno GP
    op = f.args[0]
    if op == "+":
        return mean_vector(f.args[1], x) + mean_vector(f.args[2], x)
    if op == "+known":
        b = f.args[1]
        return (float(b) if _is_real(b) else _map_points(b, x)) + mean_vector(f.args[2], x)
    if op == "*":
        s = f.args[1]
        return (float(s) if _is_real(s) else _map_points(s, x)) * mean_vector(f.args[2], x)
    if op == "o":
        return mean_vector(f.args[1], warp(f.args[2], x))
    if op == "conv":
        H, W, ph, pw = conv_geometry(f, x)
        out = np.zeros(len(x))
        for xp in extract_patches(x, (ph, pw), (H, W)):
            out = out + mean_vector(f.args[1], xp)
        return out
    if op == "stencil":
        _, g, A, w = f.args
        out = np.zeros(len(x))
        for q in range(len(w)):
            out = out + w[q] * mean_vector(g, warp(Shift(A[:, q] if isinstance(x, ColVecs) else A[0, q]), x))
        return out
    if op == "deriv":
        return _deriv_mean(f.args[1], x)
    if op == "cross":
        return np.concatenate([mean_vector(g, b) for g, b in zip(f.args[1], blocks(x))])
    raise ValueError(op)
