"""Kernel descriptions of the drop-in surface (the KernelFunctions.jl names Stheno re-exports,
/root/reference/src/Stheno.jl:4-6).  Pure descriptions: no arithmetic happens here -- a kernel
expands into (kind, coef, param, input_chain) leaf terms that the HIP assembly kernel
evaluates (stheno.jl_amd/csrc/kernelmatrix.hip).  `input_chain` is the kernel-level input
transformation (KernelFunctions `TransformedKernel`): a tuple of steps applied to the raw points in
order -- ("scale", s) for ScaleTransform(s) / with_lengthscale, ("periodic", f) for
PeriodicTransform(f) (/root/reference/examples/extended_mauna_loa/script.jl:129), ("sincos", r) for the
embedding behind PeriodicKernel(r) -- evaluated on the host (O(N D)) when the spec is built.

Products of kernels (`k1 * k2`, KernelFunctions KernelProduct) expand into chains of such leaves:
`leaf_products()` returns [(coef, [(kind, param, input_chain), ...])], one entry per product of primitives,
which the library multiplies entry by entry (include/sthenomi_kprod.h, csrc/kprod.hip).
"""
from __future__ import annotations

import numpy as np

from . import lib as _lib


def _push(step, chain):
    """chain with `step` applied FIRST (outer transforms act on the raw input before inner ones);
    adjacent scalings are merged so that equal maps get equal chains."""
    if chain and step[0] == "scale" and chain[0][0] == "scale":
        s = step[1] * chain[0][1]
        return ((("scale", s),) if s != 1.0 else ()) + tuple(chain[1:])
    if step[0] == "scale" and step[1] == 1.0:
        return tuple(chain)
    return (step,) + tuple(chain)


def apply_chain(chain, X):
    """the D x n (ColVecs-layout) points the kernel reads, from the raw D x n points X"""
    for kind, v in chain:
        if kind == "scale":
            X = v * X
        elif kind == "periodic":
            if X.shape[0] != 1:
                raise ValueError("PeriodicTransform acts on 1-D inputs")
            t = (2.0 * np.pi * v) * X
            X = np.vstack([np.sin(t), np.cos(t)])      # KernelFunctions order: [sin, cos]
        elif kind == "sincos":
            # x_d -> [sin 2 pi x_d, cos 2 pi x_d] / (2 r_d): squared distances become sum_d sin^2(pi (x_d - y_d)) / r_d^2,
            # so SE over these points is KernelFunctions' PeriodicKernel(r); rows: the D sines, then the D cosines
            h = 0.5 / _sincos_r(v, X.shape[0])[:, None]
            t = (2.0 * np.pi) * X
            X = np.vstack([np.sin(t) * h, np.cos(t) * h])
        else:
            raise ValueError(kind)
    return np.asfortranarray(X)


def chain_vjp(chain, X, gout):
    """cotangent of the raw points given the cotangent of apply_chain(chain, X)"""
    stack = [X]
    for kind, v in chain[:-1]:
        stack.append(apply_chain(((kind, v),), stack[-1]))
    g = np.asarray(gout, dtype=np.float64)
    for (kind, v), xin in zip(reversed(chain), reversed(stack)):
        if kind == "scale":
            g = v * g
        elif kind == "sincos":
            D = xin.shape[0]
            h = (np.pi / _sincos_r(v, D))[:, None]          # 2 pi / (2 r_d)
            t = (2.0 * np.pi) * xin
            g = h * (np.cos(t) * g[:D, :] - np.sin(t) * g[D:, :])
        else:
            t = (2.0 * np.pi * v) * xin
            g = (2.0 * np.pi * v) * (np.cos(t) * g[0:1, :] - np.sin(t) * g[1:2, :])
    return g


def _sincos_r(v, D):
    """the D lengthscales of a ("sincos", r) step: r a float or a tuple of D floats"""
    r = np.full(D, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
    if r.shape != (D,):
        raise ValueError(f"PeriodicKernel: {r.size} lengthscales for inputs of dimension {D}")
    return r


def chain_scale(chain):
    """the scale of a pure-scaling chain (1.0 for the empty chain); None if the chain is not a scaling"""
    if not chain:
        return 1.0
    if len(chain) == 1 and chain[0][0] == "scale":
        return chain[0][1]
    return None


class Kernel:
    def __add__(self, other):
        return KernelSum([self, other])

    def __mul__(self, s):
        if isinstance(s, Kernel):
            return KernelProduct([self, s])          # k1 * k2 (KernelFunctions KernelProduct)
        return ScaledKernel(self, float(s))

    def __rmul__(self, s):
        return ScaledKernel(self, float(s))

    def __matmul__(self, transform):
        """k @ t  ==  k ∘ t  (TransformedKernel)"""
        return TransformedKernel(self, transform)

    def leaf_terms(self):
        """list of (kind, coef, param, input_chain): the leaves of a product-free kernel"""
        out = []
        for coef, factors in self.leaf_products():
            if len(factors) != 1:
                raise NotImplementedError("leaf_terms: this kernel contains a product of kernels; use leaf_products()")
            (kind, param, chain), = factors
            out.append((kind, coef, param, chain))
        return out

    def leaf_products(self):
        """list of (coef, [(kind, param, input_chain), ...]): the kernel as a sum of products of primitives.  Products of
        sums are distributed, scalings are pulled into coef, transforms are pushed onto every factor below them."""
        return [(c, [(k, p, ch)]) for (k, c, p, ch) in self.leaf_terms()]


class _Simple(Kernel):
    kind = None

    def leaf_terms(self):
        return [(self.kind, 1.0, 0.0, ())]


class SEKernel(_Simple):
    kind = _lib.SE


SqExponentialKernel = SEKernel


class Matern12Kernel(_Simple):
    kind = _lib.MATERN12


ExponentialKernel = Matern12Kernel


class Matern32Kernel(_Simple):
    kind = _lib.MATERN32


class Matern52Kernel(_Simple):
    kind = _lib.MATERN52


class WhiteKernel(_Simple):
    kind = _lib.WHITE


class ConstantKernel(Kernel):
    def __init__(self, c=1.0):
        self.c = float(c)

    def leaf_terms(self):
        return [(_lib.CONST, 1.0, self.c, ())]


class ScaledKernel(Kernel):
    def __init__(self, kernel, s2):
        self.kernel, self.s2 = kernel, float(s2)

    def leaf_terms(self):
        return [(k, c * self.s2, p, s) for (k, c, p, s) in self.kernel.leaf_terms()]

    def leaf_products(self):
        return [(c * self.s2, fs) for (c, fs) in self.kernel.leaf_products()]


class KernelSum(Kernel):
    def __init__(self, kernels):
        self.kernels = list(kernels)

    def leaf_terms(self):
        out = []
        for k in self.kernels:
            out.extend(k.leaf_terms())
        return out

    def leaf_products(self):
        out = []
        for k in self.kernels:
            out.extend(k.leaf_products())
        return out


class KernelProduct(Kernel):
    """k1 * k2 * ...: the entrywise product (KernelFunctions KernelProduct)"""

    def __init__(self, kernels):
        self.kernels = []
        for k in kernels:
            self.kernels.extend(k.kernels if isinstance(k, KernelProduct) else [k])

    def leaf_products(self):
        out = [(1.0, [])]
        for k in self.kernels:
            out = [(c * kc, fs + kfs) for (c, fs) in out for (kc, kfs) in k.leaf_products()]
        return out


class RationalQuadraticKernel(Kernel):
    """(1 + d^2 / (2 alpha))^-alpha"""

    def __init__(self, alpha=2.0):
        self.alpha = float(alpha)
        if not self.alpha > 0.0:
            raise ValueError("RationalQuadraticKernel: alpha must be > 0")

    def leaf_terms(self):
        return [(_lib.RQ, 1.0, self.alpha, ())]


class LinearKernel(Kernel):
    """x'y + c"""

    def __init__(self, c=0.0):
        self.c = float(c)
        if not self.c >= 0.0:
            raise ValueError("LinearKernel: c must be >= 0")

    def leaf_terms(self):
        return [(_lib.LINEAR, 1.0, self.c, ())]


class PolynomialKernel(Kernel):
    """(x'y + c)^degree: a chain of `degree` LINEAR factors"""

    def __init__(self, degree=2, c=0.0):
        self.degree, self.c = int(degree), float(c)
        if self.degree < 1 or self.degree != degree:
            raise ValueError("PolynomialKernel: degree must be a positive integer")
        if not self.c >= 0.0:
            raise ValueError("PolynomialKernel: c must be >= 0")

    def leaf_products(self):
        return [(1.0, [(_lib.LINEAR, self.c, ())] * self.degree)]


class PeriodicKernel(Kernel):
    """exp(-sum_d sin^2(pi (x_d - y_d)) / r_d^2 / 2) (KernelFunctions PeriodicKernel; period 1): SE over the host-side
    embedding x_d -> [sin 2 pi x_d, cos 2 pi x_d] / (2 r_d).  No device work of its own."""

    def __init__(self, r=1.0):
        self.r = float(r) if np.ndim(r) == 0 else tuple(float(v) for v in np.asarray(r, dtype=np.float64).ravel())
        if not np.all(np.asarray(self.r) > 0.0):
            raise ValueError("PeriodicKernel: r must be > 0")

    def leaf_terms(self):
        return [(_lib.SE, 1.0, 0.0, (("sincos", self.r),))]


class ScaleTransformedKernel(Kernel):
    """k o ScaleTransform(s)"""

    def __init__(self, kernel, s):
        self.kernel, self.s = kernel, float(s)

    def leaf_terms(self):
        return [(k, c, p, _push(("scale", self.s), ch)) for (k, c, p, ch) in self.kernel.leaf_terms()]

    def leaf_products(self):
        return [(c, [(k, p, _push(("scale", self.s), ch)) for (k, p, ch) in fs]) for (c, fs) in self.kernel.leaf_products()]


class ScaleTransform:
    def __init__(self, s):
        self.s = float(s)

    def step(self):
        return ("scale", self.s)


class PeriodicTransform:
    """x -> [sin(2 pi f x), cos(2 pi f x)] for 1-D inputs (KernelFunctions.PeriodicTransform [EXT];
    Stheno's own `periodic(f, freq)` warp uses [cos, sin]: same kernel values)."""

    def __init__(self, f):
        self.f = float(f)

    def step(self):
        return ("periodic", self.f)


class TransformedKernel(Kernel):
    """k ∘ t for t a ScaleTransform or PeriodicTransform (written `k @ t` here)."""

    def __init__(self, kernel, transform):
        self.kernel, self.transform = kernel, transform

    def leaf_terms(self):
        st = self.transform.step()
        return [(k, c, p, _push(st, ch)) for (k, c, p, ch) in self.kernel.leaf_terms()]

    def leaf_products(self):
        st = self.transform.step()
        return [(c, [(k, p, _push(st, ch)) for (k, p, ch) in fs]) for (c, fs) in self.kernel.leaf_products()]


def with_lengthscale(kernel, l):
    return ScaleTransformedKernel(kernel, 1.0 / float(l))
