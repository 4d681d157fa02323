"""Kernel descriptions of the drop-in surface (the KernelFunctions.jl names Stheno re-exports,
/root/reference/src/Stheno.jl:4-6).  Pure descriptions: no arithmetic happens here -- a kernel
expands into (kind, coef, param, input_chain) leaf terms that the HIP assembly kernel
evaluates (stheno.jl_amd/csrc/kernelmatrix.hip).  `input_chain` is the kernel-level input
transformation (KernelFunctions `TransformedKernel`): a tuple of steps applied to the raw points in
order -- ("scale", s) for ScaleTransform(s) / with_lengthscale, ("periodic", f) for
PeriodicTransform(f) (/root/reference/examples/extended_mauna_loa/script.jl:129), ("sincos", r) for the
embedding behind PeriodicKernel(r), ("linear", A) / ("ard", v) / ("select", idx) for KernelFunctions' LinearTransform,
ARDTransform and SelectTransform -- evaluated on the host (O(N D)) when the spec is built.  Matrices, vectors and index
lists are stored as tuples of floats / ints: equal maps give equal (hashable) chains, so equal views are uploaded once.

Products of kernels (`k1 * k2`, KernelFunctions KernelProduct) expand into chains of such leaves:
`leaf_products()` returns [(coef, [(kind, param, input_chain), ...])], one entry per product of primitives,
which the library multiplies entry by entry (include/sthenomi_kprod.h, csrc/kprod.hip).
"""
from __future__ import annotations

import numpy as np

from . import lib as _lib


def _push(step, chain):
    """chain with `step` applied FIRST (outer transforms act on the raw input before inner ones);
    adjacent scalings are merged so that equal maps get equal chains.  ("linear", A), ("ard", v) and ("select", idx) steps
    arrive with canonical payloads (tuples of floats / ints, from the transforms' step()), so equal matrices, vectors and index
    lists compare and hash equal as they are; they are kept apart from the scalings around them, so that `d_transform` stays
    the derivative with respect to the matrix or vector the caller wrote."""
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
        elif kind == "linear":
            A = _linear_A(v, X.shape[0])
            X = A @ X
        elif kind == "ard":
            X = _ard_v(v, X.shape[0])[:, None] * X
        elif kind == "select":
            X = X[list(v), :]
        elif kind == "sincos":
            # x_d -> [sin 2 pi x_d, cos 2 pi x_d] / (2 r_d): squared distances become sum_d sin^2(pi (x_d - y_d)) / r_d^2,
            # so SE over these points is KernelFunctions' PeriodicKernel(r); rows: the D sines, then the D cosines
            h = 0.5 / _sincos_r(v, X.shape[0])[:, None]
            t = (2.0 * np.pi) * X
            X = np.vstack([np.sin(t) * h, np.cos(t) * h])
        else:
            raise ValueError(kind)
    return np.asfortranarray(X)


def _linear_A(v, D):
    """the d x D matrix of a ("linear", A) step"""
    A = np.asarray(v, dtype=np.float64)
    if A.ndim != 2 or A.shape[1] != D:
        raise ValueError(f"LinearTransform: a matrix of shape {A.shape} for inputs of dimension {D}")
    return A


def _ard_v(v, D):
    """the D factors of an ("ard", v) step"""
    a = np.asarray(v, dtype=np.float64)
    if a.shape != (D,):
        raise ValueError(f"ARDTransform: {a.size} factors for inputs of dimension {D}")
    return a


def chain_vjp(chain, X, gout, transforms=None):
    """cotangent of the raw points given the cotangent of apply_chain(chain, X).  transforms: a list that receives, in
    chain order, the cotangent of every ("linear", A) step's matrix (g X_in') and every ("ard", v) step's vector
    (the row sums of g * X_in), X_in the points that step reads and g the cotangent of what it returns"""
    stack = [np.asarray(X, dtype=np.float64)]
    for kind, v in chain[:-1]:
        stack.append(apply_chain(((kind, v),), stack[-1]))
    g = np.asarray(gout, dtype=np.float64)
    found = []
    for (kind, v), xin in zip(reversed(chain), reversed(stack)):
        if kind == "scale":
            g = v * g
        elif kind == "linear":
            found.append(g @ xin.T)
            g = _linear_A(v, xin.shape[0]).T @ g
        elif kind == "ard":
            found.append(np.sum(g * xin, axis=1))
            g = _ard_v(v, xin.shape[0])[:, None] * g
        elif kind == "select":
            gin = np.zeros(xin.shape)
            np.add.at(gin, list(v), g)
            g = gin
        elif kind == "sincos":
            D = xin.shape[0]
            h = (np.pi / _sincos_r(v, D))[:, None]          # 2 pi / (2 r_d)
            t = (2.0 * np.pi) * xin
            g = h * (np.cos(t) * g[:D, :] - np.sin(t) * g[D:, :])
        else:
            t = (2.0 * np.pi * v) * xin
            g = (2.0 * np.pi * v) * (np.cos(t) * g[0:1, :] - np.sin(t) * g[1:2, :])
    if transforms is not None:
        transforms.extend(reversed(found))
    return g


def _sincos_r(v, D):
    """the D lengthscales of a ("sincos", r) step: r a float or a tuple of D floats"""
    r = np.full(D, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
    if r.shape != (D,):
        raise ValueError(f"PeriodicKernel: {r.size} lengthscales for inputs of dimension {D}")
    return r


def chain_direction(chain, v):
    """a direction v (length D) in the raw points' coordinates seen through the chain's Jacobian -- the direction, in the
    coordinates of apply_chain(chain, X), along which the kernel is differentiated when the process is differentiated along
    v; None if a step is not linear (periodic, sincos)"""
    v = np.asarray(v, dtype=np.float64)
    for kind, p in chain:
        if kind == "scale":
            v = p * v
        elif kind == "linear":
            v = _linear_A(p, v.shape[0]) @ v
        elif kind == "ard":
            v = _ard_v(p, v.shape[0]) * v
        elif kind == "select":
            v = v[list(p)]
        else:
            return None
    return v


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


def MaternKernel(nu=1.5):
    """KernelFunctions' MaternKernel(nu) at the three half-integer orders with a closed form: the existing kinds.  Any other
    nu is GeneralMaternKernel(nu), which evaluates a Bessel function per entry on the product path."""
    kinds = {0.5: Matern12Kernel, 1.5: Matern32Kernel, 2.5: Matern52Kernel}
    if float(nu) not in kinds:
        raise NotImplementedError(f"MaternKernel(nu = {nu!r}): this constructor maps to the closed-form Matern kinds, nu must "
                                  "be 1/2, 3/2 or 5/2; GeneralMaternKernel(nu) takes any nu in (0, 32]")
    return kinds[float(nu)]()


class GeneralMaternKernel(Kernel):
    """2^(1-nu) / Gamma(nu) x^nu K_nu(x), x = sqrt(2 nu) d, d the Euclidean distance, nu in (0, 32] (KernelFunctions
    MaternKernel(nu), scikit-learn Matern(nu=nu)); evaluated on the product path (include/sthenomi_kprod.h: SGP_MATERN_NU).
    nu is held fixed: gradient records carry d_param = 0 for it."""

    def __init__(self, nu=1.5):
        self.nu = float(nu)
        if not 0.0 < self.nu <= _lib.MATERN_NU_MAX:
            raise ValueError(f"GeneralMaternKernel: nu must be finite and in (0, {_lib.MATERN_NU_MAX:g}]")

    def leaf_terms(self):
        return [(_lib.MATERN_NU, 1.0, self.nu, ())]


class CosineKernel(_Simple):
    """cos(pi d) (KernelFunctions CosineKernel); evaluated on the product path (include/sthenomi_kprod.h)"""
    kind = _lib.COSINE


class GammaExponentialKernel(Kernel):
    """exp(-d^gamma), d the Euclidean distance, gamma in (0, 2] (KernelFunctions >= 0.9): gamma = 1 is ExponentialKernel,
    gamma = 2 is SEKernel o ScaleTransform(sqrt 2)"""

    def __init__(self, gamma=2.0):
        self.gamma = float(gamma)
        if not 0.0 < self.gamma <= 2.0:
            raise ValueError("GammaExponentialKernel: gamma must be in (0, 2]")

    def leaf_terms(self):
        return [(_lib.GAMMAEXP, 1.0, self.gamma, ())]


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


class NeuralNetworkKernel(_Simple):
    """asin(x'y / sqrt((1 + x'x)(1 + y'y))) (KernelFunctions NeuralNetworkKernel, Williams' arcsine kernel); evaluated on the
    product path (include/sthenomi_kprod.h: SGP_NEURALNET)"""
    kind = _lib.NEURALNET


class FBMKernel(Kernel):
    """(|x|^2h + |y|^2h - |x - y|^2h) / 2, h in (0, 1] (KernelFunctions FBMKernel): fractional Brownian motion, the Wiener
    process at h = 1/2 and x'y at h = 1; evaluated on the product path (SGP_FBM, param = h)"""

    def __init__(self, h=0.5):
        self.h = float(h)
        if not 0.0 < self.h <= 1.0:
            raise ValueError("FBMKernel: h must be in (0, 1]")

    def leaf_terms(self):
        return [(_lib.FBM, 1.0, self.h, ())]


class ExponentiatedKernel(_Simple):
    """exp(x'y) (KernelFunctions ExponentiatedKernel); evaluated on the product path (SGP_EXPONENTIATED)"""
    kind = _lib.EXPONENTIATED


def WienerKernel(i=0):
    """KernelFunctions' WienerKernel{i}: the i-times integrated Wiener process, i = 0 .. 3, a function of |x|, |y| and
    |x - y| (include/sthenomi_kprod.h: SGP_WIENER, param = i).  i = -1 is WhiteKernel(), as in KernelFunctions.  i >= 1 is not
    known to be positive definite beyond the half line."""
    if i == -1:
        return WhiteKernel()
    if isinstance(i, bool) or i not in (0, 1, 2, 3):
        raise ValueError(f"WienerKernel: i must be -1, 0, 1, 2 or 3, not {i!r}")
    return _WienerKernel(int(i))


class _WienerKernel(Kernel):
    def __init__(self, i):
        self.i = i

    def leaf_terms(self):
        return [(_lib.WIENER, 1.0, float(self.i), ())]


class PiecewisePolynomialKernel(Kernel):
    """max(1 - d, 0)^(j + q) p_q(d), j = floor(dim / 2) + q + 1, q = degree in 0 .. 3 (KernelFunctions
    PiecewisePolynomialKernel{q}(dim), Rasmussen & Williams eq. 4.21): compactly supported, exactly 0 beyond distance 1.
    Positive definite on inputs of dimension <= dim only: build_spec raises ValueError where the kernel reads more.
    Evaluated on the product path (SGP_PIECEWISE0 .. 3: the code carries q, param = j)."""

    def __init__(self, degree=0, *, dim):
        if isinstance(degree, bool) or degree not in (0, 1, 2, 3):
            raise ValueError(f"PiecewisePolynomialKernel: degree must be 0, 1, 2 or 3, not {degree!r}")
        if isinstance(dim, bool) or dim != int(dim) or dim < 1:
            raise ValueError(f"PiecewisePolynomialKernel: dim must be a positive integer, not {dim!r}")
        self.degree, self.dim = int(degree), int(dim)
        self.j = self.dim // 2 + self.degree + 1
        if self.j > _lib.PIECEWISE_J_MAX:
            raise ValueError(f"PiecewisePolynomialKernel: j = dim // 2 + degree + 1 = {self.j} is beyond {_lib.PIECEWISE_J_MAX}")

    def leaf_terms(self):
        return [(_lib.PIECEWISE0 + self.degree, 1.0, float(self.j), ())]


def piecewise_max_dim(kind, j):
    """the largest input dimension at which a SGP_PIECEWISE term (kind, param = j) is positive definite: j = floor(dim / 2) +
    q + 1 gives dim <= 2 (j - q - 1) + 1"""
    return 2 * (int(j) - (kind - _lib.PIECEWISE0) - 1) + 1


def RationalKernel(alpha=2.0):
    """(1 + d^2 / alpha)^-alpha (KernelFunctions RationalKernel): RationalQuadraticKernel(alpha) o ScaleTransform(sqrt 2), a
    name on the host; d / d alpha comes back in d_param"""
    if not float(alpha) > 0.0:
        raise ValueError("RationalKernel: alpha must be > 0")
    return TransformedKernel(RationalQuadraticKernel(alpha), ScaleTransform(np.sqrt(2.0)))


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


class LinearTransform:
    """x -> A x, A of shape d x D (KernelFunctions.LinearTransform)"""

    def __init__(self, A):
        A = np.asarray(A, dtype=np.float64)
        if A.ndim != 2 or A.size == 0:
            raise ValueError("LinearTransform: A must be a non-empty matrix")
        self.A = A

    def step(self):
        return ("linear", tuple(tuple(float(a) for a in row) for row in self.A))


class ARDTransform:
    """x -> v .* x (KernelFunctions.ARDTransform)"""

    def __init__(self, v):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim != 1 or v.size == 0:
            raise ValueError("ARDTransform: v must be a non-empty vector")
        self.v = v

    def step(self):
        return ("ard", tuple(float(a) for a in self.v))


class SelectTransform:
    """x -> x[idx] (KernelFunctions.SelectTransform; 0-based here)"""

    def __init__(self, idx):
        raw = np.asarray(idx).ravel()
        if raw.size == 0 or np.any(raw != np.floor(raw)) or np.any(raw < 0):
            raise ValueError("SelectTransform: idx must be a non-empty list of coordinates >= 0")
        self.idx = tuple(int(i) for i in raw)

    def step(self):
        return ("select", self.idx)


class TransformedKernel(Kernel):
    """k ∘ t for t a ScaleTransform, PeriodicTransform, LinearTransform, ARDTransform or SelectTransform (written
    `k @ t` here)."""

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


def gaborkernel(sqexponential_transform=None, cosine_transform=None):
    """(SEKernel o sqexponential_transform) * (CosineKernel o cosine_transform) (KernelFunctions.gaborkernel); None: the
    identity"""
    a, b = SEKernel(), CosineKernel()
    if sqexponential_transform is not None:
        a = a @ sqexponential_transform
    if cosine_transform is not None:
        b = b @ cosine_transform
    return a * b


def _mixture_args(alphas, gammas, omegas, alpha_ndim):
    al = np.asarray(alphas, dtype=np.float64)
    ga, om = np.asarray(gammas, dtype=np.float64), np.asarray(omegas, dtype=np.float64)
    if ga.ndim != 2 or ga.shape != om.shape or al.ndim != alpha_ndim or al.shape[-1] != ga.shape[1] or ga.size == 0:
        raise ValueError("spectral mixture: gammas and omegas must be D x Q, alphas of length Q (product kernel: D x Q)")
    return al, ga, om


def spectral_mixture_kernel(alphas, gammas, omegas, h=None):
    """k(x, y) = sum_q alpha_q h(gamma_q' t) cos(pi omega_q' t),  t = x - y,  h(s) = h(s, 0) (default SEKernel: exp(-s^2 / 2))
    with gammas, omegas of shape D x Q and alphas of length Q (KernelFunctions.spectral_mixture_kernel): a sum of Q products
    of two one-dimensional factors, h on the projection gamma_q' x and CosineKernel on omega_q' x."""
    al, ga, om = _mixture_args(alphas, gammas, omegas, 1)
    h = SEKernel() if h is None else h
    row = lambda M, q: LinearTransform(M[:, q][None, :])      # noqa: E731  (the projection x -> M_q' x)
    return KernelSum([float(al[q]) * ((h @ row(ga, q)) * (CosineKernel() @ row(om, q))) for q in range(ga.shape[1])])


def spectral_mixture_product_kernel(alphas, gammas, omegas, h=None):
    """k(x, y) = prod_d sum_q alpha_dq h(gamma_dq t_d) cos(pi omega_dq t_d),  t = x - y, with alphas, gammas, omegas of shape
    D x Q (KernelFunctions.spectral_mixture_product_kernel): the product over the coordinates of one-dimensional spectral
    mixtures.  leaf_products() distributes it into Q^D chains of 2 D factors; beyond the limits of a chain (8 factors) the
    library refuses it."""
    al, ga, om = _mixture_args(alphas, gammas, omegas, 2)
    if al.shape != ga.shape:
        raise ValueError("spectral_mixture_product_kernel: alphas, gammas and omegas must all be D x Q")
    return KernelProduct([spectral_mixture_kernel(al[d], ga[d:d + 1], om[d:d + 1], h) @ SelectTransform([d])
                          for d in range(ga.shape[0])])
