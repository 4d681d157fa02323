"""Kernel descriptions of the drop-in surface (the KernelFunctions.jl names Stheno re-exports,
/root/reference/src/Stheno.jl:4-6).  Pure descriptions: no arithmetic happens here -- a kernel
expands into (kind, coef, param, input_chain) leaf terms that the HIP assembly kernel
evaluates (stheno.jl_amd/csrc/kernelmatrix.hip).  `input_chain` is the kernel-level input
transformation (KernelFunctions `TransformedKernel`): a tuple of steps applied to the raw points in
order -- ("scale", s) for ScaleTransform(s) / with_lengthscale, ("periodic", f) for
PeriodicTransform(f) (/root/reference/examples/extended_mauna_loa/script.jl:129), ("sincos", r) for the
embedding behind PeriodicKernel(r), ("linear", A) / ("ard", v) / ("select", idx) for KernelFunctions' LinearTransform,
ARDTransform and SelectTransform, ("lengthscale", fn) for the row l(X) that GibbsKernel appends below the location rows
(always the last step), ("bias", s) for the constant row s that NNGPKernel / NTKKernel append (likewise) -- evaluated on
the host (O(N D)) when the spec is built.  Matrices, vectors and index
lists are stored as tuples of floats / ints: equal maps give equal (hashable) chains, so equal views are uploaded once
(a lengthscale step compares by its callable).

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
        elif kind == "lengthscale":
            X = np.vstack([X, _lengthscale_row(v, X)])     # the Gibbs kind's points: the location, then l(x)
        elif kind == "bias":
            X = np.vstack([X, np.full((1, X.shape[1]), float(v))])     # the arc-cosine kinds' first-layer bias: a constant row
        elif kind == "blur":
            # the blur kind's points: the location, then the variances of the footprint (zeros for a view without a node)
            S = np.zeros(X.shape) if v.S is None else v.S
            if S.shape != X.shape:
                raise ValueError(f"blur: variance rows of shape {S.shape} for points of shape {X.shape}")
            X = np.vstack([X, S])
        elif kind == "sincos":
            # x_d -> [sin 2 pi x_d, cos 2 pi x_d] / (2 r_d): squared distances become sum_d sin^2(pi (x_d - y_d)) / r_d^2,
            # so SE over these points is KernelFunctions' PeriodicKernel(r); rows: the D sines, then the D cosines
            h = 0.5 / _sincos_r(v, X.shape[0])[:, None]
            t = (2.0 * np.pi) * X
            X = np.vstack([np.sin(t) * h, np.cos(t) * h])
        else:
            raise ValueError(kind)
    return np.asfortranarray(X)


class BlurRows:
    """what a ("blur", rows) step appends below the location rows (always the last step of its chain): S, the D x n variances
    in the kernel's coordinates (None: zeros, a view that passed no blur node), and how they came from the outermost node's
    variances s: S[i] = fac[i] * s[sel[i]] (+ the nested nodes' shares).  Compares by identity: flatten.py hands one object to
    every path that reads the same view"""

    def __init__(self, S=None, sel=None, fac=None, nrows=0):
        self.S, self.sel, self.fac, self.nrows = S, sel, fac, nrows

    def through(self, chain):
        """these rows seen through a kernel's input chain: a diagonal factor a multiplies a variance by a^2, a select selects"""
        if self.S is None:
            return self
        S, sel, fac = self.S, self.sel, self.fac
        for kind, v in chain:
            if kind == "select":
                S, sel, fac = S[list(v), :], sel[list(v)], fac[list(v)]
                continue
            if kind == "scale" and np.ndim(v) == 0:
                a = np.full(S.shape[0], float(v))
            elif kind == "ard":
                a = _ard_v(v, S.shape[0])
            elif kind == "linear" and np.array_equal(_linear_A(v, S.shape[0]), np.diag(np.diag(_linear_A(v, S.shape[0])))):
                a = np.diag(_linear_A(v, S.shape[0])).copy()   # (a square diagonal matrix)
            else:
                raise NotImplementedError(f"blur: the kernel's input transform `{kind}` below the node is not supported (only "
                                          "ScaleTransform / ARDTransform / SelectTransform / with_lengthscale and diagonal "
                                          "linear maps keep a Gaussian footprint axis-aligned)")
            S, fac = (a * a)[:, None] * S, fac * a * a
        return BlurRows(S, sel, fac, self.nrows)

    def node_cotangent(self, gS):
        """the cotangent of the outermost node's D x n variances given that of S"""
        out = np.zeros((self.nrows, gS.shape[1]))
        np.add.at(out, self.sel, self.fac[:, None] * gS)
        return out


BLUR_ZERO_ROWS = BlurRows()


def _lengthscale_row(fn, X):
    """l(X) of a ("lengthscale", fn) step: n positive finite values for the D x n points X"""
    l = np.asarray(fn(X), dtype=np.float64).reshape(-1)
    if l.shape[0] != X.shape[1] or not np.all(np.isfinite(l)) or not np.all(l > 0.0):
        raise ValueError(f"GibbsKernel: lengthscale must return {X.shape[1]} positive finite values for {X.shape[1]} points")
    return l


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
    (the row sums of g * X_in), X_in the points that step reads and g the cotangent of what it returns, and of every
    ("lengthscale", fn) step's appended row l(X_in) (length n): that step's location rows pass through with l held fixed"""
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
        elif kind == "lengthscale":
            found.append(g[-1, :].copy())
            g = g[:-1, :]
        elif kind == "bias":
            g = g[:-1, :]
        elif kind == "blur":
            found.append(g[g.shape[0] // 2:, :].copy())
            g = g[:g.shape[0] // 2, :]
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
    v; None if a step is not linear (periodic, sincos, lengthscale)"""
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
        if len(self.kernels) > 1 and any(f[0] in _lib.ADDITIVE_OF.values() for _, fs in out for f in fs):
            raise NotImplementedError("a product of kernels with an additive factor (AdditiveKernel) is not supported (the "
                                      "additive kinds are no factors of the library's product chains)")
        if len(self.kernels) > 1 and any(f[0] in (_lib.NNGP, _lib.NTK) for _, fs in out for f in fs):
            raise NotImplementedError("a product of kernels with an arc-cosine factor (NNGPKernel / NTKKernel) is not supported "
                                      "(the arc-cosine kinds are no factors of the library's product chains)")
        if len(self.kernels) > 1 and any(f[0] == _lib.GIBBS for _, fs in out for f in fs):
            raise NotImplementedError("a product of kernels with a GibbsKernel factor is not supported (the Gibbs kind is "
                                      "no factor of the library's product chains)")
        return out


class GibbsKernel(Kernel):
    """KernelFunctions' GibbsKernel(; lengthscale): a squared-exponential whose lengthscale depends on the point,
        k(x, y) = (2 lx ly / (lx^2 + ly^2))^(power / 2) exp(-|x - y|^2 / (lx^2 + ly^2)),   lx = lengthscale(x).
    `lengthscale`: a callable that takes the D x n points the kernel sees (after the transforms around it) and returns n
    positive finite values (ValueError otherwise).  power = 1 is KernelFunctions' kernel; power = D is the form of Paciorek and
    Schervish, the one that is positive definite in D dimensions (a power below D is not in general).  Evaluated on the
    device (include/sthenomi.h: SGP_GIBBS): the host appends the row l(X) to the points, O(n)."""

    def __init__(self, lengthscale, power=1):
        if not callable(lengthscale):
            raise TypeError("GibbsKernel: lengthscale must be a callable of the D x n points")
        if power != int(power) or not 1 <= int(power) <= _lib.GIBBS_MAX_POWER:
            raise ValueError(f"GibbsKernel: power must be an integer in 1 .. {_lib.GIBBS_MAX_POWER}")
        self.lengthscale, self.power = lengthscale, int(power)

    def leaf_terms(self):
        return [(_lib.GIBBS, 1.0, float(self.power), (("lengthscale", self.lengthscale),))]


class _ArcCosine(Kernel):
    """depth hidden ReLU layers, weight variance 2 (norms pass through the layers), first-layer bias variance `bias` >= 0: the
    kernel sees the points with one constant coordinate sqrt(bias) appended (a ("bias", sqrt(bias)) chain step, always the
    last), so the user dimension is <= 15 with a bias and <= 16 without.  Without a bias a 1-D model is degenerate: the
    cosine of the angle between two numbers is +-1"""
    kind = None

    def __init__(self, depth, bias=0.0):
        name = type(self).__name__
        if (isinstance(depth, bool) or not np.isreal(depth) or not np.isfinite(depth) or depth != int(depth)
                or not 1 <= int(depth) <= _lib.ARCCOS_MAX_DEPTH):
            raise ValueError(f"{name} (arc-cosine): depth must be an integer in 1 .. {_lib.ARCCOS_MAX_DEPTH}")
        if not (float(bias) >= 0.0 and np.isfinite(float(bias))):
            raise ValueError(f"{name} (arc-cosine): bias must be a finite variance >= 0")
        self.depth, self.bias = int(depth), float(bias)

    def leaf_terms(self):
        return [(self.kind, 1.0, float(self.depth), (("bias", float(np.sqrt(self.bias))),) if self.bias > 0.0 else ())]


class NNGPKernel(_ArcCosine):
    """The covariance of a depth-`depth` fully connected ReLU network in the infinite-width limit (the arc-cosine kernel of Cho
    and Saul iterated; Lee et al.): K = |x| |y| c_L, c_{l+1} = kappa_1(c_l) from the cosine c_0 of the angle between the points
    (include/sthenomi.h: SGP_NNGP).  One layer recursion per entry on the device; a sum over depths shares it."""
    kind = _lib.NNGP


class NTKKernel(_ArcCosine):
    """The neural tangent kernel of the same network (Jacot et al.): K = |x| |y| t_L, t_{l+1} = c_{l+1} + t_l kappa_0(c_l)
    (include/sthenomi.h: SGP_NTK); k(x, x) = (depth + 1) |x|^2"""
    kind = _lib.NTK


class AdditiveKernel(Kernel):
    """The additive kernel of Duvenaud, Nickisch and Rasmussen of one order: the elementary symmetric polynomial e_order of the
    D one-dimensional base kernels, k(x, y) = sum over d_1 < .. < d_order of prod_i base(x_{d_i}, y_{d_i}).  `base`: SEKernel,
    Matern12Kernel / ExponentialKernel, Matern32Kernel or Matern52Kernel, as constructed (no transform inside: lengthscales
    come from an ARDTransform / ScaleTransform / with_lengthscale around the AdditiveKernel).  `order`: an integer in
    1 .. min(D, 8), D the dimension of the points the kernel sees (the library checks it against D).  Evaluated on the device
    by one recurrence per point pair (include/sthenomi.h: SGP_ADDITIVE_*)."""

    def __init__(self, base, order):
        if type(base) not in (SEKernel, Matern12Kernel, Matern32Kernel, Matern52Kernel):
            raise TypeError("AdditiveKernel: the additive base must be SEKernel, Matern12Kernel (ExponentialKernel), "
                            "Matern32Kernel or Matern52Kernel; put transforms around the AdditiveKernel")
        if order != int(order) or not 1 <= int(order) <= _lib.ADDITIVE_MAX_ORDER:
            raise ValueError(f"AdditiveKernel: the additive order must be an integer in 1 .. {_lib.ADDITIVE_MAX_ORDER}")
        self.base, self.order = base, int(order)

    def leaf_terms(self):
        return [(_lib.ADDITIVE_OF[self.base.kind], 1.0, float(self.order), ())]


def additive_kernel(base, variances):
    """sum_r variances[r - 1] * AdditiveKernel(base, r), r = 1 .. len(variances): the full additive model up to that order.  All
    its terms read one view of the points, so they flatten to one launch group: one recurrence per point pair for all orders"""
    variances = [float(v) for v in variances]
    if not variances:
        raise ValueError("additive_kernel: at least one variance (the additive model's first order)")
    return KernelSum([ScaledKernel(AdditiveKernel(base, r + 1), v) for r, v in enumerate(variances)])


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
