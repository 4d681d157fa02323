"""FiniteGP operator surface: f(x, s2), logpdf, rand, posterior, marginals, mean/cov/var,
VFE / elbo, SparseFiniteGP -- the AbstractGPs.jl API Stheno inherits and
src/gp/sparse_finite_gp.jl:30-62, routed through the C-ABI (include/sthenomi.h).

Every number comes out of libsthenomi.so (HIP, gfx950).  The host only flattens the model
(flatten.py), evaluates prior means (O(N)) and draws Z for `rand` from the caller's RNG.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import kernels as _kernels
from . import lib as _lib
from .flatten import build_spec, chain_input_gradients, stencil_node_gradients, zero_spec
from .gp import SthenoAbstractGP, mean_vector
from .gppp import GPPP
from .inputs import BlockData, eltype as _eltype


def _ctx():
    return _lib.default_context()


def _f64(a, order="F"):
    return np.require(np.asarray(a, dtype=np.float64), requirements=["F" if order == "F" else "C", "A"])


class FiniteGP:
    """f(x, Sigma_y): Sigma_y real -> s2*I, vector -> Diagonal, matrix -> dense; default 1e-18."""

    def __init__(self, f, x, noise=1e-18):
        self.f, self.x, self.noise = f, x, noise

    def __len__(self):
        return len(self.x)


# ---- a prior-like object is anything below; dispatch by type ---------------------------------
def _refuse_patch_gradient(*specs):
    """gradients through patch_convolve or stencil terms are not implemented (the library refuses them too): never a
    silently wrong gradient"""
    if any(sp.has_stencil for sp in specs):
        raise NotImplementedError("gradients through stencil covariance terms are not supported here: call "
                                  "logpdf_and_gradient_stencil / elbo_and_gradient_stencil")
    if any(sp.has_patch for sp in specs):
        raise NotImplementedError("gradients through patch_convolve (convolutional) covariance terms are not supported "
                                  "here: call logpdf_and_gradient_conv / elbo_and_gradient_conv")


def _refuse_product_gradient(what, *specs):
    """`what` through product chains / the RQ and LINEAR kinds is not implemented (the library refuses it too)"""
    if any(sp.has_kprod for sp in specs):
        raise NotImplementedError(f"{what} through a product of kernels (or a RationalQuadratic / Linear / Polynomial kernel, "
                                  "which runs on the product path) is not supported: logpdf_and_gradient(fx, y) is, and "
                                  "logpdf_and_gradient_param / elbo_and_gradient_param carry inputs, scales and the ELBO")


def _refuse_deriv(what, *specs):
    """`what` through derivative terms (`derivative`; include/sthenomi.h: SGP_DERIV_*) is not implemented (the library refuses
    it too): logpdf_and_gradient(fx, y) and its batch / pool forms return d_coef and d_inscale"""
    if any(sp.has_deriv for sp in specs):
        raise NotImplementedError(f"{what} through derivative covariance terms is not supported: logpdf_and_gradient(fx, y) "
                                  "returns d_coef and d_inscale of a model with derivative(f)")


def _is_prior(f):
    return isinstance(f, (GPPP, SthenoAbstractGP))


def _prior_spec(f, x, x2=None):
    spec, _, _ = build_spec(f, x, None, x2)
    return spec


def _kernelmatrix(spec):
    K = np.zeros((spec.N, spec.M), order="F")
    if spec.N and spec.M:
        _lib.check(_ctx().lib.sgp_kernelmatrix(_ctx().handle, spec.ref(), _lib.dptr(K), spec.N), "sgp_kernelmatrix")
    return K


def _kernelmatrix_f32(spec):
    K = np.zeros((spec.N, spec.M), dtype=np.float32, order="F")
    if spec.N and spec.M:
        rc = _ctx().lib.sgp_kernelmatrix_f32(_ctx().handle, spec.ref(), K.ctypes.data_as(C.POINTER(C.c_float)), spec.N)
        _lib.check(rc, "sgp_kernelmatrix_f32")
    return K


def _is_f32(fx, y=None):
    """Float32 model (the reference is type-stable in Float32, test/gp/util.jl:76-88): inputs given in
    Float32 (and, where there are observations, y in Float32) select the fp32 device path."""
    if _eltype(fx.x) != np.float32:
        return False
    return y is None or getattr(y, "dtype", None) == np.float32


def _kernelmatrix_diag(spec):
    out = np.zeros(spec.N)
    if spec.N:
        _lib.check(_ctx().lib.sgp_kernelmatrix_diag(_ctx().handle, spec.ref(), _lib.dptr(out)), "sgp_kernelmatrix_diag")
    return out


def _noise_dense(noise, n):
    a = np.asarray(noise, dtype=np.float64)
    if a.ndim == 0:
        return float(a) * np.eye(n)
    if a.ndim == 1:
        return np.diag(a)
    return a


def _noise_diag(noise, n):
    a = np.asarray(noise, dtype=np.float64)
    if a.ndim == 0:
        return np.full(n, float(a))
    if a.ndim == 1:
        return a
    return np.diag(a).copy()


# ---- statistics of the underlying process ------------------------------------------------------
def prior_mean(f, x):
    if _is_prior(f):
        return mean_vector(f, x)
    return f.mean(x)


def _model_type(out, *inputs):
    """ONE output-type rule for the whole operator surface: results come back in the element type of the inputs they were
    asked at -- Float32 when every input is Float32 (test/gp/util.jl:76-88 checks `rand` / `logpdf` of Float32 models for
    exactly that), Float64 otherwise -- whichever arithmetic produced them (the fp32 device paths cover logpdf, cov, rand
    and posterior moments; everything else is computed in fp64 and rounded here).  None / tuples pass through."""
    if out is None or not all(_eltype(x) == np.float32 for x in inputs):
        return out
    if isinstance(out, tuple):
        return tuple(_model_type(o, *inputs) for o in out)
    return np.float32(out) if np.ndim(out) == 0 else np.asarray(out).astype(np.float32, copy=False)


def prior_cov(f, x, x2=None):
    if _is_prior(f):
        if _eltype(x) == np.float32 and (x2 is None or _eltype(x2) == np.float32):
            spec = _prior_spec(f, x, x2)
            if spec.f32_supported():
                return _kernelmatrix_f32(spec)                   # fp32 assembly on the device
            # beyond the fp32 kernels' limits (input dimension > 16, very many terms per block pair): the fp64
            # kernels take any dimension and term count; the result is rounded to the model's type
            return _kernelmatrix(spec).astype(np.float32)
        return _kernelmatrix(_prior_spec(f, x, x2))
    return f.cov(x, x2)          # (posteriors round to the model's type themselves)


def prior_var(f, x):
    if _is_prior(f):
        return _model_type(_kernelmatrix_diag(_prior_spec(f, x)), x)
    return f.var(x)


def mean(fx):
    if isinstance(fx, SparseFiniteGP):     # sparse_finite_gp.jl:37
        return mean(fx.fobs)
    m = prior_mean(fx.f, fx.x)
    return m.astype(np.float32) if _eltype(fx.x) == np.float32 else m


def cov(fx, gx=None):
    if isinstance(fx, SparseFiniteGP):     # sparse_finite_gp.jl:39-43: explicit error, use cov(f.fobs)
        raise RuntimeError(_COV_ERR)
    if gx is None:
        K = prior_cov(fx.f, fx.x)
        return K + _noise_dense(fx.noise, len(fx)).astype(K.dtype)
    # src/gp/util.jl:12-14: cov(fx, gx) = cov(fx.f, gx.f, fx.x, gx.x) -- no noise
    if _is_prior(fx.f) and _is_prior(gx.f):
        spec, _, _ = build_spec(fx.f, fx.x, gx.f, gx.x)
        return _model_type(_kernelmatrix(spec), fx.x, gx.x)
    raise TypeError("cov(fx, gx) needs two FiniteGPs of one Stheno model")


def var(fx):
    if isinstance(fx, SparseFiniteGP):
        return var(fx.fobs)
    return _model_type(prior_var(fx.f, fx.x) + _noise_diag(fx.noise, len(fx)), fx.x)


def mean_and_cov(fx):
    return mean(fx), cov(fx)


def mean_and_var(fx):
    if isinstance(fx, SparseFiniteGP):
        return mean_and_var(fx.fobs)
    if isinstance(fx.f, (PosteriorGP, ApproxPosteriorGP)):
        m, v = fx.f.mean_and_var(fx.x)
        v = v + _noise_diag(fx.noise, len(fx))
        if _eltype(fx.x) == np.float32:
            return m.astype(np.float32), v.astype(np.float32)
        return m, v
    m, v = mean(fx), var(fx)
    return m, (v.astype(np.float32) if _eltype(fx.x) == np.float32 else v)


def _mean_varies(f, x):
    """whether mean(f, .) is a function of the point somewhere under f (the walk of gp.mean_vector): a callable mean, a
    callable offset, or a callable scale in front of anything -- a constant per block is not"""
    from .gp import AtomicGP, GP, _is_real
    from .gppp import extract_components
    from .inputs import blocks, is_pair_vector, regroup_pairs
    if isinstance(f, GPPP):
        node, v = extract_components(f, x)
        return _mean_varies(node, v)
    if is_pair_vector(x):
        x = regroup_pairs(x)
    if isinstance(f, AtomicGP):
        if isinstance(f.gp, GP):
            return not (f.gp.mean_spec is None or _is_real(f.gp.mean_spec))
        return _mean_varies(f.gp, x)
    op = f.args[0]
    if op == "cross":
        return any(_mean_varies(g, b) for g, b in zip(f.args[1], blocks(x)))
    if op == "+":
        return _mean_varies(f.args[1], x) or _mean_varies(f.args[2], x)
    if op in ("+known", "*"):
        return not _is_real(f.args[1]) or _mean_varies(f.args[2], x)
    if op == "o":
        return _mean_varies(f.args[1], x)      # (a warp of the points leaves a constant a constant)
    if op in ("conv", "stencil"):
        return _mean_varies(f.args[1], x)
    raise ValueError(op)


def mean_and_var_and_gradient(fx):
    """mean_and_var(fx) for fx = post(x*[, noise]) of an exact or VFE posterior together with the gradients of every
    mean_i and var_i with respect to its own test point x*_i (include/sthenomi_predgrad.h): one call against the kept
    factor, K(x*, x) assembled once, nothing factored -- what maximising an acquisition function over x* needs.

    Returns a dict: `mean`, `var` (the noise added to var only; equal to mean_and_var(fx)); `d_mean`, `d_var`: one (D, n)
    array per block of fx.x -- column i is d mean_i / d x*_i (d var_i / d x*_i), the spec-input gradients mapped back
    through the model's Stretch / Select / Periodic / Shift warps and the kernels' input scales by
    flatten.chain_input_gradients (blocks sharing one input object: its convention); `inputs_mean`, `inputs_var`,
    `inputs_var_prior`: the raw per-spec-input arrays of the library; `_cross`, `_prior`: the two specs they belong to.

    Not covered (NotImplementedError): a test-side term with a function-valued scale, a test-side prior mean that is a
    function of the point, products of kernels / patch / stencil terms, a multi-GPU context, posteriors that answer
    through explicit covariances.  A Float32 model is answered from the fp64 factor, as cov is."""
    if isinstance(fx, SparseFiniteGP):
        raise NotImplementedError("mean_and_var_and_gradient takes post(x*) of a posterior, not a SparseFiniteGP")
    f = fx.f
    if isinstance(f, ExplicitPosteriorGP):
        raise NotImplementedError("mean_and_var_and_gradient: an ExplicitPosteriorGP answers through explicit covariances, "
                                  "which carry no test points to differentiate")
    if not isinstance(f, (PosteriorGP, ApproxPosteriorGP)):
        raise NotImplementedError("mean_and_var_and_gradient takes post(x*) of an exact or VFE posterior")
    ctx = _ctx()
    if getattr(ctx, "is_multi", False):
        raise NotImplementedError("mean_and_var_and_gradient is not supported on a multi-GPU context (the factor is sharded)")
    cross, pss, ms = _cross_side(f, fx.x)
    _refuse_deriv("mean_and_var_and_gradient", cross, pss)
    _refuse_patch_gradient(cross, pss)
    _refuse_product_gradient("mean_and_var_and_gradient", cross, pss)
    if (any(rs is not None for rs in cross.term_row_scale) or any(rs is not None for rs in pss.term_row_scale)
            or any(cs is not None for cs in pss.term_col_scale)):
        raise NotImplementedError("mean_and_var_and_gradient: a test-side term with a function-valued scale is not supported "
                                  "(the library holds row scales fixed)")
    if _mean_varies(f.prior, fx.x):
        raise NotImplementedError("mean_and_var_and_gradient: a test-side prior mean that is a function of the point is not "
                                  "supported (zero and constant means are)")
    ns = cross.N
    mo, vo = np.zeros(ns), np.zeros(ns)
    gm = [np.zeros(np.asarray(a).shape, order="F") for a in cross.inputs]
    gv = [np.zeros(np.asarray(a).shape, order="F") for a in cross.inputs]
    gp = [np.zeros(np.asarray(a).shape, order="F") for a in pss.inputs]
    stem, h = f._stem, f._ensure()
    rc = getattr(ctx.predgrad, stem + "_predict_grad_x")(h, cross.ref(), pss.ref(), _lib.dptr(ms), _lib.dptr(mo), _lib.dptr(vo),
                                                        _dptrs(gm), _dptrs(gv), _dptrs(gp))
    _lib.check(rc, stem + "_predict_grad_x")
    d_mean = chain_input_gradients(cross, gm)[0]
    d_var = [a + b for a, b in zip(chain_input_gradients(cross, gv)[0], chain_input_gradients(pss, gp)[0])]
    m, v = _model_type((mo, vo), fx.x, *f._train_inputs())
    v = v + _noise_diag(fx.noise, len(fx))
    if _eltype(fx.x) == np.float32:
        m, v = m.astype(np.float32), v.astype(np.float32)
    return {"mean": m, "var": v, "d_mean": d_mean, "d_var": d_var, "inputs_mean": gm, "inputs_var": gv,
            "inputs_var_prior": gp, "_cross": cross, "_prior": pss}


class Normal:
    def __init__(self, mu, sigma):
        self.mu, self.sigma = mu, sigma

    def __eq__(self, other):
        return self.mu == other.mu and self.sigma == other.sigma


def marginals(fx):
    """Vector of Normal(mean_i, sqrt(var_i)) (test/gp/util.jl:15-20)."""
    if isinstance(fx, SparseFiniteGP):
        return marginals(fx.fobs)
    m, v = mean_and_var(fx)
    return [Normal(a, b) for a, b in zip(m, np.sqrt(v))]


# ---- logpdf / rand ---------------------------------------------------------------------------
def _spec_mean_noise(fx):
    """(spec, mean, noise_kind, noise_buf) for the C-ABI; explicit-covariance processes
    (posteriors) enter as a zero-term spec + dense noise = their covariance."""
    n = len(fx)
    if _is_prior(fx.f):
        spec = _prior_spec(fx.f, fx.x)
        kind, buf = _lib._noise_args(fx.noise, n)
        return spec, mean_vector(fx.f, fx.x), kind, buf
    Cm = fx.f.cov(fx.x) + _noise_dense(fx.noise, n)
    return zero_spec(n), fx.f.mean(fx.x), _lib.NOISE_DENSE, np.asfortranarray(Cm)


def _postfx_route(fx):
    """rand / logpdf of a posterior FiniteGP against the kept factor (include/sthenomi_postfx.h): the posterior covariance
    is formed, S* added and the sum factored where the factor lives, instead of cov(f_post, x*) coming down to the host
    and going back up as dense noise (_spec_mean_noise).  The values are those of that route bit for bit.

    Returns (library, entry-point stem, handle, cross, prior_ss, mean_s, noise kind, noise buffer), or None where the host
    route stays: a process that is neither the exact nor the VFE posterior, a multi-GPU context (the factor is sharded),
    a context without the library (the NumPy double of the CPU suites), and a model all of whose inputs are Float32 --
    there the one output-type rule rounds mean and covariance to Float32 BEFORE they are factored, which only the host
    route reproduces."""
    f = fx.f
    if not isinstance(f, (PosteriorGP, ApproxPosteriorGP)):
        return None
    ctx = _ctx()
    lib = None if getattr(ctx, "is_multi", False) else getattr(ctx, "postfx", None)
    if lib is None:
        return None
    if all(_eltype(x) == np.float32 for x in (fx.x, *f._train_inputs())):
        return None
    kind, nbuf = _lib._noise_args(fx.noise, len(fx))
    cross, pss, ms = _cross_side(f, fx.x)
    return lib, f._stem, f._ensure(), cross, pss, ms, kind, nbuf


def logpdf(fx, y):
    """logpdf(fx, y::Vector) -> float;  logpdf(fx, Y::Matrix) -> one value per column."""
    if isinstance(fx, SparseFiniteGP):
        Y = np.asarray(y, dtype=np.float64)
        if Y.ndim == 2:
            return np.array([elbo(VFE(fx.finducing), fx.fobs, Y[:, j]) for j in range(Y.shape[1])])
        return elbo(VFE(fx.finducing), fx.fobs, Y)
    f32 = _is_prior(fx.f) and _is_f32(fx, y)
    if f32 and np.ndim(y) == 1 and np.ndim(fx.noise) <= 1 and _prior_spec(fx.f, fx.x).f32_supported():
        return logpdf_f32(fx, y)
    # Float32 models the fp32 kernels do not cover (matrix Y, dense Sigma_y, input dimension > 16, more than
    # 64 / dimension terms per block pair) are computed in fp64 and returned in the model's type, so that
    # `logpdf(fx, y) isa Float32` (test/gp/util.jl:76-88) holds whichever path ran
    Y = np.asarray(y, dtype=np.float64)
    vec = Y.ndim == 1
    Y = _f64(Y.reshape(len(fx), -1))
    if Y.shape[0] != len(fx):
        raise ValueError("length(y) != length(fx)")
    out = np.zeros(Y.shape[1])
    route = _postfx_route(fx)
    if route is not None:
        lib, stem, h, cross, pss, ms, kind, nbuf = route
        rc = getattr(lib, stem + "_logpdf")(h, cross.ref(), pss.ref(), _lib.dptr(ms), kind, _lib.dptr(nbuf), _lib.dptr(Y),
                                            Y.shape[0], Y.shape[1], _lib.dptr(out))
        _lib.check(rc, stem + "_logpdf")
        return float(out[0]) if vec else out
    spec, m, kind, nbuf = _spec_mean_noise(fx)
    m = _f64(m)
    rc = _ctx().lib.sgp_logpdf(_ctx().handle, spec.ref(), _lib.dptr(m), kind, _lib.dptr(nbuf), _lib.dptr(Y),
                               Y.shape[0], Y.shape[1], _lib.dptr(out))
    _lib.check(rc, "sgp_logpdf")
    if f32:
        return np.float32(out[0]) if vec else out.astype(np.float32)
    return float(out[0]) if vec else out


# ---- the batch / pool calls: what their four host functions share --------------------------------
def _members(name, fxs, ys, grad, divert_f32):
    """The member loop of `name` (a batch / pool function): -> (keep, down).  keep[q] = (spec, mean, noise kind, noise
    buffer, y) of member down[q], alive until the library call returns; with divert_f32 the Float32 models are left out of
    both (they run through their own call)."""
    keep, down = [], []
    for b, (fx, y) in enumerate(zip(fxs, ys)):
        if isinstance(fx, SparseFiniteGP):
            raise NotImplementedError(f"{name} takes FiniteGPs (use {'elbo_and_gradient' if grad else 'elbo'} for a SparseFiniteGP)")
        if grad and not _is_prior(fx.f):
            raise NotImplementedError("gradients are implemented for prior Stheno processes")
        yv = _f64(np.asarray(y, dtype=np.float64).ravel())
        if yv.shape[0] != len(fx):
            raise ValueError("length(y) != length(fx)")
        f32 = divert_f32 and _is_prior(fx.f) and _is_f32(fx, y)
        if grad:
            kind, nbuf = _lib._noise_args(fx.noise, len(fx))
            spec = _prior_spec(fx.f, fx.x)
            _refuse_patch_gradient(spec)
            _refuse_product_gradient(f"{name}: the gradient batch / pool", spec)
            if f32:
                continue
            m = mean_vector(fx.f, fx.x)
        else:
            if f32:
                continue
            spec, m, kind, nbuf = _spec_mean_noise(fx)
        keep.append((spec, _f64(m), kind, nbuf, yv))
        down.append(b)
    return keep, down


def _dptrs(arrs):
    return (C.POINTER(C.c_double) * len(arrs))(*[_lib.dptr(a) for a in arrs])


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _member_args(keep):
    """The pointer arrays of a batch / pool call over `keep`: (specs, means, noise kinds, noises, ys)."""
    nb = len(keep)
    for k in keep:
        k[0].ref()           # (patch terms: their geometry ids on the context)
    return ((C.POINTER(_lib.sgp_cov_spec) * nb)(*[C.pointer(k[0].c) for k in keep]), _dptrs([k[1] for k in keep]),
            (C.c_int * nb)(*[int(k[2]) for k in keep]), _dptrs([k[3] for k in keep]), _dptrs([k[4] for k in keep]))


def _grad_buffers(spec, kind, n):
    """gy, gm, gn, gc, gs: the output buffers of the gradient entry points for one model."""
    # dense Sigma_y (round 4): the gradient w.r.t. the matrix is the cotangent G = (alpha alpha' - C^-1) / 2 itself, N x N
    gn = np.zeros((n, n), order="F") if kind == _lib.NOISE_DENSE else np.zeros(n if kind == _lib.NOISE_DIAG else 1)
    nt = max(1, spec.n_terms)
    return np.zeros(n), np.zeros(n), gn, np.zeros(nt), np.zeros(nt)


def _grad_record(spec, kind, lp, bufs, inputs=None, x=None, scales=None, rowscale=None, gp=None):
    """gp: the d / d param array of sgp_logpdf_grad_param (specs with product chains): the term records then carry d_param
    and `_raw` gains the array"""
    gy, gm, gn, gc, gs = bufs
    return dict(logpdf=float(lp), y=gy, mean=gm, noise=(gn if kind != _lib.NOISE_SCALAR else float(gn[0])),
                terms=_term_records(spec, gc, gs, True, gp), inputs=inputs, x=x, scales=scales,
                _raw=(gc, gs) if gp is None else (gc, gs, gp), _rowscale=rowscale, _spec=spec)


def _logpdf_grad_spec(fx, y):
    """What every logpdf gradient does before its family's refusals: the prior check, y as a float64 vector, the spec."""
    if not _is_prior(fx.f):
        raise NotImplementedError("gradients are implemented for prior Stheno processes")
    return _f64(np.asarray(y, dtype=np.float64).ravel()), _prior_spec(fx.f, fx.x)


def _logpdf_grad_frame(fx, yv, spec):
    """... and after them: the mean, the noise, the output buffers and the 12 leading arguments every sgp_logpdf_grad* entry
    point takes (context through grad_inscale) -> (noise kind, lp, buffers, arguments).  A caller adds its tail pointers,
    names its entry point and finishes through _grad_record."""
    m = _f64(mean_vector(fx.f, fx.x))
    kind, nbuf = _lib._noise_args(fx.noise, len(fx))
    lp = np.zeros(1)
    bufs = _grad_buffers(spec, kind, len(fx))
    d = _lib.dptr
    return kind, lp, bufs, (_ctx().handle, spec.ref(), d(m), kind, d(nbuf), d(yv), d(lp)) + tuple(d(b) for b in bufs)


def _grad_failed(spec, info):
    return dict(logpdf=float("nan"), info=int(info), y=None, mean=None, noise=None, terms=None, inputs=None, x=None,
                scales=None, _raw=None, _rowscale=None, _spec=spec)


def _grad_members(keep, call):
    """One gradient batch / pool call over `keep`: call(specs, means, kinds, noises, ys, lp, five output pointer arrays,
    infos) runs it; -> (one dict per member, infos)."""
    outs = [_grad_buffers(spec, kind, len(yv)) for spec, _, kind, _, yv in keep]
    lp = np.zeros(len(keep))
    infos = np.zeros(len(keep), dtype=np.int32)
    call(*_member_args(keep), _lib.dptr(lp), [_dptrs([o[q] for o in outs]) for q in range(5)], _iptr(infos))
    return [_grad_failed(k[0], infos[q]) if infos[q] else _grad_record(k[0], k[2], lp[q], outs[q])
            for q, k in enumerate(keep)], infos


def logpdf_batch(fxs, ys, return_infos=False):
    """[logpdf(fx, y) for fx, y in zip(fxs, ys)] in ONE library call (sgp_logpdf_batch): the members are independent models
    -- restarts of an optimiser, cross-validation folds, a population of hyper-parameter candidates.  Members of one padded
    size (equal N, or folds that differ by a point or two inside one 128-column tile) with scalar / diagonal noise are
    factored as one task pool of the dataflow kernel (their diagonal chains hide each other);
    every value is bit-equal to the member's own `logpdf`.  A member that is not positive definite gives NaN (and, with
    return_infos=True, its LAPACK info in the second result) instead of raising, so that one bad candidate does not lose the
    others."""
    fxs, ys = list(fxs), list(ys)
    if len(fxs) != len(ys):
        raise ValueError("logpdf_batch: one y per model")
    if not fxs:
        return (np.zeros(0), np.zeros(0, dtype=np.int32)) if return_infos else np.zeros(0)
    keep, _ = _members("logpdf_batch", fxs, ys, False, False)
    kinds = {k[2] for k in keep}
    if len(kinds) != 1 or _lib.NOISE_DENSE in kinds:
        # mixed or dense noise kinds: member by member (same values; sgp_logpdf_batch takes one noise kind)
        vals, infos = [], []
        for fx, y in zip(fxs, ys):
            try:
                vals.append(float(logpdf(fx, y)))
                infos.append(0)
            except _lib.PosDefException as e:
                vals.append(float("nan"))
                infos.append(e.info)
        return (np.array(vals), np.array(infos, dtype=np.int32)) if return_infos else np.array(vals)
    specs, means, _, noises, yp = _member_args(keep)
    out = np.zeros(len(keep))
    infos = np.zeros(len(keep), dtype=np.int32)
    rc = _ctx().lib.sgp_logpdf_batch(_ctx().handle, len(keep), specs, means, kinds.pop(), noises, yp, _lib.dptr(out),
                                     _iptr(infos))
    _lib.check(rc, "sgp_logpdf_batch")
    return (out, infos) if return_infos else out


def logpdf_f32(fx, y):
    """logpdf(fx, y) on the fp32 device path (sgp_logpdf_f32: fp32 assembly, fp32 blocked Cholesky on
    v_mfma_f32_32x32x2_f32, fp32 forward substitution) -> np.float32.  Selected automatically by `logpdf`
    when the inputs and y are Float32."""
    n = len(fx)
    yv = _f64(np.asarray(y, dtype=np.float64).ravel())
    if yv.shape[0] != n:
        raise ValueError("length(y) != length(fx)")
    spec = _prior_spec(fx.f, fx.x)
    _refuse_deriv("logpdf_f32: the fp32 path", spec)
    if spec.has_stencil:
        raise NotImplementedError("stencil terms have no fp32 path: call logpdf, which runs them in fp64")
    if spec.has_kprod:
        raise NotImplementedError("a product of kernels (and the RationalQuadratic / Linear / Polynomial kernels, which run "
                                  "on the product path) has no fp32 path: call logpdf, which runs them in fp64")
    m = _f64(mean_vector(fx.f, fx.x))
    kind, nbuf = _lib._noise_args(fx.noise, n)
    if kind == _lib.NOISE_DENSE:
        # (`logpdf` itself takes a Float32 model with dense Sigma_y through the fp64 factorisation and returns Float32)
        raise ValueError("logpdf_f32 is the explicit fp32 kernel path (scalar / diagonal Sigma_y); call logpdf for a dense Sigma_y")
    out = np.zeros(1)
    rc = _ctx().lib.sgp_logpdf_f32(_ctx().handle, spec.ref(), _lib.dptr(m), kind, _lib.dptr(nbuf), _lib.dptr(yv), _lib.dptr(out))
    _lib.check(rc, "sgp_logpdf_f32")
    return np.float32(out[0])


def _scale_records(spec, grs, more=()):
    """Per-term row-scale gradients -> one record per function scale `sigma * f` and input collection it was
    mapped over: {node, x, values (= sigma.(x)), d_values (= d logpdf / d values)}.  A path's scale vector is the
    product of its factors' values; a vector carried by several terms gets the sum of their gradients.
    `more`: further (spec, per-term gradients, "row" | "col") triples whose vectors join the same records (the ELBO
    reads one scale vector through K(z,z), K(x,z) and diag K(x,x))."""
    by_vec = {}
    for sp, grads, side in ((spec, grs, "row"),) + tuple(more):
        vecs = sp.term_row_scale if side == "row" else sp.term_col_scale
        for t, g in enumerate(grads or []):
            if g is None:
                continue
            r = vecs[t]
            if id(r) in by_vec:
                by_vec[id(r)][1] += g
            else:
                by_vec[id(r)] = [r, g.copy()]
    out, index = [], {}
    for r, g in by_vec.values():
        fac = getattr(r, "factors", [])
        for k, (node, x, vals) in enumerate(fac):
            others = np.ones(len(vals))
            for l, (_, _, v) in enumerate(fac):
                if l != k:
                    others = others * v
            key = (id(node), id(x))
            if key in index:
                out[index[key]]["d_values"] += g * others
            else:
                index[key] = len(out)
                out.append(dict(node=node, x=x, values=np.asarray(vals, dtype=np.float64).copy(), d_values=g * others))
    return out


def logpdf_and_gradient(fx, y, inputs=False, scales=False):
    """logpdf(fx, y) and its reverse-mode gradient (what Zygote derives on the reference path).
    scales=True adds `scales`: one record per function-valued scale (`sigma * f`, product.jl:25-48) and input
    collection it is mapped over, {node, x, values, d_values} with d_values[i] = d logpdf / d sigma(x_i); the
    gradient of a parameter theta of sigma is sum_i d_values[i] * d sigma(x_i) / d theta.
    inputs=True adds `inputs`: one (dim, n) array per spec input (g["_spec"].inputs[k]) with
    d logpdf / d (the points the terms read -- after Stretch / Select / Periodic; for
    stretch(f, a) the gradient w.r.t. the user's x is a * that array).

    Returns a dict: logpdf; y, mean (d/dy, d/d mean, N each); noise (scalar for f(x, s2), vector for
    f(x, v)); terms: one record per flattened covariance term of the lower block pairs
    {I, J, kind, coef, row_input, col_input, d_coef, d_inscale} where d_coef / d_inscale already
    include the mirror-image pair (J, I).  d_inscale is the derivative w.r.t. a common scale g of the
    term's inputs (stretch(f, g)); a lengthscale l = 1/g gives d/dl = -g^2 d_inscale.

    A model with derivative(f) (include/sthenomi.h: SGP_DERIV_*) is taken with inputs=False, scales=False: the records of its
    derivative terms carry "deriv": (p or None, q or None), the differentiated coordinate of the row / column side.  Their
    d_inscale keeps its meaning -- both inputs scaled by g, the differentiation taken with respect to the scaled points -- so
    the chain to a scalar stretch a below the node (stretch(f, a), or with_lengthscale(k, 1 / a)), whose Jacobian factor a
    sits in the coefficient once per differentiated side, is, with m the number of differentiated sides of the term,
        d / da = (m * coef * d_coef + d_inscale) / a.

    A model with a product of kernels (or a RationalQuadratic / Linear / Polynomial kernel) goes through
    sgp_logpdf_grad_param (include/sthenomi_kprod.h): every factor of a chain is a term record of its own, with `chain` (the
    index of its head's record), `factor` (its position), d_coef (the head's; 0 on the others), its own d_inscale, and
    d_param, the derivative w.r.t. the kernel's parameter (alpha of RQ, gamma of GammaExponential, h of FBM, c of Linear / Constant; 0 for nu
    of GeneralMaternKernel, which is held fixed).  inputs / scales of such
    models come from logpdf_and_gradient_param."""
    yv, spec = _logpdf_grad_spec(fx, y)
    _refuse_patch_gradient(spec)
    if inputs or scales:
        _refuse_deriv("logpdf_and_gradient: inputs=True / scales=True", spec)
        _refuse_product_gradient("logpdf_and_gradient: inputs=True / scales=True", spec)
    kind, lp, bufs, args = _logpdf_grad_frame(fx, yv, spec)
    if spec.has_kprod:
        if _ctx().is_multi:
            raise NotImplementedError("a product of kernels is not supported on a multi-GPU context")
        gp = np.zeros(max(1, spec.n_terms))
        _lib.check(_ctx().kprod.sgp_logpdf_grad_param(*args, _lib.dptr(gp)), "sgp_logpdf_grad_param")
        return _grad_record(spec, kind, lp[0], bufs, gp=gp)
    gx = ptrs = grs = None
    if inputs:
        gx = _input_buffers(spec)[0]
        ptrs = _dptrs(gx)       # (len(gx) slots: a spec without inputs hands these two entry points an empty table, not one NULL)
    if scales:
        grs, sptrs = _scale_arrays(spec, "row")
        _lib.check(_ctx().lib.sgp_logpdf_grad_xs(*args, ptrs, sptrs), "sgp_logpdf_grad_xs")
    elif inputs:
        _lib.check(_ctx().lib.sgp_logpdf_grad_x(*args, ptrs), "sgp_logpdf_grad_x")
    else:
        _lib.check(_ctx().lib.sgp_logpdf_grad(*args), "sgp_logpdf_grad")
    # x: the same gradient mapped back through the model's input transformations onto the blocks of
    # fx.x (one (D, n) array per block; blocks sharing one input object get their joint gradient in
    # the first of them)
    xb = chain_input_gradients(spec, gx)[0] if inputs else None
    return _grad_record(spec, kind, lp[0], bufs, gx, xb, _scale_records(spec, grs) if scales else None, grs)


def _attach_d_transform(records, spec, gx):
    """`d_transform` on every factor record whose kernel-level input chain holds a ("linear", A) or ("ard", v) step
    (kernels.LinearTransform / ARDTransform): the cotangent of that step's matrix (d x D) or vector, formed on the host from
    the cotangents gx of the views the library returned -- g X_in' per view (O(N D d)), summed over every view of the spec
    that was made by this chain.  It belongs to the transform, not to the block pair: records whose factors read through one
    chain carry one and the same array (do not add them up).  A chain with several such steps gives a tuple, in chain
    order."""
    totals = {}
    for k, g in enumerate(gx):
        org = spec.input_origin[k] if spec.input_origin is not None else None
        if org is None or g is None or not any(st[0] in ("linear", "ard") for st in org[3]):
            continue
        found = []
        _kernels.chain_vjp(org[3], org[4], g, found)
        if org[3] in totals:
            totals[org[3]] = [a + b for a, b in zip(totals[org[3]], found)]
        else:
            totals[org[3]] = found
    for r in records:
        org = spec.input_origin[r["row_input"]] if spec.input_origin is not None else None
        if org is not None and org[3] in totals:
            t = totals[org[3]]
            r["d_transform"] = t[0] if len(t) == 1 else tuple(t)
    return records


def _refuse_param_family(what, *specs):
    """what the superset family of include/sthenomi_kprod_grad.h does not carry: patch / stencil sides, a multi-GPU context"""
    _refuse_deriv(what, *specs)
    _refuse_patch_gradient(*specs)
    if getattr(_ctx(), "is_multi", False):
        raise NotImplementedError(f"{what}: a product of kernels (the gradients of include/sthenomi_kprod_grad.h) is not "
                                  "supported on a multi-GPU context")


def logpdf_and_gradient_param(fx, y, inputs=False, scales=False):
    """logpdf_and_gradient for every model it takes AND for models with a product of kernels (or a RationalQuadratic /
    Linear / Polynomial / Periodic kernel), through sgp_logpdf_grad_param_xs (include/sthenomi_kprod_grad.h): the same dict,
    with every term record in the chain form -- `chain`, `factor`, `d_param` (see logpdf_and_gradient) -- and inputs=True /
    scales=True carried through the factors of a product: `inputs` holds d logpdf / d (the view each factor reads), `x` the
    same mapped back onto the blocks of fx.x through every factor's own transform (with_lengthscale, the periodic embedding)
    and the model's warps, `scales` one record per function-valued scale.  With inputs=True a factor that reads its points
    through a LinearTransform or an ARDTransform also carries `d_transform`, the derivative with respect to that transform's
    matrix or vector (_attach_d_transform): the frequencies and bandwidths of a spectral mixture.  Single-GPU contexts; no
    patch / stencil terms."""
    yv, spec = _logpdf_grad_spec(fx, y)
    _refuse_param_family("logpdf_and_gradient_param", spec)
    kind, lp, bufs, args = _logpdf_grad_frame(fx, yv, spec)
    gp = np.zeros(max(1, spec.n_terms))
    gx, ptrs = _input_buffers(spec) if inputs else (None, None)
    grs, sptrs = _scale_arrays(spec, "row") if scales else (None, None)
    _lib.check(_ctx().kprod_grad.sgp_logpdf_grad_param_xs(*args, _lib.dptr(gp), ptrs, sptrs), "sgp_logpdf_grad_param_xs")
    xb = chain_input_gradients(spec, gx)[0] if inputs else None
    rec = _grad_record(spec, kind, lp[0], bufs, gx, xb, _scale_records(spec, grs) if scales else None, grs, gp=gp)
    if inputs:
        _attach_d_transform(rec["terms"], spec, gx)
    return rec


def _refuse_conv_family(what, *specs):
    """what the entry points of include/sthenomi_conv_grad.h refuse: a multi-GPU context, stencil terms"""
    _refuse_deriv(what, *specs)
    if getattr(_ctx(), "is_multi", False):
        raise NotImplementedError(f"{what} is not supported on a multi-GPU context")
    if any(sp.has_stencil for sp in specs):
        raise NotImplementedError(f"{what}: gradients through stencil covariance terms are not supported here: call "
                                  "logpdf_and_gradient_stencil / elbo_and_gradient_stencil")
    if any(sp.has_patch for sp in specs) and any(sp.has_kprod for sp in specs):
        raise NotImplementedError(f"{what}: a model with both patch_convolve terms and a product of kernels is not "
                                  "supported (the records of a product carry d_param, which these calls do not return)")


def logpdf_and_gradient_conv(fx, y):
    """logpdf_and_gradient(fx, y) for every model it takes AND for models with patch_convolve (convolutional) terms, through
    sgp_logpdf_grad_conv (include/sthenomi_conv_grad.h): the same dict -- logpdf, y, mean, noise, and one record per
    flattened term of the lower block pairs with d_coef / d_inscale (the mirror pair folded in).  For a patch term
    coef rs cs sum_pq k(patch_p x, patch_q x') the record's d_coef is the derivative w.r.t. that coefficient (the kernel's
    variance times the model's scalings) and d_inscale the derivative w.r.t. a common scale g of the images (a scalar stretch
    under patch_convolve; a lengthscale l = 1 / g gives d / dl = -g^2 d_inscale), exactly as for a plain term; the record also
    carries row_geom / col_geom.  No inputs / scales: gradients with respect to images are not formed.  Single-GPU contexts,
    no stencil terms."""
    yv, spec = _logpdf_grad_spec(fx, y)
    _refuse_conv_family("logpdf_and_gradient_conv", spec)
    if spec.has_kprod:
        return logpdf_and_gradient(fx, y)
    kind, lp, bufs, args = _logpdf_grad_frame(fx, yv, spec)
    _lib.check(_ctx().conv_grad.sgp_logpdf_grad_conv(*args), "sgp_logpdf_grad_conv")
    return _grad_record(spec, kind, lp[0], bufs)


def _refuse_stencil_family(what, *specs):
    """what the entry points of include/sthenomi_stencil_grad.h refuse: a multi-GPU context; and what their records cannot
    carry"""
    _refuse_deriv(what, *specs)
    if getattr(_ctx(), "is_multi", False):
        raise NotImplementedError(f"{what} is not supported on a multi-GPU context")
    if any(sp.has_patch or sp.has_stencil for sp in specs) and any(sp.has_kprod for sp in specs):
        raise NotImplementedError(f"{what}: a model with both stencil or patch_convolve terms and a product of kernels is not "
                                  "supported (the records of a product carry d_param, which these calls do not return)")


def _input_buffers(spec):
    """one zero (dim, n) array per spec input -- None for an input that a patched side reads (it holds images) -- and the
    ctypes pointer table"""
    img = _patched_inputs(spec) if spec.has_patch else ()
    arrs = [None if k in img else np.zeros(np.asarray(a).shape, order="F") for k, a in enumerate(spec.inputs)]
    return arrs, (C.POINTER(C.c_double) * max(1, len(arrs)))(*[_lib.dptr(a) for a in arrs])


def _stencil_tables(spec):
    """the output tables of include/sthenomi_stencil_wo.h for `spec`: gw[t][side] (Q) and go[t][side] (Q x D in memory: the
    layout of sgp_stencil.offsets), None on a plain side, and the two ctypes tables of 2 pointers per term"""
    nt = spec.n_terms
    gw = [[None if st is None else np.zeros(len(st[1])) for st in spec.term_stencils[t]] for t in range(nt)]
    go = [[None if st is None else np.zeros(st[0].shape[::-1]) for st in spec.term_stencils[t]] for t in range(nt)]
    tab = lambda g: (C.POINTER(C.c_double) * max(1, 2 * nt))(*[_lib.dptr(a) for row in g for a in row])    # noqa: E731
    return gw, go, tab(gw), tab(go)


def _attach_stencil_gradients(records, spec, gw, go, into):
    """d_row_weights / d_row_offsets / d_col_weights / d_col_offsets on the records of stencil terms (None on a plain side;
    offsets D x Q; the mirror term folded in with its sides swapped), and the chain back to the model's stencil nodes added
    onto `into` (flatten.stencil_node_gradients)"""
    go = [[None if a is None else a.T for a in row] for row in go]
    for r in records:
        t, mt = r["t"], r.get("mirror_t")
        if spec.term_stencils[t] == (None, None):
            continue
        for side, name in enumerate(("row", "col")):
            w, o = gw[t][side], go[t][side]
            if w is not None and mt is not None:
                w, o = w + gw[mt][1 - side], o + go[mt][1 - side]
            r[f"d_{name}_weights"], r[f"d_{name}_offsets"] = w, (None if o is None else np.array(o))
    return stencil_node_gradients(spec, gw, go, into)


def logpdf_and_gradient_stencil(fx, y, inputs=False, stencils=False):
    """logpdf_and_gradient(fx, y, inputs=inputs) for every model it takes AND for models with stencil terms (`stencil`,
    `quadrature_convolve`) or patch_convolve terms, through sgp_logpdf_grad_stencil (include/sthenomi_stencil_grad.h): the
    same dict.  For a stencil term coef rs cs sum_pq w_p v_q k(x - a_p, x' - b_q) the record's d_coef is the derivative
    w.r.t. that coefficient (the kernel's variance times the model's scalings) and d_inscale the derivative w.r.t. a common
    scale g of the points and the offsets (a lengthscale l = 1 / g gives d / dl = -g^2 d_inscale), exactly as for a plain
    term; the record also carries row_stencil / col_stencil.  inputs=True adds `inputs` and `x`: the stored points of a
    stencil side are the unshifted ones (shifting is a translation), so the chain back through Stretch / Shift / Select is
    that of a plain term; the entry of an input that holds images is None.  Single-GPU contexts.

    stencils=True adds the gradients with respect to the stencils' own weights and offsets, through
    sgp_logpdf_grad_stencil_wo (include/sthenomi_stencil_wo.h); everything else keeps its bits.  Each record of a stencil term
    also carries d_row_weights (Q), d_row_offsets (D x Q), d_col_weights, d_col_offsets: the derivative with respect to the
    stencil the library reads on that side (offsets in the kernel's scaled coordinates), None on a plain side, the mirror
    term folded in with its sides swapped.  The result carries `stencils`: one entry per `stencil(...)` node of the model that
    the observed processes reach, {"node", "d_offsets" (D x Q, the node's own shape), "d_weights" (Q)} -- the chain back
    through the kernel's scalar input scale, the Stretch / Select maps below the node and nested stencils
    (flatten.stencil_node_gradients); a scalar scale above or below the node belongs to the term's coefficient."""
    yv, spec = _logpdf_grad_spec(fx, y)
    _refuse_stencil_family("logpdf_and_gradient_stencil", spec)
    if spec.has_kprod:
        rec = logpdf_and_gradient_param(fx, y, inputs=True) if inputs else logpdf_and_gradient(fx, y)
        if stencils:
            rec["stencils"] = []       # (a model with a product of kernels has no stencil terms)
        return rec
    kind, lp, bufs, args = _logpdf_grad_frame(fx, yv, spec)
    gx, ptrs = _input_buffers(spec) if inputs else (None, None)
    if stencils:
        gw, go, pw, po = _stencil_tables(spec)
        _lib.check(_ctx().stencil_wo.sgp_logpdf_grad_stencil_wo(*args, ptrs, pw, po), "sgp_logpdf_grad_stencil_wo")
    else:
        _lib.check(_ctx().stencil_grad.sgp_logpdf_grad_stencil(*args, ptrs), "sgp_logpdf_grad_stencil")
    xb = chain_input_gradients(spec, gx)[0] if inputs else None
    rec = _grad_record(spec, kind, lp[0], bufs, gx, xb)
    if stencils:
        rec["stencils"] = list(_attach_stencil_gradients(rec["terms"], spec, gw, go, {}).values())
        rec["_raw_stencils"] = (gw, go)
    return rec


def logpdf_and_gradient_batch(fxs, ys, return_infos=False):
    """[logpdf_and_gradient(fx, y) for fx, y in zip(fxs, ys)] in ONE library call (sgp_logpdf_grad_batch): the step of several
    independent hyper-parameter chains at once -- restarts, cross-validation folds, a population of candidates.  Members of one
    padded size with scalar / diagonal noise are factored as one task pool of the dataflow kernel and their C^-1 computed by
    one launch; every dict holds what the member's own `logpdf_and_gradient(fx, y)` returns (inputs=False, scales=False), bit
    for bit.  A member that is not positive definite gives a dict with logpdf = NaN, `info` = its LAPACK info and no
    gradients, instead of raising; return_infos=True also returns the infos as an array."""
    fxs, ys = list(fxs), list(ys)
    if len(fxs) != len(ys):
        raise ValueError("logpdf_and_gradient_batch: one y per model")
    if not fxs:
        return ([], np.zeros(0, dtype=np.int32)) if return_infos else []
    keep, _ = _members("logpdf_and_gradient_batch", fxs, ys, True, False)
    kinds = {k[2] for k in keep}
    if len(kinds) != 1 or _lib.NOISE_DENSE in kinds:
        # mixed or dense noise kinds: member by member (same values; sgp_logpdf_grad_batch takes one noise kind)
        res, infos = [], []
        for fx, y, k in zip(fxs, ys, keep):
            try:
                res.append(logpdf_and_gradient(fx, y))
                infos.append(0)
            except _lib.PosDefException as e:
                res.append(_grad_failed(k[0], e.info))
                infos.append(e.info)
        return (res, np.array(infos, dtype=np.int32)) if return_infos else res

    def call(specs, means, _, noises, yp, lp, outs, infos):
        rc = _ctx().batch.sgp_logpdf_grad_batch(_ctx().handle, len(keep), specs, means, kinds.pop(), noises, yp, lp, *outs, infos)
        _lib.check(rc, "sgp_logpdf_grad_batch")

    res, infos = _grad_members(keep, call)
    return (res, infos) if return_infos else res


def _pool_report(rep):
    return dict(pool_launches=int(rep.pool_launches), pooled_members=int(rep.pooled_members),
                single_members=int(rep.single_members), distinct_sizes=int(rep.distinct_sizes))


def _pool_result(vals, infos, rep, return_infos, return_report):
    res = (vals,)
    if return_infos:
        res += (infos,)
    if return_report:
        res += (rep,)
    return res if len(res) > 1 else vals


def logpdf_pool(fxs, ys, return_infos=False, return_report=False):
    """[logpdf(fx, y) for fx, y in zip(fxs, ys)] in ONE library call (sgp_logpdf_pool) for members of DIFFERENT sizes and
    noise kinds -- folds that straddle a tile boundary, a learning curve N = 512 ... 8192, one GP per series.  Members with
    scalar or diagonal noise are factored as ONE ragged task pool of the dataflow kernel, each in the geometry of its own
    call; a dense-noise or posterior member goes down as dense noise and runs through its own call inside the library.
    Every value is bit-equal to the member's own `logpdf`.  A Float32 model is evaluated by its own `logpdf` (the fp32
    kernels) and its value widened, so that contract holds for it too; the report counts it as single.  A member that is
    not positive definite gives NaN (return_infos=True: its LAPACK info) instead of raising.  return_report=True adds a dict:
    pool_launches, pooled_members, single_members, distinct_sizes."""
    fxs, ys = list(fxs), list(ys)
    if len(fxs) != len(ys):
        raise ValueError("logpdf_pool: one y per model")
    n_all = len(fxs)
    vals = np.zeros(n_all)
    infos = np.zeros(n_all, dtype=np.int32)
    rep = dict(pool_launches=0, pooled_members=0, single_members=0, distinct_sizes=0)
    keep, down = _members("logpdf_pool", fxs, ys, False, True)
    for b, (fx, y) in enumerate(zip(fxs, ys)):
        if b in down:
            continue
        try:                         # a Float32 model: its own call, widened
            vals[b] = float(logpdf(fx, y))
        except _lib.PosDefException as e:
            vals[b], infos[b] = float("nan"), e.info
        rep["single_members"] += 1
    if keep:
        out = np.zeros(len(keep))
        inf = np.zeros(len(keep), dtype=np.int32)
        crep = _lib.sgp_pool_report()
        rc = _ctx().pool.sgp_logpdf_pool(_ctx().handle, len(keep), *_member_args(keep), _lib.dptr(out), _iptr(inf),
                                         C.byref(crep))
        _lib.check(rc, "sgp_logpdf_pool")
        vals[down], infos[down] = out, inf
        for k, v in _pool_report(crep).items():
            rep[k] += v
    return _pool_result(vals, infos, rep, return_infos, return_report)


def logpdf_and_gradient_pool(fxs, ys, return_infos=False, return_report=False):
    """[logpdf_and_gradient(fx, y) for fx, y in zip(fxs, ys)] in ONE library call (sgp_logpdf_grad_pool) for members of
    DIFFERENT sizes and noise kinds: one ragged launch of the dataflow kernel factors every poolable member's matrix, (y - m)'
    row and inv(L)', C^-1 is one launch per distinct padded size.  Every dict holds what the member's own
    `logpdf_and_gradient(fx, y)` returns (inputs=False, scales=False), bit for bit; a member that is not positive definite
    gives a dict with logpdf = NaN, `info` and no gradients.  A Float32 model is evaluated by its own call (counted as
    single).  return_infos / return_report as in `logpdf_pool`."""
    fxs, ys = list(fxs), list(ys)
    if len(fxs) != len(ys):
        raise ValueError("logpdf_and_gradient_pool: one y per model")
    n_all = len(fxs)
    infos = np.zeros(n_all, dtype=np.int32)
    rep = dict(pool_launches=0, pooled_members=0, single_members=0, distinct_sizes=0)
    res = [None] * n_all
    keep, down = _members("logpdf_and_gradient_pool", fxs, ys, True, True)
    for b, (fx, y) in enumerate(zip(fxs, ys)):
        if b in down:
            continue
        try:
            res[b] = logpdf_and_gradient(fx, y)
        except _lib.PosDefException as e:
            res[b], infos[b] = _grad_failed(_prior_spec(fx.f, fx.x), e.info), e.info
        rep["single_members"] += 1
    if keep:
        crep = _lib.sgp_pool_report()

        def call(specs, means, kinds, noises, yp, lp, outs, inf):
            rc = _ctx().pool.sgp_logpdf_grad_pool(_ctx().handle, len(keep), specs, means, kinds, noises, yp, lp, *outs, inf,
                                                  C.byref(crep))
            _lib.check(rc, "sgp_logpdf_grad_pool")

        got, inf = _grad_members(keep, call)
        for q, b in enumerate(down):
            res[b], infos[b] = got[q], inf[q]
        for k, v in _pool_report(crep).items():
            rep[k] += v
    return _pool_result(res, infos, rep, return_infos, return_report)


def _draw(rng, n, s):
    """Z = randn(rng, n, s) in Julia's column-major fill order, from the caller's RNG."""
    if hasattr(rng, "standard_normal"):
        z = rng.standard_normal(n * s)
    else:
        z = rng.randn(n * s)
    return np.asfortranarray(np.asarray(z, dtype=np.float64).reshape((n, s), order="F"))


def rand(rng, fx, S=None, Z=None):
    """rand(rng, fx) -> vector; rand(rng, fx, S) -> N x S.  m .+ L Z with Z from `rng`
    (pass Z explicitly to reuse a caller-side draw)."""
    if isinstance(fx, SparseFiniteGP):
        return rand(rng, fx.fobs, S, Z)     # sparse_finite_gp.jl:47-50: samples from the dense fobs
    n = len(fx)
    s = 1 if S is None else int(S)
    if Z is None:
        Z = _draw(rng, n, s)
    Z = _f64(np.asarray(Z, dtype=np.float64).reshape(n, s))
    route = _postfx_route(fx)
    if route is not None:
        lib, stem, h, cross, pss, ms, kind, nbuf = route
        out = np.zeros((n, s), order="F")
        rc = getattr(lib, stem + "_rand")(h, cross.ref(), pss.ref(), _lib.dptr(ms), kind, _lib.dptr(nbuf), _lib.dptr(Z), n, s,
                                          _lib.dptr(out), n)
        _lib.check(rc, stem + "_rand")
        if _eltype(fx.x) == np.float32:      # (as below: returned in the model's type)
            out = out.astype(np.float32)
        return out[:, 0].copy() if S is None else out
    spec, m, kind, nbuf = _spec_mean_noise(fx)
    m = _f64(m)
    if _is_prior(fx.f) and _eltype(fx.x) == np.float32 and kind != _lib.NOISE_DENSE and spec.f32_supported():
        # Float32 model: the fp32 factor and an fp32 MFMA product L Z (sgp_rand_f32); `rand(rng, fx) isa Vector{Float32}`
        out32 = np.zeros((n, s), dtype=np.float32, order="F")
        rc = _ctx().lib.sgp_rand_f32(_ctx().handle, spec.ref(), _lib.dptr(m), kind, _lib.dptr(nbuf), _lib.dptr(Z), n, s,
                                     out32.ctypes.data_as(C.POINTER(C.c_float)), n)
        _lib.check(rc, "sgp_rand_f32")
        return out32[:, 0].copy() if S is None else out32
    out = np.zeros((n, s), order="F")
    rc = _ctx().lib.sgp_rand(_ctx().handle, spec.ref(), _lib.dptr(m), kind, _lib.dptr(nbuf), _lib.dptr(Z), n, s,
                             _lib.dptr(out), n)
    _lib.check(rc, "sgp_rand")
    if _eltype(fx.x) == np.float32:      # Float32 model: computed in fp64 on the device, returned in the model's type
        out = out.astype(np.float32)
    return out[:, 0].copy() if S is None else out


# ---- posteriors --------------------------------------------------------------------------------
def _cross_side(post, xs, want_prior=True):
    """(cross, prior_ss or None, mean_s) of a kept posterior at the test points xs: the spec of K(x*, x) against the points
    the factor was made from, the symmetric spec of K(x*, x*) and the prior mean at x* -- what every entry point that reads
    the kept factor takes (predict, rand / logpdf of post(x*), the prediction gradients)."""
    cross, _, _ = build_spec(post.prior, xs, post.prior, post._train_inputs()[0])
    pss = _prior_spec(post.prior, xs) if want_prior else None
    return cross, pss, _f64(mean_vector(post.prior, xs))


class _KeptPosterior:
    """What the posteriors share: a handle `_h` on factors kept in HBM and the moments read off them.  A subclass gives
    `_stem` (its entry points are <stem>_predict, _destroy, and for rand / logpdf / the prediction gradients _rand, _logpdf,
    _predict_grad_x), `_train_inputs()`, `_ensure()` where its handle can be rebuilt, and -- where the cross side is not a
    pair of specs -- `_reader` and `_typed`."""

    _stem = "sgp_posterior"

    def _ensure(self):
        return self._h

    def __del__(self):  # pragma: no cover
        try:
            if self._h:
                getattr(_lib.load(), self._stem + "_destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def __call__(self, xs, noise=1e-18):
        return FiniteGP(self, xs, noise)

    def _reader(self, xs, want_var, want_cov):
        """(N*, call): call(handle, mean_out, var_out, cov_out, ldcov) -> (entry point, rc)"""
        cross, pss, ms = _cross_side(self, xs, want_var or want_cov)
        name = self._stem + "_predict"

        def call(h, *outs):
            return name, getattr(_ctx().lib, name)(h, cross.ref(), pss.ref() if pss is not None else None, _lib.dptr(ms), *outs)
        return cross.N, call

    def _typed(self, out, *xs):
        return _model_type(out, *xs, *self._train_inputs())

    def _predict(self, xs, want_mean, want_var, want_cov):
        ns, call = self._reader(xs, want_var, want_cov)
        mo = np.zeros(ns) if want_mean else None
        vo = np.zeros(ns) if want_var else None
        co = np.zeros((ns, ns), order="F") if want_cov else None
        name, rc = call(self._ensure(), _lib.dptr(mo), _lib.dptr(vo), _lib.dptr(co), max(ns, 1))
        _lib.check(rc, name)
        return mo, vo, co

    def mean(self, xs):
        return self._typed(self._predict(xs, True, False, False)[0], xs)

    def var(self, xs):
        return self._typed(self._predict(xs, False, True, False)[1], xs)

    def cov(self, xs, zs=None):
        if zs is None:
            return self._typed(self._predict(xs, False, False, True)[2], xs)
        # cov(post, x*, z*) = K(x*, z*) - V_x*' V_z*: the off-diagonal block of the joint covariance over [x*; z*]
        joint = self._predict(BlockData([xs, zs]) if not isinstance(xs, BlockData) else _concat(xs, zs),
                              False, False, True)[2]
        nx = len(xs)
        return self._typed(joint[:nx, nx:], xs, zs)

    def mean_and_var(self, xs):
        m, v, _ = self._predict(xs, True, True, False)
        return self._typed((m, v), xs)

    def mean_and_cov(self, xs):
        m, _, c = self._predict(xs, True, False, True)
        return self._typed((m, c), xs)


def _concat(xs, zs):
    zb = zs.X if isinstance(zs, BlockData) else [zs]
    return BlockData(list(xs.X) + list(zb))


# ---- exact posterior ---------------------------------------------------------------------------
class PosteriorGP(_KeptPosterior):
    """posterior(fx, y): keeps L and L^-1 (y - m) in HBM (sgp_post); data = (alpha, x, delta)."""

    def __init__(self, prior, x, handle, alpha, delta, noise=None, y=None, mean_x=None):
        self.prior, self.x, self._h, self._alpha, self.delta = prior, x, handle, alpha, delta
        self.noise, self.y = noise, y      # kept for sequential conditioning (posterior of a posterior)
        self._mean_x = mean_x

    def _ensure(self):
        """The fp64 factor in HBM.  A Float32 model (handle None at construction) answers mean / var from the fp32
        one-shot path (sgp_posterior_mean_var_f32) and only builds the fp64 factor when cov / alpha are asked for."""
        if self._h is None:
            n = len(self.y)
            spec = _prior_spec(self.prior, self.x)
            kind, nbuf = _lib._noise_args(self.noise, n)
            alpha = np.zeros(n)
            h = C.c_void_p()
            rc = _ctx().lib.sgp_posterior_create(_ctx().handle, spec.ref(), _lib.dptr(self._mean_x), kind, _lib.dptr(nbuf),
                                                 _lib.dptr(self.y), _lib.dptr(alpha), C.byref(h))
            _lib.check(rc, "sgp_posterior_create")
            self._h, self._alpha = h, alpha
        return self._h

    @property
    def alpha(self):
        self._ensure()
        return self._alpha

    def _train_inputs(self):
        return (self.x,)


def _stack_observations(p1, fx2, y2):
    """(x, Sigma_y, y) of the data a posterior was conditioned on followed by the observations fx2 / y2: the old points in
    their old block order, the new ones in further blocks.  Two equal scalar noises stay a scalar, a dense Sigma_y on either
    side makes the stacked noise dense (block diagonal), anything else a diagonal."""
    if p1.noise is None:
        raise NotImplementedError("this posterior does not carry its observation model")
    n1, n2 = len(p1.x), len(fx2)
    a1, a2 = np.asarray(p1.noise, dtype=np.float64), np.asarray(fx2.noise, dtype=np.float64)
    if a1.ndim > 1 or a2.ndim > 1:
        # a dense Sigma_y on either side: the stacked observation noise is block diagonal (dense noise kind)
        noise = np.zeros((n1 + n2, n1 + n2))
        noise[:n1, :n1] = _noise_dense(a1, n1)
        noise[n1:, n1:] = _noise_dense(a2, n2)
    elif a1.ndim == 0 and a2.ndim == 0 and float(a1) == float(a2):
        noise = float(a1)
    else:
        noise = np.concatenate([_noise_diag(a1, n1), _noise_diag(a2, n2)])
    x1 = p1.x if isinstance(p1.x, BlockData) else BlockData([p1.x])
    xx = _concat(x1, fx2.x)
    yy = np.concatenate([p1.y, np.asarray(y2, dtype=np.float64).ravel()])
    return xx, noise, yy


def posterior(fx, y, y_vfe=None):
    """posterior(fx, y)  |  posterior(VFE(fz), fx, y)  |  posterior(SparseFiniteGP, y)"""
    if isinstance(fx, VFE):                  # posterior(VFE(fz), fx, y)  (sparse_finite_gp.jl:60-62)
        return posterior_vfe(fx, y, y_vfe)
    if isinstance(fx, SparseFiniteGP):
        return posterior_vfe(VFE(fx.finducing), fx.fobs, y)
    if isinstance(fx.f, PosteriorGP):
        # Sequential conditioning (AbstractGPs: posterior(f_post(x2, s2), y2) is again a PosteriorGP): the
        # posterior given (x1, y1) and then (x2, y2) IS the prior conditioned on the stacked data, which is
        # one factorisation of the joint covariance on the device instead of a Schur-complement update.
        xx, noise, yy = _stack_observations(fx.f, fx, y)
        return posterior(FiniteGP(fx.f.prior, xx, noise), yy)
    if not _is_prior(fx.f):
        # a process that is not a prior Stheno process but answers mean / var / cov -- the approximate (VFE) posterior, which the
        # reference returns as an ordinary AbstractGP (sparse_finite_gp.jl:60-62): conditioned through explicit covariances
        return ExplicitPosteriorGP(fx.f, fx.x, fx.noise, y)
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    n = len(fx)
    if y.shape[0] != n:
        raise ValueError("length(y) != length(fx)")
    m = _f64(mean_vector(fx.f, fx.x))
    post = PosteriorGP(fx.f, fx.x, None, None, y - m, fx.noise, y.copy(), mean_x=m)
    # Factor ONCE, here, and keep the handle -- for Float32 models as well (advisor, round 3: a Float32 posterior used to
    # re-assemble and re-factorise the whole covariance in fp32 on EVERY mean / var call, reported a covariance that is not
    # positive definite only at the first prediction, and switched to fp64-rounded values once `cov` / `alpha` had built
    # the fp64 factor, so a result depended on the call history).  Every prediction now runs against this one fp64
    # factor; Float32 models get their results rounded by the one output-type rule (_model_type).  The one-shot fp32
    # path (one fp32 factorisation with x* riding along as bordered rows) is the explicit posterior_mean_and_var_f32.
    post._ensure()                 # PosDefException here, as `cholesky` throws in the reference's posterior
    return post


def update_posterior(post, fx2, y2=None, reserve=None):
    """update_posterior(f_post, fx2, y2) [AbstractGPs]: the posterior given the data of `post` AND the observations y2 of
    fx2 = f(x2, s2), by extending the kept Cholesky factor with the rows of the new data (sgp_posterior_extend:
    O(N^2 k + N k^2 + k^3) for k new points) instead of factoring the stacked covariance from scratch.

    Returns a PosteriorGP on the stacked data that TAKES OVER the factor in HBM; `post` stays usable -- it rebuilds a factor
    of its own the next time it is asked something.  reserve: the number of points the factor buffer is sized for when it
    has to grow (a loop that keeps adding points passes the size it will reach and pays one reallocation).
    A dense Sigma_y on either side or a multi-GPU context go through the stacked one-shot `posterior` -- the same posterior, to rounding.  A stacked covariance that is not positive definite raises
    PosDefException with the failing leading minor; `post` is then exactly what it was.

    A VFE posterior (posterior(VFE(fz), fx, y)) takes the two AbstractGPs methods of its own: update_posterior(post, fx2, y2)
    absorbs the new data with the inducing points fixed (_update_vfe_data), update_posterior(post, fz_new) re-conditions the
    data already seen on new inducing points (_update_vfe_inducing)."""
    if isinstance(post, ApproxPosteriorGP):
        return _update_vfe_inducing(post, fx2) if y2 is None else _update_vfe_data(post, fx2, y2)
    if not isinstance(post, PosteriorGP):
        raise TypeError("update_posterior extends an exact PosteriorGP (posterior(fx, y)) or a VFE posterior")
    if y2 is None:
        raise TypeError("update_posterior(f_post, fx2, y2): y2 is missing (only a VFE posterior takes update_posterior(post, fz_new))")
    if not isinstance(fx2, FiniteGP) or not (fx2.f is post.prior or fx2.f is post):
        raise ValueError("update_posterior: fx2 must be the posterior's prior process (or the posterior itself) at the new points")
    xx, noise, yy = _stack_observations(post, fx2, y2)
    n = len(yy)
    if len(fx2) != n - len(post.y):
        raise ValueError("length(y2) != length(fx2)")
    if np.ndim(noise) > 1 or getattr(_ctx(), "is_multi", False):
        return posterior(FiniteGP(post.prior, xx, noise), yy)
    spec = _prior_spec(post.prior, xx)
    m = _f64(mean_vector(post.prior, xx))
    yy = _f64(yy)
    kind, nbuf = _lib._noise_args(noise, n)
    alpha, lp = np.zeros(n), np.zeros(1)
    reserve_n = 0 if reserve is None else max(int(reserve), n)
    h = post._ensure()
    rc = _ctx().extend.sgp_posterior_extend(h, spec.ref(), _lib.dptr(m), kind, _lib.dptr(nbuf), _lib.dptr(yy), n - len(post.y),
                                            reserve_n, _lib.dptr(alpha), _lib.dptr(lp))
    _lib.check(rc, "sgp_posterior_extend")      # rc > 0: PosDefException(info); the old posterior is untouched
    post._h = None                              # the new object owns the factor; the old one rebuilds its own on demand
    new = PosteriorGP(post.prior, xx, h, alpha, yy - m, noise, yy.copy(), mean_x=m)
    new.logpdf_y = float(lp[0])                 # logpdf(f(x_all, Sigma_y), y_all): the call computes it on the way
    return new


def posterior_mean_and_var_f32(fx, y, xs):
    """mean_and_var(posterior(fx, y)(xs)) of a Float32 model in ONE fp32 factorisation (sgp_posterior_mean_var_f32: K(x*, x)
    rides through the fp32 Cholesky as bordered rows) -- the explicit fast path for "condition once, predict once"; nothing
    is kept.  fx: FiniteGP of a prior process with scalar / diagonal noise within the fp32 kernels' limits."""
    if not _is_prior(fx.f):
        raise NotImplementedError("the fp32 one-shot posterior takes a prior process")
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    spec = _prior_spec(fx.f, fx.x)
    cross, _, _ = build_spec(fx.f, xs, fx.f, fx.x)
    pss = _prior_spec(fx.f, xs)
    _refuse_deriv("posterior_mean_and_var_f32: the fp32 path", spec, cross, pss)
    kind, nbuf = _lib._noise_args(fx.noise, len(y))
    if kind == _lib.NOISE_DENSE or not spec.f32_supported() or not cross.f32_supported():
        raise NotImplementedError("beyond the fp32 kernels' limits (dense noise, input dimension > 16, too many terms)")
    ns = cross.N
    m, ms = _f64(mean_vector(fx.f, fx.x)), _f64(mean_vector(fx.f, xs))
    mo32, vo32 = np.zeros(ns, dtype=np.float32), np.zeros(ns, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = _ctx().lib.sgp_posterior_mean_var_f32(_ctx().handle, spec.ref(), _lib.dptr(m), kind, _lib.dptr(nbuf), _lib.dptr(y),
                                               cross.ref(), pss.ref(), _lib.dptr(ms), fp(mo32), fp(vo32))
    _lib.check(rc, "sgp_posterior_mean_var_f32")
    return mo32, vo32


# ---- VFE / sparse --------------------------------------------------------------------------------
class VFE:
    def __init__(self, fz):
        self.fz = fz


class SparseFiniteGP:
    """SparseFiniteGP(fobs, finducing): logpdf == elbo, posterior == VFE posterior."""

    def __init__(self, fobs, finducing):
        self.fobs, self.finducing = fobs, finducing

    def __len__(self):
        return len(self.fobs)


_COV_ERR = ("The covariance matrix of a sparse GP can often be dense and can cause the computer to run out of "
            "memory. If you are sure you have enough memory, you can use `cov(f.fobs)`.")


def sparse_cov(f):
    raise RuntimeError(_COV_ERR)      # sparse_finite_gp.jl:39-43


def _vfe_args(vfe, fx):
    fz = vfe.fz
    if fz.f is not fx.f:
        raise AssertionError("VFE requires fz.f === fx.f")
    if not _is_prior(fx.f):
        raise NotImplementedError("VFE needs a prior Stheno process")
    n, m = len(fx), len(fz)
    zz = _prior_spec(fz.f, fz.x)
    xz, _, _ = build_spec(fx.f, fx.x, fz.f, fz.x)
    a = np.asarray(fx.noise, dtype=np.float64)
    if a.ndim > 1:
        raise ValueError("elbo needs isotropic or diagonal observation noise")
    nk, nbuf = _lib._noise_args(fx.noise, n)
    zk, zbuf = _lib._noise_args(fz.noise, m)
    mean_x = _f64(mean_vector(fx.f, fx.x))
    return zz, xz, mean_x, nk, nbuf, zk, zbuf


def elbo(vfe, fx, y=None):
    if isinstance(vfe, SparseFiniteGP):      # elbo(f::SparseFiniteGP, y)
        return elbo(VFE(vfe.finducing), vfe.fobs, fx)
    zz, xz, mean_x, nk, nbuf, zk, zbuf = _vfe_args(vfe, fx)
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    var_x = _f64(prior_var(fx.f, fx.x))
    out = np.zeros(1)
    rc = _ctx().lib.sgp_elbo(_ctx().handle, zz.ref(), xz.ref(), _lib.dptr(var_x), _lib.dptr(mean_x), nk,
                             _lib.dptr(nbuf), zk, _lib.dptr(zbuf), _lib.dptr(y), _lib.dptr(out))
    _lib.check(rc, "sgp_elbo")
    return float(out[0])


def _chain_keys(spec):
    """per term: (signature of its chain = the (kind, row_input, col_input, param) of every factor, its position in the chain,
    the index of the chain's head) -- a plain term is a chain of one.  Two chains of a pair may share a factor, so a factor is
    identified by its chain."""
    tp, keys = spec._term_ptr, [None] * spec.n_terms
    for p in range(len(tp) - 1):
        t = int(tp[p])
        while t < int(tp[p + 1]):
            e = t + 1
            while e < int(tp[p + 1]) and (spec._terms[e].kind & _lib.KIND_TIMES_PREV):
                e += 1
            sig = tuple((spec._terms[f].kind, spec._terms[f].row_input, spec._terms[f].col_input, spec._terms[f].param)
                        for f in range(t, e))
            for f in range(t, e):
                keys[f] = (sig, f - t, t)
            t = e
    return keys


def _term_records_kprod(spec, gc, gs, gp, symmetric=True):
    """_term_records in the chain form (a spec with product chains, or any spec of the *_param functions): one record per
    factor.  symmetric=False: every pair keeps its own records (K(x, z) of the ELBO, the diagonal)."""
    nrb, ncb = len(spec.row_len), len(spec.col_len)
    tp, out, index, rec_of = spec._term_ptr, [], {}, {}
    sid, keys = spec.term_scale_ids, _chain_keys(spec)
    for I in range(nrb):
        for J in range(min(I + 1, ncb) if symmetric else ncb):
            for t in range(tp[I * ncb + J], tp[I * ncb + J + 1]):
                T = spec._terms[t]
                sig, pos, head = keys[t]
                index[(I, J, sig, pos, sid[head][0], sid[head][1])] = rec_of[t] = len(out)
                out.append(dict(I=I, J=J, kind=T.kind & _lib.KIND_MASK, coef=spec._terms[head].coef, param=T.param,
                                row_input=T.row_input, col_input=T.col_input, row_scaled=sid[head][0] is not None,
                                col_scaled=sid[head][1] is not None, t=t, mirror_t=None, chain=rec_of[head], factor=pos,
                                d_coef=float(gc[t]), d_inscale=float(gs[t]), d_param=float(gp[t])))
    for I in range(nrb if symmetric else 0):
        for J in range(I + 1, ncb):
            for t in range(tp[I * ncb + J], tp[I * ncb + J + 1]):
                sig, pos, head = keys[t]
                msig = tuple((k, ci, ri, prm) for (k, ri, ci, prm) in sig)
                k = index.get((J, I, msig, pos, sid[head][1], sid[head][0]))
                if k is None:
                    raise AssertionError("symmetric spec without a mirror term: flattener invariant broken")
                out[k]["mirror_t"] = t
                out[k]["d_coef"] += float(gc[t])
                out[k]["d_inscale"] += float(gs[t])
                out[k]["d_param"] += float(gp[t])
    return out


def _deriv_sides(kind, param):
    """(p or None, q or None): the differentiated coordinate of the row / column side of a term of a derivative kind; None
    for every other kind"""
    if (int(kind) & _lib.KIND_MASK) not in _lib.DERIV_OF.values():
        return None
    a, b = divmod(int(param), _lib.DERIV_PARAM_BASE)
    return (a - 1 if a else None, b - 1 if b else None)


def _mirror_param(kind, param):
    """the param of a term's mirror image in pair (J, I): a derivative term's sides swap, every other param stays"""
    if _deriv_sides(kind, param) is None:
        return param
    a, b = divmod(int(param), _lib.DERIV_PARAM_BASE)
    return float(_lib.DERIV_PARAM_BASE * b + a)


def _swap_sides(key):
    """(row, col[, row stencil, col stencil]) of a term's geometry key seen from the mirror pair"""
    return key[1::-1] + key[:1:-1]


def _term_records(spec, gc, gs, symmetric, gp=None):
    """One record per flattened term.  For a symmetric spec the mirror-image pair (J, I) is folded
    into the lower pair (I >= J).  The mirror of a term with row / column scale vectors (rs, cs) is
    the term of (J, I) with the inputs AND the scales swapped -- several terms of one block pair may
    differ only in their scales (f3 = f1 + sin * f1 over two blocks), so the scale identities are
    part of the match."""
    if gp is not None:
        return _term_records_kprod(spec, gc, gs, gp)
    nrb, ncb = len(spec.row_len), len(spec.col_len)
    tp, out, index = spec._term_ptr, [], {}
    sid = spec.term_scale_ids
    geo = [tuple(g) for g in spec.term_geoms]        # a patch term's geometries (None, None for a plain one) are part of it
    if spec.has_stencil:                             # ... and so are a stencil term's stencils: several terms of one pair may
        geo = [g + tuple(None if st is None else (st[0].shape, st[0].tobytes(), st[1].tobytes()) for st in sts)   # differ in
               for g, sts in zip(geo, spec.term_stencils)]                                                        # them alone
    for I in range(nrb):
        for J in range(ncb):
            for t in range(tp[I * ncb + J], tp[I * ncb + J + 1]):
                T = spec._terms[t]
                if symmetric and I < J:
                    continue
                index[(I, J, T.kind, T.row_input, T.col_input, T.param, sid[t][0], sid[t][1]) + geo[t]] = len(out)
                out.append(dict(I=I, J=J, kind=T.kind, coef=T.coef, row_input=T.row_input, col_input=T.col_input,
                                row_scaled=sid[t][0] is not None, col_scaled=sid[t][1] is not None,
                                t=t, mirror_t=None, d_coef=float(gc[t]), d_inscale=float(gs[t])))
                if _deriv_sides(T.kind, T.param) is not None:
                    out[-1]["deriv"] = _deriv_sides(T.kind, T.param)
                if spec.has_patch:
                    out[-1].update(row_geom=geo[t][0], col_geom=geo[t][1])
                if spec.has_stencil:
                    out[-1].update(row_stencil=spec.term_stencils[t][0], col_stencil=spec.term_stencils[t][1])
    if symmetric:
        for I in range(nrb):
            for J in range(I + 1, ncb):
                for t in range(tp[I * ncb + J], tp[I * ncb + J + 1]):
                    T = spec._terms[t]
                    k = index.get((J, I, T.kind, T.col_input, T.row_input, _mirror_param(T.kind, T.param), sid[t][1], sid[t][0]) +
                                  _swap_sides(geo[t]))
                    if k is None:
                        raise AssertionError("symmetric spec without a mirror term: flattener invariant broken")
                    out[k]["mirror_t"] = t
                    out[k]["d_coef"] += float(gc[t])
                    out[k]["d_inscale"] += float(gs[t])
    return out


def _scale_arrays(spec, side):
    """one zero array per term that carries a row ("row") / column ("col") scale vector, None elsewhere + the ctypes
    pointer table"""
    nt = max(1, spec.n_terms)
    vecs = spec.term_row_scale if side == "row" else spec.term_col_scale
    arrs = [None] * nt
    for t in range(spec.n_terms):
        if vecs[t] is not None:
            arrs[t] = np.zeros(len(vecs[t]))
    return arrs, (C.POINTER(C.c_double) * nt)(*[_lib.dptr(a) if a is not None else None for a in arrs])


def _elbo_grad_specs(vfe, fx, y):
    """What every ELBO gradient does before its family's refusals: _vfe_args, y as a float64 vector and the spec of
    diag K(x,x) -> the specs (zz, xz, xx) the refusals look at, and what _elbo_grad_frame goes on from."""
    zz, xz, *rest = _vfe_args(vfe, fx)
    yv = _f64(np.asarray(y, dtype=np.float64).ravel())
    return (zz, xz, _prior_spec(fx.f, fx.x)), (len(fx), len(vfe.fz), yv, *rest)


def _elbo_grad_frame(specs, head, per_term=2):
    """... and after them: var(f, x) (a library call: sgp_kernelmatrix_diag), the output buffers, per spec the per-term arrays
    (gc, gs), with per_term=3 (gc, gs, gp), and the leading arguments of the two calls every family makes:
    `args`, those of its sgp_elbo_grad* entry point (context through grad_z_noise, then the per-term arrays of zz and of xz),
    and `dargs`, those of its sgp_kernelmatrix_diag_grad* entry point (context, xx, the weights d elbo / d var, the per-term
    arrays of xx).  A caller adds its tail pointers and names its entry points."""
    (zz, xz, xx), (n, m, yv, mean_x, nk, nbuf, zk, zbuf) = specs, head
    var_x = _f64(_kernelmatrix_diag(xx))
    out = np.zeros(1)
    gy, gm, gv = np.zeros(n), np.zeros(n), np.zeros(n)
    gn = np.zeros(n if nk == _lib.NOISE_DIAG else 1)
    gzn = np.zeros((m, m), order="F") if zk == _lib.NOISE_DENSE else np.zeros(m if zk == _lib.NOISE_DIAG else 1)
    raw = {k: tuple(np.zeros(max(1, sp.n_terms)) for _ in range(per_term)) for k, sp in zip(("zz", "xz", "xx"), specs)}
    d = _lib.dptr
    args = (_ctx().handle, zz.ref(), xz.ref(), d(var_x), d(mean_x), nk, d(nbuf), zk, d(zbuf), d(yv), d(out), d(gy), d(gm),
            d(gn), d(gv), d(gzn)) + tuple(d(a) for a in raw["zz"] + raw["xz"])
    dargs = (_ctx().handle, xx.ref(), d(gv)) + tuple(d(a) for a in raw["xx"])
    return dict(specs=specs, args=args, dargs=dargs, out=out, bufs=(gy, gm, gn, gv, gzn), raw=raw, kinds=(nk, zk))


def _elbo_scale_arrays(specs):
    """the five places the bound reads a function-valued scale -- zz rows, xz rows, xz columns, xx rows, xx columns: their
    _scale_arrays -> (the five lists of arrays, the five pointer tables)"""
    zz, xz, xx = specs
    both = [_scale_arrays(sp, side) for sp, side in ((zz, "row"), (xz, "row"), (xz, "col"), (xx, "row"), (xx, "col"))]
    return [a for a, _ in both], [p for _, p in both]


def _elbo_grad_result(F, gin=(None, None, None), scale_arrs=None):
    """The dict every ELBO gradient returns, from its frame after the two calls.  gin: the input-gradient arrays of
    (zz, xz, xx) where they were asked for: their chain rule back onto the blocks of fx.x and fz.x gives `x` and `z` (no
    xx arrays -- the _conv family forms none -- no `x`).  scale_arrs: the arrays of _elbo_scale_arrays."""
    (zz, xz, xx), (gy, gm, gn, gv, gzn), raw, (nk, zk) = F["specs"], F["bufs"], F["raw"], F["kinds"]
    records = _term_records if len(raw["zz"]) == 2 else _term_records_kprod
    xx_terms = [r for r in records(xx, *raw["xx"], False) if r["I"] == r["J"]] if len(xx.row_len) else []
    gxz, gxx, gdx = gin
    xb = zb = None
    if gxz is not None:   # chain rule back onto the blocks of fx.x and fz.x (through every factor's own view)
        zr, _ = chain_input_gradients(zz, gxz)
        xr, zc = chain_input_gradients(xz, gxx)
        zb = [a + b for a, b in zip(zr, zc)]
        if gdx is not None:
            xd, _ = chain_input_gradients(xx, gdx)
            xb = [a + b for a, b in zip(xr, xd)]
    S = scale_arrs
    return dict(elbo=float(F["out"][0]), y=gy, mean=gm, noise=(gn if nk == _lib.NOISE_DIAG else float(gn[0])), x=xb, z=zb,
                z_noise=(gzn if zk != _lib.NOISE_SCALAR else float(gzn[0])), var=gv,
                zz_terms=records(zz, *raw["zz"], True), xz_terms=records(xz, *raw["xz"], False),
                xx_terms=xx_terms, zz_inputs=gxz, xz_inputs=gxx,
                scales=(_scale_records(zz, S[0], more=((xz, S[1], "row"), (xz, S[2], "col"), (xx, S[3], "row"), (xx, S[4], "col")))
                        if S else None),
                _raw=raw, _specs=dict(zz=zz, xz=xz, xx=xx),
                # the library's per-term scale arrays (zz rows, xz rows, xz columns, xx rows, xx columns; None without
                # scales=True) and the diagonal's input arrays, as they came back: what `scales`, `x` and `z` are built from
                _scale_arrays=S, _xx_inputs=gdx)


def elbo_and_gradient(vfe, fx, y=None, inputs=False, scales=False):
    """elbo(VFE(fz), fx, y) and its reverse-mode gradient (what Zygote derives through
    AbstractGPs.elbo on the reference path; sgp_elbo_grad).

    Returns a dict: elbo; y, mean (N each); noise (scalar or N); z_noise (scalar, M, or M x M for a dense Sigma_z:
    d/d Sigma_z);
    zz_terms / xz_terms / xx_terms: per flattened covariance term of K(z,z), K(x,z) and diag K(x,x)
    {I, J, kind, coef, row_input, col_input, d_coef, d_inscale} (see logpdf_and_gradient).
    inputs=True adds zz_inputs / xz_inputs: d elbo / d (input points) per entry of
    g["_specs"]["zz"].inputs and g["_specs"]["xz"].inputs (the inducing points appear in both).
    scales=True adds `scales`: one record per function-valued scale (`sigma * f`, product.jl:25-48) and input collection
    it is mapped over -- {node, x, values, d_values} with d_values[i] = d elbo / d sigma(x_i), summed over the three
    places the bound reads sigma: K(z,z), K(x,z) (row side at x, column side at z) and diag K(x,x)."""
    if isinstance(vfe, SparseFiniteGP):
        return elbo_and_gradient(VFE(vfe.finducing), vfe.fobs, fx, inputs=inputs, scales=scales)
    specs, head = _elbo_grad_specs(vfe, fx, y)
    _refuse_deriv("elbo_and_gradient", *specs)
    _refuse_patch_gradient(*specs)
    _refuse_product_gradient("elbo_and_gradient", *specs)
    F = _elbo_grad_frame(specs, head)
    lib, args, dargs = _ctx().lib, F["args"], F["dargs"]
    # (inputs: var(f, x) depends on x wherever a diagonal term reads two different views of x; scales: and on sigma(x):
    # var_i = sum_t coef rs_i cs_i k_t)
    (gxz, pz), (gxx, px), (gdx, pd) = [_input_buffers(sp) if inputs else (None, None) for sp in specs]
    S, (prz, prx, pcx, pdr, pdc) = _elbo_scale_arrays(specs) if scales else (None, [None] * 5)
    if scales:
        _lib.check(lib.sgp_elbo_grad_xs(*args, pz, px, prz, prx, pcx), "sgp_elbo_grad_xs")
        rc = lib.sgp_kernelmatrix_diag_grad_xs(*dargs, pd, pdr, pdc)
    elif inputs:
        _lib.check(lib.sgp_elbo_grad_x(*args, pz, px), "sgp_elbo_grad_x")
        rc = lib.sgp_kernelmatrix_diag_grad_x(*dargs, pd)
    else:
        _lib.check(lib.sgp_elbo_grad(*args), "sgp_elbo_grad")
        rc = lib.sgp_kernelmatrix_diag_grad(*dargs)
    _lib.check(rc, "sgp_kernelmatrix_diag_grad")
    return _elbo_grad_result(F, (gxz, gxx, gdx), S)


def _patched_inputs(spec):
    """the inputs of `spec` that a patched side reads: they hold images"""
    out = set()
    for t, (rg, cg) in enumerate(spec.term_geoms):
        if rg is not None:
            out.add(int(spec._terms[t].row_input))
        if cg is not None:
            out.add(int(spec._terms[t].col_input))
    return out


def elbo_and_gradient_conv(vfe, fx, y=None, inputs=False):
    """elbo_and_gradient for every model it takes (without a product of kernels) AND for models with patch_convolve
    (convolutional) terms, through sgp_elbo_grad_conv and sgp_kernelmatrix_diag_grad_conv (include/sthenomi_conv_grad.h): the
    same dict (see elbo_and_gradient; `scales` is None).  inputs=True adds zz_inputs / xz_inputs -- an entry that holds images
    (an input read by a patched side) is None -- and `z`: the gradient with respect to the inducing points, block by block
    of fz.x, for the blocks no patched side reads (the inducing patches of the plain process under patch_convolve); the
    other blocks are zeros.  `x` is None: gradients with respect to the observed images are not formed.  Single-GPU
    contexts, no stencil terms."""
    if isinstance(vfe, SparseFiniteGP):
        return elbo_and_gradient_conv(VFE(vfe.finducing), vfe.fobs, fx, inputs=inputs)
    specs, head = _elbo_grad_specs(vfe, fx, y)
    _refuse_conv_family("elbo_and_gradient_conv", *specs)
    _refuse_product_gradient("elbo_and_gradient_conv", *specs)
    F = _elbo_grad_frame(specs, head)
    lib = _ctx().conv_grad
    (gxz, pz), (gxx, px) = [_input_buffers(sp) if inputs else (None, None) for sp in specs[:2]]
    _lib.check(lib.sgp_elbo_grad_conv(*F["args"], pz, px), "sgp_elbo_grad_conv")
    _lib.check(lib.sgp_kernelmatrix_diag_grad_conv(*F["dargs"]), "sgp_kernelmatrix_diag_grad_conv")
    return _elbo_grad_result(F, (gxz, gxx, None))


def elbo_and_gradient_stencil(vfe, fx, y=None, inputs=False, stencils=False):
    """elbo_and_gradient for every model it takes (without a product of kernels) AND for models with stencil terms (`stencil`,
    `quadrature_convolve`) or patch_convolve terms, through sgp_elbo_grad_stencil and sgp_kernelmatrix_diag_grad_stencil
    (include/sthenomi_stencil_grad.h): the same dict (see elbo_and_gradient; `scales` is None).  inputs=True adds zz_inputs /
    xz_inputs, `x` and `z` as elbo_and_gradient does -- a stencil side's stored points are the unshifted ones, so the chain back
    onto the blocks of fx.x and fz.x is that of a plain term; an entry that holds images (an input read by a patched side) is
    None and contributes nothing.  Single-GPU contexts.

    stencils=True adds the gradients with respect to the stencils' own weights and offsets, through sgp_elbo_grad_stencil_wo
    and sgp_kernelmatrix_diag_grad_stencil_wo (include/sthenomi_stencil_wo.h), as logpdf_and_gradient_stencil does: the records
    of zz_terms / xz_terms / xx_terms carry d_row_weights, d_row_offsets, d_col_weights, d_col_offsets, and `stencils` holds
    one entry per stencil node, summed over the three places the bound reads it (K(z,z), K(x,z), diag K(x,x))."""
    if isinstance(vfe, SparseFiniteGP):
        return elbo_and_gradient_stencil(VFE(vfe.finducing), vfe.fobs, fx, inputs=inputs, stencils=stencils)
    specs, head = _elbo_grad_specs(vfe, fx, y)
    _refuse_stencil_family("elbo_and_gradient_stencil", *specs)
    _refuse_product_gradient("elbo_and_gradient_stencil", *specs)
    F = _elbo_grad_frame(specs, head)
    zz, xz, xx = specs
    # (var(f, x) depends on x wherever a diagonal term reads two different views of x)
    (gxz, pz), (gxx, px), (gdx, pd) = [_input_buffers(sp) if inputs else (None, None) for sp in specs]
    if stencils:
        wo = _ctx().stencil_wo
        tz, tx, td = _stencil_tables(zz), _stencil_tables(xz), _stencil_tables(xx)
        _lib.check(wo.sgp_elbo_grad_stencil_wo(*F["args"], pz, px, tz[2], tz[3], tx[2], tx[3]), "sgp_elbo_grad_stencil_wo")
        _lib.check(wo.sgp_kernelmatrix_diag_grad_stencil_wo(*F["dargs"], pd, td[2], td[3]),
                   "sgp_kernelmatrix_diag_grad_stencil_wo")
    else:
        lib = _ctx().stencil_grad
        _lib.check(lib.sgp_elbo_grad_stencil(*F["args"], pz, px), "sgp_elbo_grad_stencil")
        _lib.check(lib.sgp_kernelmatrix_diag_grad_stencil(*F["dargs"], pd), "sgp_kernelmatrix_diag_grad_stencil")
    rec = _elbo_grad_result(F, (gxz, gxx, gdx))
    if stencils:
        nodes = {}
        for key, sp, tb in (("zz_terms", zz, tz), ("xz_terms", xz, tx), ("xx_terms", xx, td)):
            _attach_stencil_gradients(rec[key], sp, tb[0], tb[1], nodes)
        rec["stencils"] = list(nodes.values())
        rec["_raw_stencils"] = dict(zz=tz[:2], xz=tx[:2], xx=td[:2])
    return rec


def elbo_and_gradient_param(vfe, fx, y=None, inputs=False, scales=False):
    """elbo_and_gradient for every model it takes AND for models with a product of kernels, through sgp_elbo_grad_param and
    sgp_kernelmatrix_diag_grad_param (include/sthenomi_kprod_grad.h): the same dict, with zz_terms / xz_terms / xx_terms in
    the chain form (`chain`, `factor`, `d_param`; see logpdf_and_gradient) and `_raw` carrying the d / d param arrays.
    With inputs=True the records of factors behind a LinearTransform / ARDTransform carry `d_transform` per spec (see
    logpdf_and_gradient_param): the derivative of the bound is the sum over the three specs' distinct chains.
    Single-GPU contexts; no patch / stencil terms."""
    if isinstance(vfe, SparseFiniteGP):
        return elbo_and_gradient_param(VFE(vfe.finducing), vfe.fobs, fx, inputs=inputs, scales=scales)
    specs, head = _elbo_grad_specs(vfe, fx, y)
    _refuse_param_family("elbo_and_gradient_param", *specs)
    F = _elbo_grad_frame(specs, head, per_term=3)
    lib = _ctx().kprod_grad
    # (var(f, x) depends on x where a factor reads two views)
    (gxz, pz), (gxx, px), (gdx, pd) = gin = [_input_buffers(sp) if inputs else (None, None) for sp in specs]
    S, (prz, prx, pcx, pdr, pdc) = _elbo_scale_arrays(specs) if scales else (None, [None] * 5)
    _lib.check(lib.sgp_elbo_grad_param(*F["args"], pz, px, prz, prx, pcx), "sgp_elbo_grad_param")
    _lib.check(lib.sgp_kernelmatrix_diag_grad_param(*F["dargs"], pd, pdr, pdc), "sgp_kernelmatrix_diag_grad_param")
    rec = _elbo_grad_result(F, (gxz, gxx, gdx), S)
    if inputs:
        for key, sp, (g, _) in zip(("zz_terms", "xz_terms", "xx_terms"), specs, gin):
            _attach_d_transform(rec[key], sp, g)
    return rec


class ApproxPosteriorGP(_KeptPosterior):
    """posterior(VFE(fz), fx, y): keeps Lz, the factor of A A' + I and the sums over the data points in HBM (sgp_sparse_post).
    vfe / batches: the VFE object and the observation batches (x, Sigma_y, y) it was conditioned on, by reference -- what
    update_posterior needs to rebuild a posterior whose handle moved on, or to re-condition on other inducing points."""

    _stem = "sgp_sparse_posterior"

    def __init__(self, prior, z, handle, vfe=None, batches=None, created=None):
        self.prior, self.z, self._h = prior, z, handle
        self.vfe, self.batches = vfe, batches
        # the leading batches that went through the handle's create call (the later ones through updates), and
        # 1/2 sum var / s2 over them -- the term sgp_sparse_posterior_update's elbo_out cannot know (_create_trace)
        self._created = len(batches) if (created is None and batches) else created
        self._trace0 = None

    def _ensure(self):
        """The factors in HBM: a posterior whose handle update_posterior handed to its successor rebuilds one of its own
        from the stacked batches the next time it is asked something."""
        if self._h is None:
            if self.vfe is None or not self.batches:
                raise NotImplementedError("this sparse posterior does not carry its observations")
            self._h = _vfe_create(self.vfe, _stacked_fx(self.prior, self.batches), _stacked_y(self.batches))
            self._created, self._trace0 = len(self.batches), None
        return self._h

    def _create_trace(self):
        """sum_n var(f, x_n) / s2_n over the points the handle's create call was given (it takes no var_x)"""
        if self._trace0 is None:
            t = 0.0
            for x, s, _ in self.batches[:self._created]:
                t += float(np.sum(np.asarray(prior_var(self.prior, x), dtype=np.float64) / _noise_diag(s, len(x))))
            self._trace0 = t
        return self._trace0

    def _train_inputs(self):
        return (self.z,)


class ExplicitPosteriorGP(_KeptPosterior):
    """posterior(g(x2, S2), y2) for a process g whose covariance is not a sum of kernel terms (round 5): g answers
    mean / var / cov itself (the approximate posterior does, on the device); the factor of cov(g, x2) + S2 is built by
    sgp_posterior_create on the zero-term spec with dense noise, predictions go through sgp_posterior_predict_explicit with
    cov(g, x*, x2), var / cov(g, x*) and mean(g, x*) evaluated by g.  AbstractGPs [EXT]: posterior(fx::FiniteGP, y) for any
    AbstractGP; reference: test/gp/sparse_finite_gp.jl (the VFE posterior used as a GP)."""

    def __init__(self, base, x, noise, y):
        n = len(x)
        y = _f64(np.asarray(y, dtype=np.float64).ravel())
        if y.shape[0] != n:
            raise ValueError("length(y) != length(fx)")
        self.base, self.x, self.noise, self.y = base, x, noise, y
        m, Cm = base.mean_and_cov(x)
        self._mean_x = _f64(np.asarray(m, dtype=np.float64))
        Cm = np.asfortranarray(np.asarray(Cm, dtype=np.float64) + _noise_dense(noise, n))
        self._spec = zero_spec(n)
        alpha = np.zeros(n)
        h = C.c_void_p()
        rc = _ctx().lib.sgp_posterior_create(_ctx().handle, self._spec.ref(), _lib.dptr(self._mean_x), _lib.NOISE_DENSE,
                                             _lib.dptr(Cm), _lib.dptr(y), _lib.dptr(alpha), C.byref(h))
        _lib.check(rc, "sgp_posterior_create")
        self._h, self.alpha, self.delta = h, alpha, y - self._mean_x

    def _train_inputs(self):
        return (self.x,)

    def _reader(self, xs, want_var, want_cov):
        ns = len(xs)
        cross = np.asfortranarray(np.asarray(self.base.cov(xs, self.x), dtype=np.float64))       # ns x N
        ms = _f64(np.asarray(self.base.mean(xs), dtype=np.float64))
        pv = _f64(np.asarray(self.base.var(xs), dtype=np.float64)) if want_var else None
        pc = np.asfortranarray(np.asarray(self.base.cov(xs), dtype=np.float64)) if want_cov else None

        def call(h, *outs):
            rc = _ctx().lib.sgp_posterior_predict_explicit(h, _lib.dptr(cross), max(ns, 1), ns, _lib.dptr(pv), _lib.dptr(pc),
                                                           max(ns, 1), _lib.dptr(ms), *outs)
            return "sgp_posterior_predict_explicit", rc
        return ns, call

    def _typed(self, out, *xs):       # base answered in its own type
        return out


def _vfe_create(vfe, fx, y):
    zz, xz, mean_x, nk, nbuf, zk, zbuf = _vfe_args(vfe, fx)
    y = _f64(np.asarray(y, dtype=np.float64).ravel())
    h = C.c_void_p()
    rc = _ctx().lib.sgp_sparse_posterior_create(_ctx().handle, zz.ref(), xz.ref(), _lib.dptr(mean_x), nk,
                                                _lib.dptr(nbuf), zk, _lib.dptr(zbuf), _lib.dptr(y), C.byref(h))
    _lib.check(rc, "sgp_sparse_posterior_create")
    return h


def posterior_vfe(vfe, fx, y):
    h = _vfe_create(vfe, fx, y)
    return ApproxPosteriorGP(fx.f, vfe.fz.x, h, vfe=vfe, batches=[(fx.x, fx.noise, y)])


def _stacked_fx(prior, batches):
    """FiniteGP of the prior at the stacked inputs of the batches: one batch as it came, several as a BlockData of their
    blocks in order; two equal scalar noises stay a scalar, anything else becomes a diagonal."""
    if len(batches) == 1:
        return FiniteGP(prior, batches[0][0], batches[0][1])
    blocks = []
    for x, _, _ in batches:
        blocks += list(x.X) if isinstance(x, BlockData) else [x]
    ns = [np.asarray(s, dtype=np.float64) for _, s, _ in batches]
    if all(a.ndim == 0 and float(a) == float(ns[0]) for a in ns):
        noise = float(ns[0])
    else:
        noise = np.concatenate([_noise_diag(a, len(x)) for a, (x, _, _) in zip(ns, batches)])
    return FiniteGP(prior, BlockData(blocks), noise)


def _vfe_on_batches(vfe, prior, batches):
    """posterior(vfe, f(x_all, Sigma_y), y_all) on the stacked batches, which the new object keeps one by one: ALL of them
    went through its handle's create call (ApproxPosteriorGP._created, the points of _create_trace)."""
    fx = _stacked_fx(prior, batches)
    h = _vfe_create(vfe, fx, _stacked_y(batches))
    return ApproxPosteriorGP(prior, vfe.fz.x, h, vfe=vfe, batches=batches)


def _stacked_y(batches):
    return np.concatenate([np.asarray(y, dtype=np.float64).ravel() for _, _, y in batches])


def _check_vfe_batch(post, fx2):
    if not isinstance(fx2, FiniteGP) or fx2.f is not post.prior:
        raise ValueError("update_posterior: fx2 must be the sparse posterior's prior process at the new points")
    if np.asarray(fx2.noise, dtype=np.float64).ndim > 1:
        raise ValueError("elbo needs isotropic or diagonal observation noise")
    if post.vfe is None or not post.batches:
        raise NotImplementedError("this sparse posterior does not carry its observations")


def _update_vfe_data(post, fx2, y2):
    """update_posterior(f_post_approx, fx2, y2) [AbstractGPs, VFE]: the new rows join the sums the posterior keeps and
    A A' + I is factored afresh (sgp_sparse_posterior_update: O(n_new M^2 + M^3 / 3), whatever came before).  The returned
    ApproxPosteriorGP TAKES OVER the handle and carries elbo_y, the ELBO of all the data; `post` stays usable -- it rebuilds
    factors of its own from its batches the next time it is asked something.  A multi-GPU context goes through the stacked
    one-shot posterior(VFE, ...) and takes elbo_y from sgp_elbo on the stacked data."""
    _check_vfe_batch(post, fx2)
    y2 = _f64(np.asarray(y2, dtype=np.float64).ravel())
    n2 = len(fx2)
    if y2.shape[0] != n2:
        raise ValueError("length(y2) != length(fx2)")
    batches = list(post.batches) + [(fx2.x, fx2.noise, y2)]
    if getattr(_ctx(), "is_multi", False):
        new = _vfe_on_batches(post.vfe, post.prior, batches)
        new.elbo_y = elbo(post.vfe, _stacked_fx(post.prior, batches), _stacked_y(batches))   # (no update ran: sgp_elbo)
        return new
    fz = post.vfe.fz
    xz, _, _ = build_spec(fx2.f, fx2.x, fz.f, fz.x)
    kind, nbuf = _lib._noise_args(fx2.noise, n2)
    mean2 = _f64(mean_vector(fx2.f, fx2.x))
    var2 = _f64(prior_var(fx2.f, fx2.x))
    out = np.zeros(1)
    h = post._ensure()
    trace0 = post._create_trace()
    rc = _ctx().vfe_update.sgp_sparse_posterior_update(h, xz.ref(), _lib.dptr(var2), _lib.dptr(mean2), kind, _lib.dptr(nbuf),
                                                       _lib.dptr(y2), _lib.dptr(out))
    _lib.check(rc, "sgp_sparse_posterior_update")   # rc > 0: PosDefException(info); the old posterior is untouched
    post._h = None                                  # the new object owns the factors; the old one rebuilds its own on demand
    new = ApproxPosteriorGP(post.prior, post.z, h, vfe=post.vfe, batches=batches, created=post._created)
    new._trace0 = trace0
    # elbo(VFE(fz), f(x_all, Sigma_y), y_all): the call computes it on the way, up to the trace term of the points the
    # create call was given (it takes no var_x)
    new.elbo_y = float(out[0]) - 0.5 * trace0
    return new


def _update_vfe_inducing(post, fz_new):
    """update_posterior(f_post_approx, fz_new) [AbstractGPs, VFE]: the data already seen, conditioned on the inducing points
    of fz_new -- posterior(VFE(fz_new), f(x_all, Sigma_y), y_all) on the stacked kept batches, and that very call."""
    if not isinstance(fz_new, FiniteGP) or fz_new.f is not post.prior:
        raise ValueError("update_posterior: fz_new must be the sparse posterior's prior process at the new inducing points")
    if post.vfe is None or not post.batches:
        raise NotImplementedError("this sparse posterior does not carry its observations")
    return _vfe_on_batches(VFE(fz_new), post.prior, list(post.batches))
