"""ctypes binding of libsthenomi.so (include/sthenomi.h).

This is the only place the Python host touches native code.  There is deliberately no
CPU fallback: if the HIP library is missing or no gfx950 device is visible, every entry
point raises (`SthenoMIError`), so a silently-eager test run is impossible.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi.so")
BENCH_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_bench.so")
BATCH_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_batch.so")
POOL_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_pool.so")
EXTEND_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_extend.so")
EXTEND_BENCH_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_extend_bench.so")
POSTFX_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_postfx.so")
PREDGRAD_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_predgrad.so")
VFE_UPDATE_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_vfe_update.so")
CONV_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_conv.so")
CONV_GRAD_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_conv_grad.so")
STENCIL_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_stencil.so")
STENCIL_GRAD_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_stencil_grad.so")
STENCIL_WO_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_stencil_wo.so")
KPROD_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_kprod.so")
KPROD_GRAD_LIB_PATH = os.path.join(_HERE, "csrc", "libsthenomi_kprod_grad.so")

# kernel kinds / noise kinds (sthenomi.h enums)
SE, MATERN12, MATERN32, MATERN52, WHITE, CONST = range(6)
RQ, LINEAR = 6, 7                  # evaluated by the product-chain path only (include/sthenomi_kprod.h)
COSINE, GAMMAEXP = 16, 17          # the same path (8 .. 15 are no kinds)
MATERN_NU = 20                     # general-nu Matern, the same path (18, 19 are no kinds); nu in (0, MATERN_NU_MAX]
MATERN_NU_MAX = 32.0
KIND_TIMES_PREV = 0x100            # SGP_KIND_TIMES_PREV: the term multiplies the chain begun before it
KIND_MASK = 0xff
KPROD_MAX_FACTORS, KPROD_MAX_DIM = 8, 16      # include/sthenomi_kprod.h: the limits of a chain
NOISE_SCALAR, NOISE_DIAG, NOISE_DENSE = range(3)


class SthenoMIError(RuntimeError):
    pass


class PosDefException(SthenoMIError):
    """Mirrors LinearAlgebra.PosDefException(info) thrown by `cholesky` on the reference path."""

    def __init__(self, info, msg=""):
        super().__init__(f"PosDefException: matrix is not positive definite; "
                         f"Cholesky factorization failed (info={info}). {msg}")
        self.info = info


class sgp_input(C.Structure):
    _fields_ = [("dim", C.c_int64), ("n", C.c_int64), ("ld", C.c_int64),
                ("x", C.POINTER(C.c_double))]


class sgp_term(C.Structure):
    _fields_ = [("kind", C.c_int32), ("row_input", C.c_int32), ("col_input", C.c_int32),
                ("reserved", C.c_int32), ("coef", C.c_double), ("param", C.c_double),
                ("row_scale", C.POINTER(C.c_double)), ("col_scale", C.POINTER(C.c_double))]


class sgp_cov_spec(C.Structure):
    _fields_ = [("n_row_blocks", C.c_int32), ("n_col_blocks", C.c_int32),
                ("row_len", C.POINTER(C.c_int64)), ("col_len", C.POINTER(C.c_int64)),
                ("n_inputs", C.c_int32), ("inputs", C.POINTER(sgp_input)),
                ("term_ptr", C.POINTER(C.c_int32)), ("terms", C.POINTER(sgp_term)),
                ("symmetric", C.c_int32), ("reserved", C.c_int32)]


class sgp_panel_src(C.Structure):
    """a factored column panel, packed (sgp_dev_panel_update_batch)"""
    _fields_ = [("base", C.c_void_p), ("ld", C.c_int64), ("row0", C.c_int64), ("w", C.c_int64)]


class sgp_panel_dst(C.Structure):
    """an owned column panel, packed, and the range of sources applied to it"""
    _fields_ = [("base", C.c_void_p), ("ld", C.c_int64), ("c0", C.c_int64), ("w", C.c_int64),
                ("src_first", C.c_int32), ("src_count", C.c_int32)]


_lib = None
_lib_lock = threading.Lock()

_P = C.c_void_p
_D = C.POINTER(C.c_double)
_SIGS = {
    "sgp_abi_version": (C.c_int, []),
    "sgp_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "sgp_ctx_create_multi": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(_P)]),
    "sgp_ctx_ndev": (C.c_int, [_P]),
    "sgp_ctx_transport": (C.c_char_p, [_P]),
    "sgp_ctx_factor_schedule": (C.c_char_p, [_P, C.c_int64]),
    "sgp_ctx_factor_work": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sgp_cov_spec_suggest_order": (C.c_int, [C.POINTER(sgp_cov_spec), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sgp_ctx_multi_stats": (C.c_int, [_P, _D, C.c_int64, C.POINTER(C.c_int64)]),
    "sgp_ctx_multi_owners": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]),
    "sgp_ctx_multi_profile": (C.c_int, [_P, C.c_int]),
    "sgp_ctx_multi_profile_get": (C.c_int, [_P, _D, C.c_int64, C.POINTER(C.c_int64)]),
    "sgp_ctx_destroy": (C.c_int, [_P]),
    "sgp_ctx_trim": (C.c_int, [_P]),
    "sgp_ctx_stage_timing": (C.c_int, [_P, C.c_int]),
    "sgp_ctx_stage_ms": (C.c_int, [_P, _D]),
    "sgp_last_error": (C.c_char_p, []),
    "sgp_kernelmatrix": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int64]),
    "sgp_kernelmatrix_diag": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D]),
    "sgp_logpdf": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, C.c_int64,
                             C.c_int64, _D]),
    "sgp_logpdf_batch": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(sgp_cov_spec)), C.POINTER(_D), C.c_int, C.POINTER(_D),
                                   C.POINTER(_D), _D, C.POINTER(C.c_int)]),
    "sgp_logpdf_f32": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, _D]),
    "sgp_kernelmatrix_f32": (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(C.c_float), C.c_int64]),
    "sgp_rand_f32": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, C.c_int64, C.c_int64,
                               C.POINTER(C.c_float), C.c_int64]),
    "sgp_posterior_mean_var_f32": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, C.POINTER(sgp_cov_spec),
                                             C.POINTER(sgp_cov_spec), _D, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sgp_logpdf_grad": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D]),
    "sgp_logpdf_grad_x": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D,
                                    C.POINTER(_D)]),
    "sgp_logpdf_grad_xs": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D,
                                     C.POINTER(_D), C.POINTER(_D)]),
    "sgp_rand": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, C.c_int64, C.c_int64,
                           _D, C.c_int64]),
    "sgp_posterior_create": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, _D,
                                       C.POINTER(_P)]),
    "sgp_posterior_predict": (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D,
                                        _D, _D, _D, C.c_int64]),
    "sgp_posterior_predict_explicit": (C.c_int, [_P, _D, C.c_int64, C.c_int64, _D, _D, C.c_int64, _D, _D, _D, _D, C.c_int64]),
    "sgp_posterior_destroy": (C.c_int, [_P]),
    "sgp_elbo_grad": (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D, _D, C.c_int, _D, C.c_int,
                                _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D]),
    "sgp_elbo_grad_x": (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D, _D, C.c_int, _D, C.c_int,
                                  _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, C.POINTER(_D), C.POINTER(_D)]),
    "sgp_elbo_grad_xs": (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D, _D, C.c_int, _D, C.c_int,
                                   _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, C.POINTER(_D), C.POINTER(_D),
                                   C.POINTER(_D), C.POINTER(_D), C.POINTER(_D)]),
    "sgp_kernelmatrix_diag_grad_xs": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, _D, _D, C.POINTER(_D), C.POINTER(_D),
                                                C.POINTER(_D)]),
    "sgp_kernelmatrix_diag_grad": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, _D, _D]),
    "sgp_kernelmatrix_diag_grad_x": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, _D, _D, C.POINTER(_D)]),
    "sgp_elbo": (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D, _D, C.c_int,
                           _D, C.c_int, _D, _D, _D]),
    "sgp_sparse_posterior_create": (C.c_int, [_P, C.POINTER(sgp_cov_spec),
                                              C.POINTER(sgp_cov_spec), _D, C.c_int, _D, C.c_int,
                                              _D, _D, C.POINTER(_P)]),
    "sgp_sparse_posterior_predict": (C.c_int, [_P, C.POINTER(sgp_cov_spec),
                                               C.POINTER(sgp_cov_spec), _D, _D, _D, _D, C.c_int64]),
    "sgp_sparse_posterior_destroy": (C.c_int, [_P]),
    "sgp_dspec_create": (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(_P)]),
    "sgp_dspec_destroy": (C.c_int, [_P]),
    "sgp_geometry": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sgp_dev_logpdf": (C.c_int, [_P, _P, _P, _P, C.c_int, _D, _P, _P, C.c_int64, C.c_int64, _D, _D]),
    "sgp_dev_assemble_cols": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int64,
                                        C.c_int64, _P, C.c_int, _D, _P, _P, C.c_int64, C.c_int64,
                                        _P]),
    "sgp_dev_panel_factor": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _P,
                                       _P]),
    "sgp_dev_panel_update": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int64,
                                       C.c_int64, C.c_int64, C.c_int64, _P]),
    "sgp_dev_panel_update_batch": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int64, _P]),
    "sgp_dev_rowsumsq": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P]),
    "sgp_elbo_part_len": (C.c_int, [C.c_int64, C.POINTER(C.c_int64)]),
    "sgp_dev_elbo_partial": (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D, _D, C.c_int, _D,
                                       C.c_int, _D, _D, _P, C.c_int64]),
    "sgp_dev_elbo_finish": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _D]),
    "sgp_dev_assemble_cross_rows": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64, _P]),
    "sgp_dev_rows_dot": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "sgp_dev_rows_gram": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int64, _P]),
}
# include/sthenomi_bench.h: micro-benchmark / diagnosis / test hooks, exported by libsthenomi_bench.so (round 6), NOT by the product
# library -- bench.py, tools/ and the GPU tests reach them through bench_lib() / Context.bench
_SIGS_BENCH = {
    "sgp_bench_df_fallbacks": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "sgp_bench_multi_fault": (C.c_int, [_P, C.c_int, C.c_int64]),
    "sgp_bench_multi_broken": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "sgp_bench_multi_profile_pieces": (C.c_int, [_P, _D, C.c_int64, C.POINTER(C.c_int64)]),
    "sgp_bench_multi_stall": (C.c_int, [_P, C.c_int, C.c_int64, C.c_double]),
    "sgp_bench_mfma_f64": (C.c_int, [_P, C.c_int, _D, _D]),
    "sgp_bench_hbm": (C.c_int, [_P, C.c_int64, C.c_int, _D, _D]),
    "sgp_bench_potrf": (C.c_int, [_P, C.c_int, _D, C.POINTER(C.c_longlong)]),
    "sgp_bench_cumask": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(C.c_uint)]),
    "sgp_bench_potrf_contended": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int, C.c_int, _D, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "sgp_bench_gemm_stamps": (C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(C.c_longlong), C.c_int64, C.POINTER(C.c_int64)]),
    "sgp_bench_gemm": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, _D, _D]),
}

# include/sthenomi_batch.h: the batched gradient, exported by libsthenomi_batch.so (it links against the product library and
# works on its contexts) -- the host mirror reaches it through batch_lib() / Context.batch
_SIGS_BATCH = {
    "sgp_logpdf_grad_batch": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(sgp_cov_spec)), C.POINTER(_D), C.c_int,
                                        C.POINTER(_D), C.POINTER(_D), _D, C.POINTER(_D), C.POINTER(_D), C.POINTER(_D),
                                        C.POINTER(_D), C.POINTER(_D), C.POINTER(C.c_int)]),
}

# include/sthenomi_pool.h: independent models of DIFFERENT sizes and noise kinds in one call, exported by libsthenomi_pool.so
# (it links against the product library and works on its contexts) -- the host mirror reaches it through pool_lib() /
# Context.pool
class sgp_pool_report(C.Structure):
    _fields_ = [("pool_launches", C.c_int32), ("pooled_members", C.c_int32), ("single_members", C.c_int32),
                ("distinct_sizes", C.c_int32)]


_SIGS_POOL = {
    "sgp_logpdf_pool": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(sgp_cov_spec)), C.POINTER(_D), C.POINTER(C.c_int),
                                  C.POINTER(_D), C.POINTER(_D), _D, C.POINTER(C.c_int), C.POINTER(sgp_pool_report)]),
    "sgp_logpdf_grad_pool": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(sgp_cov_spec)), C.POINTER(_D), C.POINTER(C.c_int),
                                       C.POINTER(_D), C.POINTER(_D), _D, C.POINTER(_D), C.POINTER(_D), C.POINTER(_D),
                                       C.POINTER(_D), C.POINTER(_D), C.POINTER(C.c_int), C.POINTER(sgp_pool_report)]),
}

# include/sthenomi_extend.h: extending a kept factor with new data, exported by libsthenomi_extend.so (it links against the
# product library and works on its posteriors) -- update_posterior reaches it through extend_lib() / Context.extend
_SIGS_EXTEND = {
    "sgp_posterior_extend": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, C.c_int64, C.c_int64, _D, _D]),
}

# include/sthenomi_postfx.h: rand / logpdf of a posterior FiniteGP against the kept factor, exported by libsthenomi_postfx.so (it
# links against the product library and works on its posteriors) -- rand / logpdf reach it through postfx_lib() / Context.postfx
_POSTFX_RAND = (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, C.c_int64, C.c_int64, _D,
                          C.c_int64])
_POSTFX_LOGPDF = (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, C.c_int64, C.c_int64, _D])
_SIGS_POSTFX = {
    "sgp_posterior_rand": _POSTFX_RAND,
    "sgp_posterior_logpdf": _POSTFX_LOGPDF,
    "sgp_sparse_posterior_rand": _POSTFX_RAND,
    "sgp_sparse_posterior_logpdf": _POSTFX_LOGPDF,
}

# include/sthenomi_predgrad.h: posterior mean and variance with their gradients with respect to the test points, exported by
# libsthenomi_predgrad.so (it links against the product library and works on its posteriors) -- mean_and_var_and_gradient
# reaches it through predgrad_lib() / Context.predgrad
PREDGRAD_COL_CHUNK = 512                           # SGP_PREDGRAD_COL_CHUNK
_PREDGRAD = (C.c_int, [_P, C.POINTER(sgp_cov_spec), C.POINTER(sgp_cov_spec), _D, _D, _D, C.POINTER(_D), C.POINTER(_D),
                       C.POINTER(_D)])
_SIGS_PREDGRAD = {
    "sgp_posterior_predict_grad_x": _PREDGRAD,
    "sgp_sparse_posterior_predict_grad_x": _PREDGRAD,
}

# include/sthenomi_vfe_update.h: new data into a kept sparse (VFE) posterior, exported by libsthenomi_vfe_update.so (it links
# against the product library and works on its posteriors) -- update_posterior reaches it through vfe_update_lib() / Context.vfe_update
_SIGS_VFE_UPDATE = {
    "sgp_sparse_posterior_update": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, _D, C.c_int, _D, _D, _D]),
    "sgp_sparse_posterior_count": (C.c_int, [_P, C.POINTER(C.c_int64)]),
}

# include/sthenomi_extend_bench.h: the measurement hook of the extension (libsthenomi_extend_bench.so; tools and tests only)
_SIGS_EXTEND_BENCH = {
    "sgp_bench_extend_row_solve": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _D]),
}


# include/sthenomi_conv.h: patch-geometry registration, exported by libsthenomi_conv.so (it links against the product library
# and works on its contexts) -- Spec.bind reaches it through conv_lib()
class sgp_patch_geom(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("patch_h", C.c_int32), ("patch_w", C.c_int32)]


_SIGS_CONV = {
    "sgp_conv_geom": (C.c_int, [_P, C.POINTER(sgp_patch_geom), C.POINTER(C.c_int32)]),
}


STENCIL_MAX_POINTS, STENCIL_MAX_DIM = 64, 16      # include/sthenomi_stencil.h: the limits of a stencil


# include/sthenomi_stencil.h: stencil registration, exported by libsthenomi_stencil.so (links against the product library and
# works on its contexts) -- Spec.bind reaches it through stencil_lib()
class sgp_stencil(C.Structure):
    _fields_ = [("dim", C.c_int32), ("npoints", C.c_int32), ("offsets", C.POINTER(C.c_double)),
                ("weights", C.POINTER(C.c_double))]


_SIGS_STENCIL = {
    "sgp_stencil_register": (C.c_int, [_P, C.POINTER(sgp_stencil), C.POINTER(C.c_int32)]),
}


# include/sthenomi_kprod.h: the parameter gradient through product chains and plain terms alike, exported by
# libsthenomi_kprod.so (links against the product library and works on its contexts) -- logpdf_and_gradient reaches it through
# kprod_lib()
_SIGS_KPROD = {
    "sgp_logpdf_grad_param": (C.c_int, [_P, C.POINTER(sgp_cov_spec), _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D, _D]),
}


# include/sthenomi_kprod_grad.h: the supersets of sgp_logpdf_grad_xs / sgp_kernelmatrix_diag_grad_xs / sgp_elbo_grad_xs that carry
# product chains and return d / d param, exported by libsthenomi_kprod_grad.so -- logpdf_and_gradient_param and
# elbo_and_gradient_param reach them through kprod_grad_lib() / Context.kprod_grad
_SPEC = C.POINTER(sgp_cov_spec)
_DD = C.POINTER(_D)
_SIGS_KPROD_GRAD = {
    "sgp_logpdf_grad_param_xs": (C.c_int, [_P, _SPEC, _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D, _D, _DD, _DD]),
    "sgp_kernelmatrix_diag_grad_param": (C.c_int, [_P, _SPEC, _D, _D, _D, _D, _DD, _DD, _DD]),
    "sgp_elbo_grad_param": (C.c_int, [_P, _SPEC, _SPEC, _D, _D, C.c_int, _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D,
                                      _D, _D, _D, _D, _D, _D, _DD, _DD, _DD, _DD, _DD]),
}


# include/sthenomi_conv_grad.h: sgp_logpdf_grad / sgp_kernelmatrix_diag_grad / sgp_elbo_grad_x with patch terms carried through,
# exported by libsthenomi_conv_grad.so -- logpdf_and_gradient_conv and elbo_and_gradient_conv reach them through
# conv_grad_lib() / Context.conv_grad
_SIGS_CONV_GRAD = {
    "sgp_logpdf_grad_conv": (C.c_int, [_P, _SPEC, _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D]),
    "sgp_kernelmatrix_diag_grad_conv": (C.c_int, [_P, _SPEC, _D, _D, _D]),
    "sgp_elbo_grad_conv": (C.c_int, [_P, _SPEC, _SPEC, _D, _D, C.c_int, _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D,
                                     _D, _D, _D, _D, _DD, _DD]),
}


# include/sthenomi_stencil_grad.h: the same three with stencil terms carried through and the input points on both sides, exported
# by libsthenomi_stencil_grad.so -- logpdf_and_gradient_stencil and elbo_and_gradient_stencil reach them through
# stencil_grad_lib() / Context.stencil_grad
_SIGS_STENCIL_GRAD = {
    "sgp_logpdf_grad_stencil": (C.c_int, [_P, _SPEC, _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D, _DD]),
    "sgp_kernelmatrix_diag_grad_stencil": (C.c_int, [_P, _SPEC, _D, _D, _D, _DD]),
    "sgp_elbo_grad_stencil": (C.c_int, [_P, _SPEC, _SPEC, _D, _D, C.c_int, _D, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D,
                                        _D, _D, _D, _D, _DD, _DD]),
}


def stencil_grad_symbols():
    """Names include/sthenomi_stencil_grad.h declares: the entry points of libsthenomi_stencil_grad.so."""
    return sorted(_SIGS_STENCIL_GRAD)


# include/sthenomi_stencil_wo.h: the same three plus the gradients with respect to the stencils' own weights and offsets (two
# tables of 2 pointers per term; the ELBO: one pair for zz, one for xz), exported by libsthenomi_stencil_wo.so --
# logpdf_and_gradient_stencil(..., stencils=True) and elbo_and_gradient_stencil(..., stencils=True) reach them through
# stencil_wo_lib() / Context.stencil_wo
_SIGS_STENCIL_WO = {
    "sgp_logpdf_grad_stencil_wo": (C.c_int, _SIGS_STENCIL_GRAD["sgp_logpdf_grad_stencil"][1] + [_DD, _DD]),
    "sgp_kernelmatrix_diag_grad_stencil_wo": (C.c_int, _SIGS_STENCIL_GRAD["sgp_kernelmatrix_diag_grad_stencil"][1] + [_DD, _DD]),
    "sgp_elbo_grad_stencil_wo": (C.c_int, _SIGS_STENCIL_GRAD["sgp_elbo_grad_stencil"][1] + [_DD, _DD, _DD, _DD]),
}


def stencil_wo_symbols():
    """Names include/sthenomi_stencil_wo.h declares: the entry points of libsthenomi_stencil_wo.so."""
    return sorted(_SIGS_STENCIL_WO)


def conv_grad_symbols():
    """Names include/sthenomi_conv_grad.h declares: the entry points of libsthenomi_conv_grad.so."""
    return sorted(_SIGS_CONV_GRAD)


def kprod_grad_symbols():
    """Names include/sthenomi_kprod_grad.h declares: the entry points of libsthenomi_kprod_grad.so."""
    return sorted(_SIGS_KPROD_GRAD)


def kprod_symbols():
    """Names include/sthenomi_kprod.h declares: the entry points of libsthenomi_kprod.so."""
    return sorted(_SIGS_KPROD)


def stencil_symbols():
    """Names include/sthenomi_stencil.h declares: the entry points of libsthenomi_stencil.so."""
    return sorted(_SIGS_STENCIL)


def conv_symbols():
    """Names include/sthenomi_conv.h declares: the entry points of libsthenomi_conv.so."""
    return sorted(_SIGS_CONV)


def extend_symbols():
    """Names include/sthenomi_extend.h declares: the entry points of libsthenomi_extend.so."""
    return sorted(_SIGS_EXTEND)


def postfx_symbols():
    """Names include/sthenomi_postfx.h declares: the entry points of libsthenomi_postfx.so."""
    return sorted(_SIGS_POSTFX)


def predgrad_symbols():
    """Names include/sthenomi_predgrad.h declares: the entry points of libsthenomi_predgrad.so."""
    return sorted(_SIGS_PREDGRAD)


def vfe_update_symbols():
    """Names include/sthenomi_vfe_update.h declares: the entry points of libsthenomi_vfe_update.so."""
    return sorted(_SIGS_VFE_UPDATE)


def batch_symbols():
    """Names include/sthenomi_batch.h declares: the entry points of libsthenomi_batch.so."""
    return sorted(_SIGS_BATCH)


def pool_symbols():
    """Names include/sthenomi_pool.h declares: the entry points of libsthenomi_pool.so."""
    return sorted(_SIGS_POOL)


def exported_symbols():
    """Names include/sthenomi.h declares (used by the CPU-side symbol test)."""
    return sorted(_SIGS)


def bench_symbols():
    """Names include/sthenomi_bench.h declares: the entry points of libsthenomi_bench.so."""
    return sorted(_SIGS_BENCH)


_bench = None


def bench_lib():
    """dlopen libsthenomi_bench.so (micro-benchmarks, diagnosis and test hooks: include/sthenomi_bench.h).  It links against
    the product library and works on contexts created there; nothing on a product path loads it."""
    global _bench
    load()
    with _lib_lock:
        if _bench is not None:
            return _bench
        if not os.path.exists(BENCH_LIB_PATH):
            raise SthenoMIError(f"{BENCH_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(BENCH_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_BENCH.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _bench = lib
        return lib


_batch = None


def batch_lib():
    """dlopen libsthenomi_batch.so (include/sthenomi_batch.h) after the product library it links against."""
    global _batch
    load()
    with _lib_lock:
        if _batch is not None:
            return _batch
        if not os.path.exists(BATCH_LIB_PATH):
            raise SthenoMIError(f"{BATCH_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(BATCH_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_BATCH.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _batch = lib
        return lib


_pool = None


def pool_lib():
    """dlopen libsthenomi_pool.so (include/sthenomi_pool.h) after the product library it links against."""
    global _pool
    load()
    with _lib_lock:
        if _pool is not None:
            return _pool
        if not os.path.exists(POOL_LIB_PATH):
            raise SthenoMIError(f"{POOL_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(POOL_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_POOL.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _pool = lib
        return lib


_extend = None


def extend_lib():
    """dlopen libsthenomi_extend.so (include/sthenomi_extend.h) after the product library it links against."""
    global _extend
    load()
    with _lib_lock:
        if _extend is not None:
            return _extend
        if not os.path.exists(EXTEND_LIB_PATH):
            raise SthenoMIError(f"{EXTEND_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(EXTEND_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_EXTEND.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _extend = lib
        return lib


_vfe_update = None


def vfe_update_lib():
    """dlopen libsthenomi_vfe_update.so (include/sthenomi_vfe_update.h) after the product library it links against."""
    global _vfe_update
    load()
    with _lib_lock:
        if _vfe_update is not None:
            return _vfe_update
        if not os.path.exists(VFE_UPDATE_LIB_PATH):
            raise SthenoMIError(
                f"{VFE_UPDATE_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(VFE_UPDATE_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_VFE_UPDATE.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _vfe_update = lib
        return lib


_postfx = None


def postfx_lib():
    """dlopen libsthenomi_postfx.so (include/sthenomi_postfx.h) after the product library it links against."""
    global _postfx
    load()
    with _lib_lock:
        if _postfx is not None:
            return _postfx
        if not os.path.exists(POSTFX_LIB_PATH):
            raise SthenoMIError(f"{POSTFX_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(POSTFX_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_POSTFX.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _postfx = lib
        return lib


_predgrad = None


def predgrad_lib():
    """dlopen libsthenomi_predgrad.so (include/sthenomi_predgrad.h) after the product library it links against."""
    global _predgrad
    load()
    with _lib_lock:
        if _predgrad is not None:
            return _predgrad
        if not os.path.exists(PREDGRAD_LIB_PATH):
            raise SthenoMIError(f"{PREDGRAD_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(PREDGRAD_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_PREDGRAD.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _predgrad = lib
        return lib


_extend_bench = None


def extend_bench_lib():
    """dlopen libsthenomi_extend_bench.so (include/sthenomi_extend_bench.h); nothing on a product path loads it."""
    global _extend_bench
    load()
    with _lib_lock:
        if _extend_bench is not None:
            return _extend_bench
        if not os.path.exists(EXTEND_BENCH_LIB_PATH):
            raise SthenoMIError(f"{EXTEND_BENCH_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(EXTEND_BENCH_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_EXTEND_BENCH.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _extend_bench = lib
        return lib


_conv = None


def conv_lib():
    """dlopen libsthenomi_conv.so (include/sthenomi_conv.h) after the product library it links against."""
    global _conv
    load()
    with _lib_lock:
        if _conv is not None:
            return _conv
        if not os.path.exists(CONV_LIB_PATH):
            raise SthenoMIError(f"{CONV_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(CONV_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_CONV.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _conv = lib
        return lib


_conv_grad = None


def conv_grad_lib():
    """dlopen libsthenomi_conv_grad.so (include/sthenomi_conv_grad.h) after the product library it links against."""
    global _conv_grad
    load()
    with _lib_lock:
        if _conv_grad is not None:
            return _conv_grad
        if not os.path.exists(CONV_GRAD_LIB_PATH):
            raise SthenoMIError(f"{CONV_GRAD_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(CONV_GRAD_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_CONV_GRAD.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _conv_grad = lib
        return lib


_stencil_grad = None


def stencil_grad_lib():
    """dlopen libsthenomi_stencil_grad.so (include/sthenomi_stencil_grad.h) after the product library it links against."""
    global _stencil_grad
    load()
    with _lib_lock:
        if _stencil_grad is not None:
            return _stencil_grad
        if not os.path.exists(STENCIL_GRAD_LIB_PATH):
            raise SthenoMIError(f"{STENCIL_GRAD_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(STENCIL_GRAD_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_STENCIL_GRAD.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _stencil_grad = lib
        return lib


_stencil_wo = None


def stencil_wo_lib():
    """dlopen libsthenomi_stencil_wo.so (include/sthenomi_stencil_wo.h) after the product library it links against."""
    global _stencil_wo
    load()
    with _lib_lock:
        if _stencil_wo is not None:
            return _stencil_wo
        if not os.path.exists(STENCIL_WO_LIB_PATH):
            raise SthenoMIError(f"{STENCIL_WO_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(STENCIL_WO_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_STENCIL_WO.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _stencil_wo = lib
        return lib


_stencil = None


def stencil_lib():
    """dlopen libsthenomi_stencil.so (include/sthenomi_stencil.h) after the product library it links against."""
    global _stencil
    load()
    with _lib_lock:
        if _stencil is not None:
            return _stencil
        if not os.path.exists(STENCIL_LIB_PATH):
            raise SthenoMIError(f"{STENCIL_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(STENCIL_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_STENCIL.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _stencil = lib
        return lib


_kprod = None


def kprod_lib():
    """dlopen libsthenomi_kprod.so (include/sthenomi_kprod.h) after the product library it links against."""
    global _kprod
    load()
    with _lib_lock:
        if _kprod is not None:
            return _kprod
        if not os.path.exists(KPROD_LIB_PATH):
            raise SthenoMIError(f"{KPROD_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(KPROD_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_KPROD.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _kprod = lib
        return lib


_kprod_grad = None


def kprod_grad_lib():
    """dlopen libsthenomi_kprod_grad.so (include/sthenomi_kprod_grad.h) after the product library it links against."""
    global _kprod_grad
    load()
    with _lib_lock:
        if _kprod_grad is not None:
            return _kprod_grad
        if not os.path.exists(KPROD_GRAD_LIB_PATH):
            raise SthenoMIError(f"{KPROD_GRAD_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(KPROD_GRAD_LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS_KPROD_GRAD.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _kprod_grad = lib
        return lib


def load():
    """dlopen libsthenomi.so (after torch, so both share one HIP runtime) and type its symbols."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise SthenoMIError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        try:  # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7): load it first
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the pure C-ABI
            pass
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGS.items():
            if not hasattr(lib, name) and os.environ.get("SGP_ALLOW_MISSING_SYMBOLS"):
                continue        # (A/B runs against an older build of the library: tools/r05_call7.sh)
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def last_error():
    return load().sgp_last_error().decode("utf-8", "replace")


def check(rc, what=""):
    if rc == 0:
        return
    msg = last_error()
    if rc > 0:
        raise PosDefException(rc, msg)
    raise SthenoMIError(f"{what} failed (rc={rc}): {msg}")


def dptr(a):
    """double* of a numpy array (or NULL)."""
    if a is None:
        return C.cast(None, _D)
    return a.ctypes.data_as(_D)


class Context:
    """One sgp_ctx (one GPU, one stream).  `default_context()` gives a process-wide one."""

    def __init__(self, device=0, devices=None):
        """device: one GPU.  devices=[...]: a multi-GPU context (sgp_ctx_create_multi): logpdf, rand, the posterior, the
        gradients, the covariance entry points, the ELBO and its gradients are sharded over the listed GPUs inside the
        library (include/sthenomi.h lists what is not)."""
        lib = load()
        h = _P()
        if devices is not None:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            check(lib.sgp_ctx_create_multi(arr, len(devices), C.byref(h)), "sgp_ctx_create_multi")
            device = int(devices[0])
        else:
            check(lib.sgp_ctx_create(int(device), C.byref(h)), "sgp_ctx_create")
        self.handle = h
        self.device = device
        self.is_multi = devices is not None
        self.lib = lib

    @property
    def bench(self):
        """libsthenomi_bench.so (sthenomi_bench.h): `ctx.bench.sgp_bench_*(ctx.handle, ...)`"""
        return bench_lib()

    @property
    def batch(self):
        """libsthenomi_batch.so (sthenomi_batch.h): `ctx.batch.sgp_logpdf_grad_batch(ctx.handle, ...)`"""
        return batch_lib()

    @property
    def pool(self):
        """libsthenomi_pool.so (sthenomi_pool.h): `ctx.pool.sgp_logpdf_pool(ctx.handle, ...)`"""
        return pool_lib()

    @property
    def kprod(self):
        """libsthenomi_kprod.so (sthenomi_kprod.h): `ctx.kprod.sgp_logpdf_grad_param(ctx.handle, ...)`"""
        return kprod_lib()

    @property
    def kprod_grad(self):
        """libsthenomi_kprod_grad.so (sthenomi_kprod_grad.h): `ctx.kprod_grad.sgp_elbo_grad_param(ctx.handle, ...)`"""
        return kprod_grad_lib()

    @property
    def conv_grad(self):
        """libsthenomi_conv_grad.so (sthenomi_conv_grad.h): `ctx.conv_grad.sgp_logpdf_grad_conv(ctx.handle, ...)`"""
        return conv_grad_lib()

    @property
    def stencil_grad(self):
        """libsthenomi_stencil_grad.so (sthenomi_stencil_grad.h): `ctx.stencil_grad.sgp_logpdf_grad_stencil(ctx.handle, ...)`"""
        return stencil_grad_lib()

    @property
    def stencil_wo(self):
        """libsthenomi_stencil_wo.so (sthenomi_stencil_wo.h): `ctx.stencil_wo.sgp_logpdf_grad_stencil_wo(ctx.handle, ...)`"""
        return stencil_wo_lib()

    @property
    def extend(self):
        """libsthenomi_extend.so (sthenomi_extend.h): `ctx.extend.sgp_posterior_extend(post_handle, ...)`"""
        return extend_lib()

    @property
    def postfx(self):
        """libsthenomi_postfx.so (sthenomi_postfx.h): `ctx.postfx.sgp_posterior_logpdf(post_handle, ...)`"""
        return postfx_lib()

    @property
    def predgrad(self):
        """libsthenomi_predgrad.so (sthenomi_predgrad.h): `ctx.predgrad.sgp_posterior_predict_grad_x(post_handle, ...)`"""
        return predgrad_lib()

    @property
    def vfe_update(self):
        """libsthenomi_vfe_update.so (sthenomi_vfe_update.h): `ctx.vfe_update.sgp_sparse_posterior_update(post_handle, ...)`"""
        return vfe_update_lib()

    @property
    def ndev(self):
        return int(self.lib.sgp_ctx_ndev(self.handle))

    @property
    def transport(self):
        return self.lib.sgp_ctx_transport(self.handle).decode()

    def factor_schedule(self, N):
        """Which schedule the blocked Cholesky of an N-point covariance runs on this context."""
        return self.lib.sgp_ctx_factor_schedule(self.handle, int(N)).decode()

    def factor_work(self):
        """(executed, dense) tile products of the last factorisation's contractions: they differ when the model has
        independent components whose exact zero blocks the factorisation skipped (sthenomi.h: sgp_ctx_factor_work)."""
        e, d = C.c_double(), C.c_double()
        check(self.lib.sgp_ctx_factor_work(self.handle, C.byref(e), C.byref(d)), "sgp_ctx_factor_work")
        return e.value, d.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sgp_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def set_default_context(ctx):
    """Route the host mirror's calls (logpdf, posterior, ...) through `ctx`; returns the previous one.
    With a multi-GPU context (Context(devices=[...])) logpdf is sharded over its GPUs."""
    global _default_ctx
    prev, _default_ctx = _default_ctx, ctx
    return prev


def default_context():
    global _default_ctx
    if _default_ctx is None:
        devs = os.environ.get("SGP_DEVICES")         # e.g. "0,1,2,3,4,5,6,7": one process, all GPUs
        if devs:
            _default_ctx = Context(devices=[int(d) for d in devs.split(",") if d.strip() != ""])
            return _default_ctx
        dev = int(os.environ.get("LOCAL_RANK", "0"))
        try:
            import torch
            if torch.cuda.is_available() and dev >= torch.cuda.device_count():
                dev = 0
        except Exception:
            pass
        _default_ctx = Context(dev)
    return _default_ctx


class Spec:
    """Owns the numpy buffers and ctypes arrays behind one sgp_cov_spec.

    row_len / col_len : block lengths
    inputs            : list of (D x n) float64 Fortran-ordered arrays (ColVecs layout)
    pairs             : dict (I, J) -> list of term tuples
                        (kind, row_input, col_input, coef, param, row_scale|None, col_scale|None)
    """

    def __init__(self, row_len, col_len, inputs, pairs, symmetric, geoms=None, stencils=None):
        """geoms: dict (I, J) -> [(row_geom, col_geom)] aligned with pairs[(I, J)], a geometry being None (plain side) or
        (H, W, ph, pw) -- patch terms (include/sthenomi_conv.h); their geometry ids are registered on the context the
        spec is used with (bind).
        stencils: dict (I, J) -> [(row_stencil, col_stencil)] aligned the same way, a stencil being None (plain side) or
        (offsets D x Q, weights Q) -- stencil terms (include/sthenomi_stencil.h), registered by bind likewise."""
        self.row_len = np.asarray(row_len, dtype=np.int64)
        self.col_len = np.asarray(col_len, dtype=np.int64)
        self.N = int(self.row_len.sum())
        self.M = int(self.col_len.sum())
        self.symmetric = bool(symmetric)
        self._keep = []
        self.inputs = []
        for x in inputs:
            x = np.asarray(x, dtype=np.float64)
            if x.ndim == 1:
                x = x.reshape(1, -1)
            x = np.asfortranarray(x)
            self.inputs.append(x)
        nrb, ncb = len(self.row_len), len(self.col_len)
        self._in_arr = (sgp_input * max(1, len(self.inputs)))()
        for k, x in enumerate(self.inputs):
            self._in_arr[k].dim = x.shape[0]
            self._in_arr[k].n = x.shape[1]
            self._in_arr[k].ld = x.shape[0]
            self._in_arr[k].x = dptr(x)
        term_ptr = [0]
        terms = []
        self.term_geoms = []
        self.term_stencils = []
        for I in range(nrb):
            for J in range(ncb):
                pt = pairs.get((I, J), [])
                terms.extend(pt)
                self.term_geoms.extend((geoms or {}).get((I, J), [(None, None)] * len(pt)))
                self.term_stencils.extend((stencils or {}).get((I, J), [(None, None)] * len(pt)))
                term_ptr.append(len(terms))
        self.has_patch = any(g != (None, None) for g in self.term_geoms)
        self.has_stencil = any(st != (None, None) for st in self.term_stencils)
        # product chains / the RQ, LINEAR, COSINE and GAMMAEXP kinds (include/sthenomi_kprod.h): a term whose kind carries KIND_TIMES_PREV
        # continues the chain of the term before it
        self.has_kprod = any((int(t[0]) & KIND_TIMES_PREV) or (int(t[0]) & KIND_MASK) > CONST for t in terms)
        self._bound = None
        self.n_terms = len(terms)
        self._term_ptr = np.asarray(term_ptr, dtype=np.int32)
        self._terms = (sgp_term * max(1, len(terms)))()
        # identity of each term's scale vectors (the flattener's own merge key): a term of pair (I, J)
        # with scales (rs, cs) is mirrored in pair (J, I) by the term with (cs, rs)
        self.term_scale_ids = [(None if rs is None else id(rs), None if cs is None else id(cs))
                               for (_, _, _, _, _, rs, cs) in terms]
        self.term_row_scale = [rs for (_, _, _, _, _, rs, _) in terms]   # the flattener's own vectors (with factors)
        self.term_col_scale = [cs for (_, _, _, _, _, _, cs) in terms]
        self._keep.extend(terms)
        for k, (kind, ri, ci, coef, param, rs, cs) in enumerate(terms):
            t = self._terms[k]
            t.kind, t.row_input, t.col_input, t.reserved = int(kind), int(ri), int(ci), 0
            t.coef, t.param = float(coef), float(param)
            if rs is not None:
                rs = np.ascontiguousarray(rs, dtype=np.float64)
                self._keep.append(rs)
            if cs is not None:
                cs = np.ascontiguousarray(cs, dtype=np.float64)
                self._keep.append(cs)
            t.row_scale = dptr(rs)
            t.col_scale = dptr(cs)
        s = sgp_cov_spec()
        s.n_row_blocks, s.n_col_blocks = nrb, ncb
        s.row_len = self.row_len.ctypes.data_as(C.POINTER(C.c_int64))
        s.col_len = self.col_len.ctypes.data_as(C.POINTER(C.c_int64))
        s.n_inputs = len(self.inputs)
        s.inputs = self._in_arr
        s.term_ptr = self._term_ptr.ctypes.data_as(C.POINTER(C.c_int32))
        s.terms = self._terms
        s.symmetric = 1 if symmetric else 0
        s.reserved = 0
        self.c = s

    def bind(self, ctx):
        """Write the ids of `ctx` of the patch terms' geometries (sgp_conv_geom) and of the stencil terms' stencils
        (sgp_stencil_register) into their sgp_term.reserved; a spec with neither needs none.  Returns self."""
        if (self.has_patch or self.has_stencil) and self._bound != ctx.handle.value:
            if self.has_stencil and getattr(ctx, "is_multi", False):
                raise NotImplementedError("stencil terms are not supported on a multi-GPU context")
            ids = {}
            for k, sides in enumerate(zip(self.term_geoms, self.term_stencils)):
                code = 0
                for side, (g, st) in enumerate(zip(*sides)):
                    if g is not None:
                        if ("g", g) not in ids:
                            geom = sgp_patch_geom(*[int(v) for v in g])
                            gid = C.c_int32()
                            check(conv_lib().sgp_conv_geom(ctx.handle, C.byref(geom), C.byref(gid)), "sgp_conv_geom")
                            ids[("g", g)] = gid.value
                        code |= ids[("g", g)] << (16 * side)
                    elif st is not None:
                        key = ("s", st[0].shape, st[0].tobytes(), st[1].tobytes())
                        if key not in ids:
                            o = np.ascontiguousarray(st[0].T, dtype=np.float64)     # column-major D x Q
                            w = np.ascontiguousarray(st[1], dtype=np.float64)
                            desc = sgp_stencil(int(st[0].shape[0]), int(st[0].shape[1]), dptr(o), dptr(w))
                            sid = C.c_int32()
                            check(stencil_lib().sgp_stencil_register(ctx.handle, C.byref(desc), C.byref(sid)),
                                  "sgp_stencil_register")
                            ids[key] = sid.value
                        code |= ids[key] << (16 * side)
                self._terms[k].reserved = code
            self._bound = ctx.handle.value
        return self

    def ref(self, ctx=None):
        """sgp_cov_spec* for a call on `ctx` (default: the default context, which every host-mirror operator uses)."""
        if self.has_patch or self.has_stencil:
            self.bind(ctx if ctx is not None else default_context())
        return C.byref(self.c)

    def f32_supported(self):
        """The fp32 device kernels (csrc/f32.hip: assemble_f32) take input dimension <= 16 and, per block pair,
        (number of terms) x (dimension rounded up to a power of two) <= 64; anything else runs on the fp64 path."""
        if self.has_patch or self.has_stencil or self.has_kprod:
            return False                 # patch / stencil / product terms: fp64 only (a Float32 model runs there and is rounded back)
        tp = self._term_ptr
        for p in range(len(tp) - 1):
            t0, t1 = int(tp[p]), int(tp[p + 1])
            if t1 == t0:
                continue
            d = max(self.inputs[int(self._terms[t].row_input)].shape[0] for t in range(t0, t1))
            dmax = 1
            while dmax < d:
                dmax *= 2
            if dmax > 16 or (t1 - t0) * dmax > 64:
                return False
        return True


def _noise_args(noise, N):
    """(kind, buffer) for a FiniteGP noise: scalar -> s2*I, vector -> Diagonal, matrix -> dense."""
    a = np.asarray(noise, dtype=np.float64)
    if a.ndim == 0:
        return NOISE_SCALAR, np.array([float(a)], dtype=np.float64)
    if a.ndim == 1:
        if a.shape[0] != N:
            raise ValueError("diagonal noise has the wrong length")
        return NOISE_DIAG, np.ascontiguousarray(a)
    if a.shape != (N, N):
        raise ValueError("dense noise has the wrong shape")
    return NOISE_DENSE, np.asfortranarray(a)
