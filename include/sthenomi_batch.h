/* sthenomi_batch.h -- batched gradient entry point, exported by libsthenomi_batch.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h), in a header and a library of its own: the product header's
 * entry points are a fixed table that its C consumers check one by one (tests/capi_smoke.c), so an entry point added
 * after that table was fixed lives here.  libsthenomi_batch.so links against libsthenomi.so and works on the contexts,
 * specs and error state created there (sgp_ctx_create, sgp_last_error, ...); a host that wants this call loads both.
 * Plain C like the product header. */
#ifndef STHENOMI_BATCH_H
#define STHENOMI_BATCH_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* logpdf AND its gradient (sthenomi.h: sgp_logpdf_grad) of nspec INDEPENDENT models in one call: the optimiser loop of
 * hyper-parameter learning needs value and gradient at every step (/root/reference/examples/getting_started/script.jl:154-213,
 * extended_mauna_loa/script.jl:195, flux_integration/), and a host runs several such chains at once (restarts, folds,
 * candidates).  Member b takes specs[b], means[b], noises[b], ys[b] as sgp_logpdf_batch does and writes logpdf_out[b],
 * grad_y[b], grad_mean[b], grad_noise[b], grad_coef[b], grad_inscale[b] -- exactly what (and bit-equal to what) its own
 * sgp_logpdf_grad call writes.  Any of the five gradient pointer arrays may be NULL (that output is skipped for every
 * member), and any element of them (skipped for that member).  Noise SCALAR or DIAG pools; DENSE is accepted and runs member
 * by member.  Members of one PADDED size below the hybrid schedule's gradient range (16384 columns) and up to
 * SGP_BATCH_MAX_N are assembled side by side and factored -- matrix, (y - m)' row and inv(L)' -- by ONE launch of the
 * dataflow kernel; their C^-1 = inv(L)' inv(L) are ONE launch too (docs/05).  Anything else runs member by member, and so does
 * the rest of a batch for which device memory runs out.  A member whose matrix is not positive definite gets
 * logpdf_out[b] = NaN, infos[b] = its info and its gradients untouched; with infos == NULL the call returns the first such
 * info.  Gradients w.r.t. the input points and row scales are not part of the batch (sgp_logpdf_grad_x / _xs). */
int sgp_logpdf_grad_batch(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                          int noise_kind, const double* const* noises, const double* const* ys, double* logpdf_out,
                          double* const* grad_y, double* const* grad_mean, double* const* grad_noise,
                          double* const* grad_coef, double* const* grad_inscale, int* infos);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_BATCH_H */
