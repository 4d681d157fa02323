/* sthenomi_pool.h -- logpdf (and its gradient) of independent models of DIFFERENT sizes in one call, exported by
 * libsthenomi_pool.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h) in a header and a library of its own, like sthenomi_batch.h:
 * libsthenomi_pool.so links against libsthenomi.so and works on the contexts, specs and error state created there; a host
 * that wants these calls loads both.  Plain C like the product header.
 *
 * sgp_logpdf_batch / sgp_logpdf_grad_batch pool their members only when all of them share one padded size and one noise
 * kind.  The loops that evaluate one model on data sets of different sizes -- cross-validation folds that straddle a tile
 * boundary, learning curves, one GP per series or sensor, candidates over different subsets; the reference runs such a loop
 * member by member (examples/getting_started/script.jl:154-213) -- are served here: the members, each assembled with the
 * geometry of its own call, are factored by ONE launch of the dataflow kernel as a ragged task pool (docs/03), so their
 * diagonal chains hide each other whatever their sizes. */
#ifndef STHENOMI_POOL_H
#define STHENOMI_POOL_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what a call did (optional) */
typedef struct {
  int32_t pool_launches;   /* ragged dataflow launches this call made                      */
  int32_t pooled_members;  /* members factored inside them                                 */
  int32_t single_members;  /* members that ran through their own call                      */
  int32_t distinct_sizes;  /* distinct padded sizes among the pooled members               */
} sgp_pool_report;

/* out[b] = what sgp_logpdf(ctx, specs[b], means[b], noise_kinds[b], noises[b], ys[b], N_b, 1, .) writes, bit for bit.
 * means may be NULL, and any element of it.  The noise kind is per member: SCALAR and DIAG members pool together; a DENSE
 * member, a member beyond SGP_BATCH_MAX_N, and every member of a multi-GPU context or of one with the dataflow kernel
 * switched off runs through its own call.  More than 16 poolable members are sorted by task count and cut into launches of
 * at most 16; results always return in input order.  A member whose matrix is not positive definite gets out[b] = NaN and
 * infos[b] = its info, the others keep their values; with infos == NULL the call returns the first such info.  When device
 * memory runs out the remaining members run through their own calls. */
int sgp_logpdf_pool(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                    const int* noise_kinds, const double* const* noises, const double* const* ys, double* out, int* infos,
                    sgp_pool_report* report /* may be NULL */);

/* logpdf AND gradient: member b gets exactly what (and bit-equal to what) its own sgp_logpdf_grad call writes into
 * logpdf_out[b], grad_y[b], grad_mean[b], grad_noise[b], grad_coef[b], grad_inscale[b].  Any of the five pointer arrays may
 * be NULL, and any element of them.  Poolable members (SCALAR / DIAG noise, padded size up to SGP_BATCH_MAX_N and below the
 * hybrid schedule's gradient range) are factored -- matrix, (y - m)' row and inv(L)' -- by one ragged launch, each with the
 * border pattern of its own size; C^-1 = inv(L)' inv(L) is one launch per distinct padded size.  Specs with stencil or patch
 * terms are refused, as in sgp_logpdf_grad.  NaN / infos as above; a failed member's gradients are left untouched. */
int sgp_logpdf_grad_pool(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                         const int* noise_kinds, const double* const* noises, const double* const* ys, double* logpdf_out,
                         double* const* grad_y, double* const* grad_mean, double* const* grad_noise,
                         double* const* grad_coef, double* const* grad_inscale, int* infos, sgp_pool_report* report);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_POOL_H */
