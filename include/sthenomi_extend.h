/* sthenomi_extend.h -- extending a kept Cholesky factor with new data, exported by libsthenomi_extend.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h), in a header and a library of its own like sthenomi_batch.h:
 * libsthenomi.so keeps exporting exactly the product header.  libsthenomi_extend.so links against libsthenomi.so and works
 * on the contexts, posteriors and error state created there (sgp_ctx_create, sgp_posterior_create, sgp_last_error, ...); a
 * host that wants this call loads both.  Plain C like the product header. */
#ifndef STHENOMI_EXTEND_H
#define STHENOMI_EXTEND_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* update_posterior(f_post, fx2, y2)  [AbstractGPs update_posterior; extends chol(C11) by the rows of the new data]
 * post      : a posterior made by sgp_posterior_create on a single-GPU context, N points.
 * spec_all  : symmetric spec of the STACKED data: the N old points in their old block order, then n_new new points
 *             in further blocks (what the host already builds for sequential conditioning).  The caller guarantees
 *             that the first N points / their terms are those the posterior was created with.
 * mean_all, y_all : N + n_new values (mean_all may be NULL == zeros).
 * noise_kind/noise: SGP_NOISE_SCALAR (one value, must be the old one) or SGP_NOISE_DIAG (N + n_new values).
 * reserve_n : 0, or a number of points >= N + n_new to size the factor buffer for when it has to be reallocated.
 * alpha_out : N + n_new values or NULL;  logpdf_out: logpdf(f(x_all, noise), y_all) or NULL.
 * rc 0; > 0: LAPACK info of the stacked matrix (failing leading minor, counted from the first OLD point), the
 * posterior is left exactly as it was; < 0: refused (dense noise, a sharded posterior, size mismatch, dead context).
 *
 * Columns [0, c0) of the factor, c0 = 128 floor(N / 128), are kept; the rows from c0 on are assembled afresh, solved against
 * the kept columns and their trailing block is factored: O(N^2 k + N k^2 + k^3) for k new points instead of the
 * O((N + k)^3) of sgp_posterior_create on the stacked data.  After a successful call every entry point that takes the
 * sgp_post* (sgp_posterior_predict, sgp_posterior_predict_explicit, sgp_posterior_destroy) sees the posterior of
 * N + n_new points.
 *
 * MEMORY.  While N + n_new fits the columns the factor buffer was allocated with, the call works in place.  Otherwise a
 * buffer for max(N + n_new, reserve_n) points is allocated and the kept lower tiles are copied over; the old buffer is
 * freed only after success, so for the duration of the call BOTH are resident -- two 34 GB buffers at N = 65 536.  A loop
 * that adds points repeatedly passes the size it will reach as reserve_n on its first call and pays that once.  An in-place
 * call first saves what it overwrites of the old posterior -- rows [c0, m_tot) over the old columns, up to 256 x N doubles
 * (134 MB at N = 65 536) of scratch from the context's cache -- so that a failed call can put the bits back.
 *
 * With sgp_ctx_stage_timing on, the stages of a call are added to the slots 0 buffer (reallocation, tile copy, save),
 * 1 assembly of the row window, 2 row solve, 3 trailing update, 4 factorisation of the trailing block, 5 scalars and alpha. */
int sgp_posterior_extend(sgp_post* post, const sgp_cov_spec* spec_all, const double* mean_all, int noise_kind,
                         const double* noise, const double* y_all, int64_t n_new, int64_t reserve_n,
                         double* alpha_out, double* logpdf_out);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_EXTEND_H */
