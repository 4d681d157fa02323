/* sthenomi_vfe_update.h -- absorbing new data into a kept sparse (VFE) posterior, exported by libsthenomi_vfe_update.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h), in a header and a library of its own like sthenomi_extend.h:
 * libsthenomi.so keeps exporting exactly the product header.  libsthenomi_vfe_update.so links against libsthenomi.so and
 * works on the contexts, posteriors and error state created there (sgp_ctx_create, sgp_sparse_posterior_create,
 * sgp_last_error, ...); a host that wants these calls loads both.  Plain C like the product header. */
#ifndef STHENOMI_VFE_UPDATE_H
#define STHENOMI_VFE_UPDATE_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* update_posterior(f_post_approx, fx2, y2)  [AbstractGPs, VFE]: absorb n_new observations, inducing points fixed.
 * post       : a posterior made by sgp_sparse_posterior_create on a single-GPU context.
 * xz_new     : the spec of cov(f, x_new, z): rows are the new points in any blocks, columns are the inducing blocks the
 *              posterior was created with (their total is checked against M).  That they are the same z, kernel and
 *              Sigma_z is the caller's guarantee, as in sgp_posterior_extend.  Product chains (sthenomi_kprod.h) are taken
 *              wherever sgp_sparse_posterior_create takes them.
 * var_x_new  : n_new prior variances var(f, x_new) (required: the ELBO's trace term is kept up to date).
 * mean_x_new : n_new prior means, NULL == zeros;  y_new: the n_new observations.
 * noise_kind / noise_new : SGP_NOISE_SCALAR (one value) or SGP_NOISE_DIAG (n_new values), independent of the kind and the
 *              values used before: every row carries its own s2 into the sums.
 * elbo_out   : NULL, or receives the ELBO (sgp_elbo's formula) on the kept scalars of ALL the points absorbed so far, the new
 *              ones included.  One term of it the posterior cannot know: sgp_sparse_posterior_create takes no var_x, so the
 *              kept sum of var / s2 starts at zero and counts the points of the updates only.  The value is therefore
 *              the ELBO of all the points PLUS 1/2 sum_n var_n / s2_n over the points the create call was given -- a
 *              constant of the handle, which a caller who has var(f, x) of those points (sgp_kernelmatrix_diag, as for
 *              sgp_elbo) subtracts.  Every other term covers all the points.
 * rc 0; > 0: LAPACK info of A A' + I over all the points (the posterior is left exactly as it was); < 0: refused, the
 * posterior is left exactly as it was and sgp_last_error() names this entry point -- a NULL argument other than
 * mean_x_new / elbo_out, no new points, a column count other than M, dense noise, a posterior without sums (created on a
 * multi-GPU context), a multi-GPU context, a context that was destroyed or is not the one that created the posterior.
 *
 * A VFE posterior depends on the data only through sums over the data points: sum_n a_n a_n', A delta and the four scalars
 * sum log s2, delta' delta, sum var / s2, |A|_F^2 (a_n = Lz^-1 k(z, x_n) / s_n).  sgp_sparse_posterior_create keeps them,
 * and this call adds the new rows' terms -- the rows go through the kernels the create call sends them through (assembly,
 * row solve against the kept Lz, transposition + column sums, split-K Gram accumulated in chunk order) -- and factors
 * A A' + I afresh: O(n_new M^2 + M^3 / 3), whatever the number of points absorbed before; nothing of size N is kept.  After
 * a successful call every entry point that takes the sgp_sparse_post* (sgp_sparse_posterior_predict,
 * sgp_sparse_posterior_rand / _logpdf, another update) sees the posterior of all the points.
 *
 * MEMORY.  Every posterior made by sgp_sparse_posterior_create on a single-GPU context holds the sums in one more
 * (m_pad + 128) x m_pad + m_pad + 8 doubles (m_pad = M rounded up to 128): 138 MB at M = 4096, filled by one
 * device-to-device copy inside the create call.  An update works on scratch of twice that size from the context's cache
 * (the new sums and the new factor) and copies both over the kept buffers once the factorisation has succeeded.
 *
 * With sgp_ctx_stage_timing on, the stages of a call are added to the slots 0 buffers (uploads, the scratch copy of the
 * sums), 1 assembly, 2 row solve, 3 transposition + column sums, 4 Gram, 5 prepare + factor + scalars + the copies back. */
int sgp_sparse_posterior_update(sgp_sparse_post* post, const sgp_cov_spec* xz_new, const double* var_x_new,
                                const double* mean_x_new, int noise_kind, const double* noise_new,
                                const double* y_new, double* elbo_out);

/* data points absorbed so far: those of sgp_sparse_posterior_create plus those of every successful update.
 * rc < 0: NULL argument, or a posterior without sums (created on a multi-GPU context). */
int sgp_sparse_posterior_count(sgp_sparse_post* post, int64_t* n_out);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_VFE_UPDATE_H */
