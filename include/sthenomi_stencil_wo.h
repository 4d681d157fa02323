/* sthenomi_stencil_wo.h -- gradients of logpdf, the diagonal and the ELBO with respect to a stencil's own weights and offsets
 * (include/sthenomi_stencil.h), through libsthenomi_stencil_wo.so.
 *
 * An extension in a header and a library of its own, as include/sthenomi_stencil_grad.h is: that header's three entry points
 * are a fixed table.  libsthenomi_stencil_wo.so links against libsthenomi.so and works on the contexts, specs, stencils and
 * error state created there.  Plain C like the product header.
 *
 * A stencil term of a block pair is K_ij = coef rs_i cs_j sum_p w_p sum_q v_q k(d2_pq), with delta_pq = (x_i - a_p) -
 * (y_j - b_q) and d2_pq = |delta_pq|^2 (a plain side is the one-point stencil {0, 1}).  With the cotangent G that the call
 * contracts for grad_coef[t] (logpdf: (alpha alpha' - C^-1) / 2; the ELBO: its G_zz and G_xz; the diagonal: diag(w), entries
 * (i, i) only), W_ij = G_ij coef rs_i cs_j and kappa' = d k / d (d^2):
 *     grad_weights_row[p]    =  sum_ij W_ij sum_q v_q k(d2_pq)
 *     grad_weights_col[q]    =  sum_ij W_ij sum_p w_p k(d2_pq)
 *     grad_offsets_row[:, p] = -sum_ij W_ij w_p sum_q v_q 2 kappa'(d2_pq) delta_pq
 *     grad_offsets_col[:, q] = +sum_ij W_ij v_q sum_p w_p 2 kappa'(d2_pq) delta_pq
 * (Matern-1/2 contributes 0 to the offsets where a shifted pair coincides, as for the input points.)  These are the
 * derivatives of the call's value with respect to that term's own copy of the stencil: a stencil shared by several terms --
 * the mirror pair's term of a symmetric spec among them -- collects the sum of their entries, which is the caller's to form.
 *
 * Tables.  grad_weights / grad_offsets hold 2 pointers per element of spec->terms in the caller's order: [2 t] for the row
 * side of term t, [2 t + 1] for its column side.  A table may be NULL, and so may any entry (not asked for).  A weights entry
 * points at npoints doubles, an offsets entry at dim x npoints doubles laid out as sgp_stencil.offsets.  Entries are
 * overwritten, not accumulated; the terms of a pair that the call does not read (an empty block; off the diagonal in
 * sgp_kernelmatrix_diag_grad_stencil_wo) receive zeros.
 *
 * Every output these entry points share with their _stencil counterparts is bit for bit that entry point's, whether or not the
 * tables are given.  Per-workgroup partial sums are reduced in a fixed order and every element is written by one thread: two
 * calls with the same arguments return the same bits.  The limits of sthenomi_stencil.h hold (64 points, dimension 16).
 *
 * Refused (rc < 0, each by name): a non-NULL entry for a plain side ("plain side"), for a patch term or for a product chain
 * term, and whatever the _stencil entry points refuse: a multi-GPU context, a grad_inputs entry of an image input, product
 * chains in the ELBO.
 *
 * What is NOT formed, each a later extension: row- and column-scale gradients of stencil terms; the batch and pool gradients;
 * the *_param family; fp32; multi-GPU contexts. */
#ifndef STHENOMI_STENCIL_WO_H
#define STHENOMI_STENCIL_WO_H

#include "sthenomi_stencil_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sgp_logpdf_grad_stencil plus the two tables. */
int sgp_logpdf_grad_stencil_wo(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind, const double* noise,
                               const double* y, double* logpdf_out, double* grad_y, double* grad_mean, double* grad_noise,
                               double* grad_coef, double* grad_inscale, double* const* grad_inputs,
                               double* const* grad_weights, double* const* grad_offsets);

/* sgp_kernelmatrix_diag_grad_stencil plus the two tables: sum_i w[i] d var_i / d (weights, offsets) of the diagonal pairs. */
int sgp_kernelmatrix_diag_grad_stencil_wo(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w, double* grad_coef,
                                          double* grad_inscale, double* const* grad_inputs, double* const* grad_weights,
                                          double* const* grad_offsets);

/* sgp_elbo_grad_stencil plus one pair of tables for the terms of zz and one for those of xz. */
int sgp_elbo_grad_stencil_wo(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                             const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                             const double* z_noise, const double* y, double* elbo_out, double* grad_y, double* grad_mean,
                             double* grad_noise, double* grad_var_x, double* grad_z_noise, double* grad_coef_zz,
                             double* grad_inscale_zz, double* grad_coef_xz, double* grad_inscale_xz,
                             double* const* grad_inputs_zz, double* const* grad_inputs_xz, double* const* grad_weights_zz,
                             double* const* grad_offsets_zz, double* const* grad_weights_xz, double* const* grad_offsets_xz);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_STENCIL_WO_H */
