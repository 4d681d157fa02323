/* sthenomi_predgrad.h -- posterior mean and variance at test points together with their gradients with respect to those
 * points, exported by libsthenomi_predgrad.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h), in a header and a library of its own like sthenomi_postfx.h:
 * libsthenomi.so keeps exporting exactly the product header.  libsthenomi_predgrad.so links against libsthenomi.so and works
 * on the contexts, posteriors and error state created there; a host that wants these calls loads both.  Plain C like the
 * product header.
 *
 * What they are for: the "look" step of condition - look - add a few points - condition again.  An acquisition function of
 * mean_and_var(f_post(x*)) is maximised over x*, which needs d mean_i / d x*_i and d var_i / d x*_i.  Without these calls a host
 * takes central differences through 2 D calls of sgp_posterior_predict, each of which assembles K(x*, x) and solves its rows
 * again.  Here K* is assembled once, V = K* L^-T is shared between the values and the gradients, and nothing is factored.
 *
 * cross, prior_ss, mean_s : exactly those of sgp_posterior_predict / sgp_sparse_posterior_predict -- K(x*, x) (K(x*, z) for the
 *                           sparse posterior), K(x*, x*) (symmetric; required for var_out, grad_var_inputs and
 *                           grad_var_prior_inputs) and the prior mean at the N* points (NULL == zeros).
 * mean_out, var_out       : N* values each; bit for bit what the predict call answers for the same arguments (the same kernels
 *                           in the same order).
 *
 * With term t of cross block pair (I, J)   K*_ij = coef rs_i kappa(|xr_i - xc_j|^2) cs_j   and
 *   exact  : C = L L', alpha = C^-1 (y - m), B = K* C^-1 = (K* L^-T) L^-1
 *   sparse : B' = K*z Lz^-T, C' = B' Le^-T, alpha = Lz^-T Le^-T u, B = B' Lz^-1 - C' Le^-1 Lz^-1
 *   mean_i = m*_i + sum_j K*_ij alpha_j,   var_i = k**_ii - sum_j K*_ij B_ij
 * the gradients are packed dim_k x n_k column-major arrays, one per spec input, written for the inputs some term reads on its
 * ROW side (the others may be NULL and are not touched):
 *   grad_mean_inputs[k][:, i] = sum over the terms with row input k, sum_j alpha_j coef rs_i cs_j kappa'(d2_ij) 2 (xr_i - xc_j)
 *   grad_var_inputs[k][:, i]  = the same sum with alpha_j replaced by -2 B_ij
 *   grad_var_prior_inputs[k]  = the part of d var_i / d x from k**_ii, by prior_ss's own diagonal terms: what
 *                               sgp_kernelmatrix_diag_grad_x gives for w = 1 (+ into the row input, - into the column input, 0
 *                               where a term reads one input on both sides); [prior_ss->n_inputs]
 * Point i of the prediction depends on row i only: these are per-point Jacobians, not a summed cotangent.  Any of the five
 * outputs and any entry of the three arrays may be NULL.
 *
 * Conventions, as in sgp_logpdf_grad_x: row and column scales are held fixed; Matern-1/2 at a coincident pair contributes 0;
 * any input dimension.  The sums over the columns are formed per SGP_PREDGRAD_COL_CHUNK columns and added in ascending chunk
 * order by one writer per element: two calls give the same bits.
 *
 * rc 0; < 0: refused, sgp_last_error() names the entry point -- a NULL post or cross, a destroyed context, a "multi-GPU"
 * posterior (its factor is sharded), sizes that do not match the posterior or each other, a spec with a "product" chain or a
 * kind beyond the six plain ones, with a "patch" (convolutional) term or with a "stencil" term.  The posterior is only read. */
#ifndef STHENOMI_PREDGRAD_H
#define STHENOMI_PREDGRAD_H

#include "sthenomi.h"

/* columns one workgroup of the prediction-gradient contraction walks; the partial sums of the chunks are added in order */
#define SGP_PREDGRAD_COL_CHUNK 512

#ifdef __cplusplus
extern "C" {
#endif

int sgp_posterior_predict_grad_x(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                                 double* mean_out, double* var_out, double* const* grad_mean_inputs,
                                 double* const* grad_var_inputs, double* const* grad_var_prior_inputs);
int sgp_sparse_posterior_predict_grad_x(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                        const double* mean_s, double* mean_out, double* var_out,
                                        double* const* grad_mean_inputs, double* const* grad_var_inputs,
                                        double* const* grad_var_prior_inputs);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_PREDGRAD_H */
