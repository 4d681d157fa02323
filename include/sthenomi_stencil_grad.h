/* sthenomi_stencil_grad.h -- gradients of logpdf, the diagonal and the ELBO through stencil terms
 * (include/sthenomi_stencil.h), through libsthenomi_stencil_grad.so.
 *
 * An extension in a header and a library of its own, as include/sthenomi_conv_grad.h is: the product header's entry points are
 * a fixed table, and its gradient entry points keep refusing stencil terms, as do those of sthenomi_conv_grad.h and
 * sthenomi_kprod_grad.h.  libsthenomi_stencil_grad.so links against libsthenomi.so and works on the contexts, specs, stencils
 * and error state created there.  Plain C like the product header.
 *
 * A stencil term of a block pair is K_ij = coef rs_i cs_j sum_p w_p sum_q v_q k(x_i - a_p, y_j - b_q) (a plain side is the
 * one-point stencil {0, 1}).  With the cotangent G of the call (logpdf: (alpha alpha' - C^-1) / 2; the ELBO: its G_xz and
 * G_zz; the diagonal: diag(w))
 *     grad_coef[t]    = sum_ij G_ij rs_i cs_j sum_pq w_p v_q k
 *     grad_inscale[t] = sum_ij G_ij coef rs_i cs_j sum_pq w_p v_q d k(g a, g b) / dg |_{g = 1}   (a, b: the shifted points --
 *                       a common scale of points and offsets alike)
 * exactly as for a plain term, one entry per element of spec->terms in the caller's order.  Both sides hold real points, so
 * the gradient with respect to the input points is formed on both sides and in every entry point:
 *     grad_inputs[row input][:, i] += sum_j G_ij coef rs_i cs_j sum_pq w_p v_q 2 kappa'(d2_pq) ((x_i - a_p) - (y_j - b_q))
 * and the column input receives the same sum of the transposed cotangent with the sides and stencils swapped (kappa' = d k /
 * d (d^2); Matern-1/2 contributes 0 where a shifted pair coincides, as everywhere else).  Shifting is a translation: the
 * gradient belongs to the stored, unshifted points.  Per-workgroup partial sums are reduced in a fixed order and every
 * input-gradient column is written by one thread: two calls with the same arguments return the same bits.  The limits of
 * sthenomi_stencil.h hold (64 points, dimension 16).
 *
 * Gradients with respect to a stencil's own weights and offsets come from include/sthenomi_stencil_wo.h (the same three with
 * two more tables, libsthenomi_stencil_wo.so).  What is NOT formed, each a later extension: row- and
 * column-scale gradients of stencil terms (the _xs family); the batch and pool gradients (sgp_logpdf_grad_batch / _pool); the
 * *_param family (d / d param, include/sthenomi_kprod_grad.h); fp32; multi-GPU contexts.  Everything else that takes a gradient
 * keeps refusing stencil terms by name: sgp_logpdf_grad*, sgp_elbo_grad*, sgp_kernelmatrix_diag_grad*, the *_conv and
 * *_param families.  These three refuse (rc < 0, each by name): a multi-GPU context, a non-NULL grad_inputs entry of an input
 * that a patch (convolutional) side reads -- it holds images -- and, sgp_elbo_grad_stencil, product chains, as sgp_elbo_grad
 * does. */
#ifndef STHENOMI_STENCIL_GRAD_H
#define STHENOMI_STENCIL_GRAD_H

#include "sthenomi_stencil.h"
#include "sthenomi_conv_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sgp_logpdf_grad_conv for every spec that function takes (patch terms and product chains included), plus stencil terms, plus
 * the input points: grad_inputs (NULL: none) holds one pointer per spec input (NULL: not asked for), each dim x n packed, as
 * sgp_logpdf_grad_x.  On a spec without stencil terms logpdf_out, grad_y, grad_mean, grad_noise, grad_coef and grad_inscale
 * are bit for bit sgp_logpdf_grad_conv's. */
int sgp_logpdf_grad_stencil(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind, const double* noise,
                            const double* y, double* logpdf_out, double* grad_y, double* grad_mean, double* grad_noise,
                            double* grad_coef, double* grad_inscale, double* const* grad_inputs);

/* sgp_kernelmatrix_diag_grad_conv plus stencil terms: sum_i w[i] d var_i / d theta over the diagonal block pairs of `spec`,
 * and (grad_inputs as above; NULL: none) its gradient with respect to the input points: the row input of a term receives
 * + and its column input - the same per-point sum, so a term that reads one input on both sides contributes nothing.  For
 * a one-sided patch term of a diagonal pair the plain side's entry must be NULL as well (rc < 0 otherwise): not formed. */
int sgp_kernelmatrix_diag_grad_stencil(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w, double* grad_coef,
                                       double* grad_inscale, double* const* grad_inputs);

/* sgp_elbo_grad_conv plus stencil terms in zz and xz: exactly its arguments and outputs; elbo_out is bit for bit sgp_elbo's
 * value.  grad_inputs_zz / grad_inputs_xz may be NULL, and so may any entry. */
int sgp_elbo_grad_stencil(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                          const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind, const double* z_noise,
                          const double* y, double* elbo_out, double* grad_y, double* grad_mean, double* grad_noise,
                          double* grad_var_x, double* grad_z_noise, double* grad_coef_zz, double* grad_inscale_zz,
                          double* grad_coef_xz, double* grad_inscale_xz, double* const* grad_inputs_zz,
                          double* const* grad_inputs_xz);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_STENCIL_GRAD_H */
