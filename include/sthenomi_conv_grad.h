/* sthenomi_conv_grad.h -- gradients of logpdf, the diagonal and the ELBO through patch (convolutional) terms
 * (include/sthenomi_conv.h), through libsthenomi_conv_grad.so.
 *
 * An extension in a header and a library of its own, as include/sthenomi_conv.h is: the product header's entry points are a
 * fixed table, and its gradient entry points keep refusing patch terms.  libsthenomi_conv_grad.so links against
 * libsthenomi.so and works on the contexts, specs and error state created there.  Plain C like the product header.
 *
 * A patch term of a block pair is K_ij = coef rs_i cs_j sum_p sum_q k(patch_p x_i, patch_q x'_j) (one of the sums is absent
 * when that side is plain).  With the cotangent G of the call (logpdf: (alpha alpha' - C^-1) / 2; the ELBO: its G_xz and G_zz)
 *     grad_coef[t]    = sum_ij G_ij rs_i cs_j sum_pq k
 *     grad_inscale[t] = sum_ij G_ij coef rs_i cs_j sum_pq d k(g a, g b) / dg |_{g = 1}
 * exactly as for a plain term, one entry per element of spec->terms in the caller's order.  Per-workgroup partial sums are
 * reduced in a fixed order: two calls with the same arguments return the same bits.  The limits of sthenomi_conv.h hold
 * (height * width <= 3072, patch_h * patch_w <= 64).
 *
 * What these three refuse (rc < 0, each by name): stencil terms (include/sthenomi_stencil.h; include/sthenomi_stencil_grad.h
 * carries them, and patch terms with them), a multi-GPU context, and --
 * sgp_elbo_grad_conv -- product chains, as sgp_elbo_grad does.  Gradients with respect to the images of a patched side are
 * not formed.  Everything else that takes a gradient keeps refusing patch terms: sgp_logpdf_grad*, sgp_elbo_grad*,
 * sgp_kernelmatrix_diag_grad*, the batch and pool gradients, the *_param family, fp32. */
#ifndef STHENOMI_CONV_GRAD_H
#define STHENOMI_CONV_GRAD_H

#include "sthenomi_conv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sgp_logpdf_grad for any spec that function takes (product chains included), plus patch terms: same arguments and outputs.
 * On a spec without patch terms every output is bit for bit sgp_logpdf_grad's. */
int sgp_logpdf_grad_conv(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind, const double* noise,
                         const double* y, double* logpdf_out, double* grad_y, double* grad_mean, double* grad_noise,
                         double* grad_coef, double* grad_inscale);

/* sgp_kernelmatrix_diag_grad plus patch terms: sum_i w[i] d var_i / d theta over the diagonal block pairs of `spec` */
int sgp_kernelmatrix_diag_grad_conv(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w, double* grad_coef,
                                    double* grad_inscale);

/* sgp_elbo_grad_x plus patch terms in zz and xz: same arguments and outputs; elbo_out is bit for bit sgp_elbo's value.
 * grad_inputs_zz / grad_inputs_xz may be NULL (no input gradients), and so may any entry.  The entry of an input that a
 * patched side reads holds images and must be NULL (rc < 0 otherwise).  The plain side of a one-sided term -- the inducing
 * patches z of cov(f, g, x, z) -- receives
 *     grad_inputs[k][:, j] += sum_i G_ij coef rs_i cs_j sum_p 2 kappa'(|patch_p x_i - z_j|^2) (z_j - patch_p x_i)
 * (kappa' = d k / d (d^2); Matern-1/2 contributes 0 at coincident points, as everywhere else). */
int sgp_elbo_grad_conv(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                       const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind, const double* z_noise,
                       const double* y, double* elbo_out, double* grad_y, double* grad_mean, double* grad_noise,
                       double* grad_var_x, double* grad_z_noise, double* grad_coef_zz, double* grad_inscale_zz,
                       double* grad_coef_xz, double* grad_inscale_xz, double* const* grad_inputs_zz,
                       double* const* grad_inputs_xz);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_CONV_GRAD_H */
