/* sthenomi_kprod_grad.h -- the gradients that carry product chains (include/sthenomi_kprod.h) beyond the kernel parameters of
 * logpdf: the points the factors read, function-valued scales, the diagonal, and everything behind the ELBO, through
 * libsthenomi_kprod_grad.so.
 *
 * An extension in a header and a library of its own, as include/sthenomi_kprod.h is: that header's entry points are a fixed
 * table.  libsthenomi_kprod_grad.so links against libsthenomi.so and works on the contexts, specs and error state created
 * there.  Plain C like the product header.
 *
 * What still refuses product chains outright (rc < 0, a message naming "product"), each a pull request of its own:
 * sgp_logpdf_grad_batch, sgp_logpdf_grad_pool, the fp32 entry points (sgp_*_f32), every multi-GPU context, and products with
 * patch or stencil sides (refused wherever a spec is uploaded). */
#ifndef STHENOMI_KPROD_GRAD_H
#define STHENOMI_KPROD_GRAD_H

#include "sthenomi_kprod.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The superset family: what sgp_logpdf_grad_xs, sgp_kernelmatrix_diag_grad_xs and sgp_elbo_grad_xs return, for any spec they
 * take AND for specs with product chains, plus d / d param per term (the convention of sgp_logpdf_grad_param).  fp64, a
 * single-GPU context (a multi-GPU context refuses all three with rc < 0), no patch or stencil sides.  Every output may be NULL;
 * the arrays of pointers are indexed as their namesakes in include/sthenomi.h (grad_inputs by spec input, the scale arrays by
 * element of spec->terms; an entry may be NULL).  Outputs shared with the namesake are bit for bit the namesake's on a spec
 * without chains, and sgp_logpdf_grad_param's on any spec.
 *
 * For a chain with head h write W_ij = G_ij coef_h rs_i cs_j and E^f_ij = prod_{f' != f} k_f' (formed from prefix and suffix
 * products, never by division: a factor that is exactly 0 gives exact zeros for the others' share and finite values for its
 * own).  Factor f reads x^f (its row_input) and x'^f (its col_input).  Row side of a block pair:
 *     grad_inputs[row_input(f)][:, i] += sum_j W_ij E^f_ij d k_f / d x (x^f_i, x'^f_j)
 *     grad_rowscale[h][i]             += sum_j G_ij coef_h cs_j prod_f k_f                       (only heads carry scales)
 * with d k / d x = 2 kappa'(d^2) (x - x') for the distance kinds (SE / Matern: as on the plain path, Matern-1/2 contributing 0
 * at coincident points; RQ: kappa' = -1/2 (1 + u)^(-alpha - 1), u = d^2 / (2 alpha), finite where d^2 or u overflows), x' for
 * SGP_LINEAR, 0 for SGP_CONST and SGP_WHITE.  Several factors of one chain may read one input: their sums land in one array.
 * A symmetric spec takes the row side twice (k(x, y) = k(y, x) for every kind, SGP_LINEAR included); the rectangular xz spec
 * of the ELBO takes a row pass for x and a transposed pass for z.
 *
 * On the diagonal, var_i = coef_h rs_i cs_i prod_f k_f(xr^f_i, xc^f_i): a distance kind gives the row input + and the column
 * input - 2 kappa' (xr - xc) (they cancel when both are one array); SGP_LINEAR gives the row input xc and the column input xr,
 * both added when they are one array. */
int sgp_logpdf_grad_param_xs(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind, const double* noise,
                             const double* y, double* logpdf_out, double* grad_y, double* grad_mean, double* grad_noise,
                             double* grad_coef, double* grad_inscale, double* grad_param, double* const* grad_inputs,
                             double* const* grad_rowscale);
/* sum_i w[i] d var_i / d theta over the diagonal of `spec` */
int sgp_kernelmatrix_diag_grad_param(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w, double* grad_coef,
                                     double* grad_inscale, double* grad_param, double* const* grad_inputs,
                                     double* const* grad_rowscale, double* const* grad_colscale);
/* elbo_out is bit for bit sgp_elbo's value */
int sgp_elbo_grad_param(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                        const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind, const double* z_noise,
                        const double* y, double* elbo_out, double* grad_y, double* grad_mean, double* grad_noise,
                        double* grad_var_x, double* grad_z_noise, double* grad_coef_zz, double* grad_inscale_zz,
                        double* grad_param_zz, double* grad_coef_xz, double* grad_inscale_xz, double* grad_param_xz,
                        double* const* grad_inputs_zz, double* const* grad_inputs_xz, double* const* grad_rowscale_zz,
                        double* const* grad_rowscale_xz, double* const* grad_colscale_xz);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_KPROD_GRAD_H */
