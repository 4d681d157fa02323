/* sthenomi_conv.h -- patch (convolutional) covariance terms, registered through libsthenomi_conv.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h), in a header and a library of its own, as
 * include/sthenomi_batch.h is: the product header's entry points are a fixed table.  libsthenomi_conv.so links against
 * libsthenomi.so and works on the contexts, specs and error state created there.  Plain C like the product header.
 *
 * The process f = patch_convolve(g) sums g over every ph x pw patch, stride 1, of an H x W image
 * (the reference's examples/convolutional_gp/script.jl: the convolutional GP of van der Wilk et al., 2017).  Patch (p, q)
 * of image n is reshape(X[p:p+ph-1, q:q+pw-1, n], :): column-major, row index fastest; P = (H - ph + 1)(W - pw + 1).
 *   cov(f, f, x, x')[i, j] = sum_p sum_q k_g(patch_p x_i, patch_q x'_j)
 *   cov(f, g, x, z)[i, j]  = sum_p k_g(patch_p x_i, z_j)          (and its mirror image)
 *
 * A term of a sgp_cov_spec reads patches through its `reserved` field:
 *     reserved = row_geom_id | (col_geom_id << 16),   id 0: that side is read plainly.
 * A patched side's sgp_input holds raw images: dim = height * width, one column-major image per column.  The other side's
 * dim is patch_h * patch_w, or it is patched too with the same patch size.  Every entry point that creates a spec
 * (sgp_dspec_create and all that take a sgp_cov_spec) checks the ids against the context and fails with rc < 0 on an
 * unknown one.  reserved == 0 everywhere is the product header's plain spec.
 *
 * Patch terms run on every fp64 operator of a single-GPU context: sgp_kernelmatrix / _diag, sgp_logpdf (_batch),
 * sgp_rand, the posterior, sgp_elbo and the sparse posterior.  Their gradients come from include/sthenomi_conv_grad.h
 * (sgp_logpdf_grad_conv, sgp_kernelmatrix_diag_grad_conv, sgp_elbo_grad_conv; libsthenomi_conv_grad.so).  These refuse them
 * with rc < 0: the gradient entry points of the other headers (sgp_*_grad*, sgp_logpdf_grad_batch / _pool, the *_param
 * family), the fp32 entry points (sgp_*_f32) and every multi-GPU context.
 * Limits: height * width <= 3072, patch_h * patch_w <= 64. */
#ifndef STHENOMI_CONV_H
#define STHENOMI_CONV_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t height, width;     /* image size; images are column-major, height fastest */
  int32_t patch_h, patch_w;  /* patch size, 1 <= patch_h <= height, 1 <= patch_w <= width */
} sgp_patch_geom;

/* Register a geometry on ctx; *id_out >= 1 stays valid for the context's lifetime.  An equal geometry registered before
 * returns the same id.  A multi-GPU context refuses (rc < 0). */
int sgp_conv_geom(sgp_ctx* ctx, const sgp_patch_geom* geom, int32_t* id_out);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_CONV_H */
