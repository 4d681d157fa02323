/* sthenomi_stencil.h -- stencil covariance terms, registered through libsthenomi_stencil.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h), in a header and a library of its own, as
 * include/sthenomi_conv.h is: the product header's entry points are a fixed table.  libsthenomi_stencil.so links against
 * libsthenomi.so and works on the contexts, specs and error state created there.  Plain C like the product header.
 *
 * A stencil process is a weighted sum of shifted views of one process f:
 *     g(x) = sum_q w_q f(x - a_q),   q = 1 .. npoints
 * (the sign of Stheno's Shift).  The reference's examples/quadrature-convolution (Gauss-Hermite quadrature),
 * examples/custom_affine_transformations (f(x) + f(x + 3)) and examples/differentiation (finite differences) are such sums.
 *   cov(g, g', x, y)[i, j] = sum_p w_p sum_q v_q k_f(x_i - a_p, y_j - b_q)
 *   cov(g, f, x, y)[i, j]  = sum_p w_p k_f(x_i - a_p, y_j)          (and its mirror image)
 *
 * A term of a sgp_cov_spec reads a stencil through its `reserved` field, with ids from the same per-context table as the
 * patch geometries of include/sthenomi_conv.h:
 *     reserved = row_id | (col_id << 16),   id 0: that side is read plainly.
 * Both sides' inputs hold the unshifted points, of the same dim; a stencil's dim equals the dim of the side it is on.  A
 * term cannot pair a patch side with a stencil side.  Every entry point that creates a spec checks the ids against the
 * context and fails with rc < 0 on an unknown one.
 *
 * Stencil terms run on every fp64 operator of a single-GPU context: sgp_kernelmatrix / _diag, sgp_logpdf (_batch),
 * sgp_rand, the posterior, sgp_elbo and the sparse posterior.  Their gradients come from include/sthenomi_stencil_grad.h
 * (sgp_logpdf_grad_stencil, sgp_kernelmatrix_diag_grad_stencil, sgp_elbo_grad_stencil; libsthenomi_stencil_grad.so), and the
 * gradients with respect to a stencil's own weights and offsets from include/sthenomi_stencil_wo.h (the same three names
 * with _wo; libsthenomi_stencil_wo.so).  These
 * refuse them with rc < 0 and a message naming "stencil": the gradient entry points of the other headers (sgp_*_grad*,
 * sgp_logpdf_grad_batch / _pool, the *_conv and *_param families), the fp32 entry points (sgp_*_f32) and every multi-GPU
 * context (which registers none).
 * Limits: 1 <= npoints <= 64, 1 <= dim <= 16, finite offsets and weights; anything else fails with rc < 0. */
#ifndef STHENOMI_STENCIL_H
#define STHENOMI_STENCIL_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t dim, npoints;
  const double* offsets;  /* dim x npoints, column-major: offset q at offsets[q * dim .. q * dim + dim - 1] */
  const double* weights;  /* npoints */
} sgp_stencil;

/* Register a stencil on ctx (the arrays are copied); *id_out >= 1 stays valid for the context's lifetime.  A bitwise-equal
 * stencil registered before returns the same id.  A multi-GPU context refuses (rc < 0). */
int sgp_stencil_register(sgp_ctx* ctx, const sgp_stencil* st, int32_t* id_out);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_STENCIL_H */
