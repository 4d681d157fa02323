// update_posterior for a sparse (VFE) posterior: absorb new data with the inducing points fixed (include/sthenomi_vfe_update.h).
//
// A VFE posterior depends on the data only through sums over the data points -- sum_n a_n a_n', A delta and four scalars, the
// "part" of vfe_part_len (capi.hip) -- and sgp_sparse_posterior_create keeps them (sgp_sparse_post::d_sums) next to Lz.  A
// batch of n new points is absorbed in O(n M^2 + M^3 / 3), whatever the number of points absorbed before:
//   S' <- the kept sums                                     (a scratch copy from the context's cache)
//   S' += the batch's rows                                  (capi.hip: the row-chunk loop of vfe_rows_partial in append mode --
//                                                            assembly, row solve against the kept Lz, transposition + column
//                                                            sums, split-K Gram with beta = 1 from the first chunk on)
//   F  <- G' + I, row m_pad = (A delta)', zeros elsewhere   (vfe_prepare_factor_kernel: one pass over the buffer)
//   the bordered factorisation of F, its logdet, the border row's sum of squares          (as capi.hip: vfe_finish)
// Only when the factorisation succeeded do S', F and the inverse diagonal blocks replace what the posterior holds: they are
// copied over its buffers, three device-to-device copies after the last check, so a refused or failed call leaves the
// posterior bit for bit what it was.
// Every launch is ordered on the context's stream; no kernel here waits on another workgroup.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_vfe_update.h"

#include <string>

using namespace sgp;

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

// The working factor buffer from the sums, EVERY 128 x 128 tile of the (T + 1) x T tile grid written once: workgroup
// (tr, tc) = (blockIdx.x, blockIdx.y).
//   tc <= tr < T : F = G (+ 1 on the diagonal of a diagonal tile)          -- the lower tiles the factorisation reads
//   tr == T      : row 0 of the border tile row = (A delta)', rows 1 .. 127 zero (they ride through the factorisation)
//   tr < tc      : zero (never read; the scratch buffer comes from the cache, so they are defined, not left-overs)
// 256 threads: a wave moves one column of the tile per pass with 16-byte loads and stores (the leading dimension is a
// multiple of 128 and both bases are allocation starts, so every access is aligned).  Bounds: tr <= T, tc < T by the grid;
// rows tr 128 + [0, 128) < ld = (T + 1) 128, columns tc 128 + [0, 128) < T 128.
__global__ __launch_bounds__(256) void vfe_prepare_factor_kernel(const double* __restrict__ G, const double* __restrict__ dots,
                                                                 double* __restrict__ F, long ld, long T) {
  const long tr = blockIdx.x, tc = blockIdx.y;
  if (tr > T || tc >= T) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long off = tr * TILE + 2 * lane + tc * TILE * ld;
  const int r_in = 2 * lane;   // this lane's two rows inside the tile: r_in, r_in + 1
#pragma unroll 8
  for (int j = 0; j < TILE / 4; ++j) {
    const int col = w + 4 * j;
    d2 v;
    if (tr == T) {
      v.x = lane == 0 ? dots[tc * TILE + col] : 0.0;
      v.y = 0.0;
    } else if (tr < tc) {
      v.x = 0.0;
      v.y = 0.0;
    } else {
      v = *(const d2*)(G + off + col * ld);
      if (tr == tc) {
        if (r_in == col) v.x += 1.0;
        if (r_in + 1 == col) v.y += 1.0;
      }
    }
    *(d2*)(F + off + col * ld) = v;
  }
}

const char* const WHO = "sgp_sparse_posterior_update";

int update_impl(sgp_sparse_post* post, const sgp_cov_spec* xz_new, const double* var_x_new, const double* mean_x_new,
                int noise_kind, const double* noise_new, const double* y_new, double* elbo_out) {
  sgp_ctx* ctx = post->ctx;
  CtxScope scope(ctx);
  SpecGuard gx;
  CHECK_RC(drv_dspec_create(ctx, xz_new, &gx.ds));
  const long n_new = gx.ds->N, M = post->M, m_pad = post->m_pad, ldg = post->ldg, T = m_pad / TILE;
  REFUSE_UNLESS(gx.ds->M == M, WHO, "the columns of xz_new are not the inducing points the posterior was created with");
  REFUSE_UNLESS(n_new >= 1, WHO, "no new data points");
  const long part_len = drv_vfe_part_len(m_pad), wg_len = T * drv_invd_stride();
  hipStream_t s = ctx->stream;
  StageTimer tm(ctx, s);
  tm.mark(0);
  DevBuf dS, dF, dwg;
  CHECK_RC(dS.alloc((size_t)part_len));
  CHECK_RC(dF.alloc((size_t)(ldg * m_pad)));
  CHECK_RC(dwg.alloc((size_t)wg_len));
  SGP_HIP(hipMemcpyAsync(dS.p, post->d_sums, sizeof(double) * part_len, hipMemcpyDeviceToDevice, s));
  // ---- the batch's rows join the sums (stage slots 0 - 4 as vfe_rows_partial)
  CHECK_RC(drv_vfe_rows_append(ctx, gx.ds, M, var_x_new, mean_x_new, noise_kind, noise_new, y_new, post->dLz, post->d_wz, dS.p,
                               tm));
  // ---- prepare + factor + scalars (slot 5), as capi.hip: vfe_finish
  tm.mark(5);
  double* d_dots = dS.p + ldg * m_pad;
  double* d_sc = d_dots + m_pad;
  hipLaunchKernelGGL(vfe_prepare_factor_kernel, dim3((unsigned)(T + 1), (unsigned)T), dim3(256), 0, s, (const double*)dS.p,
                     (const double*)d_dots, dF.p, ldg, T);
  SGP_HIP(hipGetLastError());
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  CHECK_RC(drv_chol_sub(ctx, dF.p, ldg, m_pad, ldg, dwg.p, s));
  CHECK_RC(launch_sum_array(ctx->d_slots, T, d_sc + 4, s));
  CHECK_RC(launch_rowsumsq(dF.p + m_pad, ldg, m_pad, 1, d_sc + 5, 0, s));
  double h[6];
  SGP_HIP(hipMemcpyAsync(h, d_sc, sizeof(double) * 6, hipMemcpyDeviceToHost, s));
  const int info = drv_fetch_info(ctx, s);   // drains the stream
  if (info < 0) {
    tm.finish();
    return -3;
  }
  if (info > 0) {
    tm.finish();
    set_error(std::string(WHO) + ": A A' + I is not positive definite (leading minor " + std::to_string(info) + ")");
    return info;
  }
  // ---- success: the new sums, factor and inverse blocks replace the kept ones
  SGP_HIP(hipMemcpyAsync(post->d_sums, dS.p, sizeof(double) * part_len, hipMemcpyDeviceToDevice, s));
  SGP_HIP(hipMemcpyAsync(post->dG, dF.p, sizeof(double) * ldg * m_pad, hipMemcpyDeviceToDevice, s));
  SGP_HIP(hipMemcpyAsync(post->d_wg, dwg.p, sizeof(double) * wg_len, hipMemcpyDeviceToDevice, s));
  tm.finish();
  SGP_HIP(hipStreamSynchronize(s));
  post->n_total += n_new;
  if (elbo_out) {
    // the formula of sgp_elbo (capi.hip: sgp_elbo_impl) on the kept scalars of all the points absorbed so far; h[2], the
    // sum of var / s2, counts the updates' points only -- the create call has no var_x (see the header)
    const double tmp = h[0] + h[4] + h[1] - h[5];
    const double dtc = -0.5 * ((double)post->n_total * 1.8378770664093453 + tmp);
    elbo_out[0] = dtc - 0.5 * (h[2] - h[3]);
  }
  return 0;
}

}  // namespace

namespace sgp {

int drv_sparse_posterior_update(sgp_sparse_post* post, const sgp_cov_spec* xz_new, const double* var_x_new,
                                const double* mean_x_new, int noise_kind, const double* noise_new, const double* y_new,
                                double* elbo_out) {
  REFUSE_UNLESS(post && xz_new && var_x_new && noise_new && y_new, WHO, "NULL argument");
  sgp_ctx* ctx = post->ctx;
  REFUSE_UNLESS(drv_ctx_is_live(ctx, post->ctx_serial), WHO, "the context this posterior was created on has been destroyed");
  REFUSE_UNLESS(!ctx->multi, WHO, "not supported on a multi-GPU context (create the posterior on the stacked data)");
  REFUSE_UNLESS(post->d_sums != nullptr, WHO,
                "this posterior keeps no sums over its data points (a posterior created on a multi-GPU context keeps none)");
  REFUSE_UNLESS(noise_kind == SGP_NOISE_SCALAR || noise_kind == SGP_NOISE_DIAG, WHO,
                "Sigma_y must be isotropic or diagonal (as in AbstractGPs.elbo)");
  REFUSE_UNLESS(xz_new->n_row_blocks >= 1 && xz_new->n_col_blocks >= 1 && xz_new->row_len && xz_new->col_len, WHO,
                "xz_new has no blocks");
  long n_new = 0, m_cols = 0;
  for (int i = 0; i < xz_new->n_row_blocks; ++i) n_new += xz_new->row_len[i];
  for (int i = 0; i < xz_new->n_col_blocks; ++i) m_cols += xz_new->col_len[i];
  REFUSE_UNLESS(m_cols == post->M, WHO, "the columns of xz_new are not the inducing points the posterior was created with");
  REFUSE_UNLESS(n_new >= 1, WHO, "no new data points");
  // (a dataflow time-out reruns the call on the launch-based schedule: the posterior is untouched until the call succeeded)
  return drv_with_df_fallback(ctx, [&]() {
    return update_impl(post, xz_new, var_x_new, mean_x_new, noise_kind, noise_new, y_new, elbo_out);
  });
}

int drv_sparse_posterior_count(sgp_sparse_post* post, int64_t* n_out) {
  REFUSE_UNLESS(post && n_out, "sgp_sparse_posterior_count", "NULL argument");
  REFUSE_UNLESS(post->d_sums != nullptr, "sgp_sparse_posterior_count",
                "this posterior keeps no sums over its data points (a posterior created on a multi-GPU context keeps none)");
  *n_out = post->n_total;
  return 0;
}

}  // namespace sgp
