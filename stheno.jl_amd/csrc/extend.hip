// update_posterior: extend a kept Cholesky factor by the rows of new data (include/sthenomi_extend.h).
//
// The factor of the stacked covariance [[C11, C12], [C21, C22]] shares its first columns with chol(C11): appending points
// leaves columns [0, c0) of L unchanged, c0 = 128 floor(N / 128) -- the partial tile column [c0, n_pad) held identity
// padding next to its real columns and is recomputed with the new rows rather than patched.  The driver restarts the
// factorisation at c0 on a sub-matrix of the kept buffer:
//   assemble rows [c0, n_pad') of the stacked spec (lower tiles) + identity padding + the (y - m)' border row (all columns)
//   R = rows [c0, m_tot') x columns [0, c0)  <-  R L11^-T        (the border row rides along: its head is the old z)
//   A[c0:, c0:n_pad') -= R R'                                     (lower tiles, K = c0)
//   the bordered factorisation of the sub-matrix at (c0, c0)      (capi.hip: chol_bordered, dense)
// Every launch is ordered on the context's stream; no kernel here waits on another workgroup.
#include "ctx.h"
#include "driver.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace sgp;

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

// Tile-wise relayout of the lower triangle between two leading dimensions: workgroup k copies the 128 x 128 tile (tr, tc),
// tc <= tr < T, k = tr (tr + 1) / 2 + tc -- the grid covers the lower tiles only (the strictly upper tiles hold no factor
// values).  256 threads: a wave moves one column of the tile per pass with 16-byte loads and stores (both leading
// dimensions are multiples of 128 and the bases are allocation starts, so every access is aligned).
__global__ __launch_bounds__(256) void tile_relayout_lower_kernel(const double* __restrict__ src, long lds,
                                                                   double* __restrict__ dst, long ldd, long T) {
  const long k = blockIdx.x;
  long tr = (long)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
  while (tr * (tr + 1) / 2 > k) --tr;
  while ((tr + 1) * (tr + 2) / 2 <= k) ++tr;
  const long tc = k - tr * (tr + 1) / 2;
  if (tr >= T || tc > tr) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double* sp = src + tr * TILE + 2 * lane + tc * TILE * lds;
  double* dp = dst + tr * TILE + 2 * lane + tc * TILE * ldd;
#pragma unroll 8
  for (int j = 0; j < TILE / 4; ++j) {
    const long col = w + 4 * j;
    *(d2*)(dp + col * ldd) = *(const d2*)(sp + col * lds);
  }
}

// out[b] = 2 sum_i log L[i, i] over the 128-block b < T0 of the kept columns (one workgroup of 128 threads per block, a
// fixed tree: two wave sums, then their sum); out[T0 + q] = slots[q], q < T1: the contributions the trailing factorisation
// left.  launch_sum_array over out then gives the logdet of the whole factor in a fixed order.
__global__ __launch_bounds__(128) void logdet_blocks_kernel(const double* __restrict__ L, long ld, long T0,
                                                            const double* __restrict__ slots, long T1,
                                                            double* __restrict__ out) {
  __shared__ double sh[2];
  const long b = blockIdx.x;
  if (b >= T0) {
    if (threadIdx.x == 0 && b - T0 < T1) out[b] = slots[b - T0];
    return;
  }
  const long i = b * TILE + threadIdx.x;
  double v = log(L[i + i * ld]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) out[b] = 2.0 * (sh[0] + sh[1]);
}

constexpr long WB = 4 * TILE;   // column block of the row solve (capi.hip: row_trsm)
// The deep products of the extension have few C tiles (2 - 4 tile rows for a few to a few hundred new points): one launch
// is then 8 - 16 workgroups on 256 CUs with K up to N, and its time is the latency of one workgroup's k loop.  Up to this
// many C tiles per launch they are split over K (launch_gemm_nt_splitk + launch_splitk_reduce); above it drv_row_trsm /
// launch_gemm_nt_update run as they are.  Measured (profiles/r08_extend.json, N = 4096 / 16 384 / 32 768): the row solve of
// 2 tile rows (8 tiles per launch) takes 2.1 / 20.6 / 71.3 ms split against 2.9 / 36.1 / 137.0 ms as single launches, and
// that of 9 tile rows (36 tiles) 2.1 / 20.3 / 71.8 against 2.9 / 36.3 / 137.6 ms -- split wins at both, so the rule covers
// what was measured plus the tenth tile row an unaligned N adds to 1024 new points; beyond that nothing has been timed.
constexpr long SPLITK_MAX_TILES = 40;
constexpr long SPLITK_TARGET_WGS = 256;

// K slices of a product with `tiles` C tiles: the power of two that brings the launch to about one workgroup per CU, whose
// slices stay whole 16-column chunks and at least a tile deep (1: no split)
int extend_nsplit(long tiles, long K) {
  int ns = 1;
  while (ns < 32 && tiles * (ns * 2) <= SPLITK_TARGET_WGS && K % (16L * ns * 2) == 0 && K / (ns * 2) >= TILE) ns *= 2;
  return ns;
}
bool few_tiles(long tiles, long ld_a, long ld_b) { return tiles <= SPLITK_MAX_TILES && ld_a <= 65536 && ld_b <= 65536; }

// doubles of slab scratch the split-K row solve of `nrows` rows against n columns needs
size_t row_solve_scratch(long nrows, long n) {
  size_t need = 1;
  for (long c = WB; c < n; c += WB) {
    const long wb = std::min(WB, n - c);
    const int ns = extend_nsplit((nrows / TILE) * (wb / TILE), c);
    if (ns > 1) need = std::max(need, (size_t)splitk_slabs(nrows, c, ns) * (size_t)(nrows * wb));
  }
  return need;
}

// R <- R L^-T as capi.hip's row_trsm (512-column blocks, left-looking), the deep product of every block split over K: the
// slabs are summed in ascending k and applied with alpha = -1; the in-block part is row_trsm's own
int row_solve_splitk(double* R, long ldr, long nrows, const double* L, long ldl, const double* d_inv, long n, double* part,
                     hipStream_t s) {
  for (long c = 0; c < n; c += WB) {
    const long wb = std::min(WB, n - c);
    if (c > 0) {
      const int ns = extend_nsplit((nrows / TILE) * (wb / TILE), c);
      if (ns > 1) {
        const long stride = nrows * wb;
        CHECK_RC(launch_gemm_nt_splitk(R, ldr, L + c, ldl, part, nrows, nrows, wb, c, ns, stride, 0, s));
        CHECK_RC(launch_splitk_reduce(part, stride, ns, R + c * ldr, ldr, nrows, wb, -1.0, 1.0, 0, s, 0, nrows));
      } else {
        CHECK_RC(launch_gemm_nt(R, ldr, L + c, ldl, R + c * ldr, ldr, nrows, wb, c, -1.0, 1.0, -(1L << 40), 0, 0, s));
      }
    }
    CHECK_RC(drv_row_trsm_block(R, ldr, nrows, L, ldl, d_inv, c, wb, s));
  }
  return 0;
}

int row_solve(sgp_ctx* ctx, int schedule, double* R, long ldr, long nrows, const double* L, long ldl, const double* d_inv,
              long n, double* part, hipStream_t s) {
  if (schedule == 1) return row_solve_splitk(R, ldr, nrows, L, ldl, d_inv, n, part, s);
  return drv_row_trsm(ctx, R, ldr, nrows, L, ldl, d_inv, n, s);
}

struct ExtendArgs {
  sgp_post* post;
  const sgp_cov_spec* spec_all;
  const double *mean_all, *noise, *y_all;
  int noise_kind;
  long n_new, reserve_n;
  double *alpha_out, *logpdf_out;
};

int extend_impl(const ExtendArgs& a) {
  sgp_post* post = a.post;
  sgp_ctx* ctx = post->ctx;
  CtxScope scope(ctx);
  SpecGuard g;
  CHECK_RC(drv_dspec_create(ctx, a.spec_all, &g.ds));
  const long N0 = post->N, N1 = N0 + a.n_new, c0 = N0 / TILE * TILE, IS = drv_invd_stride();
  CHECK_ARG(g.ds->N == N1, "sgp_posterior_extend: spec_all does not have N + n_new points");
  int64_t np1_, mt1_;
  sgp_geometry(N1, 1, &np1_, &mt1_);
  const long np1 = np1_, mt1 = mt1_, T0 = c0 / TILE, T1 = (np1 - c0) / TILE;
  CHECK_ARG(np1 / TILE <= ctx->n_slots, "sgp_posterior_extend: matrix too large for the logdet slot buffer");
  hipStream_t s = ctx->stream;
  StageTimer tm(ctx, s);
  DevBuf dmean, dY, dnoise;
  if (a.mean_all) CHECK_RC(dmean.upload(a.mean_all, N1));
  CHECK_RC(dY.upload(a.y_all, N1));
  if (a.noise_kind == SGP_NOISE_DIAG) CHECK_RC(dnoise.upload(a.noise, N1));
  const double sigma2 = a.noise_kind == SGP_NOISE_SCALAR ? a.noise[0] : 0.0;
  tm.mark(0);

  // ---- the buffer: in place while the new size fits what was allocated, else a new one with the kept lower tiles copied
  const bool inplace = np1 <= post->n_cap && mt1 <= post->ld;
  double *A = post->dA, *W = post->d_wall;
  long ld = post->ld, n_cap = post->n_cap;
  struct NewBuf {   // freed on every exit that does not hand them to the posterior
    double *A = nullptr, *W = nullptr;
    ~NewBuf() {
      if (A) hipFree(A);
      if (W) hipFree(W);
    }
  } fresh;
  // in place: what the call overwrites of the OLD posterior -- rows [c0, m_tot) of its columns (the partial tile column, the
  // rows of the old points of that tile in the kept columns, the solved border row) and the d_wall block of that tile column
  DevBuf save, save_w;
  const long sr = post->m_tot - c0, sw = post->n_pad / TILE - T0;
  if (inplace) {
    CHECK_RC(save.alloc((size_t)sr * post->n_pad));
    SGP_HIP(hipMemcpy2DAsync(save.p, sizeof(double) * sr, A + c0, sizeof(double) * ld, sizeof(double) * sr, (size_t)post->n_pad,
                             hipMemcpyDeviceToDevice, s));
    if (sw > 0) {
      CHECK_RC(save_w.alloc((size_t)sw * IS));
      SGP_HIP(hipMemcpyAsync(save_w.p, W + T0 * IS, sizeof(double) * sw * IS, hipMemcpyDeviceToDevice, s));
    }
  } else {
    int64_t ncap_, ld_;
    sgp_geometry(std::max(N1, a.reserve_n), 1, &ncap_, &ld_);
    n_cap = ncap_;
    ld = ld_;
    if (hipMalloc(&fresh.A, sizeof(double) * (size_t)ld * n_cap) != hipSuccess ||
        hipMalloc(&fresh.W, sizeof(double) * (size_t)(n_cap / TILE) * IS) != hipSuccess) {
      (void)hipGetLastError();
      set_error("sgp_posterior_extend: hipMalloc of the larger factor buffer failed (the old one stays resident until success)");
      return -2;
    }
    A = fresh.A;
    W = fresh.W;
    if (T0 > 0) {
      hipLaunchKernelGGL(tile_relayout_lower_kernel, dim3((unsigned)(T0 * (T0 + 1) / 2)), dim3(256), 0, s,
                         (const double*)post->dA, post->ld, A, ld, T0);
      SGP_HIP(hipGetLastError());
      SGP_HIP(hipMemcpyAsync(W, post->d_wall, sizeof(double) * T0 * IS, hipMemcpyDeviceToDevice, s));
    }
  }
  auto restore = [&]() -> int {   // a failed in-place extension leaves the bits the posterior had
    if (!inplace) return 0;
    SGP_HIP(hipMemcpy2DAsync(A + c0, sizeof(double) * ld, save.p, sizeof(double) * sr, sizeof(double) * sr, (size_t)post->n_pad,
                             hipMemcpyDeviceToDevice, s));
    if (sw > 0) SGP_HIP(hipMemcpyAsync(W + T0 * IS, save_w.p, sizeof(double) * sw * IS, hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipStreamSynchronize(s));
    return 0;
  };

  double lp = 0.0;
  DevBuf dal;
  auto body = [&]() -> int {
    SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
    tm.mark(1);
    // ---- rows [c0, n_pad') of the stacked covariance, identity padding, raw (y - m)' for ALL columns at row n_pad'
    CHECK_RC(drv_assemble(g.ds, A, ld, T0, np1 / TILE, 0, np1 / TILE, 1, a.noise_kind, sigma2, dnoise.p, s));
    CHECK_RC(launch_fill_pad(A, ld, N1, np1, 0, np1, mt1, c0, s));
    CHECK_RC(launch_border_rows(A, ld, np1, N1, 0, np1, dY.p, N1, 1, a.mean_all ? dmean.p : nullptr, s));
    const long nrows = mt1 - c0;
    if (c0 > 0) {
      // ---- R <- R L11^-T, then the trailing block A[c0:, c0:n_pad') -= R R'; the schedule by the C tiles of a launch
      tm.mark(2);
      double* R = A + c0;
      const long rt = nrows / TILE, ut = T1 * (T1 + 1) / 2 + T1;
      const bool rs_split = few_tiles(rt * (WB / TILE), ld, ld);
      const int un = few_tiles(ut, ld, ld) ? extend_nsplit(ut, c0) : 1;
      DevBuf part;
      size_t need = rs_split ? row_solve_scratch(nrows, c0) : 1;
      if (un > 1) need = std::max(need, (size_t)splitk_slabs(nrows, c0, un) * (size_t)(nrows * (np1 - c0)));
      CHECK_RC(part.alloc(need));
      CHECK_RC(row_solve(ctx, rs_split ? 1 : 0, R, ld, nrows, A, ld, W, c0, part.p, s));
      tm.mark(3);
      double* C = A + c0 + c0 * ld;
      if (un > 1) {
        const long stride = nrows * (np1 - c0);
        CHECK_RC(launch_gemm_nt_splitk(R, ld, R, ld, part.p, nrows, nrows, np1 - c0, c0, un, stride, 1, s));
        CHECK_RC(launch_splitk_reduce(part.p, stride, un, C, ld, nrows, np1 - c0, -1.0, 1.0, 1, s, 0, nrows));
      } else {
        CHECK_RC(launch_gemm_nt_update(R, ld, C, ld, nrows, np1 - c0, c0, s));
      }
      SGP_HIP(hipStreamSynchronize(s));   // (the slab scratch goes back to the cache at scope exit)
    }
    tm.mark(4);
    CHECK_RC(drv_chol_sub(ctx, A + c0 + c0 * ld, ld, np1 - c0, nrows, W + T0 * IS, s));
    tm.mark(5);
    // ---- logdet over the kept columns + the slots of the trailing block, |z|^2 from the border row, alpha
    DevBuf dl, dz;
    CHECK_RC(dl.alloc((size_t)(T0 + T1)));
    hipLaunchKernelGGL(logdet_blocks_kernel, dim3((unsigned)(T0 + T1)), dim3(128), 0, s, (const double*)A, ld, T0,
                       (const double*)ctx->d_slots, T1, dl.p);
    SGP_HIP(hipGetLastError());
    CHECK_RC(launch_sum_array(dl.p, T0 + T1, ctx->d_scal, s));
    CHECK_RC(launch_rowsumsq(A + np1, ld, N1, 1, ctx->d_scal + 16, 0, s));
    CHECK_RC(launch_logpdf_final(ctx->d_scal, ctx->d_scal + 16, N1, 1, ctx->d_scal + 17, s));
    if (a.alpha_out) {
      CHECK_RC(dz.alloc((size_t)np1));
      CHECK_RC(dal.alloc((size_t)np1));
      CHECK_RC(drv_copy_strided(A + np1, ld, np1, dz.p, s));
      CHECK_RC(drv_back_substitute(A, ld, W, np1 - TILE, 0, np1, dz.p, dal.p, s));
    }
    SGP_HIP(hipMemcpyAsync(&lp, ctx->d_scal + 17, sizeof(double), hipMemcpyDeviceToHost, s));
    const int info = drv_fetch_info(ctx, s);   // (drains the stream)
    if (info < 0) return -3;
    if (info > 0) {
      set_error("matrix is not positive definite; Cholesky factorization failed at leading minor " + std::to_string(c0 + info));
      return (int)(c0 + info);
    }
    if (a.alpha_out) SGP_HIP(hipMemcpy(a.alpha_out, dal.p, sizeof(double) * N1, hipMemcpyDeviceToHost));
    return 0;
  };
  const int rc = body();
  if (rc != 0) {
    const std::string why = sgp_last_error();
    hipStreamSynchronize(s);
    (void)hipGetLastError();
    restore();
    set_error(why);
    return rc;
  }
  tm.finish();
  if (!inplace) {
    hipFree(post->dA);
    hipFree(post->d_wall);
    post->dA = fresh.A;
    post->d_wall = fresh.W;
    fresh.A = fresh.W = nullptr;
  }
  post->N = N1;
  post->n_pad = np1;
  post->m_tot = mt1;
  post->ld = ld;
  post->n_cap = n_cap;
  post->noise_kind = a.noise_kind;
  post->sigma2 = sigma2;
  if (a.logpdf_out) *a.logpdf_out = lp;
  return 0;
}

long spec_rows(const sgp_cov_spec* sp) {
  long n = 0;
  for (int i = 0; i < sp->n_row_blocks; ++i) n += (long)sp->row_len[i];
  return n;
}

}  // namespace

namespace sgp {

int drv_posterior_extend(sgp_post* post, const sgp_cov_spec* spec_all, const double* mean_all, int noise_kind,
                         const double* noise, const double* y_all, int64_t n_new, int64_t reserve_n, double* alpha_out,
                         double* logpdf_out) {
  CHECK_ARG(post && spec_all && noise && y_all, "sgp_posterior_extend: NULL argument");
  sgp_ctx* ctx = post->ctx;
  CHECK_ARG(drv_ctx_is_live(ctx, post->ctx_serial),
            "sgp_posterior_extend: the context this posterior was created on has been destroyed");
  CHECK_ARG(!post->mp && !ctx->multi,
            "sgp_posterior_extend: a posterior of a multi-GPU context (sharded factor) cannot be extended");
  CHECK_ARG(post->noise_kind != SGP_NOISE_DENSE,
            "sgp_posterior_extend: a posterior created with dense noise cannot be extended (its kept columns are not the spec's)");
  CHECK_ARG(noise_kind == SGP_NOISE_SCALAR || noise_kind == SGP_NOISE_DIAG,
            "sgp_posterior_extend: noise kind must be SCALAR or DIAG (dense noise is not supported)");
  CHECK_ARG(spec_all->symmetric && spec_all->n_row_blocks == spec_all->n_col_blocks,
            "sgp_posterior_extend: spec_all must be symmetric");
  CHECK_ARG(n_new >= 1, "sgp_posterior_extend: n_new must be at least 1");
  CHECK_ARG(spec_rows(spec_all) == post->N + n_new, "sgp_posterior_extend: spec_all does not have N + n_new points");
  CHECK_ARG(reserve_n == 0 || reserve_n >= post->N + n_new, "sgp_posterior_extend: reserve_n must be 0 or >= N + n_new");
  CHECK_ARG(noise_kind != SGP_NOISE_SCALAR || (post->noise_kind == SGP_NOISE_SCALAR && noise[0] == post->sigma2),
            "sgp_posterior_extend: a scalar noise must be the value the posterior was created with");
  const ExtendArgs a{post, spec_all, mean_all, noise, y_all, noise_kind, (long)n_new, (long)reserve_n, alpha_out, logpdf_out};
  return drv_with_df_fallback(ctx, [&]() { return extend_impl(a); });
}

int drv_extend_row_solve_ms(sgp_post* post, int64_t tile_rows, int schedule, int reps, double* ms_out) {
  CHECK_ARG(post && ms_out, "sgp_bench_extend_row_solve: NULL argument");
  sgp_ctx* ctx = post->ctx;
  CHECK_ARG(drv_ctx_is_live(ctx, post->ctx_serial),
            "sgp_bench_extend_row_solve: the context this posterior was created on has been destroyed");
  CHECK_ARG(!post->mp && !ctx->multi, "sgp_bench_extend_row_solve: not available for a sharded factor");
  CHECK_ARG(tile_rows >= 1 && tile_rows <= 64 && reps >= 1 && (schedule == 0 || schedule == 1),
            "sgp_bench_extend_row_solve: bad arguments");
  CtxScope scope(ctx);
  const long c0 = post->N / TILE * TILE, nrows = tile_rows * TILE;
  CHECK_ARG(c0 > 0, "sgp_bench_extend_row_solve: the posterior has no whole tile column");
  hipStream_t s = ctx->stream;
  DevBuf R, part;
  CHECK_RC(R.alloc((size_t)nrows * c0));
  CHECK_RC(part.alloc(schedule == 1 ? row_solve_scratch(nrows, c0) : 1));
  struct Ev {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Ev() {
      for (auto x : e)
        if (x) hipEventDestroy(x);
    }
  } ev;
  SGP_HIP(hipEventCreate(&ev.e[0]));
  SGP_HIP(hipEventCreate(&ev.e[1]));
  for (int r = 0; r < reps; ++r) {
    SGP_HIP(hipMemsetAsync(R.p, 0, sizeof(double) * nrows * c0, s));
    SGP_HIP(hipEventRecord(ev.e[0], s));
    CHECK_RC(row_solve(ctx, schedule, R.p, nrows, nrows, post->dA, post->ld, post->d_wall, c0, part.p, s));
    SGP_HIP(hipEventRecord(ev.e[1], s));
    SGP_HIP(hipEventSynchronize(ev.e[1]));
    float ms = 0;
    SGP_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    ms_out[r] = ms;
  }
  return 0;
}

}  // namespace sgp
