// Posterior mean and variance at test points with their gradients with respect to those points
// (include/sthenomi_predgrad.h), against the kept factor.
//
//   V (and C'), mean, var                  the solved cross rows and what is read off them: kept.h, shared with predict --
//                                          the same bits (the sparse posterior: V = B' against Lz, C' = B' Le^-T)
//   alpha <- L^-T z                        the single-vector back substitution (sparse: against Le, then Lz)
//   B     <- V L^-1                        row_backsolve below (sparse: B = (B' - C' Le^-1) Lz^-1)
//   d mean_i / d x*_i = sum_j alpha_j coef rs_i cs_j kappa'(d2_ij) 2 (xr_i - xc_j),  d var_i / d x*_i: alpha_j -> -2 B_ij
//                                          predgrad_kernel + predgrad_reduce_kernel, one launch pair per term of a block pair
//   the k**_ii part of d var_i / d x*_i    launch_diag_grad_inputs with w = 1
// Nothing is factored; every launch is ordered on the context's stream; no kernel waits on another workgroup and none uses
// atomics: every output element has one writer and sums its addends in an order the shapes alone decide.
#include "kept.h"
#include "kern_grad.h"
#include "potrf_diag.h"
#include "../../include/sthenomi_predgrad.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace sgp;

namespace {

constexpr long NOMASK = -(1L << 40);   // launch_gemm_nt's mask_off: every tile
constexpr int CHUNK = SGP_PREDGRAD_COL_CHUNK;
static_assert(CHUNK % TILE == 0 && CHUNK <= 512, "a chunk is whole 128-column tiles, at most 512 columns");

// ---------------------------------------------------------------------------------------
// (a) R <- R L^-1 for nrows (multiple of 128) rows against an n_pad x n_pad lower factor with its kept inverse blocks
// ---------------------------------------------------------------------------------------
// The 128-column diagonal step X <- X inv(L_cc), modelled on the panel solve (panel_solve.h) and the single-vector
// backsolve_diag_kernel (capi.hip): blocked substitution over the eight 16-column sub-blocks, 7 -> 0,
//   T_c = B_c - sum_{p > c} X_p L_pc,   X_c = T_c W_c + (T_c - (T_c W_c) L_cc) W_c,   W_c = the kept inv(L_cc)
// -- the inverse product plus one refinement step against L_cc itself (an inverse product alone is not backward stable on
// these matrices: capi.hip, solve_rows).  One workgroup owns RB_ROWS rows; thread (r, m) owns column m of the current
// sub-block of row r and forms its sums over k in ascending order.  The 36 lower 16x16 blocks of L_cc sit in LDS as
// [k][m] (L[16 p + k][16 c + m] at (p (p + 1) / 2 + c) * 256 + 16 k + m: the threads of a row read consecutive words), the
// inverse blocks likewise, the rows with a padded stride (the four rows of a wave on different banks).
constexpr int RB_ROWS = 16;
constexpr int RB_XLD = TILE + 1;
constexpr size_t RB_LDS = (size_t)(36 * 256 + 8 * 256 + RB_ROWS * RB_XLD + 3 * RB_ROWS * 16) * sizeof(double);

__global__ __launch_bounds__(256) void row_backsolve_diag_kernel(double* X, long ldx, long nrows, const double* L, long ldl,
                                                                const double* inv) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* sL = smem;                      // 36 blocks
  double* sW = sL + 36 * 256;             // 8 inverse blocks, [k][m], lower (k >= m)
  double* xs = sW + 8 * 256;              // RB_ROWS x 128 (stride RB_XLD)
  double* ts = xs + RB_ROWS * RB_XLD;     // RB_ROWS x 16 each
  double* x1s = ts + RB_ROWS * 16;
  double* rs = x1s + RB_ROWS * 16;
  const int t = threadIdx.x;
  const long row0 = (long)blockIdx.x * RB_ROWS;
  for (int idx = t; idx < 36 * 256; idx += 256) {
    const int blk = idx >> 8, e = idx & 255, k = e & 15, m = e >> 4;
    int p, c;
    block_rc(blk, p, c);
    double v = L[(16 * p + k) + (long)(16 * c + m) * ldl];
    if (p == c && k < m) v = 0.0;   // (the strict upper triangle of a diagonal block is not part of the factor)
    sL[blk * 256 + k * 16 + m] = v;
  }
  for (int idx = t; idx < 8 * 256; idx += 256) {
    const int c = idx >> 8, e = idx & 255, k = e & 15, m = e >> 4;
    sW[c * 256 + k * 16 + m] = k >= m ? inv[c * 256 + m * 16 + k] : 0.0;   // inv(L_cc)[k][m] at + 16 m + k
  }
  for (int idx = t; idx < RB_ROWS * TILE; idx += 256) {
    const int r = idx & (RB_ROWS - 1), j = idx >> 4;
    xs[r * RB_XLD + j] = (row0 + r < nrows) ? X[(row0 + r) + (long)j * ldx] : 0.0;
  }
  __syncthreads();
  const int r = t >> 4, m = t & 15;
  const double* xrow = xs + r * RB_XLD;
  for (int c = 7; c >= 0; --c) {
    double acc = 0.0;
    for (int p = c + 1; p < 8; ++p) {
      const double* Lpc = sL + (p * (p + 1) / 2 + c) * 256 + m;
#pragma unroll
      for (int k = 0; k < 16; ++k) acc = fma(xrow[16 * p + k], Lpc[k * 16], acc);
    }
    const double tv = xrow[16 * c + m] - acc;
    ts[r * 16 + m] = tv;
    __syncthreads();
    const double* Wc = sW + c * 256 + m;
    const double* Lcc = sL + (c * (c + 1) / 2 + c) * 256 + m;
    double x1 = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) x1 = fma(ts[r * 16 + k], Wc[k * 16], x1);
    x1s[r * 16 + m] = x1;
    __syncthreads();
    double rr = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) rr = fma(x1s[r * 16 + k], Lcc[k * 16], rr);
    rs[r * 16 + m] = tv - rr;   // T - X1 L_cc
    __syncthreads();
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) d = fma(rs[r * 16 + k], Wc[k * 16], d);
    xs[r * RB_XLD + 16 * c + m] = x1 + d;
    __syncthreads();
  }
  for (int idx = t; idx < RB_ROWS * TILE; idx += 256) {
    const int rr = idx & (RB_ROWS - 1), j = idx >> 4;
    if (row0 + rr < nrows) X[(row0 + rr) + (long)j * ldx] = xs[rr * RB_XLD + j];
  }
}

int launch_row_backsolve_diag(double* X, long ldx, long nrows, const double* Lcc, long ldl, const double* inv, hipStream_t s) {
  if (nrows <= 0) return 0;
  SGP_LDS_ATTR_ONCE(row_backsolve_diag_kernel, RB_LDS);
  hipLaunchKernelGGL(row_backsolve_diag_kernel, dim3((unsigned)((nrows + RB_ROWS - 1) / RB_ROWS)), dim3(256), RB_LDS, s, X, ldx,
                     nrows, Lcc, ldl, inv);
  SGP_HIP(hipGetLastError());
  return 0;
}

// Blocked right to left, mirroring the forward row solve (capi.hip: row_trsm): a 512-column block first receives everything to
// its right in ONE deep product, then is solved in place in 128-column steps with K = 128 updates of the block's columns to
// their left.  The product kernel forms A B' only and the operand here is L[k, c] untransposed, so the block's column panel
// (rows c0 .. n_pad) is copied transposed into `scratch` (wb x (n_pad - c0) doubles, ld = wb) first: n_pad^2 / 2 elements per
// call against nrows n_pad^2 flops.  Only the tiles on and below the diagonal of the factor are used.
int row_backsolve(double* R, long ldr, long nrows, const double* L, long ldl, const double* d_invall, long n_pad,
                  double* scratch, hipStream_t s) {
  const long WB = 4 * TILE, stride = drv_invd_stride();
  for (long c0 = (n_pad - 1) / WB * WB; c0 >= 0; c0 -= WB) {
    const long wb = std::min(WB, n_pad - c0), right = n_pad - c0 - wb;
    // LT[a + b * wb] = L[c0 + b, c0 + a]
    CHECK_RC(launch_transpose_add(L + c0 + c0 * ldl, ldl, n_pad - c0, wb, scratch, wb, nullptr, s));
    // (leading dimensions beyond ~64k rows: 512-column slices of the contraction, as row_trsm)
    const long KC = (ldr > 65536 || right == 0) ? WB : right;
    for (long k0 = 0; k0 < right; k0 += KC)
      CHECK_RC(launch_gemm_nt(R + (c0 + wb + k0) * ldr, ldr, scratch + (wb + k0) * wb, wb, R + c0 * ldr, ldr, nrows, wb,
                              std::min(KC, right - k0), -1.0, 1.0, NOMASK, 0, 0, s));
    for (long c = c0 + wb - TILE; c >= c0; c -= TILE) {
      CHECK_RC(launch_row_backsolve_diag(R + c * ldr, ldr, nrows, L + c + c * ldl, ldl, d_invall + (c / TILE) * stride, s));
      if (c > c0)
        CHECK_RC(launch_gemm_nt(R + c * ldr, ldr, scratch + (c - c0) * wb, wb, R + c0 * ldr, ldr, nrows, c - c0, TILE, -1.0, 1.0,
                                NOMASK, 0, 0, s));
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// (b) the prediction-gradient contraction of ONE term over one block pair
// ---------------------------------------------------------------------------------------
// Grid: (128-row tiles of the pair) x (chunks of CHUNK columns).  A workgroup walks its chunk in 128-column tiles staged in
// LDS (column points, cs, alpha), thread = one row x 64 columns as grad_inputs_kernel; kappa' is evaluated once per pair and
// feeds both accumulators: alpha_j for the mean, -2 B_ij for the variance (B read along i: coalesced).  The two column halves
// are combined in fixed order and ONE partial of 2 D sums per (row, chunk) is written:
//   part[((chunk * nr + row) * 2 + which) * D + d],  which = 0 mean, 1 variance
// Rows beyond nr and columns beyond nc contribute nothing.  Bm / alpha may be NULL (that accumulator stays 0).
template <int DMAX>
__global__ __launch_bounds__(256) void predgrad_kernel(const double* Bm, long ldb, const double* alpha, long r0, long nr, long c0,
                                                       long nc, DevTerm T, double* part) {
  __shared__ double sx[TILE * DMAX];
  __shared__ double scs[TILE], sal[TILE];
  __shared__ double comb[TILE * 2 * DMAX];
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  const long lrow = (long)blockIdx.x * TILE + trow;
  const bool live = lrow < nr;
  const long grow = r0 + lrow;
  const long cbeg = (long)blockIdx.y * CHUNK, cend = min(nc, cbeg + (long)CHUNK);
  double xr[DMAX], am[DMAX], av[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    xr[d] = (live && d < T.dim) ? T.xr[lrow * T.ldr + d] : 0.0;
    am[d] = av[d] = 0.0;
  }
  const double wrow = live ? 2.0 * T.coef * (T.rs ? T.rs[lrow] : 1.0) : 0.0;
  for (long ct = cbeg; ct < cend; ct += TILE) {
    __syncthreads();
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long lc = ct + p;
      sx[idx] = (lc < cend && d < T.dim) ? T.xc[lc * T.ldc + d] : 0.0;
    }
    if (t < TILE) {
      const long lc = ct + t;
      scs[t] = (lc < cend) ? (T.cs ? T.cs[lc] : 1.0) : 0.0;   // 0 kills the padding columns
      sal[t] = (lc < cend && alpha) ? alpha[c0 + lc] : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int p = th * 64; p < th * 64 + 64; ++p) {
        const long lc = ct + p;
        if (lc >= cend) break;
        double df[DMAX], d2 = 0.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          df[d] = xr[d] - sx[p * DMAX + d];
          d2 = fma(df[d], df[d], d2);
        }
        double k, kx;
        kern_val_dd2(T.kind, d2, T.param, k, kx);
        const double base = wrow * scs[p] * kx;
        const double wm = base * sal[p];
        const double wv = Bm ? -2.0 * Bm[grow + (c0 + lc) * ldb] * base : 0.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          am[d] = fma(wm, df[d], am[d]);
          av[d] = fma(wv, df[d], av[d]);
        }
      }
    }
  }
  __syncthreads();
  if (th == 1) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      comb[(trow * 2 + 0) * DMAX + d] = am[d];
      comb[(trow * 2 + 1) * DMAX + d] = av[d];
    }
  }
  __syncthreads();
  if (th == 0 && live) {
    double* o = part + (((long)blockIdx.y * nr + lrow) * 2) * T.dim;
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
      if (d < T.dim) {
        o[d] = am[d] + comb[(trow * 2 + 0) * DMAX + d];
        o[T.dim + d] = av[d] + comb[(trow * 2 + 1) * DMAX + d];
      }
  }
}

// Any input dimension (> 16): the dimension walked in chunks of 16, twice per 128-column tile as grad_inputs_bigd_kernel --
// pass 1 forms the 64 squared distances of a thread's row and turns them into base_j = 2 coef rs_i cs_j kappa'(d2_ij); pass 2
// forms sum_j base_j alpha_j (x_i - x'_j)[d] and sum_j -2 B_ij base_j (x_i - x'_j)[d] chunk by chunk and adds them into the
// workgroup's own partial (the first tile of the chunk writes it).
constexpr int PBD = 16;
__global__ __launch_bounds__(256) void predgrad_bigd_kernel(const double* Bm, long ldb, const double* alpha, long r0, long nr,
                                                            long c0, long nc, DevTerm T, double* part) {
  __shared__ __attribute__((aligned(16))) double sx[TILE * PBD];
  __shared__ double scs[TILE], sal[TILE];
  __shared__ double comb[TILE * 2 * PBD];
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  const long lrow = (long)blockIdx.x * TILE + trow;
  const bool live = lrow < nr;
  const long grow = r0 + lrow;
  const int D = T.dim;
  const long cbeg = (long)blockIdx.y * CHUNK, cend = min(nc, cbeg + (long)CHUNK);
  const double wrow = live ? 2.0 * T.coef * (T.rs ? T.rs[lrow] : 1.0) : 0.0;
  double* o = part + (((long)blockIdx.y * nr + (live ? lrow : 0)) * 2) * D;
  for (long ct = cbeg; ct < cend; ct += TILE) {
    double w[64];
#pragma unroll
    for (int q = 0; q < 64; ++q) w[q] = 0.0;
    // ---- pass 1: squared distances
    for (int d0 = 0; d0 < D; d0 += PBD) {
      __syncthreads();
      for (int idx = t; idx < TILE * PBD; idx += 256) {
        const int p = idx / PBD, d = idx % PBD;
        const long lc = ct + p;
        sx[idx] = (lc < cend && d0 + d < D) ? T.xc[lc * T.ldc + d0 + d] : 0.0;
      }
      if (d0 == 0 && t < TILE) {
        const long lc = ct + t;
        scs[t] = (lc < cend) ? (T.cs ? T.cs[lc] : 1.0) : 0.0;
        sal[t] = (lc < cend && alpha) ? alpha[c0 + lc] : 0.0;
      }
      __syncthreads();
      if (live) {
        double xi[PBD];
#pragma unroll
        for (int d = 0; d < PBD; ++d) xi[d] = (d0 + d < D) ? T.xr[lrow * T.ldr + d0 + d] : 0.0;
#pragma unroll
        for (int q = 0; q < 64; ++q) {
          const double* sp = &sx[(th * 64 + q) * PBD];
          double s = 0.0;
#pragma unroll
          for (int d = 0; d < PBD; ++d) {
            const double df = xi[d] - sp[d];
            s = fma(df, df, s);
          }
          w[q] += s;
        }
      }
    }
    // ---- base weights (0 for the padding columns)
#pragma unroll
    for (int q = 0; q < 64; ++q) {
      const int p = th * 64 + q;
      double k, kx;
      kern_val_dd2(T.kind, w[q], T.param, k, kx);
      w[q] = (live && ct + p < cend) ? wrow * scs[p] * kx : 0.0;
    }
    // ---- pass 2
    for (int d0 = 0; d0 < D; d0 += PBD) {
      __syncthreads();
      for (int idx = t; idx < TILE * PBD; idx += 256) {
        const int p = idx / PBD, d = idx % PBD;
        const long lc = ct + p;
        sx[idx] = (lc < cend && d0 + d < D) ? T.xc[lc * T.ldc + d0 + d] : 0.0;
      }
      __syncthreads();
      double pm[PBD], pv[PBD];
#pragma unroll
      for (int d = 0; d < PBD; ++d) pm[d] = pv[d] = 0.0;
      if (live) {
        double xi[PBD];
#pragma unroll
        for (int d = 0; d < PBD; ++d) xi[d] = (d0 + d < D) ? T.xr[lrow * T.ldr + d0 + d] : 0.0;
#pragma unroll
        for (int q = 0; q < 64; ++q) {
          const int p = th * 64 + q;
          const long lc = ct + p;
          const double* sp = &sx[p * PBD];
          const double wm = w[q] * sal[p];
          const double wv = (Bm && lc < cend) ? -2.0 * Bm[grow + (c0 + lc) * ldb] * w[q] : 0.0;
#pragma unroll
          for (int d = 0; d < PBD; ++d) {
            const double df = xi[d] - sp[d];
            pm[d] = fma(wm, df, pm[d]);
            pv[d] = fma(wv, df, pv[d]);
          }
        }
      }
      if (th == 1) {
#pragma unroll
        for (int d = 0; d < PBD; ++d) {
          comb[(trow * 2 + 0) * PBD + d] = pm[d];
          comb[(trow * 2 + 1) * PBD + d] = pv[d];
        }
      }
      __syncthreads();
      if (th == 0 && live) {
#pragma unroll
        for (int d = 0; d < PBD; ++d)
          if (d0 + d < D) {
            const double sm = pm[d] + comb[(trow * 2 + 0) * PBD + d], sv = pv[d] + comb[(trow * 2 + 1) * PBD + d];
            o[d0 + d] = ct == cbeg ? sm : o[d0 + d] + sm;
            o[D + d0 + d] = ct == cbeg ? sv : o[D + d0 + d] + sv;
          }
      }
    }
  }
}

// out[which][row * D + d] += sum over the chunks, ascending, of the partials: one thread per (row, d)
__global__ void predgrad_reduce_kernel(const double* part, long nr, int D, long nchunk, double* gm, double* gv) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nr * D) return;
  const long row = idx / D;
  const int d = (int)(idx % D);
  double sm = 0.0, sv = 0.0;
  for (long ch = 0; ch < nchunk; ++ch) {
    const double* p = part + ((ch * nr + row) * 2) * D;
    sm += p[d];
    sv += p[D + d];
  }
  if (gm) gm[idx] += sm;
  if (gv) gv[idx] += sv;
}

long predgrad_partials(long nr, long nc, int D) { return ((nc + CHUNK - 1) / CHUNK) * nr * 2 * D; }

// Bm: element (row r0 + i, column c0 + j) at Bm[(r0 + i) + (c0 + j) * ldb]; gm / gv: the row input's gradients (dim x nr)
int launch_predgrad(const double* Bm, long ldb, const double* alpha, long r0, long nr, long c0, long nc, const DevTerm& T,
                    double* part, double* gm, double* gv, hipStream_t s) {
  if (nr <= 0 || nc <= 0 || T.dim <= 0 || (!gm && !gv)) return 0;
  const long nchunk = (nc + CHUNK - 1) / CHUNK;
  dim3 grid((unsigned)((nr + TILE - 1) / TILE), (unsigned)nchunk), block(256);
#define SGP_PG(DM) hipLaunchKernelGGL((predgrad_kernel<DM>), grid, block, 0, s, Bm, ldb, alpha, r0, nr, c0, nc, T, part)
  if (T.dim <= 1) SGP_PG(1);
  else if (T.dim <= 2) SGP_PG(2);
  else if (T.dim <= 4) SGP_PG(4);
  else if (T.dim <= 8) SGP_PG(8);
  else if (T.dim <= 16) SGP_PG(16);
  else
    hipLaunchKernelGGL(predgrad_bigd_kernel, grid, block, 0, s, Bm, ldb, alpha, r0, nr, c0, nc, T, part);
#undef SGP_PG
  SGP_HIP(hipGetLastError());
  const long tot = nr * T.dim;
  hipLaunchKernelGGL(predgrad_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part, nr, T.dim, nchunk, gm, gv);
  SGP_HIP(hipGetLastError());
  return 0;
}

__global__ void fill_ones_kernel(double* p, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 1.0;
}

struct PgArgs {
  const char* who;
  const sgp_cov_spec *cross, *prior_ss;
  const double* mean_s;
  double *mean_out, *var_out;
  double* const* g_mean;
  double* const* g_var;
  double* const* g_prior;
};

bool any_asked(double* const* g, int n) {
  for (int k = 0; g && k < n; ++k)
    if (g[k]) return true;
  return false;
}

int fetch_inputs(const sgp_cov_spec* sp, const std::vector<DevBuf>& d, const std::vector<char>& written, double* const* out) {
  for (int k = 0; out && k < sp->n_inputs; ++k) {
    const sgp_input& in = sp->inputs[k];
    if (!out[k] || !written[k] || in.n == 0 || in.dim == 0) continue;
    SGP_HIP(hipMemcpy(out[k], d[k].p, sizeof(double) * in.dim * in.n, hipMemcpyDeviceToHost));
  }
  return 0;
}

int predgrad_impl(sgp_ctx* ctx, PostRef post, const PgArgs& a) {
  CtxScope scope(ctx);
  const Kept k = post.kept();
  SpecGuard gc, gp;
  CHECK_RC(drv_dspec_create(ctx, a.cross, &gc.ds));
  if (a.prior_ss) CHECK_RC(drv_dspec_create(ctx, a.prior_ss, &gp.ds));
  const sgp_dspec *dc = gc.ds, *dp = gp.ds;
  const long Ns = dc->N;
  REFUSE_UNLESS(dc->M == k.n, a.who, "the columns of the cross spec are not the points the posterior was conditioned on (sizes do not match)");
  REFUSE_UNLESS(!dp || (dp->N == Ns && dp->M == Ns && dp->nrb == dp->ncb), a.who,
                "prior_ss must be the spec of the N* test points of the cross spec (sizes do not match)");
  const bool want_gm = any_asked(a.g_mean, a.cross->n_inputs), want_gv = any_asked(a.g_var, a.cross->n_inputs);
  const bool want_gp = dp && any_asked(a.g_prior, a.prior_ss->n_inputs);
  if (Ns == 0) return 0;
  const long ns_pad = (Ns + TILE - 1) / TILE * TILE, n_pad = k.n_pad;
  hipStream_t s = ctx->stream;

  // ---- V (and C'), mean and variance
  CrossRows R;
  CHECK_RC(R.solve(ctx, k, CrossSource{dc, nullptr, 0, Ns, a.mean_s}, ns_pad, s));
  if (a.mean_out) CHECK_RC(R.mean(k, s));
  if (a.var_out) CHECK_RC(R.variance(ctx, k, dp, nullptr, s));

  // ---- alpha and B
  DevBuf dz, dal, dscr, dpart;
  const double* d_alpha = nullptr;
  std::vector<DevBuf> dgm(a.cross->n_inputs), dgv(a.cross->n_inputs), dgp(want_gp ? a.prior_ss->n_inputs : 0);
  std::vector<char> row_read(a.cross->n_inputs, 0), prior_all(want_gp ? a.prior_ss->n_inputs : 0, 1);
  if (want_gm) {
    CHECK_RC(dz.alloc(n_pad));
    CHECK_RC(dal.alloc(n_pad));
    CHECK_RC(drv_copy_strided(k.z, k.ldz, n_pad, dz.p, s));
    SGP_HIP(hipMemsetAsync(dal.p, 0, sizeof(double) * n_pad, s));
    if (k.L2) {   // alpha = Lz^-T (Le^-T u): the second substitution reads the first one's result and writes over u
      CHECK_RC(drv_back_substitute(k.L2, k.ld2, k.w2, n_pad - TILE, 0, n_pad, dz.p, dal.p, s));
      CHECK_RC(drv_back_substitute(k.L1, k.ld1, k.w1, n_pad - TILE, 0, n_pad, dal.p, dz.p, s));
      d_alpha = dz.p;
    } else {
      CHECK_RC(drv_back_substitute(k.L1, k.ld1, k.w1, n_pad - TILE, 0, n_pad, dz.p, dal.p, s));
      d_alpha = dal.p;
    }
  }
  if (want_gv) {
    CHECK_RC(dscr.alloc((size_t)std::min<long>(4 * TILE, n_pad) * n_pad));
    if (k.L2) {   // B = (B' - C' Le^-1) Lz^-1
      CHECK_RC(row_backsolve(R.V2.p, ns_pad, ns_pad, k.L2, k.ld2, k.w2, n_pad, dscr.p, s));
      CHECK_RC(drv_axpy_block(R.V.p, ns_pad, R.V2.p, ns_pad, ns_pad, n_pad, -1.0, s));
    }
    CHECK_RC(row_backsolve(R.V.p, ns_pad, ns_pad, k.L1, k.ld1, k.w1, n_pad, dscr.p, s));
  }

  // ---- the contraction, term by term
  if (want_gm || want_gv) {
    long pmax = 1;
    for (int I = 0; I < dc->nrb; ++I)
      for (int J = 0; J < dc->ncb; ++J)
        for (int t = dc->term_ptr[I * dc->ncb + J]; t < dc->term_ptr[I * dc->ncb + J + 1]; ++t) {
          row_read[dc->term_row_input[t]] = 1;
          pmax = std::max(pmax, predgrad_partials(dc->row_len[I], dc->col_len[J], dc->h_terms[t].dim));
        }
    CHECK_RC(dpart.alloc((size_t)pmax));
    for (int kx = 0; kx < a.cross->n_inputs; ++kx) {
      if (!row_read[kx]) continue;
      const size_t cnt = (size_t)std::max<long>(1, (long)dc->in_dim[kx] * dc->in_n[kx]);
      if (want_gm) {
        CHECK_RC(dgm[kx].alloc(cnt));
        SGP_HIP(hipMemsetAsync(dgm[kx].p, 0, sizeof(double) * cnt, s));
      }
      if (want_gv) {
        CHECK_RC(dgv[kx].alloc(cnt));
        SGP_HIP(hipMemsetAsync(dgv[kx].p, 0, sizeof(double) * cnt, s));
      }
    }
    for (int I = 0; I < dc->nrb; ++I)
      for (int J = 0; J < dc->ncb; ++J) {
        if (dc->row_len[I] == 0 || dc->col_len[J] == 0) continue;
        const int p = I * dc->ncb + J;
        for (int t = dc->term_ptr[p]; t < dc->term_ptr[p + 1]; ++t) {
          const int kin = dc->term_row_input[t];
          CHECK_RC(launch_predgrad(want_gv ? R.V.p : nullptr, ns_pad, d_alpha, dc->row_off[I], dc->row_len[I],
                                   dc->col_off[J], dc->col_len[J], dc->h_terms[t], dpart.p, want_gm ? dgm[kin].p : nullptr,
                                   want_gv ? dgv[kin].p : nullptr, s));
        }
      }
  }

  // ---- the k**_ii part: sgp_kernelmatrix_diag_grad_x of prior_ss for w = 1
  DevBuf dw;
  if (want_gp) {
    CHECK_RC(dw.alloc(Ns));
    hipLaunchKernelGGL(fill_ones_kernel, dim3((unsigned)((Ns + 255) / 256)), dim3(256), 0, s, dw.p, Ns);
    SGP_HIP(hipGetLastError());
    for (int kx = 0; kx < a.prior_ss->n_inputs; ++kx) {
      const size_t cnt = (size_t)std::max<long>(1, (long)dp->in_dim[kx] * dp->in_n[kx]);
      CHECK_RC(dgp[kx].alloc(cnt));
      SGP_HIP(hipMemsetAsync(dgp[kx].p, 0, sizeof(double) * cnt, s));
    }
    for (int I = 0; I < dp->nrb; ++I) {
      REFUSE_UNLESS(dp->row_len[I] == dp->col_len[I], a.who, "prior_ss: the block lengths of rows and columns differ (sizes do not match)");
      if (dp->row_len[I] == 0) continue;
      const int p = I * dp->ncb + I;
      for (int t = dp->term_ptr[p]; t < dp->term_ptr[p + 1]; ++t)
        CHECK_RC(launch_diag_grad_inputs(dw.p + dp->row_off[I], dp->row_len[I], dp->h_terms[t], dgp[dp->term_row_input[t]].p,
                                         dgp[dp->term_col_input[t]].p, s));
    }
  }

  SGP_HIP(hipStreamSynchronize(s));
  if (a.mean_out) SGP_HIP(hipMemcpy(a.mean_out, R.mu.p, sizeof(double) * Ns, hipMemcpyDeviceToHost));
  if (a.var_out) SGP_HIP(hipMemcpy(a.var_out, R.var.p, sizeof(double) * Ns, hipMemcpyDeviceToHost));
  if (want_gm) CHECK_RC(fetch_inputs(a.cross, dgm, row_read, a.g_mean));
  if (want_gv) CHECK_RC(fetch_inputs(a.cross, dgv, row_read, a.g_var));
  if (want_gp) CHECK_RC(fetch_inputs(a.prior_ss, dgp, prior_all, a.g_prior));
  return 0;
}

// the door of every entry point (kept.h), then what it refuses of its own
int enter(PostRef post, const PgArgs& a, const char* multi_refusal) {
  CHECK_RC(kept_door(post, a.cross, a.who, multi_refusal));
  sgp_ctx* ctx = post.ctx();
  for (const sgp_cov_spec* sp : {a.cross, a.prior_ss}) {
    if (!sp) continue;
    REFUSE_UNLESS(!spec_has_deriv(sp), a.who, "gradients through derivative terms are not supported");
    REFUSE_UNLESS(!spec_has_stencil(ctx, sp), a.who, "gradients through stencil terms are not supported");
    REFUSE_UNLESS(!spec_has_patch(sp), a.who, "gradients through patch (convolutional) terms are not supported");
    REFUSE_UNLESS(!spec_has_kprod(sp), a.who,
                  "gradients through product chains and the kinds beyond the six plain ones are not supported");
  }
  REFUSE_UNLESS(a.prior_ss || (!a.var_out && !a.g_var && !a.g_prior), a.who, "prior_ss is required for the variance and its gradients");
  return predgrad_impl(ctx, post, a);
}

}  // namespace

namespace sgp {

int drv_posterior_predict_grad_x(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                                 double* mean_out, double* var_out, double* const* grad_mean_inputs,
                                 double* const* grad_var_inputs, double* const* grad_var_prior_inputs) {
  const PgArgs a{"sgp_posterior_predict_grad_x", cross, prior_ss, mean_s, mean_out, var_out, grad_mean_inputs, grad_var_inputs,
                 grad_var_prior_inputs};
  return enter(post, a, "a posterior of a multi-GPU context (sharded factor) has no prediction gradient on the device");
}

int drv_sparse_posterior_predict_grad_x(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                        const double* mean_s, double* mean_out, double* var_out,
                                        double* const* grad_mean_inputs, double* const* grad_var_inputs,
                                        double* const* grad_var_prior_inputs) {
  const PgArgs a{"sgp_sparse_posterior_predict_grad_x", cross, prior_ss, mean_s, mean_out, var_out, grad_mean_inputs,
                 grad_var_inputs, grad_var_prior_inputs};
  return enter(post, a, "a posterior of a multi-GPU context has no prediction gradient on the device");
}

}  // namespace sgp
