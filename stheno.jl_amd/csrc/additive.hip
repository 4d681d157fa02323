// Additive terms (include/sthenomi.h: SGP_ADDITIVE_*): the additive kernel of Duvenaud, Nickisch and Rasmussen,
//   K_ij = coef rs_i cs_j e_r(z_0 .. z_{D-1}),   z_d = kappa_base((x_d - y_d)^2),
// e_r the elementary symmetric polynomial of order r = param of the D one-dimensional base kernels (additive_eval.h: the
// formulas and the recurrence; additive_kinds.h: the validation table).  Per-entry arithmetic: D exponentials and D R fmas,
// no contraction for the matrix pipes.
//
// A term class of its own, as the derivative and Gibbs kinds are.  The terms of one block pair that share kind, points and
// scale vectors form a GROUP (additive_kinds.h: additive_group) and differ in (coef, r) alone: a launch carries one group, the
// recurrence runs ONCE per point pair to the group's largest order R, in a table of RMAX + 1 registers per pair (RMAX in
// {2, 4, 8}, the order class), and the term loop picks e_{r_t} over wave-uniform scalars.  A model with orders 1 .. R costs D
// exponentials per entry, not one evaluation per order.
//
// Tiling of the matrix kernel: the assembly frame's two-row form (asm_frame.h) -- 128 x 128 tiles of the global grid, one
// 256-thread workgroup per tile, thread (lane, wave) owns rows 2 lane, 2 lane + 1 and the 32 columns of quarter `wave`, 16-byte
// stores on interior tiles.  LDS, staged once per tile, D the points' dimension (no padding: the coordinate loop is a run-time
// loop over LDS, the registers hold the tables):
//   [128][D] column points | [D][128] row points | rs | cs     (128 doubles each)
// A pass covers CC columns x 2 rows: CC = 4 (8 tables of 3 or 5 doubles) at RMAX = 2 and 4, CC = 2 (4 tables of 9) at RMAX = 8.
#include "additive_eval.h"
#include "additive_kinds.h"
#include "asm_frame.h"
#include <algorithm>

namespace sgp {

__host__ __device__ constexpr int additive_lds_doubles(int D) { return 2 * TILE * D + 2 * TILE; }
__host__ __device__ constexpr int additive_cc(int rmax) { return rmax == 8 ? 2 : 4; }

// the tile's points and scale vectors.  Outside the clip: point 0, scale 0
__device__ __forceinline__ void additive_stage(double* smem, const DevTerm& T, long gtr, long gtc, long r0, long c0,
                                               const TileClip& cl, int t) {
  const int D = T.dim;
  double* sc = smem;
  double* sr = sc + TILE * D;
  double* ss = sr + TILE * D;   // rs | cs
  for (int idx = t; idx < TILE * D; idx += 256) {
    const int p = idx / D, d = idx % D;
    const long gc = gtc * TILE + p, gr = gtr * TILE + p;
    sc[idx] = (gc >= cl.cbeg && gc < cl.cend) ? T.xc[(gc - c0) * T.ldc + d] : 0.0;
    sr[d * TILE + p] = (gr >= cl.rbeg && gr < cl.rend) ? T.xr[(gr - r0) * T.ldr + d] : 0.0;
  }
  if (t < TILE) {
    const long gr = gtr * TILE + t;
    ss[t] = (gr >= cl.rbeg && gr < cl.rend) ? (T.rs ? T.rs[gr - r0] : 1.0) : 0.0;
  } else {
    const int p = t - TILE;
    const long gc = gtc * TILE + p;
    ss[TILE + p] = (gc >= cl.cbeg && gc < cl.cend) ? (T.cs ? T.cs[gc - c0] : 1.0) : 0.0;
  }
}

template <int BASE, int RMAX>
__global__ __launch_bounds__(256) void assemble_additive_kernel(
    double* __restrict__ K, long ld, long r0, long nr, long c0, long nc, const DevTerm* __restrict__ terms, int nterms,
    int lower_only, int accumulate, int noise_kind, double sigma2, const double* __restrict__ noise_diag, long tile_r_first,
    long tile_c_first) {
  constexpr int CC = additive_cc(RMAX);
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  if (lower_only && gtr < gtc) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;

  TileClip cl;
  if (!tile_clip(gtr, gtc, r0, nr, c0, nc, cl)) return;   // uniform over the workgroup

  const int D = terms[0].dim;
  const double* sc = smem;
  const double* sr = sc + TILE * D;
  const double* ss = sr + TILE * D;
  additive_stage(smem, terms[0], gtr, gtc, r0, c0, cl, t);
  __syncthreads();

  const PairRows R = pair_rows(K, ld, gtr, gtc, lane, cl, accumulate, noise_kind, sigma2, noise_diag);
  const double2 rs = *reinterpret_cast<const double2*>(ss + 2 * lane);

  for (int jc = 0; jc < 32; jc += CC) {
    const int pbase = wv * 32 + jc;
    // the tables of the pass's 2 CC pairs: arrays of their own, so that each one lives in registers (a at row 2 lane, b at
    // row 2 lane + 1; 0 .. 3 the column of the pass)
    double a0[RMAX + 1], a1[RMAX + 1], a2[RMAX + 1], a3[RMAX + 1], b0[RMAX + 1], b1[RMAX + 1], b2[RMAX + 1], b3[RMAX + 1];
    esp_init<RMAX>(a0), esp_init<RMAX>(a1), esp_init<RMAX>(b0), esp_init<RMAX>(b1);
    if (CC == 4) esp_init<RMAX>(a2), esp_init<RMAX>(a3), esp_init<RMAX>(b2), esp_init<RMAX>(b3);
    const double* yp = sc + pbase * D;
    // once per point pair: D base kernels, D RMAX fmas; 2 CC independent chains per coordinate
    for (int d = 0; d < D; ++d) {
      const double2 x2 = *reinterpret_cast<const double2*>(sr + d * TILE + 2 * lane);
#define SGP_ADD_COL(q, ea, eb)                         \
  {                                                    \
    const double y = yp[(q) * D + d];                  \
    esp_step<RMAX>(ea, additive_z<BASE>(x2.x - y));    \
    esp_step<RMAX>(eb, additive_z<BASE>(x2.y - y));    \
  }
      SGP_ADD_COL(0, a0, b0)
      SGP_ADD_COL(1, a1, b1)
      if (CC == 4) {
        SGP_ADD_COL(2, a2, b2)
        SGP_ADD_COL(3, a3, b3)
      }
#undef SGP_ADD_COL
    }
    double acc0[CC], acc1[CC];
#pragma unroll
    for (int q = 0; q < CC; ++q) acc0[q] = acc1[q] = 0.0;
    for (int tm = 0; tm < nterms; ++tm) {   // (coef, r): wave-uniform scalars
      const double coef = terms[tm].coef;
      const int r = (int)terms[tm].param;
      const double w0 = coef * rs.x, w1 = coef * rs.y;
#define SGP_ADD_TERM(q, ea, eb)                                          \
  {                                                                      \
    const double cq = ss[TILE + pbase + (q)];                            \
    acc0[q] = fma(esp_pick<RMAX>(ea, r), w0 * cq, acc0[q]);              \
    acc1[q] = fma(esp_pick<RMAX>(eb, r), w1 * cq, acc1[q]);              \
  }
      SGP_ADD_TERM(0, a0, b0)
      SGP_ADD_TERM(1, a1, b1)
      if (CC == 4) {
        SGP_ADD_TERM(CC - 2, a2, b2)
        SGP_ADD_TERM(CC - 1, a3, b3)
      }
#undef SGP_ADD_TERM
    }
    store_pair_tail<CC>(K, ld, gtc * TILE + pbase, cl, R, acc0, acc1, accumulate);
  }
}

static bool additive_group_ok(const DevTerm* h_terms, int nterms) {
  if (nterms <= 0 || !additive_kind_known(h_terms[0].kind & 0xff)) return false;
  const int dim = h_terms[0].dim;
  return dim >= 1 && dim <= ADDITIVE_MAX_DIM && additive_group_order(h_terms, nterms) <= std::min(dim, ADDITIVE_MAX_ORDER);
}

// CALL(BASE, RMAX) for the group's base kind and order class
#define SGP_ADD_R(B, rmax, CALL)      \
  do {                                \
    if ((rmax) == 2) CALL(B, 2);      \
    else if ((rmax) == 4) CALL(B, 4); \
    else CALL(B, 8);                  \
  } while (0)
#define SGP_ADD_DISPATCH(base, rmax, CALL)                        \
  do {                                                            \
    if ((base) == SGP_SE) SGP_ADD_R(SGP_SE, rmax, CALL);          \
    else if ((base) == SGP_MATERN12) SGP_ADD_R(SGP_MATERN12, rmax, CALL); \
    else if ((base) == SGP_MATERN32) SGP_ADD_R(SGP_MATERN32, rmax, CALL); \
    else SGP_ADD_R(SGP_MATERN52, rmax, CALL);                     \
  } while (0)

// One group of one block pair (h_terms: host copies, d_terms: the same on the device)
int launch_assemble_additive(const AsmLaunch& L, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, hipStream_t s) {
  if (nterms <= 0 || L.empty()) return 0;
  if (!additive_group_ok(h_terms, nterms)) {
    set_error("assemble: not an additive term");
    return -1;
  }
  const int base = additive_base(h_terms[0].kind & 0xff), rmax = additive_rmax_class(additive_group_order(h_terms, nterms));
  const size_t lds = sizeof(double) * additive_lds_doubles(h_terms[0].dim);
  const dim3 grid((unsigned)L.r_cnt, (unsigned)L.c_cnt);
#define SGP_AA(B, RM)                                                                                                    \
  hipLaunchKernelGGL((assemble_additive_kernel<B, RM>), grid, dim3(256), lds, s, L.K, L.ld, L.r0, L.nr, L.c0, L.nc, d_terms, \
                     nterms, ASM_TAIL(L), L.r_first, L.c_first)
  SGP_ADD_DISPATCH(base, rmax, SGP_AA);
#undef SGP_AA
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// diagonal of one group: out[i] = (accumulate ? out[i] : 0) + sum_t e_{r_t}(i, i) (coef_t rs_i) cs_i, every operation in the
// order of the matrix kernel
// ---------------------------------------------------------------------------------------
template <int BASE, int RMAX>
__global__ __launch_bounds__(256) void diag_additive_kernel(double* out, long n, const DevTerm* terms, int nterms,
                                                            int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevTerm T = terms[0];
  const double* xr = T.xr + i * T.ldr;
  const double* xc = T.xc + i * T.ldc;
  double e[RMAX + 1];
  esp_init<RMAX>(e);
  for (int d = 0; d < T.dim; ++d) esp_step<RMAX>(e, additive_z<BASE>(xr[d] - xc[d]));
  const double rs = T.rs ? T.rs[i] : 1.0, cs = T.cs ? T.cs[i] : 1.0;
  double acc = 0.0;
  for (int tm = 0; tm < nterms; ++tm) acc = fma(esp_pick<RMAX>(e, (int)terms[tm].param), (terms[tm].coef * rs) * cs, acc);
  out[i] = accumulate ? out[i] + acc : acc;
}

int launch_diag_additive(double* out, long n, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int accumulate,
                         hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  if (!additive_group_ok(h_terms, nterms)) {
    set_error("diag: not an additive term");
    return -1;
  }
  const int base = additive_base(h_terms[0].kind & 0xff), rmax = additive_rmax_class(additive_group_order(h_terms, nterms));
#define SGP_AD(B, RM)                                                                                                    \
  hipLaunchKernelGGL((diag_additive_kernel<B, RM>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms, \
                     accumulate)
  SGP_ADD_DISPATCH(base, rmax, SGP_AD);
#undef SGP_AD
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// gradient contraction of one group, in grad_deriv_kernel's shape (deriv.hip): 128 x 128 tiles, thread = one row x 64 columns,
// per-workgroup partial sums reduced by a second kernel in a fixed order -- no atomics, the same bits on every call.  The
// tangent of the table for the input scale g (dz_d / dg = v_d = 2 s_d kappa'(s_d) at g = 1) rides through the same recurrence
// (additive_eval.h: esp_step_tangent), so that all orders come at once.  The sums are kept PER ORDER, not per term,
//   Ec[k] = sum_ij G_ij rs_i cs_j e_k            Es[k] = sum_ij G_ij rs_i cs_j de_k / dg               k = 1 .. RMAX
// and the reduction hands every term its own: gc[t] = Ec[r_t], gs[t] = coef_t Es[r_t].  A group of any length is one launch.
// ---------------------------------------------------------------------------------------
constexpr int ADDITIVE_PART = 2 * ADDITIVE_MAX_ORDER;   // doubles per workgroup: [order - 1][2]

template <int BASE, int RMAX>
__global__ __launch_bounds__(256) void grad_additive_kernel(const double* Kinv, long ldk, const double* alpha, long r0, long nr,
                                                            long c0, long nc, const DevTerm* terms, long tile_r_first,
                                                            long tile_c_first, double* partials /*[blocks][ADDITIVE_PART]*/) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) double smem[];   // additive_stage's layout | reduction
  const int D = terms[0].dim;
  const double* sc = smem;
  const double* sr = sc + TILE * D;
  const double* ss = sr + TILE * D;
  double* red = smem + additive_lds_doubles(D);   // [4 waves][ADDITIVE_PART]
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  TileClip cl;
  const bool live_tile = tile_clip(gtr, gtc, r0, nr, c0, nc, cl);
  if (!live_tile) cl.cbeg = cl.cend = cl.rbeg = cl.rend = 0;   // (nothing is read outside the pair; the partials are zeros)
  additive_stage(smem, terms[0], gtr, gtc, r0, c0, cl, t);
  __syncthreads();

  double Ec[RMAX + 1], Es[RMAX + 1];
#pragma unroll
  for (int k = 0; k <= RMAX; ++k) Ec[k] = Es[k] = 0.0;

  const long grow = gtr * TILE + trow;
  if (grow >= cl.rbeg && grow < cl.rend) {
    const double ai = alpha ? alpha[grow] : 0.0;
    const double rsv = ss[trow];
    for (int p = th * 64; p < th * 64 + 64; ++p) {
      const long gc = gtc * TILE + p;
      if (gc < cl.cbeg || gc >= cl.cend) continue;
      const double g = alpha ? 0.5 * (ai * alpha[gc] - Kinv[grow + gc * ldk]) : Kinv[grow + gc * ldk];
      double e[RMAX + 1], de[RMAX + 1];
      esp_init<RMAX>(e);
#pragma unroll
      for (int k = 0; k <= RMAX; ++k) de[k] = 0.0;
      for (int d = 0; d < D; ++d) {
        const double u = sr[d * TILE + trow] - sc[p * D + d];
        const double s = fmin(u * u, 1e300);
        double z, kx;
        additive_z<BASE>(s, z, kx);
        esp_step_tangent<RMAX>(e, de, z, (2.0 * s) * kx);
      }
      const double w = g * rsv * ss[TILE + p];
#pragma unroll
      for (int k = 1; k <= RMAX; ++k) {
        Ec[k] = fma(w, e[k], Ec[k]);
        Es[k] = fma(w, de[k], Es[k]);
      }
    }
  }
  // block reduction (fixed order): wave shuffle, then the 4 waves' sums through LDS
#pragma unroll
  for (int k = 1; k <= RMAX; ++k) {
    double a = Ec[k], b = Es[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off, 64);
      b += __shfl_xor(b, off, 64);
    }
    if ((t & 63) == 0) {
      red[(t >> 6) * ADDITIVE_PART + (k - 1) * 2 + 0] = a;
      red[(t >> 6) * ADDITIVE_PART + (k - 1) * 2 + 1] = b;
    }
  }
  __syncthreads();
  if (t < ADDITIVE_PART) {
    double s = 0.0;
    if (t < 2 * RMAX)
      for (int wv = 0; wv < 4; ++wv) s += red[wv * ADDITIVE_PART + t];
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * ADDITIVE_PART + t] = s;
  }
}

// term `blockIdx.x` of the group: out_coef = sum_b partials[b][r - 1][0], out_scale = coef sum_b partials[b][r - 1][1]; 256
// strided sums combined by a fixed tree
__global__ __launch_bounds__(256) void grad_additive_reduce_kernel(const double* partials, long nblocks, const DevTerm* terms,
                                                                   double* out_coef, double* out_scale) {
  __shared__ double sh[2][256];
  const int tm = blockIdx.x;
  const int r = (int)terms[tm].param;
  double a = 0.0, b = 0.0;
  for (long blk = threadIdx.x; blk < nblocks; blk += 256) {
    a += partials[blk * ADDITIVE_PART + (r - 1) * 2 + 0];
    b += partials[blk * ADDITIVE_PART + (r - 1) * 2 + 1];
  }
  sh[0][threadIdx.x] = a, sh[1][threadIdx.x] = b;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + off];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out_coef[tm] = sh[0][0];
    out_scale[tm] = terms[tm].coef * sh[1][0];
  }
}

long grad_additive_partials(long trc, long tcc) { return std::max<long>(1, trc * tcc) * ADDITIVE_PART; }

// One group (nterms terms at h_terms / d_terms): out_coef / out_scale point at the group's first entry; partials:
// grad_additive_partials(trc, tcc) doubles
int launch_grad_additive(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                         const DevTerm* h_terms, const DevTerm* d_terms, int nterms, long trf, long tcf, long trc, long tcc,
                         double* partials, double* out_coef, double* out_scale, hipStream_t s) {
  if (nterms <= 0 || trc <= 0 || tcc <= 0) return 0;
  if (!additive_group_ok(h_terms, nterms)) {
    set_error("grad: not an additive term");
    return -1;
  }
  const int base = additive_base(h_terms[0].kind & 0xff), rmax = additive_rmax_class(additive_group_order(h_terms, nterms));
  const size_t lds = sizeof(double) * (additive_lds_doubles(h_terms[0].dim) + 4 * ADDITIVE_PART);
  const dim3 grid((unsigned)trc, (unsigned)tcc);
#define SGP_AG(B, RM)                                                                                                       \
  hipLaunchKernelGGL((grad_additive_kernel<B, RM>), grid, dim3(256), lds, s, Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, trf, tcf, \
                     partials)
  SGP_ADD_DISPATCH(base, rmax, SGP_AG);
#undef SGP_AG
  SGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(grad_additive_reduce_kernel, dim3((unsigned)nterms), dim3(256), 0, s, partials, trc * tcc, d_terms, out_coef,
                     out_scale);
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// input points of one group, in grad_inputs_kernel's shape (grad.hip): one workgroup per 128 rows of the side `T` names as its
// row side, thread = one row x half of every column tile, the two halves combined in a fixed order; every column of gx is
// written by one thread.  With c_k the sum of the group's coefficients of order k:
//   gx[d, i] += scale sum_j G_ij rs_i cs_j A_d 2 kappa'(s_d) u_d,     A_d = sum_{m < R} c_{m+1} e_m(z without d)
// A_d by a SKIP-ONE recurrence per coordinate (O(D^2 R) fmas per pair): the table over the other D - 1 coordinates is built
// from scratch for every d, so that nothing is recovered by division or by e_k - z_d e_{k-1}, which cancel.  The pair's z_d
// and 2 kappa'(s_d) u_d are evaluated once (D exponentials) and kept in a private LDS column per thread ([D][256] each, no
// barrier: a thread reads what it wrote), because a run-time coordinate index into registers would go to scratch.
// G(i, j) at Gm[(r0 + i) sr + (c0 + j) sc]: (1, ld) for the matrix as stored, (ld, 1) for its transpose (the column side: the
// caller hands in the term with its sides swapped; the kinds are symmetric in their two points).
// ---------------------------------------------------------------------------------------
__host__ __device__ constexpr int additive_inputs_lds_doubles(int D, int dmax) {
  return 2 * D * 256 > TILE * dmax ? 2 * D * 256 : TILE * dmax;
}

template <int BASE, int RMAX, int DMAX>
__global__ __launch_bounds__(256) void grad_additive_inputs_kernel(const double* Gm, long sr, long sc, const double* alpha,
                                                                   long r0, long nr, long c0, long nc, DevTerm T,
                                                                   const DevTerm* terms /* (coef, r) of the group */, int nterms,
                                                                   double scale, double* gx /* T.dim x nr, packed */) {
  extern __shared__ __attribute__((aligned(16))) double smem[];   // zs [D][256] | ws [D][256]; then the halves' sums
  const int D = T.dim;
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  double* zs = smem + t;
  double* ws = smem + D * 256 + t;
  const long lrow = (long)blockIdx.x * TILE + trow;   // row within the block
  const bool live = lrow < nr;
  const long grow = r0 + lrow;
  double ck[RMAX + 1];   // c_k, the terms in their order (uniform scalars)
#pragma unroll
  for (int k = 0; k <= RMAX; ++k) ck[k] = 0.0;
  for (int tm = 0; tm < nterms; ++tm) {
    const int r = (int)terms[tm].param;
    const double coef = terms[tm].coef;
#pragma unroll
    for (int k = 1; k <= RMAX; ++k) ck[k] += r == k ? coef : 0.0;
  }
  double xr[DMAX], acc[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    xr[d] = (live && d < D) ? T.xr[lrow * T.ldr + d] : 0.0;
    acc[d] = 0.0;
  }
  const double ai = (alpha && live) ? alpha[grow] : 0.0;
  const double wrow = live ? (T.rs ? T.rs[lrow] : 1.0) : 0.0;
  if (live) {
    for (long ct = 0; ct * TILE < nc; ++ct) {
      for (int p = th * 64; p < th * 64 + 64; ++p) {
        const long lc = ct * TILE + p;
        if (lc >= nc) break;
        const long gc = c0 + lc;
        const double gm = Gm[grow * sr + gc * sc];
        const double g = alpha ? 0.5 * (ai * alpha[gc] - gm) : gm;
        const double* y = T.xc + lc * T.ldc;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          if (d < D) {
            const double u = xr[d] - y[d];
            double z, kx;
            additive_z<BASE>(u * u, z, kx);
            zs[d * 256] = z;
            ws[d * 256] = (2.0 * kx) * u;
          }
        }
        const double w = g * wrow * (T.cs ? T.cs[lc] : 1.0);
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          if (d < D) {
            double e[RMAX];   // e_0 .. e_{RMAX-1} of z without d
            esp_init<RMAX - 1>(e);
            for (int dd = 0; dd < D; ++dd)
              if (dd != d) esp_step<RMAX - 1>(e, zs[dd * 256]);
            double A = 0.0;
#pragma unroll
            for (int m = 0; m < RMAX; ++m) A = fma(ck[m + 1], e[m], A);
            acc[d] = fma(w * A, ws[d * 256], acc[d]);
          }
        }
      }
    }
  }
  // combine the two column halves in fixed order, then add into the input's gradient
  __syncthreads();
  double* comb = smem;   // [128][DMAX]: the private columns are no longer needed
  if (th == 1) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) comb[trow * DMAX + d] = acc[d];
  }
  __syncthreads();
  if (th == 0 && live) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
      if (d < D) gx[lrow * T.dim + d] += scale * (acc[d] + comb[trow * DMAX + d]);
  }
}

// T: the group's first term as the side to differentiate sees it (host copy, sides swapped for the column side); h_terms /
// d_terms: the group on the host and on the device, read for (coef, r) alone
int launch_grad_additive_inputs(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                                const DevTerm& T, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, double scale,
                                double* gx, hipStream_t s) {
  if (nr <= 0 || nc <= 0 || nterms <= 0 || !gx) return 0;
  if (!additive_group_ok(h_terms, nterms) || T.dim != h_terms[0].dim) {
    set_error("grad inputs: not an additive term");
    return -1;
  }
  const int base = additive_base(T.kind & 0xff), rmax = additive_rmax_class(additive_group_order(h_terms, nterms));
  const int dmax = T.dim <= 4 ? 4 : 16;
  const size_t lds = sizeof(double) * additive_inputs_lds_doubles(T.dim, dmax);
  const dim3 grid((unsigned)((nr + TILE - 1) / TILE)), block(256);
  // (an order class above the dimension class does not occur: r <= D)
#define SGP_AI(B, RM)                                                                                                          \
  do {                                                                                                                         \
    if (dmax == 4 && RM <= 4)                                                                                                  \
      hipLaunchKernelGGL((grad_additive_inputs_kernel<B, (RM <= 4 ? RM : 4), 4>), grid, block, lds, s, Gm, sr, sc, alpha, r0, nr, c0, \
                         nc, T, d_terms, nterms, scale, gx);                                                                   \
    else                                                                                                                       \
      hipLaunchKernelGGL((grad_additive_inputs_kernel<B, RM, 16>), grid, block, lds, s, Gm, sr, sc, alpha, r0, nr, c0, nc, T,  \
                         d_terms, nterms, scale, gx);                                                                          \
  } while (0)
  SGP_ADD_DISPATCH(base, rmax, SGP_AI);
#undef SGP_AI
  SGP_HIP(hipGetLastError());
  return 0;
}

}  // namespace sgp
