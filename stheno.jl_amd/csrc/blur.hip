// Blur terms (include/sthenomi.h: SGP_BLUR_SE): the squared-exponential integrated against a Gaussian footprint on either side,
//   K_ij = coef rs_i cs_j prod_d q_d^(-1/2) exp(-1/2 sum_d u_d^2 / q_d),   u = mu_i - mu'_j,  q_d = 1 + (s_d + s'_d)
// (blur_eval.h: the formulas; blur_kinds.h: the validation table).  A point carries its D variances below its D locations:
// dim = 2 D.
//
// A term class of its own, as the Gibbs kind is.  The terms of one block pair that share points and scale vectors form a GROUP
// (blur_kinds.h: blur_group) and differ in coef alone: a launch carries one group, the exponential and the normaliser are
// evaluated ONCE per point pair.
//
// Unlike the Gibbs kind a pair needs D reciprocals, so the matrix kernel has three modes, picked per group from what dspec
// creation found in the variance rows (DevTerm::wr / wc: that side's variances are all exactly 0):
//   BLUR_ROWS   the column side is plain: w_d = 1 / q_d and the normaliser depend on the row point alone.  They are staged
//               per point, held in registers, and the pair loop is the SE kernel's distance loop with one more multiply per
//               coordinate and one by the normaliser: no division.  K(blurred, plain), and cov(f, f) with w == 1.
//   BLUR_COLS   the row side is plain: the same with w_d read from LDS beside the column locations.
//   BLUR_BOTH   the reciprocals are taken per pair, the column side's s' in LDS beside its locations.
// All three run blur_eval.h's steps on the same numbers (q = 1 + (s + 0) is formed in staging exactly as per pair), so a pair
// has the same bits in every mode.
//
// Tiling: the assembly frame's two-row form (asm_frame.h) -- 128 x 128 tiles of the global grid, one 256-thread workgroup per
// tile, thread (lane, wave) owns rows 2 lane, 2 lane + 1 and the 32 columns of quarter `wave`, 16-byte stores on interior
// tiles.  LDS, staged once per tile:
//   [128][DMAX] column locations | [DMAX][128] row locations | [128][DMAX] column s' or w | [DMAX][128] row s or w |
//   rs | cs | row normaliser | column normaliser                                                     (128 doubles each)
// Padding coordinates and points outside the clip hold location 0 and variance 0 (w = 1, normaliser 1), scale 0.
#include "asm_frame.h"
#include "blur_eval.h"
#include "blur_kinds.h"
#include <algorithm>

namespace sgp {

constexpr int BCC = 4;   // columns per chunk (x 2 rows = 8 independent exp chains), as the plain kernel's
enum { BLUR_BOTH = 0, BLUR_ROWS = 1, BLUR_COLS = 2 };

// The one place that reads the flags dspec creation leaves on a blur term: DevTerm's patch fields are unused by the class
// (ph == 0), and wr / wc != 0 there means "the variance rows of the row / column side are all exactly 0" -- no width, no weight
static int blur_mode(const DevTerm& T) { return T.wc ? BLUR_ROWS : (T.wr ? BLUR_COLS : BLUR_BOTH); }

__host__ __device__ constexpr int blur_lds_doubles(int dmax) { return 4 * TILE * dmax + 4 * TILE; }

// the tile's points.  MODE says what the two variance arrays hold: BLUR_BOTH s and s'; BLUR_ROWS w of the row point (the
// column array is not read); BLUR_COLS w of the column point
template <int DMAX, int MODE>
__device__ __forceinline__ void blur_stage(double* smem, const DevTerm& T, long gtr, long gtc, long r0, long c0,
                                           const TileClip& cl, int t) {
  const int D = T.dim / 2;
  double* sc = smem;
  double* sr = sc + TILE * DMAX;
  double* vc = sr + TILE * DMAX;
  double* vr = vc + TILE * DMAX;
  double* sl = vr + TILE * DMAX;   // rs | cs | row normaliser | column normaliser
  for (int idx = t; idx < TILE * DMAX; idx += 256) {
    const int p = idx / DMAX, d = idx % DMAX;
    const long gc = gtc * TILE + p, gr = gtr * TILE + p;
    const bool cin = d < D && gc >= cl.cbeg && gc < cl.cend, rin = d < D && gr >= cl.rbeg && gr < cl.rend;
    const double* pc = T.xc + (gc - c0) * T.ldc + d;
    const double* pr = T.xr + (gr - r0) * T.ldr + d;
    sc[idx] = cin ? pc[0] : 0.0;
    sr[d * TILE + p] = rin ? pr[0] : 0.0;
    const double s_c = cin ? pc[D] : 0.0, s_r = rin ? pr[D] : 0.0;
    vc[idx] = MODE == BLUR_COLS ? 1.0 / blur_q(0.0, s_c) : s_c;
    vr[d * TILE + p] = MODE == BLUR_ROWS ? 1.0 / blur_q(s_r, 0.0) : s_r;
  }
  if (t < TILE) {
    const long gr = gtr * TILE + t;
    const bool in = gr >= cl.rbeg && gr < cl.rend;
    sl[t] = in ? (T.rs ? T.rs[gr - r0] : 1.0) : 0.0;
    double P = 1.0;
    if (MODE == BLUR_ROWS && in)
      for (int d = 0; d < D; ++d) P *= blur_q(T.xr[(gr - r0) * T.ldr + D + d], 0.0);
    sl[2 * TILE + t] = blur_rnorm(P);
  } else {
    const int p = t - TILE;
    const long gc = gtc * TILE + p;
    const bool in = gc >= cl.cbeg && gc < cl.cend;
    sl[TILE + p] = in ? (T.cs ? T.cs[gc - c0] : 1.0) : 0.0;
    double P = 1.0;
    if (MODE == BLUR_COLS && in)
      for (int d = 0; d < D; ++d) P *= blur_q(0.0, T.xc[(gc - c0) * T.ldc + D + d]);
    sl[3 * TILE + p] = blur_rnorm(P);
  }
}

// one pair of the matrix kernel: xi / vi the row point's registers, c / vcq the column point's LDS rows
template <int DMAX, int MODE>
__device__ __forceinline__ double blur_entry(const double (&xi)[DMAX], const double (&vi)[DMAX], const double* c,
                                             const double* vcq, double rn_row, double rn_col) {
  double t = 0.0, P = 1.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double u = xi[d] - c[d];
    if (MODE == BLUR_BOTH) {
      const double q = blur_q(vi[d], vcq[d]);
      t = blur_step(u, 1.0 / q, t);
      P *= q;
    } else {
      t = blur_step(u, MODE == BLUR_ROWS ? vi[d] : vcq[d], t);
    }
  }
  return blur_value(t, MODE == BLUR_BOTH ? blur_rnorm(P) : (MODE == BLUR_ROWS ? rn_row : rn_col));
}

template <int DMAX, int MODE>
__global__ __launch_bounds__(256) void assemble_blur_kernel(
    double* __restrict__ K, long ld, long r0, long nr, long c0, long nc, const DevTerm* __restrict__ terms, int nterms,
    int lower_only, int accumulate, int noise_kind, double sigma2, const double* __restrict__ noise_diag, long tile_r_first,
    long tile_c_first) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  if (lower_only && gtr < gtc) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;

  TileClip cl;
  if (!tile_clip(gtr, gtc, r0, nr, c0, nc, cl)) return;   // uniform over the workgroup

  const double* sc = smem;
  const double* sr = sc + TILE * DMAX;
  const double* vc = sr + TILE * DMAX;
  const double* vr = vc + TILE * DMAX;
  const double* sl = vr + TILE * DMAX;
  blur_stage<DMAX, MODE>(smem, terms[0], gtr, gtc, r0, c0, cl, t);
  __syncthreads();

  const PairRows R = pair_rows(K, ld, gtr, gtc, lane, cl, accumulate, noise_kind, sigma2, noise_diag);

  double xi0[DMAX], xi1[DMAX], vi0[DMAX], vi1[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double2 x2 = *reinterpret_cast<const double2*>(sr + d * TILE + 2 * lane);
    xi0[d] = x2.x;
    xi1[d] = x2.y;
    const double2 v2 = MODE == BLUR_COLS ? make_double2(0.0, 0.0) : *reinterpret_cast<const double2*>(vr + d * TILE + 2 * lane);
    vi0[d] = v2.x;
    vi1[d] = v2.y;
  }
  const double2 rs = *reinterpret_cast<const double2*>(sl + 2 * lane);
  const double2 rn = *reinterpret_cast<const double2*>(sl + 2 * TILE + 2 * lane);

  for (int jc = 0; jc < 32; jc += BCC) {
    const int pbase = wv * 32 + jc;
    // once per point pair: one exponential, one normaliser (BLUR_BOTH: and D reciprocals)
    double k0[BCC], k1[BCC];
#pragma unroll
    for (int q = 0; q < BCC; ++q) {
      const double* c = sc + (pbase + q) * DMAX;
      const double* vcq = vc + (pbase + q) * DMAX;
      const double rnc = sl[3 * TILE + pbase + q];
      k0[q] = blur_entry<DMAX, MODE>(xi0, vi0, c, vcq, rn.x, rnc);
      k1[q] = blur_entry<DMAX, MODE>(xi1, vi1, c, vcq, rn.y, rnc);
    }
    double acc0[BCC], acc1[BCC];
#pragma unroll
    for (int q = 0; q < BCC; ++q) acc0[q] = acc1[q] = 0.0;
    for (int tm = 0; tm < nterms; ++tm) {   // coef: a wave-uniform scalar
      const double coef = terms[tm].coef;
      const double w0 = coef * rs.x, w1 = coef * rs.y;
#pragma unroll
      for (int q = 0; q < BCC; ++q) {
        const double cq = sl[TILE + pbase + q];
        acc0[q] = fma(k0[q], w0 * cq, acc0[q]);
        acc1[q] = fma(k1[q], w1 * cq, acc1[q]);
      }
    }
    store_pair_tail<BCC>(K, ld, gtc * TILE + pbase, cl, R, acc0, acc1, accumulate);
  }
}

static bool blur_group_ok(const DevTerm* h_terms, int nterms) {
  return nterms > 0 && blur_kind_known(h_terms[0].kind & 0xff) && !blur_dim_refusal(h_terms[0].dim);
}

// One group of one block pair (h_terms: host copies, d_terms: the same on the device)
int launch_assemble_blur(const AsmLaunch& L, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, hipStream_t s) {
  if (nterms <= 0 || L.empty()) return 0;
  if (!blur_group_ok(h_terms, nterms)) {
    set_error("assemble: not a blur term");
    return -1;
  }
  const int dmax = blur_dmax_class(h_terms[0].dim);
  const int mode = blur_mode(h_terms[0]);
  const size_t lds = sizeof(double) * blur_lds_doubles(dmax);
  const dim3 grid((unsigned)L.r_cnt, (unsigned)L.c_cnt);
#define SGP_BL(DM, MD)                                                                                                        \
  hipLaunchKernelGGL((assemble_blur_kernel<DM, MD>), grid, dim3(256), lds, s, L.K, L.ld, L.r0, L.nr, L.c0, L.nc, d_terms, nterms, \
                     ASM_TAIL(L), L.r_first, L.c_first)
#define SGP_BLM(DM)                          \
  do {                                       \
    if (mode == BLUR_ROWS) SGP_BL(DM, BLUR_ROWS); \
    else if (mode == BLUR_COLS) SGP_BL(DM, BLUR_COLS); \
    else SGP_BL(DM, BLUR_BOTH);              \
  } while (0)
  if (dmax <= 1) SGP_BLM(1);
  else if (dmax <= 2) SGP_BLM(2);
  else if (dmax <= 4) SGP_BLM(4);
  else SGP_BLM(8);
#undef SGP_BLM
#undef SGP_BL
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// diagonal of one group: out[i] = (accumulate ? out[i] : 0) + sum_t k(i, i) (coef_t rs_i) cs_i, every operation in the order of
// the matrix kernel (over the D coordinates alone: the matrix kernel's padding leaves t and P their bits)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void diag_blur_kernel(double* out, long n, const DevTerm* terms, int nterms, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevTerm T = terms[0];
  const int D = T.dim / 2;
  const double* xr = T.xr + i * T.ldr;
  const double* xc = T.xc + i * T.ldc;
  const double k = blur_pair(xr, xr + D, xc, xc + D, D);
  const double rs = T.rs ? T.rs[i] : 1.0, cs = T.cs ? T.cs[i] : 1.0;
  double acc = 0.0;
  for (int tm = 0; tm < nterms; ++tm) acc = fma(k, (terms[tm].coef * rs) * cs, acc);
  out[i] = accumulate ? out[i] + acc : acc;
}

int launch_diag_blur(double* out, long n, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int accumulate,
                     hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  if (!blur_group_ok(h_terms, nterms)) {
    set_error("diag: not a blur term");
    return -1;
  }
  hipLaunchKernelGGL(diag_blur_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms, accumulate);
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// gradient contraction of one group, in grad_gibbs_kernel's shape: 128 x 128 tiles, thread = one row x 64 columns, per-workgroup
// partial sums reduced by a second kernel in a fixed order -- no atomics, the same bits on every call.  The terms differ in
// coef alone, so two sums serve the group:
//   A = sum_ij G_ij rs_i cs_j k(i, j)        B = sum_ij G_ij rs_i cs_j k(i, j) sum_d -(S_d w_d + (u_d w_d)^2),  S = s + s'
//   gc[t] = A                                gs[t] = coef_t B
// (the input scale g multiplies the locations of both sides, g^2 their variances).  The reciprocals are taken per pair here,
// whatever the variance rows hold.
// ---------------------------------------------------------------------------------------
template <int DMAX>
__global__ __launch_bounds__(256) void grad_blur_kernel(const double* Kinv, long ldk, const double* alpha, long r0, long nr,
                                                        long c0, long nc, const DevTerm* terms, long tile_r_first,
                                                        long tile_c_first, double* partials /*[blocks][2]*/) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) double smem[];   // blur_stage's layout | reduction
  const double* sc = smem;
  const double* sr = sc + TILE * DMAX;
  const double* vc = sr + TILE * DMAX;
  const double* vr = vc + TILE * DMAX;
  const double* sl = vr + TILE * DMAX;
  double* red = smem + blur_lds_doubles(DMAX);   // [4 waves][2]
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  TileClip cl;
  const bool live_tile = tile_clip(gtr, gtc, r0, nr, c0, nc, cl);
  if (!live_tile) cl.cbeg = cl.cend = cl.rbeg = cl.rend = 0;   // (nothing is read outside the pair; the partials are zeros)
  blur_stage<DMAX, BLUR_BOTH>(smem, terms[0], gtr, gtc, r0, c0, cl, t);
  __syncthreads();

  double A = 0.0, B = 0.0;
  const long grow = gtr * TILE + trow;
  if (grow >= cl.rbeg && grow < cl.rend) {
    const double ai = alpha ? alpha[grow] : 0.0;
    const double rsv = sl[trow];
    double xi[DMAX], si[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xi[d] = sr[d * TILE + trow], si[d] = vr[d * TILE + trow];
    for (int p = th * 64; p < th * 64 + 64; ++p) {
      const long gc = gtc * TILE + p;
      if (gc < cl.cbeg || gc >= cl.cend) continue;
      const double g = alpha ? 0.5 * (ai * alpha[gc] - Kinv[grow + gc * ldk]) : Kinv[grow + gc * ldk];
      double tt = 0.0, P = 1.0, h = 0.0;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        const double sp = vc[p * DMAX + d];
        const double q = blur_q(si[d], sp), w = 1.0 / q, u = xi[d] - sc[p * DMAX + d];
        const double a = u * w;
        tt = blur_step(u, w, tt);
        P *= q;
        h -= fma(si[d] + sp, w, a * a);
      }
      const double k = blur_value(tt, blur_rnorm(P));
      const double w = g * rsv * sl[TILE + p];
      A = fma(w, k, A);
      B = fma(w, k == 0.0 ? 0.0 : k * h, B);
    }
  }
  // block reduction (fixed order): wave shuffle, then the 4 waves' sums through LDS
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    A += __shfl_xor(A, off, 64);
    B += __shfl_xor(B, off, 64);
  }
  if ((t & 63) == 0) red[(t >> 6) * 2 + 0] = A, red[(t >> 6) * 2 + 1] = B;
  __syncthreads();
  if (t < 2) {
    double s = 0.0;
    for (int wv = 0; wv < 4; ++wv) s += red[wv * 2 + t];
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * 2 + t] = s;
  }
}

// out_coef[t] = A, out_scale[t] = coef_t B with (A, B) = sum_b partials[b]: one workgroup, 256 strided sums combined by a fixed
// tree
__global__ __launch_bounds__(256) void grad_blur_reduce_kernel(const double* partials, long nblocks, const DevTerm* terms,
                                                               int nterms, double* out_coef, double* out_scale) {
  __shared__ double sh[2][256];
  double a = 0.0, b = 0.0;
  for (long k = threadIdx.x; k < nblocks; k += 256) a += partials[k * 2], b += partials[k * 2 + 1];
  sh[0][threadIdx.x] = a, sh[1][threadIdx.x] = b;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + off];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < nterms) {
    out_coef[threadIdx.x] = sh[0][0];
    out_scale[threadIdx.x] = terms[threadIdx.x].coef * sh[1][0];
  }
}

long grad_blur_partials(long trc, long tcc) { return std::max<long>(1, trc * tcc) * 2; }

// One group (nterms terms at h_terms / d_terms): out_coef / out_scale point at the group's first entry; partials:
// grad_blur_partials(trc, tcc) doubles
int launch_grad_blur(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                     const DevTerm* h_terms, const DevTerm* d_terms, int nterms, long trf, long tcf, long trc, long tcc,
                     double* partials, double* out_coef, double* out_scale, hipStream_t s) {
  if (nterms <= 0 || trc <= 0 || tcc <= 0) return 0;
  if (!blur_group_ok(h_terms, nterms)) {
    set_error("grad: not a blur term");
    return -1;
  }
  const int dmax = blur_dmax_class(h_terms[0].dim);
  const size_t lds = sizeof(double) * (blur_lds_doubles(dmax) + 8);
  const dim3 grid((unsigned)trc, (unsigned)tcc);
#define SGP_BG(DM) \
  hipLaunchKernelGGL((grad_blur_kernel<DM>), grid, dim3(256), lds, s, Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, trf, tcf, partials)
  if (dmax <= 1) SGP_BG(1);
  else if (dmax <= 2) SGP_BG(2);
  else if (dmax <= 4) SGP_BG(4);
  else SGP_BG(8);
#undef SGP_BG
  SGP_HIP(hipGetLastError());
  for (int t = 0; t < nterms; t += 256) {
    hipLaunchKernelGGL(grad_blur_reduce_kernel, dim3(1), dim3(256), 0, s, partials, trc * tcc, d_terms + t,
                       std::min(256, nterms - t), out_coef + t, out_scale + t);
    SGP_HIP(hipGetLastError());
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// input points of one group, in grad_gibbs_inputs_kernel's shape: one workgroup per 128 rows of the side `T` names as its row
// side, thread = one row x half of every column tile, the column tile's points in LDS, the two halves combined in a fixed
// order; every column of gx is written by one thread.  With C = sum_t coef_t, a_d = u_d w_d:
//   gx[d, i]     += scale sum_j G_ij rs_i cs_j C k (-a_d)                        d < D
//   gx[D + d, i] += scale sum_j G_ij rs_i cs_j C k (a_d^2 - w_d) / 2
// G(i, j) at Gm[(r0 + i) sr + (c0 + j) sc]: (1, ld) for the matrix as stored, (ld, 1) for its transpose (the column side: the
// caller hands in the term with its sides swapped; the kind is symmetric in its two points).
// ---------------------------------------------------------------------------------------
template <int DMAX>
__global__ __launch_bounds__(256) void grad_blur_inputs_kernel(const double* Gm, long sr, long sc, const double* alpha, long r0,
                                                               long nr, long c0, long nc, DevTerm T,
                                                               const DevTerm* terms /* coef of the group */, int nterms,
                                                               double scale, double* gx /* T.dim x nr, packed */) {
  __shared__ double sx[TILE * DMAX];    // the column tile's locations
  __shared__ double sv[TILE * DMAX];    // ... variances
  __shared__ double scs[TILE];          // ... scales
  __shared__ double comb[TILE * 2 * DMAX];
  const int D = T.dim / 2;
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  const long lrow = (long)blockIdx.x * TILE + trow;   // row within the block
  const bool live = lrow < nr;
  const long grow = r0 + lrow;
  double xr[DMAX], vr[DMAX], accm[DMAX], accs[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    xr[d] = (live && d < D) ? T.xr[lrow * T.ldr + d] : 0.0;
    vr[d] = (live && d < D) ? T.xr[lrow * T.ldr + D + d] : 0.0;
    accm[d] = accs[d] = 0.0;
  }
  double csum = 0.0;
  for (int tm = 0; tm < nterms; ++tm) csum += terms[tm].coef;
  const double ai = (alpha && live) ? alpha[grow] : 0.0;
  const double wrow = live ? (T.rs ? T.rs[lrow] : 1.0) : 0.0;
  for (long ct = 0; ct * TILE < nc; ++ct) {
    __syncthreads();
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long lc = ct * TILE + p;
      const bool in = lc < nc && d < D;
      sx[idx] = in ? T.xc[lc * T.ldc + d] : 0.0;
      sv[idx] = in ? T.xc[lc * T.ldc + D + d] : 0.0;
    }
    if (t < TILE) {
      const long lc = ct * TILE + t;
      scs[t] = lc < nc ? (T.cs ? T.cs[lc] : 1.0) : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int p = th * 64; p < th * 64 + 64; ++p) {
        const long lc = ct * TILE + p;
        if (lc >= nc) break;
        const long gc = c0 + lc;
        const double gm = Gm[grow * sr + gc * sc];
        const double g = alpha ? 0.5 * (ai * alpha[gc] - gm) : gm;
        double a[DMAX], w[DMAX], tt = 0.0, P = 1.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          const double q = blur_q(vr[d], sv[p * DMAX + d]);
          const double u = xr[d] - sx[p * DMAX + d];
          w[d] = 1.0 / q;
          a[d] = u * w[d];
          tt = blur_step(u, w[d], tt);
          P *= q;
        }
        const double k = blur_value(tt, blur_rnorm(P));
        if (k == 0.0) continue;   // a dead pair: exact zeros, whatever a holds
        const double wk = (g * wrow * scs[p]) * (csum * k);
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          accm[d] = fma(wk, -a[d], accm[d]);
          accs[d] = fma(wk, 0.5 * fma(a[d], a[d], -w[d]), accs[d]);
        }
      }
    }
  }
  // combine the two column halves in fixed order, then add into the input's gradient
  __syncthreads();
  if (th == 1) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) comb[trow * 2 * DMAX + d] = accm[d], comb[trow * 2 * DMAX + DMAX + d] = accs[d];
  }
  __syncthreads();
  if (th == 0 && live) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
      if (d < D) {
        gx[lrow * T.dim + d] += scale * (accm[d] + comb[trow * 2 * DMAX + d]);
        gx[lrow * T.dim + D + d] += scale * (accs[d] + comb[trow * 2 * DMAX + DMAX + d]);
      }
  }
}

// T: the group's first term as the side to differentiate sees it (host copy, sides swapped for the column side); d_terms: the
// group on the device, read for coef alone
int launch_grad_blur_inputs(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                            const DevTerm& T, const DevTerm* d_terms, int nterms, double scale, double* gx, hipStream_t s) {
  if (nr <= 0 || nc <= 0 || nterms <= 0 || !gx) return 0;
  if (!blur_group_ok(&T, nterms)) {
    set_error("grad inputs: not a blur term");
    return -1;
  }
  const int dmax = blur_dmax_class(T.dim);
  const dim3 grid((unsigned)((nr + TILE - 1) / TILE)), block(256);
#define SGP_BI(DM) \
  hipLaunchKernelGGL((grad_blur_inputs_kernel<DM>), grid, block, 0, s, Gm, sr, sc, alpha, r0, nr, c0, nc, T, d_terms, nterms, scale, gx)
  if (dmax <= 1) SGP_BI(1);
  else if (dmax <= 2) SGP_BI(2);
  else if (dmax <= 4) SGP_BI(4);
  else SGP_BI(8);
#undef SGP_BI
  SGP_HIP(hipGetLastError());
  return 0;
}

}  // namespace sgp
