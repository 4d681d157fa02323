// Gibbs terms (include/sthenomi.h: SGP_GIBBS): a squared-exponential whose lengthscale depends on the point,
//   K_ij = coef rs_i cs_j c^(p/2) exp(-s / q),   s = |x_i - y_j|^2,  q = lx^2 + ly^2,  c = 2 lx ly / q,
// the one non-stationary kind of the library (gibbs_eval.h: the formulas; gibbs_kinds.h: the validation table).  A point
// carries its lengthscale as its last coordinate: dim = D + 1.
//
// A term class of its own, as the derivative kinds are.  The terms of one block pair that share points and scale vectors form a
// GROUP (gibbs_kinds.h: gibbs_group) and differ in (coef, p) alone: a launch carries one group, the reciprocal of q, the
// square root of c and the exponential are evaluated ONCE per point pair, and the term loop multiplies sqrt(c) p times over
// wave-uniform scalars.  A sum of a p = 1 and a p = D term costs one exponential per entry.
//
// Tiling of the matrix kernel: the assembly frame's two-row form (asm_frame.h) -- 128 x 128 tiles of the global grid, one
// 256-thread workgroup per tile, thread (lane, wave) owns rows 2 lane, 2 lane + 1 and the 32 columns of quarter `wave`, 16-byte
// stores on interior tiles.  LDS, staged once per tile:
//   [128][DMAX] column locations | [DMAX][128] row locations | lr | lr2 | lc | lc2 | rs | cs     (128 doubles each)
// The location arrays hold the D location coordinates and zeros behind them (the lengthscale never enters the distance: the
// padding adds exact zeros); l and l2 = l * l sit in arrays of their own, so that a pair reads both sides' l2 and never squares.
#include "asm_frame.h"
#include "gibbs_eval.h"
#include "gibbs_kinds.h"
#include <algorithm>

namespace sgp {

constexpr int GCC = 4;   // columns per chunk (x 2 rows = 8 independent exp chains), as the plain kernel's

__host__ __device__ constexpr int gibbs_lds_doubles(int dmax) { return 2 * TILE * dmax + 6 * TILE; }

// the tile's points: locations, lengthscales and their squares, scale vectors.  Outside the clip: location 0, l = 1, scale 0
template <int DMAX>
__device__ __forceinline__ void gibbs_stage(double* smem, const DevTerm& T, long gtr, long gtc, long r0, long c0,
                                            const TileClip& cl, int t) {
  const int D = T.dim - 1;
  double* sc = smem;
  double* sr = sc + TILE * DMAX;
  double* sl = sr + TILE * DMAX;   // lr | lr2 | lc | lc2 | rs | cs
  for (int idx = t; idx < TILE * DMAX; idx += 256) {
    const int p = idx / DMAX, d = idx % DMAX;
    const long gc = gtc * TILE + p, gr = gtr * TILE + p;
    sc[idx] = (d < D && gc >= cl.cbeg && gc < cl.cend) ? T.xc[(gc - c0) * T.ldc + d] : 0.0;
    sr[d * TILE + p] = (d < D && gr >= cl.rbeg && gr < cl.rend) ? T.xr[(gr - r0) * T.ldr + d] : 0.0;
  }
  if (t < TILE) {
    const long gr = gtr * TILE + t;
    const bool in = gr >= cl.rbeg && gr < cl.rend;
    const double l = in ? T.xr[(gr - r0) * T.ldr + D] : 1.0;
    sl[t] = l, sl[TILE + t] = l * l;
    sl[4 * TILE + t] = in ? (T.rs ? T.rs[gr - r0] : 1.0) : 0.0;
  } else {
    const int p = t - TILE;
    const long gc = gtc * TILE + p;
    const bool in = gc >= cl.cbeg && gc < cl.cend;
    const double l = in ? T.xc[(gc - c0) * T.ldc + D] : 1.0;
    sl[2 * TILE + p] = l, sl[3 * TILE + p] = l * l;
    sl[5 * TILE + p] = in ? (T.cs ? T.cs[gc - c0] : 1.0) : 0.0;
  }
}

// s = sum_d (xi_d - c_d)^2, d ascending, fma -- the plain kernels' distance
template <int DMAX>
__device__ __forceinline__ double gibbs_dist(const double (&xi)[DMAX], const double* c) {
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = xi[d] - c[d];
    s = fma(df, df, s);
  }
  return s;
}

template <int DMAX>
__global__ __launch_bounds__(256) void assemble_gibbs_kernel(
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
  const double* sl = sr + TILE * DMAX;
  gibbs_stage<DMAX>(smem, terms[0], gtr, gtc, r0, c0, cl, t);
  __syncthreads();

  const PairRows R = pair_rows(K, ld, gtr, gtc, lane, cl, accumulate, noise_kind, sigma2, noise_diag);

  double xi0[DMAX], xi1[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double2 x2 = *reinterpret_cast<const double2*>(sr + d * TILE + 2 * lane);
    xi0[d] = x2.x;
    xi1[d] = x2.y;
  }
  const double2 lr = *reinterpret_cast<const double2*>(sl + 2 * lane);
  const double2 lr2 = *reinterpret_cast<const double2*>(sl + TILE + 2 * lane);
  const double2 rs = *reinterpret_cast<const double2*>(sl + 4 * TILE + 2 * lane);

  for (int jc = 0; jc < 32; jc += GCC) {
    const int pbase = wv * 32 + jc;
    const double* sp = sc + pbase * DMAX;
    // once per point pair: one reciprocal, one square root, one exponential
    GibbsPair P0[GCC], P1[GCC];
#pragma unroll
    for (int q = 0; q < GCC; ++q) {
      const double lc = sl[2 * TILE + pbase + q], lc2 = sl[3 * TILE + pbase + q];
      P0[q] = gibbs_pair(gibbs_dist<DMAX>(xi0, sp + q * DMAX), lr.x, lr2.x, lc, lc2);
      P1[q] = gibbs_pair(gibbs_dist<DMAX>(xi1, sp + q * DMAX), lr.y, lr2.y, lc, lc2);
    }
    double acc0[GCC], acc1[GCC];
#pragma unroll
    for (int q = 0; q < GCC; ++q) acc0[q] = acc1[q] = 0.0;
    for (int tm = 0; tm < nterms; ++tm) {   // (coef, p): wave-uniform scalars
      const double coef = terms[tm].coef;
      const int p = (int)terms[tm].param;
      const double w0 = coef * rs.x, w1 = coef * rs.y;
#pragma unroll
      for (int q = 0; q < GCC; ++q) {
        const double cq = sl[5 * TILE + pbase + q];
        acc0[q] = fma(gibbs_value(P0[q], p), w0 * cq, acc0[q]);
        acc1[q] = fma(gibbs_value(P1[q], p), w1 * cq, acc1[q]);
      }
    }
    store_pair_tail<GCC>(K, ld, gtc * TILE + pbase, cl, R, acc0, acc1, accumulate);
  }
}

static bool gibbs_group_ok(const DevTerm* h_terms, int nterms) {
  const int code = h_terms[0].kind & 0xff, dim = h_terms[0].dim;
  return nterms > 0 && gibbs_kind_known(code) && dim >= 2 && dim <= GIBBS_MAX_DIM;
}

// One group of one block pair (h_terms: host copies, d_terms: the same on the device)
int launch_assemble_gibbs(const AsmLaunch& L, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, hipStream_t s) {
  if (nterms <= 0 || L.empty()) return 0;
  if (!gibbs_group_ok(h_terms, nterms)) {
    set_error("assemble: not a Gibbs term");
    return -1;
  }
  const int dmax = gibbs_dmax_class(h_terms[0].dim);
  const size_t lds = sizeof(double) * gibbs_lds_doubles(dmax);
  const dim3 grid((unsigned)L.r_cnt, (unsigned)L.c_cnt);
#define SGP_GB(DM)                                                                                                         \
  hipLaunchKernelGGL((assemble_gibbs_kernel<DM>), grid, dim3(256), lds, s, L.K, L.ld, L.r0, L.nr, L.c0, L.nc, d_terms, nterms, \
                     ASM_TAIL(L), L.r_first, L.c_first)
  if (dmax <= 2) SGP_GB(2);
  else if (dmax <= 4) SGP_GB(4);
  else if (dmax <= 8) SGP_GB(8);
  else SGP_GB(16);
#undef SGP_GB
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// diagonal of one group: out[i] = (accumulate ? out[i] : 0) + sum_t k_t(i, i) (coef_t rs_i) cs_i, every operation in the order
// of the matrix kernel (the distance over the D location coordinates alone: the matrix kernel's padding adds exact zeros)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void diag_gibbs_kernel(double* out, long n, const DevTerm* terms, int nterms, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevTerm T = terms[0];
  const int D = T.dim - 1;
  const double* xr = T.xr + i * T.ldr;
  const double* xc = T.xc + i * T.ldc;
  double s = 0.0;
  for (int d = 0; d < D; ++d) {
    const double df = xr[d] - xc[d];
    s = fma(df, df, s);
  }
  const double lx = xr[D], ly = xc[D];
  const GibbsPair P = gibbs_pair(s, lx, lx * lx, ly, ly * ly);
  const double rs = T.rs ? T.rs[i] : 1.0, cs = T.cs ? T.cs[i] : 1.0;
  double acc = 0.0;
  for (int tm = 0; tm < nterms; ++tm) acc = fma(gibbs_value(P, (int)terms[tm].param), (terms[tm].coef * rs) * cs, acc);
  out[i] = accumulate ? out[i] + acc : acc;
}

int launch_diag_gibbs(double* out, long n, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int accumulate,
                      hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  if (!gibbs_group_ok(h_terms, nterms)) {
    set_error("diag: not a Gibbs term");
    return -1;
  }
  hipLaunchKernelGGL(diag_gibbs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms, accumulate);
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// gradient contraction of up to GIBBS_GRAD_MAXT terms of one group, in grad_deriv_kernel's shape (deriv.hip): 128 x 128 tiles,
// thread = one row x 64 columns, per-workgroup partial sums reduced by a second kernel in a fixed order -- no atomics, the same
// bits on every call.
//   gc[t] = sum_ij G_ij rs_i cs_j k_t(i, j)           gs[t] = sum_ij G_ij coef_t rs_i cs_j (-2 s / q) k_t(i, j)
// (the input scale g multiplies the D location coordinates of both sides; the lengthscales stay as uploaded)
// ---------------------------------------------------------------------------------------
constexpr int GIBBS_GRAD_MAXT = 16;

template <int DMAX>
__global__ __launch_bounds__(256) void grad_gibbs_kernel(const double* Kinv, long ldk, const double* alpha, long r0, long nr,
                                                         long c0, long nc, const DevTerm* terms, int nterms, long tile_r_first,
                                                         long tile_c_first, double* partials /*[blocks][GIBBS_GRAD_MAXT][2]*/) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) double smem[];   // gibbs_stage's layout | reduction | term constants
  const double* sc = smem;
  const double* sr = sc + TILE * DMAX;
  const double* sl = sr + TILE * DMAX;
  double* red = smem + gibbs_lds_doubles(DMAX);               // [4 waves][GIBBS_GRAD_MAXT][2]
  double* scoef = red + 4 * GIBBS_GRAD_MAXT * 2;              // [GIBBS_GRAD_MAXT] the terms' coefficients
  int* spow = reinterpret_cast<int*>(scoef + GIBBS_GRAD_MAXT);   // [GIBBS_GRAD_MAXT] their p
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  TileClip cl;
  const bool live_tile = tile_clip(gtr, gtc, r0, nr, c0, nc, cl);
  if (!live_tile) cl.cbeg = cl.cend = cl.rbeg = cl.rend = 0;   // (nothing is read outside the pair; the partials are zeros)
  gibbs_stage<DMAX>(smem, terms[0], gtr, gtc, r0, c0, cl, t);
  if (t < GIBBS_GRAD_MAXT) {   // the terms' constants, read once and not per column
    scoef[t] = t < nterms ? terms[t].coef : 0.0;
    spow[t] = t < nterms ? (int)terms[t].param : 1;
  }
  __syncthreads();

  double gc_acc[GIBBS_GRAD_MAXT], gs_acc[GIBBS_GRAD_MAXT];
#pragma unroll
  for (int q = 0; q < GIBBS_GRAD_MAXT; ++q) gc_acc[q] = gs_acc[q] = 0.0;

  const long grow = gtr * TILE + trow;
  if (grow >= cl.rbeg && grow < cl.rend) {
    const double ai = alpha ? alpha[grow] : 0.0;
    const double rsv = sl[4 * TILE + trow];
    const double lx = sl[trow], lx2 = sl[TILE + trow];
    double xi[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xi[d] = sr[d * TILE + trow];
    for (int p = th * 64; p < th * 64 + 64; ++p) {
      const long gc = gtc * TILE + p;
      if (gc < cl.cbeg || gc >= cl.cend) continue;
      const double g = alpha ? 0.5 * (ai * alpha[gc] - Kinv[grow + gc * ldk]) : Kinv[grow + gc * ldk];
      const GibbsPair P = gibbs_pair(gibbs_dist<DMAX>(xi, sc + p * DMAX), lx, lx2, sl[2 * TILE + p], sl[3 * TILE + p]);
      const double w = g * rsv * sl[5 * TILE + p];
      const double m2t = P.dead ? 0.0 : -2.0 * P.t;
#pragma unroll
      for (int tm = 0; tm < GIBBS_GRAD_MAXT; ++tm) {
        if (tm < nterms) {   // (uniform; no break: the loop must unroll for the sums to stay in registers)
          const double k = gibbs_value(P, spow[tm]);
          gc_acc[tm] = fma(w, k, gc_acc[tm]);
          gs_acc[tm] = fma(w * scoef[tm], m2t * k, gs_acc[tm]);
        }
      }
    }
  }
  // block reduction (fixed order): wave shuffle, then the 4 waves' sums through LDS
#pragma unroll
  for (int tm = 0; tm < GIBBS_GRAD_MAXT; ++tm) {
    double a = gc_acc[tm], b = gs_acc[tm];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off, 64);
      b += __shfl_xor(b, off, 64);
    }
    if ((t & 63) == 0) {
      red[((t >> 6) * GIBBS_GRAD_MAXT + tm) * 2 + 0] = a;
      red[((t >> 6) * GIBBS_GRAD_MAXT + tm) * 2 + 1] = b;
    }
  }
  __syncthreads();
  if (t < GIBBS_GRAD_MAXT * 2) {
    double s = 0.0;
    for (int wv = 0; wv < 4; ++wv) s += red[wv * GIBBS_GRAD_MAXT * 2 + t];
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * GIBBS_GRAD_MAXT * 2 + t] = s;
  }
}

// out[term] = sum_b partials[b][term][component]: one workgroup per output, 256 strided sums combined by a fixed tree
__global__ __launch_bounds__(256) void grad_gibbs_reduce_kernel(const double* partials, long nblocks, double* out_coef,
                                                                double* out_scale) {
  __shared__ double sh[256];
  const int idx = blockIdx.x;   // term * 2 + component
  double s = 0.0;
  for (long b = threadIdx.x; b < nblocks; b += 256) s += partials[b * GIBBS_GRAD_MAXT * 2 + idx];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* dst = (idx & 1) ? out_scale + (idx >> 1) : out_coef + (idx >> 1);
    *dst = sh[0];
  }
}

long grad_gibbs_partials(long trc, long tcc) { return std::max<long>(1, trc * tcc) * GIBBS_GRAD_MAXT * 2; }

// One group (nterms terms at h_terms / d_terms): out_coef / out_scale point at the group's first entry; partials:
// grad_gibbs_partials(trc, tcc) doubles.  A group of more than GIBBS_GRAD_MAXT terms takes several launches.
int launch_grad_gibbs(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                      const DevTerm* h_terms, const DevTerm* d_terms, int nterms, long trf, long tcf, long trc, long tcc,
                      double* partials, double* out_coef, double* out_scale, hipStream_t s) {
  if (nterms <= 0 || trc <= 0 || tcc <= 0) return 0;
  if (!gibbs_group_ok(h_terms, nterms)) {
    set_error("grad: not a Gibbs term");
    return -1;
  }
  const int dmax = gibbs_dmax_class(h_terms[0].dim);
  const size_t lds = sizeof(double) * (gibbs_lds_doubles(dmax) + 4 * GIBBS_GRAD_MAXT * 2 + GIBBS_GRAD_MAXT) +
                     sizeof(int) * GIBBS_GRAD_MAXT;
  const dim3 grid((unsigned)trc, (unsigned)tcc);
  for (int t = 0; t < nterms; t += GIBBS_GRAD_MAXT) {
    const int cnt = std::min(GIBBS_GRAD_MAXT, nterms - t);
#define SGP_GG(DM)                                                                                                       \
  hipLaunchKernelGGL((grad_gibbs_kernel<DM>), grid, dim3(256), lds, s, Kinv, ldk, alpha, r0, nr, c0, nc, d_terms + t, cnt, trf, \
                     tcf, partials)
    if (dmax <= 2) SGP_GG(2);
    else if (dmax <= 4) SGP_GG(4);
    else if (dmax <= 8) SGP_GG(8);
    else SGP_GG(16);
#undef SGP_GG
    SGP_HIP(hipGetLastError());
    hipLaunchKernelGGL(grad_gibbs_reduce_kernel, dim3((unsigned)(cnt * 2)), dim3(256), 0, s, partials, trc * tcc, out_coef + t,
                       out_scale + t);
    SGP_HIP(hipGetLastError());
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// input points of one group, in grad_inputs_kernel's shape (grad.hip): one workgroup per 128 rows of the side `T` names as its
// row side, thread = one row x half of every column tile, the column tile's points in LDS, the two halves combined in a fixed
// order; every column of gx is written by one thread.  With A = sum_t coef_t k_t and Bh = sum_t coef_t (p_t / 2) k_t:
//   gx[d, i] += scale sum_j G_ij rs_i cs_j A (-2 (x_i - y_j)[d] / q)                       d < D
//   gx[D, i] += scale sum_j G_ij rs_i cs_j (Bh (1 / lx - 2 lx / q) + A 2 s lx / q^2)
// G(i, j) at Gm[(r0 + i) sr + (c0 + j) sc]: (1, ld) for the matrix as stored, (ld, 1) for its transpose (the column side: the
// caller hands in the term with its sides swapped; the kind is symmetric in its two points).
// ---------------------------------------------------------------------------------------
template <int DMAX>
__global__ __launch_bounds__(256) void grad_gibbs_inputs_kernel(const double* Gm, long sr, long sc, const double* alpha, long r0,
                                                                long nr, long c0, long nc, DevTerm T,
                                                                const DevTerm* terms /* (coef, p) of the group */, int nterms,
                                                                double scale, double* gx /* T.dim x nr, packed */) {
  __shared__ double sx[TILE * DMAX];
  __shared__ double slc[3 * TILE];   // lc | lc2 | cs of the column tile
  __shared__ double comb[TILE * DMAX];
  const int D = T.dim - 1;
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  const long lrow = (long)blockIdx.x * TILE + trow;   // row within the block
  const bool live = lrow < nr;
  const long grow = r0 + lrow;
  double xr[DMAX], acc[DMAX];
  double accl = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    xr[d] = (live && d < D) ? T.xr[lrow * T.ldr + d] : 0.0;
    acc[d] = 0.0;
  }
  const double lx = live ? T.xr[lrow * T.ldr + D] : 1.0;
  const double lx2 = lx * lx, rlx = 1.0 / lx;
  const double ai = (alpha && live) ? alpha[grow] : 0.0;
  const double wrow = live ? (T.rs ? T.rs[lrow] : 1.0) : 0.0;
  for (long ct = 0; ct * TILE < nc; ++ct) {
    __syncthreads();
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long lc = ct * TILE + p;
      sx[idx] = (lc < nc && d < D) ? T.xc[lc * T.ldc + d] : 0.0;
    }
    if (t < TILE) {
      const long lc = ct * TILE + t;
      const double l = lc < nc ? T.xc[lc * T.ldc + D] : 1.0;
      slc[t] = l, slc[TILE + t] = l * l;
      slc[2 * TILE + t] = lc < nc ? (T.cs ? T.cs[lc] : 1.0) : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int p = th * 64; p < th * 64 + 64; ++p) {
        const long lc = ct * TILE + p;
        if (lc >= nc) break;
        const long gc = c0 + lc;
        const double gm = Gm[grow * sr + gc * sc];
        const double g = alpha ? 0.5 * (ai * alpha[gc] - gm) : gm;
        double df[DMAX], s = 0.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          df[d] = xr[d] - sx[p * DMAX + d];
          s = fma(df[d], df[d], s);
        }
        const GibbsPair P = gibbs_pair(s, lx, lx2, slc[p], slc[TILE + p]);
        double A = 0.0, Bh = 0.0;
        for (int tm = 0; tm < nterms; ++tm) {
          const double ck = terms[tm].coef * gibbs_value(P, (int)terms[tm].param);
          A += ck;
          Bh = fma(0.5 * terms[tm].param, ck, Bh);
        }
        const double w = g * wrow * slc[2 * TILE + p];
        const double wx = P.dead ? 0.0 : w * A * (-2.0 * P.rq);
#pragma unroll
        for (int d = 0; d < DMAX; ++d) acc[d] = fma(wx, df[d], acc[d]);
        accl = fma(w, P.dead ? 0.0 : gibbs_dl(P, A, Bh, lx, rlx), accl);
      }
    }
  }
  // combine the two column halves in fixed order, then add into the input's gradient
  __syncthreads();
  if (th == 1) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) comb[trow * DMAX + d] = acc[d];
    slc[trow] = accl;   // the column tile is no longer needed
  }
  __syncthreads();
  if (th == 0 && live) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
      if (d < D) gx[lrow * T.dim + d] += scale * (acc[d] + comb[trow * DMAX + d]);
    gx[lrow * T.dim + D] += scale * (accl + slc[trow]);
  }
}

// T: the group's first term as the side to differentiate sees it (host copy, sides swapped for the column side); d_terms: the
// group on the device, read for (coef, p) alone
int launch_grad_gibbs_inputs(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                             const DevTerm& T, const DevTerm* d_terms, int nterms, double scale, double* gx, hipStream_t s) {
  if (nr <= 0 || nc <= 0 || nterms <= 0 || !gx) return 0;
  if (!gibbs_group_ok(&T, nterms)) {
    set_error("grad inputs: not a Gibbs term");
    return -1;
  }
  const int dmax = gibbs_dmax_class(T.dim);
  const dim3 grid((unsigned)((nr + TILE - 1) / TILE)), block(256);
#define SGP_GI(DM) \
  hipLaunchKernelGGL((grad_gibbs_inputs_kernel<DM>), grid, block, 0, s, Gm, sr, sc, alpha, r0, nr, c0, nc, T, d_terms, nterms, scale, gx)
  if (dmax <= 2) SGP_GI(2);
  else if (dmax <= 4) SGP_GI(4);
  else if (dmax <= 8) SGP_GI(8);
  else SGP_GI(16);
#undef SGP_GI
  SGP_HIP(hipGetLastError());
  return 0;
}

}  // namespace sgp
