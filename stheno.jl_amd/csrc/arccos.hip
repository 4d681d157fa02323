// Arc-cosine terms (include/sthenomi.h: SGP_NNGP, SGP_NTK): the covariance of a depth-L ReLU network and its tangent kernel,
//   K_ij = coef rs_i cs_j n_x n_y T(c_0),   T = c_L (NNGP) or t_L (NTK),   L = param
// (arccos_eval.h: the recursion, carried in the half angle; arccos_kinds.h: the validation table).  Per-entry arithmetic: one
// atan2, then L layer steps of one sincos, one square root and one asin each -- the assembly is bound by its arithmetic, not by
// its stores, the reverse of the other kinds.
//
// A term class of its own, as the additive and blur kinds are.  The terms of one block pair that share points, scale vectors
// and dimension and whose depths do not decrease form a GROUP (arccos_kinds.h: arccos_group); they differ in (kind, coef, L).
// A launch carries one group: the recursion runs ONCE per point pair to the group's last depth, and every term reads its c_L
// or t_L when the layer loop passes its depth, in the caller's order.  A model that sums depths 1 .. L, or NNGP + NTK, is one
// launch.
//
// Per-point work is hoisted: a tile stages the norm and the UNIT VECTOR of its 128 row and 128 column points once (D
// divisions per point, none per pair); the pair loop reads unit vectors only.  The layer loop holds h, t and the accumulator
// per pair (the input-point kernel: c' and t' too) and no per-layer table: nothing reaches scratch.
//
// Tiling of the matrix kernel: the assembly frame's two-row form (asm_frame.h) -- 128 x 128 tiles of the global grid, one
// 256-thread workgroup per tile, thread (lane, wave) owns rows 2 lane, 2 lane + 1 and the 32 columns of quarter `wave`, 16-byte
// stores on interior tiles; a pass covers ACC columns x 2 rows, 2 ACC independent recursions.  LDS, staged once per tile:
//   [128][DMAX] column unit vectors | [DMAX][128] row unit vectors | rs | cs | row norms | column norms     (128 doubles each)
// Padding coordinates and points outside the clip hold unit vector 0, norm 0, scale 0.
#include "arccos_eval.h"
#include "arccos_kinds.h"
#include "asm_frame.h"
#include <algorithm>

namespace sgp {

constexpr int ACC = 2;         // columns per pass of the matrix kernel
constexpr int ARCCOS_GT = 4;   // terms per launch of the gradient contraction: one sum each, in registers

__host__ __device__ constexpr int arccos_lds_doubles(int dmax) { return 2 * TILE * dmax + 4 * TILE; }

// the tile's points: norms and scales first (one point per thread), then the unit vectors.  Ends behind its own barrier for
// the norms; the caller places the one for the unit vectors
template <int DMAX>
__device__ __forceinline__ void arccos_stage(double* smem, const DevTerm& T, long gtr, long gtc, long r0, long c0,
                                             const TileClip& cl, int t) {
  const int D = T.dim;
  double* uc = smem;
  double* ur = uc + TILE * DMAX;
  double* sl = ur + TILE * DMAX;   // rs | cs | row norms | column norms
  if (t < TILE) {
    const long gr = gtr * TILE + t;
    const bool in = gr >= cl.rbeg && gr < cl.rend;
    sl[t] = in ? (T.rs ? T.rs[gr - r0] : 1.0) : 0.0;
    sl[2 * TILE + t] = in ? arccos_norm(T.xr + (gr - r0) * T.ldr, D) : 0.0;
  } else {
    const int p = t - TILE;
    const long gc = gtc * TILE + p;
    const bool in = gc >= cl.cbeg && gc < cl.cend;
    sl[TILE + p] = in ? (T.cs ? T.cs[gc - c0] : 1.0) : 0.0;
    sl[3 * TILE + p] = in ? arccos_norm(T.xc + (gc - c0) * T.ldc, D) : 0.0;
  }
  __syncthreads();
  for (int idx = t; idx < TILE * DMAX; idx += 256) {
    const int p = idx / DMAX, d = idx % DMAX;
    const long gc = gtc * TILE + p, gr = gtr * TILE + p;
    const bool cin = d < D && gc >= cl.cbeg && gc < cl.cend, rin = d < D && gr >= cl.rbeg && gr < cl.rend;
    uc[idx] = cin ? arccos_unit(T.xc[(gc - c0) * T.ldc + d], sl[3 * TILE + p]) : 0.0;
    ur[d * TILE + p] = rin ? arccos_unit(T.xr[(gr - r0) * T.ldr + d], sl[2 * TILE + p]) : 0.0;
  }
}

template <int DMAX>
__global__ __launch_bounds__(256) void assemble_arccos_kernel(
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

  const double* uc = smem;
  const double* ur = uc + TILE * DMAX;
  const double* sl = ur + TILE * DMAX;
  arccos_stage<DMAX>(smem, terms[0], gtr, gtc, r0, c0, cl, t);
  __syncthreads();

  const PairRows R = pair_rows(K, ld, gtr, gtc, lane, cl, accumulate, noise_kind, sigma2, noise_diag);
  const double2 rs = *reinterpret_cast<const double2*>(sl + 2 * lane);
  const double2 nrow = *reinterpret_cast<const double2*>(sl + 2 * TILE + 2 * lane);
  const int L = (int)terms[nterms - 1].param;   // the group's depths do not decrease

  for (int jc = 0; jc < 32; jc += ACC) {
    const int pbase = wv * 32 + jc;
    // once per point pair: the half angle from the staged unit vectors
    double a0[ACC], b0[ACC], a1[ACC], b1[ACC];
#pragma unroll
    for (int q = 0; q < ACC; ++q) a0[q] = b0[q] = a1[q] = b1[q] = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      const double2 x2 = *reinterpret_cast<const double2*>(ur + d * TILE + 2 * lane);
#pragma unroll
      for (int q = 0; q < ACC; ++q) {
        const double y = uc[(pbase + q) * DMAX + d];
        arccos_step(x2.x, y, a0[q], b0[q]);
        arccos_step(x2.y, y, a1[q], b1[q]);
      }
    }
    double h0[ACC], h1[ACC], t0[ACC], t1[ACC], acc0[ACC], acc1[ACC];
#pragma unroll
    for (int q = 0; q < ACC; ++q) {
      h0[q] = arccos_half_angle(a0[q], b0[q]);
      h1[q] = arccos_half_angle(a1[q], b1[q]);
      t0[q] = t1[q] = acc0[q] = acc1[q] = 0.0;
    }
    // the hot loop: L layers, 2 ACC independent recursions; the terms whose depth it passes read their value
    int tm = 0;
    for (int l = 0; l < L; ++l) {
      double c0v[ACC], c1v[ACC];
#pragma unroll
      for (int q = 0; q < ACC; ++q) {
        const ArccosLayer y0 = arccos_layer(h0[q]), y1 = arccos_layer(h1[q]);
        if (l == 0) t0[q] = 1.0 - y0.A, t1[q] = 1.0 - y1.A;   // t_0 = c_0
        t0[q] = fma(t0[q], y0.k0, y0.c);
        t1[q] = fma(t1[q], y1.k0, y1.c);
        c0v[q] = y0.c, c1v[q] = y1.c;
      }
      for (; tm < nterms && (int)terms[tm].param == l + 1; ++tm) {   // (kind, coef): wave-uniform scalars
        const bool ntk = (terms[tm].kind & 0xff) == SGP_NTK;
        const double coef = terms[tm].coef;
        const double w0 = coef * rs.x, w1 = coef * rs.y;
#pragma unroll
        for (int q = 0; q < ACC; ++q) {
          const double cq = sl[TILE + pbase + q], ncol = sl[3 * TILE + pbase + q];
          acc0[q] = fma((nrow.x * ncol) * (ntk ? t0[q] : c0v[q]), w0 * cq, acc0[q]);
          acc1[q] = fma((nrow.y * ncol) * (ntk ? t1[q] : c1v[q]), w1 * cq, acc1[q]);
        }
      }
    }
    store_pair_tail<ACC>(K, ld, gtc * TILE + pbase, cl, R, acc0, acc1, accumulate);
  }
}

static bool arccos_group_ok(const DevTerm* h_terms, int nterms) {
  if (nterms <= 0) return false;
  for (int t = 0; t < nterms; ++t)
    if (!arccos_kind_known(h_terms[t].kind & 0xff) || arccos_param_refusal(h_terms[t].param, h_terms[t].dim) ||
        (t > 0 && h_terms[t].param < h_terms[t - 1].param))
      return false;
  return true;
}

// CALL(DMAX) for the class of the points' dimension
#define SGP_ARCCOS_DISPATCH(dmax, CALL) \
  do {                                  \
    if ((dmax) <= 2) CALL(2);           \
    else if ((dmax) <= 4) CALL(4);      \
    else if ((dmax) <= 8) CALL(8);      \
    else CALL(16);                      \
  } while (0)

// One group of one block pair (h_terms: host copies, d_terms: the same on the device)
int launch_assemble_arccos(const AsmLaunch& L, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, hipStream_t s) {
  if (nterms <= 0 || L.empty()) return 0;
  if (!arccos_group_ok(h_terms, nterms)) {
    set_error("assemble: not an arc-cosine term");
    return -1;
  }
  const int dmax = arccos_dmax_class(h_terms[0].dim);
  const size_t lds = sizeof(double) * arccos_lds_doubles(dmax);
  const dim3 grid((unsigned)L.r_cnt, (unsigned)L.c_cnt);
#define SGP_NA(DM)                                                                                                          \
  hipLaunchKernelGGL((assemble_arccos_kernel<DM>), grid, dim3(256), lds, s, L.K, L.ld, L.r0, L.nr, L.c0, L.nc, d_terms, nterms, \
                     ASM_TAIL(L), L.r_first, L.c_first)
  SGP_ARCCOS_DISPATCH(dmax, SGP_NA);
#undef SGP_NA
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// diagonal of one group: out[i] = (accumulate ? out[i] : 0) + sum_t n_i n_i T_t(i, i) (coef_t rs_i) cs_i, every operation in
// the order of the matrix kernel (over the D coordinates alone: the matrix kernel's padding adds exact zeros)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void diag_arccos_kernel(double* out, long n, const DevTerm* terms, int nterms, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevTerm T = terms[0];
  const double acc = arccos_pair_sum(T.xr + i * T.ldr, T.xc + i * T.ldc, T.dim, terms, nterms, T.rs ? T.rs[i] : 1.0,
                                     T.cs ? T.cs[i] : 1.0);
  out[i] = accumulate ? out[i] + acc : acc;
}

int launch_diag_arccos(double* out, long n, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int accumulate,
                       hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  if (!arccos_group_ok(h_terms, nterms)) {
    set_error("diag: not an arc-cosine term");
    return -1;
  }
  hipLaunchKernelGGL(diag_arccos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms, accumulate);
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// gradient contraction of one group, in grad_blur_kernel's shape: 128 x 128 tiles, thread = one row x 64 columns, per-workgroup
// partial sums reduced by a second kernel in a fixed order -- no atomics, the same bits on every call.  K is linear in coef and
// homogeneous of degree 2 in a common scale g of both inputs, so ONE sum serves a term,
//   S_t = sum_ij G_ij rs_i cs_j n_i n_j T_t(i, j)        gc[t] = S_t        gs[t] = 2 coef_t S_t
// A launch carries up to ARCCOS_GT terms of the group -- one sum each, in registers -- and runs the recursion once per pair to
// the last of their depths.
// ---------------------------------------------------------------------------------------
template <int DMAX>
__global__ __launch_bounds__(256) void grad_arccos_kernel(const double* Kinv, long ldk, const double* alpha, long r0, long nr,
                                                          long c0, long nc, const DevTerm* terms, int nterms, long tile_r_first,
                                                          long tile_c_first, double* partials /*[blocks][ARCCOS_GT]*/) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) double smem[];   // arccos_stage's layout | reduction
  const double* uc = smem;
  const double* ur = uc + TILE * DMAX;
  const double* sl = ur + TILE * DMAX;
  double* red = smem + arccos_lds_doubles(DMAX);   // [4 waves][ARCCOS_GT]
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  TileClip cl;
  const bool live_tile = tile_clip(gtr, gtc, r0, nr, c0, nc, cl);
  if (!live_tile) cl.cbeg = cl.cend = cl.rbeg = cl.rend = 0;   // (nothing is read outside the pair; the partials are zeros)
  arccos_stage<DMAX>(smem, terms[0], gtr, gtc, r0, c0, cl, t);
  __syncthreads();

  int dep[ARCCOS_GT];
  bool ntk[ARCCOS_GT];
  double S[ARCCOS_GT];
#pragma unroll
  for (int k = 0; k < ARCCOS_GT; ++k) {
    dep[k] = k < nterms ? (int)terms[k].param : 0;
    ntk[k] = k < nterms && (terms[k].kind & 0xff) == SGP_NTK;
    S[k] = 0.0;
  }
  const int L = (int)terms[nterms - 1].param;

  const long grow = gtr * TILE + trow;
  if (grow >= cl.rbeg && grow < cl.rend) {
    const double ai = alpha ? alpha[grow] : 0.0;
    const double wr = sl[trow] * sl[2 * TILE + trow];   // rs_i n_i
    double xi[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xi[d] = ur[d * TILE + trow];
    for (int p = th * 64; p < th * 64 + 64; ++p) {
      const long gc = gtc * TILE + p;
      if (gc < cl.cbeg || gc >= cl.cend) continue;
      const double g = alpha ? 0.5 * (ai * alpha[gc] - Kinv[grow + gc * ldk]) : Kinv[grow + gc * ldk];
      double a2 = 0.0, b2 = 0.0;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) arccos_step(xi[d], uc[p * DMAX + d], a2, b2);
      double h = arccos_half_angle(a2, b2), tt = 0.0;
      const double w = g * wr * (sl[TILE + p] * sl[3 * TILE + p]);
      for (int l = 0; l < L; ++l) {
        const ArccosLayer y = arccos_layer(h);
        if (l == 0) tt = 1.0 - y.A;
        tt = fma(tt, y.k0, y.c);
#pragma unroll
        for (int k = 0; k < ARCCOS_GT; ++k)
          if (dep[k] == l + 1) S[k] = fma(w, ntk[k] ? tt : y.c, S[k]);
      }
    }
  }
  // block reduction (fixed order): wave shuffle, then the 4 waves' sums through LDS
#pragma unroll
  for (int k = 0; k < ARCCOS_GT; ++k) {
    double a = S[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
    if ((t & 63) == 0) red[(t >> 6) * ARCCOS_GT + k] = a;
  }
  __syncthreads();
  if (t < ARCCOS_GT) {
    double s = 0.0;
    for (int wv = 0; wv < 4; ++wv) s += red[wv * ARCCOS_GT + t];
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * ARCCOS_GT + t] = s;
  }
}

// out_coef[k] = S_k, out_scale[k] = 2 coef_k S_k with S_k = sum_b partials[b][k]: one workgroup, 256 strided sums combined by a
// fixed tree
__global__ __launch_bounds__(256) void grad_arccos_reduce_kernel(const double* partials, long nblocks, const DevTerm* terms,
                                                                 int nterms, double* out_coef, double* out_scale) {
  __shared__ double sh[ARCCOS_GT][256];
  double a[ARCCOS_GT];
#pragma unroll
  for (int k = 0; k < ARCCOS_GT; ++k) a[k] = 0.0;
  for (long b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
    for (int k = 0; k < ARCCOS_GT; ++k) a[k] += partials[b * ARCCOS_GT + k];
#pragma unroll
  for (int k = 0; k < ARCCOS_GT; ++k) sh[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off)
#pragma unroll
      for (int k = 0; k < ARCCOS_GT; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
    __syncthreads();
  }
  if ((int)threadIdx.x < nterms) {
    out_coef[threadIdx.x] = sh[threadIdx.x][0];
    out_scale[threadIdx.x] = (2.0 * terms[threadIdx.x].coef) * sh[threadIdx.x][0];
  }
}

long grad_arccos_partials(long trc, long tcc) { return std::max<long>(1, trc * tcc) * ARCCOS_GT; }

// One group (nterms terms at h_terms / d_terms): out_coef / out_scale point at the group's first entry; partials:
// grad_arccos_partials(trc, tcc) doubles, used by one chunk of ARCCOS_GT terms after the other on the stream
int launch_grad_arccos(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                       const DevTerm* h_terms, const DevTerm* d_terms, int nterms, long trf, long tcf, long trc, long tcc,
                       double* partials, double* out_coef, double* out_scale, hipStream_t s) {
  if (nterms <= 0 || trc <= 0 || tcc <= 0) return 0;
  if (!arccos_group_ok(h_terms, nterms)) {
    set_error("grad: not an arc-cosine term");
    return -1;
  }
  const int dmax = arccos_dmax_class(h_terms[0].dim);
  const size_t lds = sizeof(double) * (arccos_lds_doubles(dmax) + 4 * ARCCOS_GT);
  const dim3 grid((unsigned)trc, (unsigned)tcc);
  for (int t = 0; t < nterms; t += ARCCOS_GT) {
    const int cnt = std::min(ARCCOS_GT, nterms - t);
#define SGP_NG(DM)                                                                                                          \
  hipLaunchKernelGGL((grad_arccos_kernel<DM>), grid, dim3(256), lds, s, Kinv, ldk, alpha, r0, nr, c0, nc, d_terms + t, cnt, trf, \
                     tcf, partials)
    SGP_ARCCOS_DISPATCH(dmax, SGP_NG);
#undef SGP_NG
    SGP_HIP(hipGetLastError());
    hipLaunchKernelGGL(grad_arccos_reduce_kernel, dim3(1), dim3(256), 0, s, partials, trc * tcc, d_terms + t, cnt, out_coef + t,
                       out_scale + t);
    SGP_HIP(hipGetLastError());
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// input points of one group, in grad_blur_inputs_kernel's shape: one workgroup per 128 rows of the side `T` names as its row
// side, thread = one row x half of every column tile, the column tile's unit vectors and norms in LDS, the two halves combined
// in a fixed order; every column of gx is written by one thread.  With T' = dT / dc_0 by the forward recursion
//   c'_{l+1} = kappa_0 c'_l,   t'_{l+1} = c'_{l+1} + t'_l kappa_0 + t_l c'_l / (pi sin theta_l),   c'_0 = t'_0 = 1
// and P = sum_t coef_t T_t, Q = sum_t coef_t T'_t over the group (ONE recursion per pair),
//   gx[d, i] += scale sum_j G_ij rs_i cs_j n_j [ P xh_d + Q (yh_d - c_0 xh_d) ]
// The tangential part yh - c_0 xh is formed from the unit vectors, (yh - xh) + (1 - c_0) xh for c_0 >= 0 and
// (yh + xh) - (1 + c_0) xh otherwise: near-parallel points have Q of order 1 / theta against a tangent of order theta.  The NTK
// is not differentiable where sin theta_l = 0 (theta_0 = 0, or an exactly antipodal pair at l = 0); the 1 / sin term counts 0.
// G(i, j) at Gm[(r0 + i) sr + (c0 + j) sc]: (1, ld) for the matrix as stored, (ld, 1) for its transpose (the column side: the
// caller hands in the term with its sides swapped; the kinds are symmetric in their two points).
// ---------------------------------------------------------------------------------------
template <int DMAX>
__global__ __launch_bounds__(256) void grad_arccos_inputs_kernel(const double* Gm, long sr, long sc, const double* alpha, long r0,
                                                                 long nr, long c0, long nc, DevTerm T,
                                                                 const DevTerm* terms /* (kind, coef, L) of the group */,
                                                                 int nterms, double scale, double* gx /* T.dim x nr, packed */) {
  __shared__ double sy[TILE * DMAX];   // the column tile's unit vectors
  __shared__ double scs[TILE];         // ... scales times norms
  __shared__ double sny[TILE];         // ... norms
  __shared__ double comb[TILE * DMAX];
  const int D = T.dim;
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  const long lrow = (long)blockIdx.x * TILE + trow;   // row within the block
  const bool live = lrow < nr;
  const long grow = r0 + lrow;
  const double nx = live ? arccos_norm(T.xr + lrow * T.ldr, D) : 0.0;
  double xh[DMAX], acc[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    xh[d] = (live && d < D) ? arccos_unit(T.xr[lrow * T.ldr + d], nx) : 0.0;
    acc[d] = 0.0;
  }
  const int L = (int)terms[nterms - 1].param;
  const double ai = (alpha && live) ? alpha[grow] : 0.0;
  const double wrow = live ? (T.rs ? T.rs[lrow] : 1.0) : 0.0;
  for (long ct = 0; ct * TILE < nc; ++ct) {
    __syncthreads();
    if (t < TILE) {
      const long lc = ct * TILE + t;
      const double ny = lc < nc ? arccos_norm(T.xc + lc * T.ldc, D) : 0.0;
      sny[t] = ny;
      scs[t] = lc < nc ? (T.cs ? T.cs[lc] : 1.0) * ny : 0.0;
    }
    __syncthreads();
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long lc = ct * TILE + p;
      sy[idx] = (lc < nc && d < D) ? arccos_unit(T.xc[lc * T.ldc + d], sny[p]) : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int p = th * 64; p < th * 64 + 64; ++p) {
        const long lc = ct * TILE + p;
        if (lc >= nc) break;
        const long gc = c0 + lc;
        const double gm = Gm[grow * sr + gc * sc];
        const double g = alpha ? 0.5 * (ai * alpha[gc] - gm) : gm;
        double a2 = 0.0, b2 = 0.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) arccos_step(xh[d], sy[p * DMAX + d], a2, b2);
        double h = arccos_half_angle(a2, b2);
        double tt = 0.0, cp = 1.0, tp = 1.0, P = 0.0, Q = 0.0, A0 = 0.0, B0 = 2.0;
        int tm = 0;
        for (int l = 0; l < L; ++l) {
          const ArccosLayer y = arccos_layer(h);
          if (l == 0) tt = 1.0 - y.A, A0 = y.A, B0 = y.B;
          const double inv = (y.st > 0.0 && !(l == 0 && b2 == 0.0)) ? ARCCOS_INV_PI / y.st : 0.0;
          const double cpn = y.k0 * cp;
          tp = fma(tp, y.k0, cpn) + (tt * cp) * inv;
          tt = fma(tt, y.k0, y.c);
          cp = cpn;
          for (; tm < nterms && (int)terms[tm].param == l + 1; ++tm) {
            const bool ntk = (terms[tm].kind & 0xff) == SGP_NTK;
            P = fma(terms[tm].coef, ntk ? tt : y.c, P);
            Q = fma(terms[tm].coef, ntk ? tp : cp, Q);
          }
        }
        const double wk = g * wrow * scs[p];
        const bool acute = A0 <= 1.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          const double yh = sy[p * DMAX + d];
          const double tang = acute ? fma(A0, xh[d], yh - xh[d]) : fma(-B0, xh[d], yh + xh[d]);
          acc[d] = fma(wk, fma(Q, tang, P * xh[d]), acc[d]);
        }
      }
    }
  }
  // combine the two column halves in fixed order, then add into the input's gradient
  __syncthreads();
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
// d_terms: the group on the host and on the device, read for (kind, coef, L) alone
int launch_grad_arccos_inputs(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                              const DevTerm& T, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, double scale,
                              double* gx, hipStream_t s) {
  if (nr <= 0 || nc <= 0 || nterms <= 0 || !gx) return 0;
  if (!arccos_group_ok(h_terms, nterms) || T.dim != h_terms[0].dim) {
    set_error("grad inputs: not an arc-cosine term");
    return -1;
  }
  const int dmax = arccos_dmax_class(T.dim);
  const dim3 grid((unsigned)((nr + TILE - 1) / TILE)), block(256);
#define SGP_NI(DM) \
  hipLaunchKernelGGL((grad_arccos_inputs_kernel<DM>), grid, block, 0, s, Gm, sr, sc, alpha, r0, nr, c0, nc, T, d_terms, nterms, scale, gx)
  SGP_ARCCOS_DISPATCH(dmax, SGP_NI);
#undef SGP_NI
  SGP_HIP(hipGetLastError());
  return 0;
}

}  // namespace sgp
