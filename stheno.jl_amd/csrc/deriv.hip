// Derivative-process terms (include/sthenomi.h: SGP_DERIV_SE, SGP_DERIV_MATERN32, SGP_DERIV_MATERN52): the covariances of f
// and its partial derivatives for a stationary kernel k = kappa(|x - y|^2), in closed form per pair of points -- kappa' and
// kappa'' times coordinate differences (deriv_eval.h).  On the reference path this is the finite-difference derivative(f) of
// examples/differentiation/script.jl, "a template on which others could build".
//
// A term class of its own: the plain kernels' KIND switch and the product path's table do not know these kinds.
// The terms of one block pair that share base kind, inputs and scale vectors form a GROUP (deriv_kinds.h: deriv_group): the
// block of a gradient-observation model at D = 3 holds up to 9 two-sided terms on the same points.  A launch carries one
// group; exp, kappa' and kappa'' are evaluated ONCE per point pair and feed every (a, b) of the group.
//
// Tiling of the matrix kernel: that of assemble_block2_kernel (kernelmatrix.hip) -- 128 x 128 tiles of the global grid, one
// 256-thread workgroup per tile, thread (lane, wave) owns rows 2 lane, 2 lane + 1 and the 32 columns of quarter `wave`;
// column points [point][DMAX], row points [d][row], row and column scales staged in LDS once per tile; 16-byte stores on
// interior tiles.  The coordinate differences u_p of a term are re-formed from the staged points (an LDS address, not a
// register index: no scratch), by the very subtraction the distance used.
#include "common.h"
#include "deriv_eval.h"
#include "deriv_kinds.h"
#include <algorithm>

namespace sgp {

constexpr int DCC = 4;   // columns per chunk (x 2 rows = 8 independent exp chains), as CC2 of the plain kernel

__host__ __device__ constexpr int deriv_lds_doubles(int dmax) { return 2 * TILE * dmax + 2 * TILE; }

// s = sum_d (xi_d - c_d)^2, d ascending, fma -- the plain kernels' distance; Matern-3/2 below DERIV_TINY_S: the same sum of the
// differences scaled by DERIV_UP
template <int DMAX, int BASE>
__device__ __forceinline__ void deriv_dist(const double (&xi)[DMAX], const double* c, double& s, double& sr, bool& up) {
  s = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = xi[d] - c[d];
    s = fma(df, df, s);
  }
  sr = s, up = false;
  if (BASE == K_M32 && s < DERIV_TINY_S) {
    sr = 0.0, up = true;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      const double df = (xi[d] - c[d]) * DERIV_UP;
      sr = fma(df, df, sr);
    }
  }
}

template <int DMAX, int BASE>
__global__ __launch_bounds__(256) void assemble_deriv_kernel(
    double* __restrict__ K, long ld, long r0, long nr, long c0, long nc, const DevTerm* __restrict__ terms, int nterms,
    int lower_only, int accumulate, int noise_kind, double sigma2, const double* __restrict__ noise_diag, long tile_r_first,
    long tile_c_first) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  if (lower_only && gtr < gtc) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];   // [128][DMAX] cols | [DMAX][128] rows | rs[128] | cs[128]
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;

  long cbeg = gtc * TILE, cend = cbeg + TILE;
  if (cbeg < c0) cbeg = c0;
  if (cend > c0 + nc) cend = c0 + nc;
  long rbeg = gtr * TILE, rend = rbeg + TILE;
  if (rbeg < r0) rbeg = r0;
  if (rend > r0 + nr) rend = r0 + nr;
  if (cbeg >= cend || rbeg >= rend) return;   // uniform over the workgroup

  double* sc = smem;
  double* sr = sc + TILE * DMAX;
  double* srw = sr + TILE * DMAX;
  double* scw = srw + TILE;
  {
    const DevTerm T = terms[0];   // the group's points and scales
    const int D = T.dim;
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long gc = gtc * TILE + p, gr = gtr * TILE + p;
      sc[idx] = (d < D && gc >= cbeg && gc < cend) ? T.xc[(gc - c0) * T.ldc + d] : 0.0;
      sr[d * TILE + p] = (d < D && gr >= rbeg && gr < rend) ? T.xr[(gr - r0) * T.ldr + d] : 0.0;
    }
    if (t < TILE) {
      const long gr = gtr * TILE + t;
      srw[t] = (gr >= rbeg && gr < rend) ? (T.rs ? T.rs[gr - r0] : 1.0) : 0.0;
    } else {
      const int p = t - TILE;
      const long gc = gtc * TILE + p;
      scw[p] = (gc >= cbeg && gc < cend) ? (T.cs ? T.cs[gc - c0] : 1.0) : 0.0;
    }
  }
  __syncthreads();

  const long g0 = gtr * TILE + 2 * lane, g1 = g0 + 1;
  const bool ok0 = g0 >= rbeg && g0 < rend, ok1 = g1 >= rbeg && g1 < rend;
  const bool diag_noise = noise_kind >= 0 && gtr == gtc;
  double nv0 = 0.0, nv1 = 0.0;
  if (diag_noise) {
    nv0 = (noise_kind == 0) ? sigma2 : (ok0 ? noise_diag[g0] : 0.0);
    nv1 = (noise_kind == 0) ? sigma2 : (ok1 ? noise_diag[g1] : 0.0);
  }
  const bool full = (cend - cbeg == TILE) && (rend - rbeg == TILE) && !accumulate &&
                    ((((unsigned long long)(K + g0)) & 15ull) == 0) && ((ld & 1) == 0);

  double xi0[DMAX], xi1[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double2 x2 = *reinterpret_cast<const double2*>(sr + d * TILE + 2 * lane);
    xi0[d] = x2.x;
    xi1[d] = x2.y;
  }
  const double rs0 = srw[2 * lane], rs1 = srw[2 * lane + 1];

  for (int jc = 0; jc < 32; jc += DCC) {
    const int pbase = wv * 32 + jc;
    const double* sp = sc + pbase * DMAX;
    const double* scq = scw + pbase;
    // once per point pair: the exponential and the coefficients every term of the group reads
    DerivPair P0[DCC], P1[DCC];
#pragma unroll
    for (int q = 0; q < DCC; ++q) {
      double s, s2;
      bool up;
      deriv_dist<DMAX, BASE>(xi0, sp + q * DMAX, s, s2, up);
      P0[q] = deriv_pair<BASE, false>(s, s2, up, nullptr);
      deriv_dist<DMAX, BASE>(xi1, sp + q * DMAX, s, s2, up);
      P1[q] = deriv_pair<BASE, false>(s, s2, up, nullptr);
    }
    double acc0[DCC], acc1[DCC];
#pragma unroll
    for (int q = 0; q < DCC; ++q) acc0[q] = acc1[q] = 0.0;
    for (int tm = 0; tm < nterms; ++tm) {
      const double coef = terms[tm].coef;
      const int ab = (int)terms[tm].param;
      const int a = ab / DERIV_PARAM_BASE, b = ab % DERIV_PARAM_BASE;
      const int pa = a > 0 ? a - 1 : 0, pb = b > 0 ? b - 1 : 0;   // (a side that is not differentiated reads coordinate 0, unused)
      const double2 xa = *reinterpret_cast<const double2*>(sr + pa * TILE + 2 * lane);
      const double2 xb = *reinterpret_cast<const double2*>(sr + pb * TILE + 2 * lane);
      const double w0 = coef * rs0, w1 = coef * rs1;
#pragma unroll
      for (int q = 0; q < DCC; ++q) {
        const double ca = sp[q * DMAX + pa], cb = sp[q * DMAX + pb];
        const double cq = scq[q];
        const double v0 = deriv_entry(a, b, P0[q].A, P0[q].B, -P0[q].A, xa.x - ca, xb.x - cb, P0[q].dead);
        const double v1 = deriv_entry(a, b, P1[q].A, P1[q].B, -P1[q].A, xa.y - ca, xb.y - cb, P1[q].dead);
        acc0[q] = fma(v0, w0 * cq, acc0[q]);
        acc1[q] = fma(v1, w1 * cq, acc1[q]);
      }
    }
    if (full && !diag_noise) {
      double* kp = K + g0 + (gtc * TILE + pbase) * ld;
#pragma unroll
      for (int q = 0; q < DCC; ++q) *reinterpret_cast<double2*>(kp + q * ld) = make_double2(acc0[q], acc1[q]);
    } else if (full) {
#pragma unroll
      for (int q = 0; q < DCC; ++q) {
        const long gc = gtc * TILE + pbase + q;
        double v0 = acc0[q], v1 = acc1[q];
        if (gc == g0) v0 += nv0;
        if (gc == g1) v1 += nv1;
        *reinterpret_cast<double2*>(K + g0 + gc * ld) = make_double2(v0, v1);
      }
    } else {
#pragma unroll
      for (int q = 0; q < DCC; ++q) {
        const long gc = gtc * TILE + pbase + q;
        if (gc >= cbeg && gc < cend) {
          double v0 = acc0[q], v1 = acc1[q];
          if (diag_noise && gc == g0) v0 += nv0;
          if (diag_noise && gc == g1) v1 += nv1;
          double* p = K + g0 + gc * ld;
          if (ok0) p[0] = accumulate ? p[0] + v0 : v0;
          if (ok1) p[1] = accumulate ? p[1] + v1 : v1;
        }
      }
    }
  }
}

template <int BASE>
static int launch_assemble_deriv_b(int dmax, dim3 grid, size_t lds, hipStream_t s, double* K, long ld, long r0, long nr,
                                   long c0, long nc, const DevTerm* d_terms, int nterms, int lower_only, int accumulate,
                                   int noise_kind, double sigma2, const double* d_noise_diag, long trf, long tcf) {
#define SGP_DV(DM)                                                                                                          \
  hipLaunchKernelGGL((assemble_deriv_kernel<DM, BASE>), grid, dim3(256), lds, s, K, ld, r0, nr, c0, nc, d_terms, nterms, \
                     lower_only, accumulate, noise_kind, sigma2, d_noise_diag, trf, tcf)
  if (dmax <= 1) SGP_DV(1);
  else if (dmax <= 2) SGP_DV(2);
  else if (dmax <= 4) SGP_DV(4);
  else if (dmax <= 8) SGP_DV(8);
  else SGP_DV(16);
#undef SGP_DV
  SGP_HIP(hipGetLastError());
  return 0;
}

// One group of one block pair (h_terms: host copies, d_terms: the same on the device); arguments as launch_assemble_block
int launch_assemble_deriv(double* K, long ld, long r0, long nr, long c0, long nc, const DevTerm* h_terms,
                          const DevTerm* d_terms, int nterms, int lower_only, int accumulate, int noise_kind, double sigma2,
                          const double* d_noise_diag, long tile_r_first, long tile_c_first, long tile_r_cnt,
                          long tile_c_cnt, hipStream_t s) {
  if (nterms <= 0 || tile_r_cnt <= 0 || tile_c_cnt <= 0) return 0;
  const int code = h_terms[0].kind & 0xff, dim = h_terms[0].dim;
  if (!deriv_kind_known(code) || dim < 1 || dim > DERIV_MAX_DIM) {
    set_error("assemble: not a derivative term");
    return -1;
  }
  const int dmax = deriv_dmax_class(dim);
  const size_t lds = sizeof(double) * deriv_lds_doubles(dmax);
  const dim3 grid((unsigned)tile_r_cnt, (unsigned)tile_c_cnt);
#define SGP_DVB(B)                                                                                                      \
  return launch_assemble_deriv_b<B>(dmax, grid, lds, s, K, ld, r0, nr, c0, nc, d_terms, nterms, lower_only, accumulate, \
                                    noise_kind, sigma2, d_noise_diag, tile_r_first, tile_c_first)
  switch (deriv_base(code)) {
    case K_SE: SGP_DVB(K_SE);
    case K_M32: SGP_DVB(K_M32);
    default: SGP_DVB(K_M52);
  }
#undef SGP_DVB
}

// ---------------------------------------------------------------------------------------
// diagonal of one group: out[i] = (accumulate ? out[i] : 0) + sum_t entry_t(i, i) (coef_t rs_i) cs_i, every operation in the
// order of the matrix kernel (the distance over the group's dimension alone: the matrix kernel's padding adds exact zeros)
// ---------------------------------------------------------------------------------------
template <int BASE>
__global__ __launch_bounds__(256) void diag_deriv_kernel(double* out, long n, const DevTerm* terms, int nterms, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevTerm T = terms[0];
  const double* xr = T.xr + i * T.ldr;
  const double* xc = T.xc + i * T.ldc;
  double s = 0.0;
  for (int d = 0; d < T.dim; ++d) {
    const double df = xr[d] - xc[d];
    s = fma(df, df, s);
  }
  double s2 = s;
  bool up = false;
  if (BASE == K_M32 && s < DERIV_TINY_S) {
    s2 = 0.0, up = true;
    for (int d = 0; d < T.dim; ++d) {
      const double df = (xr[d] - xc[d]) * DERIV_UP;
      s2 = fma(df, df, s2);
    }
  }
  const DerivPair P = deriv_pair<BASE, false>(s, s2, up, nullptr);
  const double rs = T.rs ? T.rs[i] : 1.0, cs = T.cs ? T.cs[i] : 1.0;
  double acc = 0.0;
  for (int tm = 0; tm < nterms; ++tm) {
    const double coef = terms[tm].coef;
    const int ab = (int)terms[tm].param;
    const int a = ab / DERIV_PARAM_BASE, b = ab % DERIV_PARAM_BASE;
    const int pa = a > 0 ? a - 1 : 0, pb = b > 0 ? b - 1 : 0;
    const double v = deriv_entry(a, b, P.A, P.B, -P.A, xr[pa] - xc[pa], xr[pb] - xc[pb], P.dead);
    acc = fma(v, (coef * rs) * cs, acc);
  }
  out[i] = accumulate ? out[i] + acc : acc;
}

int launch_diag_deriv(double* out, long n, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int accumulate,
                      hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  const int code = h_terms[0].kind & 0xff;
  if (!deriv_kind_known(code)) {
    set_error("diag: not a derivative term");
    return -1;
  }
  const dim3 grid((unsigned)((n + 255) / 256));
  switch (deriv_base(code)) {
    case K_SE: hipLaunchKernelGGL(diag_deriv_kernel<K_SE>, grid, dim3(256), 0, s, out, n, d_terms, nterms, accumulate); break;
    case K_M32: hipLaunchKernelGGL(diag_deriv_kernel<K_M32>, grid, dim3(256), 0, s, out, n, d_terms, nterms, accumulate); break;
    default: hipLaunchKernelGGL(diag_deriv_kernel<K_M52>, grid, dim3(256), 0, s, out, n, d_terms, nterms, accumulate); break;
  }
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------
// gradient contraction of up to DERIV_GRAD_MAXT terms of one group, in launch_grad_block's shape (grad.hip): 128 x 128 tiles,
// thread = one row x 64 columns, per-workgroup partial sums reduced by a second kernel in a fixed order -- no atomics, the same
// bits on every call.
//   gc[t] = sum_ij G_ij rs_i cs_j entry_t(i, j)           gs[t] = sum_ij G_ij coef_t rs_i cs_j (u . grad_u entry_t)(i, j)
// Both sides' points are staged in LDS, for the terms' coordinate differences.
// ---------------------------------------------------------------------------------------
constexpr int DERIV_GRAD_MAXT = 16;

template <int DMAX, int BASE>
__global__ __launch_bounds__(256) void grad_deriv_kernel(const double* Kinv, long ldk, const double* alpha, long r0, long nr,
                                                         long c0, long nc, const DevTerm* terms, int nterms,
                                                         long tile_r_first, long tile_c_first,
                                                         double* partials /*[blocks][DERIV_GRAD_MAXT][2]*/) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) double smem[];   // [128][DMAX] cols | [DMAX][128] rows | cs[128] | reduction | term constants
  double* sc = smem;
  double* sr = sc + TILE * DMAX;
  double* scs = sr + TILE * DMAX;
  double* red = scs + TILE;   // [4 waves][DERIV_GRAD_MAXT][2]
  double* scoef = red + 4 * DERIV_GRAD_MAXT * 2;                        // [DERIV_GRAD_MAXT] the terms' coefficients
  int* sab = reinterpret_cast<int*>(scoef + DERIV_GRAD_MAXT);           // [DERIV_GRAD_MAXT][2] their (a, b)
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  long cbeg = gtc * TILE, cend = cbeg + TILE;
  if (cbeg < c0) cbeg = c0;
  if (cend > c0 + nc) cend = c0 + nc;
  long rbeg = gtr * TILE, rend = rbeg + TILE;
  if (rbeg < r0) rbeg = r0;
  if (rend > r0 + nr) rend = r0 + nr;
  const bool live_tile = cbeg < cend && rbeg < rend;
  const DevTerm T = terms[0];
  for (int idx = t; idx < TILE * DMAX; idx += 256) {
    const int p = idx / DMAX, d = idx % DMAX;
    const long gc = gtc * TILE + p, gr = gtr * TILE + p;
    sc[idx] = (live_tile && d < T.dim && gc >= cbeg && gc < cend) ? T.xc[(gc - c0) * T.ldc + d] : 0.0;
    sr[d * TILE + p] = (live_tile && d < T.dim && gr >= rbeg && gr < rend) ? T.xr[(gr - r0) * T.ldr + d] : 0.0;
  }
  if (t < TILE) {
    const long gc = gtc * TILE + t;
    scs[t] = (live_tile && T.cs && gc >= cbeg && gc < cend) ? T.cs[gc - c0] : 1.0;
  } else if (t - TILE < DERIV_GRAD_MAXT) {   // the terms' constants, decoded once and not per column
    const int tm = t - TILE;
    const int ab = tm < nterms ? (int)terms[tm].param : 0;
    sab[2 * tm] = ab / DERIV_PARAM_BASE, sab[2 * tm + 1] = ab % DERIV_PARAM_BASE;
    scoef[tm] = tm < nterms ? terms[tm].coef : 0.0;
  }
  __syncthreads();

  double gc_acc[DERIV_GRAD_MAXT], gs_acc[DERIV_GRAD_MAXT];
#pragma unroll
  for (int q = 0; q < DERIV_GRAD_MAXT; ++q) gc_acc[q] = gs_acc[q] = 0.0;

  const long grow = gtr * TILE + trow;
  if (live_tile && grow >= rbeg && grow < rend) {
    const long lrow = grow - r0;
    const double ai = alpha ? alpha[grow] : 0.0;
    const double rsv = T.rs ? T.rs[lrow] : 1.0;
    double xi[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xi[d] = sr[d * TILE + trow];
    for (int p = th * 64; p < th * 64 + 64; ++p) {
      const long gc = gtc * TILE + p;
      if (gc < cbeg || gc >= cend) continue;
      const double g = alpha ? 0.5 * (ai * alpha[gc] - Kinv[grow + gc * ldk]) : Kinv[grow + gc * ldk];
      const double* cp = sc + p * DMAX;
      double s, s2;
      bool up;
      deriv_dist<DMAX, BASE>(xi, cp, s, s2, up);
      DerivPairGrad Gp;
      const DerivPair P = deriv_pair<BASE, true>(s, s2, up, &Gp);
      const double w = g * rsv * scs[p];
#pragma unroll
      for (int tm = 0; tm < DERIV_GRAD_MAXT; ++tm) {
        if (tm < nterms) {   // (uniform; no break: the loop must unroll for the sums to stay in registers)
          const int a = sab[2 * tm], b = sab[2 * tm + 1];   // (decoded once per workgroup: LDS broadcasts)
          const int pa = a > 0 ? a - 1 : 0, pb = b > 0 ? b - 1 : 0;
          const double ua = sr[pa * TILE + trow] - cp[pa], ub = sr[pb * TILE + trow] - cp[pb];
          const double k = deriv_entry(a, b, P.A, P.B, -P.A, ua, ub, P.dead);
          const double dk = deriv_entry(a, b, Gp.GA, Gp.GB, Gp.GC, ua, ub, P.dead);
          gc_acc[tm] = fma(w, k, gc_acc[tm]);
          gs_acc[tm] = fma(w * scoef[tm], dk, gs_acc[tm]);
        }
      }
    }
  }
  // block reduction (fixed order): wave shuffle, then the 4 waves' sums through LDS
#pragma unroll
  for (int tm = 0; tm < DERIV_GRAD_MAXT; ++tm) {
    double a = gc_acc[tm], b = gs_acc[tm];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off, 64);
      b += __shfl_xor(b, off, 64);
    }
    if ((t & 63) == 0) {
      red[((t >> 6) * DERIV_GRAD_MAXT + tm) * 2 + 0] = a;
      red[((t >> 6) * DERIV_GRAD_MAXT + tm) * 2 + 1] = b;
    }
  }
  __syncthreads();
  if (t < DERIV_GRAD_MAXT * 2) {
    double s = 0.0;
    for (int wv = 0; wv < 4; ++wv) s += red[wv * DERIV_GRAD_MAXT * 2 + t];
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * DERIV_GRAD_MAXT * 2 + t] = s;
  }
}

// out[term] = sum_b partials[b][term][component]: one workgroup per output, 256 strided sums combined by a fixed tree
__global__ __launch_bounds__(256) void grad_deriv_reduce_kernel(const double* partials, long nblocks, double* out_coef,
                                                                double* out_scale) {
  __shared__ double sh[256];
  const int idx = blockIdx.x;   // term * 2 + component
  double s = 0.0;
  for (long b = threadIdx.x; b < nblocks; b += 256) s += partials[b * DERIV_GRAD_MAXT * 2 + idx];
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

long grad_deriv_partials(long trc, long tcc) { return std::max<long>(1, trc * tcc) * DERIV_GRAD_MAXT * 2; }

template <int BASE>
static int launch_grad_deriv_b(int dmax, dim3 grid, hipStream_t s, const double* Kinv, long ldk, const double* alpha, long r0,
                               long nr, long c0, long nc, const DevTerm* d_terms, int nterms, long trf, long tcf,
                               double* partials) {
  const size_t lds = sizeof(double) * (2 * TILE * dmax + TILE + 4 * DERIV_GRAD_MAXT * 2 + 2 * DERIV_GRAD_MAXT);
#define SGP_DG(DM)                                                                                                         \
  hipLaunchKernelGGL((grad_deriv_kernel<DM, BASE>), grid, dim3(256), lds, s, Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, \
                     nterms, trf, tcf, partials)
  if (dmax <= 1) SGP_DG(1);
  else if (dmax <= 2) SGP_DG(2);
  else if (dmax <= 4) SGP_DG(4);
  else if (dmax <= 8) SGP_DG(8);
  else SGP_DG(16);
#undef SGP_DG
  SGP_HIP(hipGetLastError());
  return 0;
}

// One group (nterms terms at h_terms / d_terms): out_coef / out_scale point at the group's first entry; partials:
// grad_deriv_partials(trc, tcc) doubles.  A group of more than DERIV_GRAD_MAXT terms takes several launches.
int launch_grad_deriv(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                      const DevTerm* h_terms, const DevTerm* d_terms, int nterms, long trf, long tcf, long trc, long tcc,
                      double* partials, double* out_coef, double* out_scale, hipStream_t s) {
  if (nterms <= 0 || trc <= 0 || tcc <= 0) return 0;
  const int code = h_terms[0].kind & 0xff, dim = h_terms[0].dim;
  if (!deriv_kind_known(code) || dim < 1 || dim > DERIV_MAX_DIM) {
    set_error("grad: not a derivative term");
    return -1;
  }
  const int dmax = deriv_dmax_class(dim);
  const dim3 grid((unsigned)trc, (unsigned)tcc);
  for (int t = 0; t < nterms; t += DERIV_GRAD_MAXT) {
    const int cnt = std::min(DERIV_GRAD_MAXT, nterms - t);
    int rc;
    switch (deriv_base(code)) {
      case K_SE:
        rc = launch_grad_deriv_b<K_SE>(dmax, grid, s, Kinv, ldk, alpha, r0, nr, c0, nc, d_terms + t, cnt, trf, tcf, partials);
        break;
      case K_M32:
        rc = launch_grad_deriv_b<K_M32>(dmax, grid, s, Kinv, ldk, alpha, r0, nr, c0, nc, d_terms + t, cnt, trf, tcf, partials);
        break;
      default:
        rc = launch_grad_deriv_b<K_M52>(dmax, grid, s, Kinv, ldk, alpha, r0, nr, c0, nc, d_terms + t, cnt, trf, tcf, partials);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(grad_deriv_reduce_kernel, dim3((unsigned)(cnt * 2)), dim3(256), 0, s, partials, trc * tcc, out_coef + t,
                       out_scale + t);
    SGP_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace sgp
