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
#include "asm_frame.h"
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

  TileClip cl;
  if (!tile_clip(gtr, gtc, r0, nr, c0, nc, cl)) return;   // uniform over the workgroup

  const double* sc = smem;
  const double* sr = sc + TILE * DMAX;
  const double* srw = sr + TILE * DMAX;
  const double* scw = srw + TILE;
  // the group's points and scales; the row weight is the row scale alone (every term brings its own coefficient)
  stage_pair_points<DMAX>(smem, terms[0], 1.0, gtr, gtc, r0, c0, cl, t);
  __syncthreads();

  const PairRows R = pair_rows(K, ld, gtr, gtc, lane, cl, accumulate, noise_kind, sigma2, noise_diag);

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
    store_pair_tail<DCC>(K, ld, gtc * TILE + pbase, cl, R, acc0, acc1, accumulate);
  }
}

template <int BASE>
static int launch_assemble_deriv_b(const AsmLaunch& L, int dmax, const DevTerm* d_terms, int nterms, hipStream_t s) {
  const size_t lds = sizeof(double) * deriv_lds_doubles(dmax);
  const dim3 grid((unsigned)L.r_cnt, (unsigned)L.c_cnt);
#define SGP_DV(DM)                                                                                                      \
  hipLaunchKernelGGL((assemble_deriv_kernel<DM, BASE>), grid, dim3(256), lds, s, L.K, L.ld, L.r0, L.nr, L.c0, L.nc, d_terms, \
                     nterms, ASM_TAIL(L), L.r_first, L.c_first)
  if (dmax <= 1) SGP_DV(1);
  else if (dmax <= 2) SGP_DV(2);
  else if (dmax <= 4) SGP_DV(4);
  else if (dmax <= 8) SGP_DV(8);
  else SGP_DV(16);
#undef SGP_DV
  SGP_HIP(hipGetLastError());
  return 0;
}

// One group of one block pair (h_terms: host copies, d_terms: the same on the device)
int launch_assemble_deriv(const AsmLaunch& L, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, hipStream_t s) {
  if (nterms <= 0 || L.empty()) return 0;
  const int code = h_terms[0].kind & 0xff, dim = h_terms[0].dim;
  if (!deriv_kind_known(code) || dim < 1 || dim > DERIV_MAX_DIM) {
    set_error("assemble: not a derivative term");
    return -1;
  }
  const int dmax = deriv_dmax_class(dim);
#define SGP_DVB(B) return launch_assemble_deriv_b<B>(L, dmax, d_terms, nterms, s)
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
  TileClip cl;
  const bool live_tile = tile_clip(gtr, gtc, r0, nr, c0, nc, cl);
  const auto [cbeg, cend, rbeg, rend] = cl;
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
