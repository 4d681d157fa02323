// Product chains (include/sthenomi_kprod.h): covariance terms that multiply several leaf kernels, each on its own view of
// the points, and the kinds that exist only here, RationalQuadratic and Linear.
//     chain value (i, j) = coef_head rs_i cs_j  prod_f k_f(x^f_i, x'^f_j)
// KernelFunctions' KernelProduct [EXT] (`k1 * k2`, reached through src/Stheno.jl:4-6); the locally periodic kernel of the
// Mauna-Loa models and the sums of products of the neural-kernel-network example are such chains.
//
// Assembly: the plain assembly's one-row tiling (kernelmatrix.hip: assemble_block_kernel) -- 128 x 128 tiles on the global
// tile grid, 256 threads, thread = one row x 64 columns, the 128 column points of EVERY factor staged in LDS point-major
// and read as wave-uniform broadcasts, the factor's row point in registers while its 8-column chunk is evaluated.  Per entry
// the same fma chain over direct differences as the plain kernels (LINEAR: the same chain over products), the old kinds'
// values from kern_eval.h's kern_eval_t (one definition: `k * ConstantKernel(1)` reproduces `k` bit for bit), the factors
// multiplied in chain order, then acc = fma(prod, cw, acc) with cw formed as the plain term forms it.
// One launch carries whole chains: as many as fit 64 KiB of LDS (terms x DMAX <= 64, DMAX = the largest factor dimension
// rounded up to a power of two); a pair with more takes several launches, each adding onto the last.  kprod_group decides
// the cut for the matrix and the diagonal alike, so var(f, x) == diag(cov(f, x)) bit for bit.
//
// Gradient: one contraction kernel with grad_block_kernel's tiling and fixed-order reductions (grad.hip), one chain per
// launch: d / d coef of the head, d / d input scale and d / d param of every factor, the products with one factor left out
// formed from prefix and suffix products (never a division: a factor that is exactly 0 -- WHITE off the diagonal, an
// underflowed SE -- gives exact zeros for itself and finite values for the others).
#include "common.h"
#include "kern_eval.h"
#include "kern_grad.h"
#include <algorithm>

namespace sgp {

enum { K_RQ = 6, K_LINEAR = 7 };
constexpr int KP_KIND_MASK = 0xff, KP_TIMES_PREV = 0x100;   // sthenomi.h: SGP_KIND_TIMES_PREV
constexpr int KP_MAXF = 8;                                  // sthenomi_kprod.h: SGP_KPROD_MAX_FACTORS
constexpr int KP_CHUNK = 8;                                 // columns per accumulator chunk

// RationalQuadratic (1 + d2 / (2 alpha))^-alpha = exp(-alpha log1p(d2 / (2 alpha))): exactly 1 at d2 == 0 (log1p(0) = 0,
// exp_nonpos(-0) = 1), exactly 0 -- never NaN -- where d2 overflowed (log1p(inf) = inf, exp_nonpos clamps its argument)
// A finite d2 whose u = d2 / (2 alpha) overflows (alpha < 1/2, points 1e154 apart) takes log(d2) - log(2 alpha) instead: with
// a small alpha the kernel is nowhere near 0 there.
__device__ __forceinline__ double rq_log1p_u(double d2, double alpha, double& u) {
  u = d2 / (2.0 * alpha);
  double l = log1p(u);
  if (u > 1.7e308 && d2 <= 1.7976931348623157e308) l = log(d2) - log(2.0 * alpha);
  return l;
}
__device__ __forceinline__ double rq_eval(double d2, double alpha) {
  double u;
  return exp_nonpos(-alpha * rq_log1p_u(d2, alpha, u));
}

template <int DMAX>
__device__ __forceinline__ double kp_d2(const double (&xi)[DMAX], const double* sp) {
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = xi[d] - sp[d];
    d2 = fma(df, df, d2);
  }
  return d2;
}
template <int DMAX>
__device__ __forceinline__ double kp_dot(const double (&xi)[DMAX], const double* sp) {
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) s = fma(xi[d], sp[d], s);
  return s;
}

// one factor over a chunk of columns: prod = k (the head) or prod * k (a continuation).  KIND is a template argument so that
// each case is straight-line code over the KP_CHUNK independent entries, as in the plain assembly
template <int DMAX, int KIND>
__device__ __forceinline__ void factor_chunk(double (&prod)[KP_CHUNK], const double (&xi)[DMAX], const double* sp,
                                             double param, bool head) {
#pragma unroll
  for (int q = 0; q < KP_CHUNK; ++q) {
    double k;
    if (KIND == K_LINEAR) k = kp_dot<DMAX>(xi, sp + q * DMAX) + param;
    else if (KIND == K_RQ) k = rq_eval(kp_d2<DMAX>(xi, sp + q * DMAX), param);
    else k = kern_eval_t<KIND>(kp_d2<DMAX>(xi, sp + q * DMAX), param);
    prod[q] = head ? k : prod[q] * k;
  }
}

template <int DMAX>
__device__ __forceinline__ void factor_chunk_any(int kind, double (&prod)[KP_CHUNK], const double (&xi)[DMAX],
                                                 const double* sp, double param, bool head) {
  switch (kind) {
    case K_SE: factor_chunk<DMAX, K_SE>(prod, xi, sp, param, head); break;
    case K_M12: factor_chunk<DMAX, K_M12>(prod, xi, sp, param, head); break;
    case K_M32: factor_chunk<DMAX, K_M32>(prod, xi, sp, param, head); break;
    case K_M52: factor_chunk<DMAX, K_M52>(prod, xi, sp, param, head); break;
    case K_WHITE: factor_chunk<DMAX, K_WHITE>(prod, xi, sp, param, head); break;
    case K_RQ: factor_chunk<DMAX, K_RQ>(prod, xi, sp, param, head); break;
    case K_LINEAR: factor_chunk<DMAX, K_LINEAR>(prod, xi, sp, param, head); break;
    default: factor_chunk<DMAX, K_CONST>(prod, xi, sp, param, head); break;
  }
}

// terms [0, nterms): whole chains (a term with KP_TIMES_PREV continues the chain of the nearest term before it without)
template <int DMAX>
__global__ __launch_bounds__(256) void assemble_kprod_kernel(
    double* K, long ld, long r0, long nr, long c0, long nc, const DevTerm* terms, int nterms, int lower_only,
    int accumulate, int noise_kind, double sigma2, const double* noise_diag, long tile_r_first, long tile_c_first) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  if (lower_only && gtr < gtc) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];  // [nterms][128][DMAX] column points
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;

  long cbeg = gtc * TILE, cend = cbeg + TILE;
  if (cbeg < c0) cbeg = c0;
  if (cend > c0 + nc) cend = c0 + nc;
  long rbeg = gtr * TILE, rend = rbeg + TILE;
  if (rbeg < r0) rbeg = r0;
  if (rend > r0 + nr) rend = r0 + nr;
  if (cbeg >= cend || rbeg >= rend) return;   // uniform over the workgroup

  for (int tm = 0; tm < nterms; ++tm) {
    const DevTerm T = terms[tm];
    const int D = T.dim;
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long gc = gtc * TILE + p;
      double v = 0.0;
      if (d < D && gc >= cbeg && gc < cend) v = T.xc[(gc - c0) * T.ldc + d];
      smem[(tm * TILE + p) * DMAX + d] = v;
    }
  }
  __syncthreads();

  const long grow = gtr * TILE + trow;
  if (grow < rbeg || grow >= rend) return;  // no further barriers below
  const long lrow = grow - r0;
  const bool diag_noise = noise_kind >= 0;
  double nval = 0.0;
  if (diag_noise) nval = (noise_kind == 0) ? sigma2 : noise_diag[grow];

  for (int jc = 0; jc < 64; jc += KP_CHUNK) {
    const int pbase = th * 64 + jc;  // point index within the tile
    if (gtc * TILE + pbase >= cend) break;
    double acc[KP_CHUNK];
#pragma unroll
    for (int q = 0; q < KP_CHUNK; ++q) acc[q] = 0.0;
    int tm = 0;
    while (tm < nterms) {
      const DevTerm H = terms[tm];   // the head of a chain: its coefficient and scales
      const double rsv = H.coef * (H.rs ? H.rs[lrow] : 1.0);
      double cw[KP_CHUNK], prod[KP_CHUNK];
#pragma unroll
      for (int q = 0; q < KP_CHUNK; ++q) {
        const long gc = gtc * TILE + pbase + q;
        cw[q] = rsv;
        if (H.cs) cw[q] = (gc >= cbeg && gc < cend) ? rsv * H.cs[gc - c0] : 0.0;
        prod[q] = 0.0;
      }
      int f = tm;
      for (;;) {
        const DevTerm T = terms[f];
        double xi[DMAX];
        {
          const double* xr = T.xr + lrow * T.ldr;
#pragma unroll
          for (int d = 0; d < DMAX; ++d) xi[d] = (d < T.dim) ? xr[d] : 0.0;
        }
        factor_chunk_any<DMAX>(T.kind & KP_KIND_MASK, prod, xi, &smem[(f * TILE + pbase) * DMAX], T.param, f == tm);
        ++f;
        if (f >= nterms || !(terms[f].kind & KP_TIMES_PREV)) break;
      }
#pragma unroll
      for (int q = 0; q < KP_CHUNK; ++q) acc[q] = fma(prod[q], cw[q], acc[q]);
      tm = f;
    }
#pragma unroll
    for (int q = 0; q < KP_CHUNK; ++q) {
      const long gc = gtc * TILE + pbase + q;
      if (gc >= cbeg && gc < cend) {
        double v = acc[q];
        if (diag_noise && gc == grow) v += nval;
        double* p = K + grow + gc * ld;
        if (accumulate) v += *p;
        *p = v;
      }
    }
  }
}

static int pow2ceil_kp(int d) {
  int p = 1;
  while (p < d) p <<= 1;
  return p;
}

// The terms [t, t + return value) of one launch: whole chains, as many as keep terms x DMAX <= 64 (64 KiB of column points);
// *dmax_out = that DMAX.  The first chain always fits: dspec_create refuses a chain beyond the limits.
int kprod_group(const DevTerm* h_terms, int t, int t1, int* dmax_out) {
  int cnt = 0, dmax = 1;
  while (t + cnt < t1) {
    int e = t + cnt + 1, dm = std::max(dmax, pow2ceil_kp(h_terms[t + cnt].dim));
    while (e < t1 && (h_terms[e].kind & KP_TIMES_PREV)) dm = std::max(dm, pow2ceil_kp(h_terms[e].dim)), ++e;
    if (cnt > 0 && (e - t) * dm > 64) break;
    cnt = e - t;
    dmax = dm;
  }
  *dmax_out = dmax;
  return cnt;
}

int launch_assemble_kprod(double* K, long ld, long r0, long nr, long c0, long nc, const DevTerm* d_terms, int nterms,
                          int dmax, int lower_only, int accumulate, int noise_kind, double sigma2,
                          const double* d_noise_diag, long tile_r_first, long tile_c_first, long tile_r_cnt,
                          long tile_c_cnt, hipStream_t s) {
  if (tile_r_cnt <= 0 || tile_c_cnt <= 0 || nterms <= 0) return 0;
  if (dmax > 16 || nterms * dmax > 64) {
    set_error("assemble: a product launch beyond terms x dimension <= 64");
    return -1;
  }
  const dim3 grid((unsigned)tile_r_cnt, (unsigned)tile_c_cnt), block(256);
#define SGP_KP(DM)                                                                                                     \
  do {                                                                                                                 \
    const size_t lds = (size_t)nterms * TILE * DM * sizeof(double);                                                    \
    hipLaunchKernelGGL(assemble_kprod_kernel<DM>, grid, block, lds, s, K, ld, r0, nr, c0, nc, d_terms, nterms,         \
                       lower_only, accumulate, noise_kind, sigma2, d_noise_diag, tile_r_first, tile_c_first);          \
  } while (0)
  if (dmax <= 1) SGP_KP(1);
  else if (dmax <= 2) SGP_KP(2);
  else if (dmax <= 4) SGP_KP(4);
  else if (dmax <= 8) SGP_KP(8);
  else SGP_KP(16);
#undef SGP_KP
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---- the diagonal: out[i] (+)= the sum of the chains of one launch group, in the assembly's operation order ------------
__device__ __forceinline__ double kp_factor_diag(const DevTerm& T, long i) {
  const int kind = T.kind & KP_KIND_MASK;
  const double* a = T.xr + i * T.ldr;
  const double* b = T.xc + i * T.ldc;
  if (kind == K_LINEAR) {
    double s = 0.0;
    for (int d = 0; d < T.dim; ++d) s = fma(a[d], b[d], s);
    return s + T.param;
  }
  double d2 = 0.0;
  for (int d = 0; d < T.dim; ++d) {
    const double df = a[d] - b[d];
    d2 = fma(df, df, d2);
  }
  if (kind == K_RQ) return rq_eval(d2, T.param);
  return kern_eval(kind, d2, T.param);
}

__global__ void diag_kprod_kernel(double* out, long n, const DevTerm* terms, int nterms, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  int tm = 0;
  while (tm < nterms) {
    const DevTerm H = terms[tm];
    double cw = H.coef * (H.rs ? H.rs[i] : 1.0);
    if (H.cs) cw = cw * H.cs[i];
    double prod = kp_factor_diag(H, i);
    int f = tm + 1;
    while (f < nterms && (terms[f].kind & KP_TIMES_PREV)) {
      const DevTerm T = terms[f];
      prod = prod * kp_factor_diag(T, i);
      ++f;
    }
    acc = fma(prod, cw, acc);
    tm = f;
  }
  out[i] = accumulate ? acc + out[i] : acc;
}

int launch_diag_kprod(double* out, long n, const DevTerm* d_terms, int nterms, int accumulate, hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  hipLaunchKernelGGL(diag_kprod_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms,
                     accumulate);
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---- gradient contraction of ONE chain --------------------------------------------------------------------------------
// k, d k / d g (both inputs scaled by g, at g = 1) and d k / d param of one factor
template <int DMAX>
__device__ __forceinline__ void kp_factor_grad(int kind, double param, const double* xr, const double* sp, double& k,
                                               double& dk, double& dp) {
  if (kind == K_LINEAR) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) s = fma(xr[d], sp[d], s);
    k = s + param;
    dk = 2.0 * s;
    dp = 1.0;
    return;
  }
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = xr[d] - sp[d];
    d2 = fma(df, df, d2);
  }
  if (kind == K_RQ) {
    // no clamp of d2 here: with a small alpha the kernel is far from 0 at d2 = 1e150.  An overflowed d2 gives u = l = inf,
    // k = 0 and, with r = u / (1 + u) taken as its limit 1, exact zeros for both derivatives
    double u;
    const double l = rq_log1p_u(d2, param, u);
    k = exp(-param * l);
    const double r = u < 1e300 ? u / (1.0 + u) : 1.0;
    dk = -(2.0 * param) * r * k;      // -d2 (1 + u)^(-alpha - 1), d2 = 2 alpha u
    dp = k == 0.0 ? 0.0 : k * (r - l);
    return;
  }
  kern_and_dscale(kind, d2, param, k, dk);
  dp = kind == G_CONST ? 1.0 : 0.0;
}

template <int DMAX>
__global__ __launch_bounds__(256) void grad_kprod_kernel(const double* Kinv, long ldk, const double* alpha, long r0, long nr,
                                                         long c0, long nc, const DevTerm* terms, int nf,
                                                         long tile_r_first, long tile_c_first,
                                                         double* partials /*[blocks][KP_MAXF][3]*/) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;   // factors x DMAX <= 64: the spec's limit
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* sx = smem;                         // [TMAX][128][DMAX] column points
  double* scs = smem + TMAX * TILE * DMAX;   // [128] column scale of the head
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  long cbeg = gtc * TILE, cend = cbeg + TILE;
  if (cbeg < c0) cbeg = c0;
  if (cend > c0 + nc) cend = c0 + nc;
  long rbeg = gtr * TILE, rend = rbeg + TILE;
  if (rbeg < r0) rbeg = r0;
  if (rend > r0 + nr) rend = r0 + nr;
  const bool live_tile = cbeg < cend && rbeg < rend;

  for (int f = 0; f < nf; ++f) {
    const DevTerm T = terms[f];
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long gc = gtc * TILE + p;
      double v = 0.0;
      if (live_tile && d < T.dim && gc >= cbeg && gc < cend) v = T.xc[(gc - c0) * T.ldc + d];
      sx[(f * TILE + p) * DMAX + d] = v;
    }
  }
  if (t < TILE) {
    const DevTerm H = terms[0];
    const long gc = gtc * TILE + t;
    scs[t] = (live_tile && H.cs && gc >= cbeg && gc < cend) ? H.cs[gc - c0] : 1.0;
  }
  __syncthreads();

  double g_coef = 0.0, gs_acc[TMAX], gp_acc[TMAX];
#pragma unroll
  for (int f = 0; f < TMAX; ++f) gs_acc[f] = gp_acc[f] = 0.0;

  const long grow = gtr * TILE + trow;
  if (live_tile && grow >= rbeg && grow < rend) {
    const long lrow = grow - r0;
    const double ai = alpha ? alpha[grow] : 0.0;
    double xr[TMAX * DMAX], param[TMAX];
    int kind[TMAX];
#pragma unroll
    for (int f = 0; f < TMAX; ++f) {
      kind[f] = G_CONST;
      param[f] = 1.0;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) xr[f * DMAX + d] = 0.0;
      if (f < nf) {
        const DevTerm T = terms[f];
        kind[f] = T.kind & KP_KIND_MASK;
        param[f] = T.param;
        const double* xp = T.xr + lrow * T.ldr;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) xr[f * DMAX + d] = (d < T.dim) ? xp[d] : 0.0;
      }
    }
    const DevTerm H = terms[0];
    const double rsv = H.rs ? H.rs[lrow] : 1.0, coef = H.coef;
    const int pbeg = th * 64;
    const long gcol0 = gtc * TILE;
    for (int p = pbeg; p < pbeg + 64; ++p) {
      const long gc = gcol0 + p;
      if (gc < cbeg || gc >= cend) continue;
      const double g = alpha ? 0.5 * (ai * alpha[gc] - Kinv[grow + gc * ldk]) : Kinv[grow + gc * ldk];
      double k[TMAX], dk[TMAX], dp[TMAX], pre[TMAX + 1];
      pre[0] = 1.0;
#pragma unroll
      for (int f = 0; f < TMAX; ++f) {
        k[f] = 1.0;
        dk[f] = dp[f] = 0.0;
        if (f < nf) kp_factor_grad<DMAX>(kind[f], param[f], &xr[f * DMAX], &sx[(f * TILE + p) * DMAX], k[f], dk[f], dp[f]);
        pre[f + 1] = pre[f] * k[f];
      }
      const double w = g * rsv * scs[p];
      g_coef = fma(w, pre[TMAX], g_coef);
      const double wc = w * coef;
      double suf = 1.0;   // the product of the factors behind f
#pragma unroll
      for (int f = TMAX - 1; f >= 0; --f) {
        if (f < nf) {
          const double excl = wc * (pre[f] * suf);
          gs_acc[f] = fma(excl, dk[f], gs_acc[f]);
          gp_acc[f] = fma(excl, dp[f], gp_acc[f]);
        }
        suf = suf * k[f];
      }
    }
  }
  // block reduction (fixed order): wave shuffle, then 4 partials through LDS
  __syncthreads();
  double* red = smem;  // reuse: [4 waves][KP_MAXF][3]
#pragma unroll
  for (int f = 0; f < KP_MAXF; ++f) {
    double a = (f == 0) ? g_coef : 0.0, b = 0.0, c = 0.0;
    if (f < TMAX) b = gs_acc[f < TMAX ? f : 0], c = gp_acc[f < TMAX ? f : 0];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off, 64);
      b += __shfl_xor(b, off, 64);
      c += __shfl_xor(c, off, 64);
    }
    if ((t & 63) == 0) {
      red[((t >> 6) * KP_MAXF + f) * 3 + 0] = a;
      red[((t >> 6) * KP_MAXF + f) * 3 + 1] = b;
      red[((t >> 6) * KP_MAXF + f) * 3 + 2] = c;
    }
  }
  __syncthreads();
  if (t < KP_MAXF * 3) {
    double s = 0.0;
    for (int wv = 0; wv < 4; ++wv) s += red[wv * KP_MAXF * 3 + t];
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * KP_MAXF * 3 + t] = s;
  }
}

// out_*[f] = sum_b partials[b][f][c]: one workgroup per output, 256 strided partial sums combined by a fixed tree.  The
// continuations' d / d coef is 0 by definition; out_param may be NULL
__global__ __launch_bounds__(256) void grad_kprod_reduce_kernel(const double* partials, long nblocks, double* out_coef,
                                                                double* out_scale, double* out_param) {
  __shared__ double sh[256];
  const int idx = blockIdx.x;  // factor * 3 + component
  double s = 0.0;
  for (long b = threadIdx.x; b < nblocks; b += 256) s += partials[b * KP_MAXF * 3 + idx];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int f = idx / 3, c = idx % 3;
    if (c == 0 && out_coef) out_coef[f] = f == 0 ? sh[0] : 0.0;
    if (c == 1 && out_scale) out_scale[f] = sh[0];
    if (c == 2 && out_param) out_param[f] = sh[0];
  }
}

template <int DMAX>
static int launch_grad_kprod_t(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                               const DevTerm* d_terms, int nf, long trf, long tcf, long trc, long tcc, double* partials,
                               hipStream_t s) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;
  if (nf > TMAX) {
    set_error("grad: a product chain beyond factors x dimension <= 64");
    return -1;
  }
  const size_t lds = (size_t)(TMAX * TILE * DMAX + TILE) * sizeof(double);
  SGP_LDS_ATTR_ONCE(grad_kprod_kernel<DMAX>, lds);
  hipLaunchKernelGGL(grad_kprod_kernel<DMAX>, dim3((unsigned)trc, (unsigned)tcc), dim3(256), lds, s, Kinv, ldk, alpha, r0,
                     nr, c0, nc, d_terms, nf, trf, tcf, partials);
  SGP_HIP(hipGetLastError());
  return 0;
}

// partials: trc x tcc x 24 doubles.  out_coef / out_scale / out_param: the chain's first entry (nf each; any may be NULL)
int launch_grad_kprod(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                      const DevTerm* d_terms, int nf, int dmax, long trf, long tcf, long trc, long tcc, double* partials,
                      double* out_coef, double* out_scale, double* out_param, hipStream_t s) {
  if (nf <= 0 || trc <= 0 || tcc <= 0) return 0;
  if (nf > KP_MAXF || dmax > 16) {
    set_error("grad: a product chain beyond the limits of include/sthenomi_kprod.h");
    return -1;
  }
  int rc;
#define SGP_KG(DM) rc = launch_grad_kprod_t<DM>(Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, nf, trf, tcf, trc, tcc, partials, s)
  if (dmax <= 1) SGP_KG(1);
  else if (dmax <= 2) SGP_KG(2);
  else if (dmax <= 4) SGP_KG(4);
  else if (dmax <= 8) SGP_KG(8);
  else SGP_KG(16);
#undef SGP_KG
  if (rc) return rc;
  hipLaunchKernelGGL(grad_kprod_reduce_kernel, dim3((unsigned)(nf * 3)), dim3(256), 0, s, partials, trc * tcc, out_coef,
                     out_scale, out_param);
  SGP_HIP(hipGetLastError());
  return 0;
}

}  // namespace sgp
