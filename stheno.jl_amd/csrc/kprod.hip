// Product chains (include/sthenomi_kprod.h): covariance terms that multiply several leaf kernels, each on its own view of
// the points, and the kinds that exist only here: RationalQuadratic, Linear, Cosine, GammaExponential, general-nu Matern and
// the kinds of x'y: NeuralNetwork, FBM, Exponentiated, and Wiener (|x|, |y|, |x - y|) and the compactly supported
// PiecewisePolynomial kinds.
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
#include "asm_frame.h"
#include "kern_eval.h"
#include "kern_grad.h"
#include "kprod_kinds_table.h"
#include <algorithm>
#include <type_traits>
#include <utility>

namespace sgp {

constexpr int KP_MAXF = SGP_KPROD_MAX_FACTORS;
constexpr int KP_CHUNK = 8;                                 // columns per accumulator chunk

#include "kprod_kinds.h"
// The launch mode of every kernel below (the template argument MN, kprod_kinds_table.h: kp_mn_of_tier of the chains' tier):
// 0 the chains hold none of MATERN_NU and the kinds above, 1 they hold MATERN_NU and none of those, 2 they hold one of
// NEURALNET / FBM / EXPONENTIATED (and possibly MATERN_NU) and none of WIENER / PIECEWISE, 3 they hold a WIENER or PIECEWISE
// factor (and possibly any other kind).  Modes 0 to 2 are what ran before WIENER and PIECEWISE existed: the compiler reports
// the registers, scratch and LDS they had (tools/kprod_resources.py; docs/03_kernels.md section 3.2e)
// Whether `kind` takes the route of the scalars (s, a, b, e) in launch mode MN, and that route's two calls.  Written so that a
// mode-2 instantiation is, once the constant conditions are folded, the very code it was before mode 3 existed.
// `(kind) >= KP_FIRST_DOT_KIND` is kp_is_dot_kind(kind) spelled out: through the function, these kernels' generated code changes
#define KP_DOT_ROUTE(MN, kind) \
  ((MN) == 3 ? ((kind) >= KP_FIRST_DOT_KIND || kp_is_wiener_or_piecewise(kind)) : ((MN) == 2 && (kind) >= KP_FIRST_DOT_KIND))
#define KP_DOT_EVAL(MN, kind, h, r) \
  ((MN) == 3 ? dotkind_eval_w(kind, h, (r).s, (r).a, (r).b, (r).e) : dotkind_eval(kind, h, (r).s, (r).a, (r).b, (r).e))
#define KP_DOT_DERIVS(MN, kind, h, r) \
  ((MN) == 3 ? dotkind_derivs_w(kind, h, (r).s, (r).a, (r).b, (r).e) : dotkind_derivs(kind, h, (r).s, (r).a, (r).b, (r).e))

// one factor of one of the three kinds over a chunk of columns
template <int DMAX, int MN>
__device__ __forceinline__ void factor_chunk_dot(int kind, double (&prod)[KP_CHUNK], const double (&xi)[DMAX], const double* sp,
                                                 double param, bool head) {
#pragma unroll
  for (int q = 0; q < KP_CHUNK; ++q) {
    const KpDot r = kp_dot_scalars<DMAX, MN == 3>(kind, xi, sp + q * DMAX);
    const double k = KP_DOT_EVAL(MN, kind, param, r);
    prod[q] = head ? k : prod[q] * k;
  }
}

// one factor over a chunk of columns: prod = k (the head) or prod * k (a continuation).  KIND is a template argument so that
// each case is straight-line code over the KP_CHUNK independent entries, as in the plain assembly
template <int DMAX, int KIND>
__device__ __forceinline__ void factor_chunk(double (&prod)[KP_CHUNK], const double (&xi)[DMAX], const double* sp,
                                             double param, bool head, const double* nuc) {
#pragma unroll
  for (int q = 0; q < KP_CHUNK; ++q) {
    double k;
    if (KIND == SGP_LINEAR) k = kp_dot<DMAX>(xi, sp + q * DMAX) + param;
    else if (KIND == SGP_RQ) k = rq_eval(kp_d2<DMAX>(xi, sp + q * DMAX), param);
    else if (KIND == SGP_COSINE) k = cosine_eval(kp_d2<DMAX>(xi, sp + q * DMAX));
    else if (KIND == SGP_GAMMAEXP) k = gexp_eval(kp_d2<DMAX>(xi, sp + q * DMAX), param);
    else if (KIND == SGP_MATERN_NU) k = matern_nu_eval(kp_d2<DMAX>(xi, sp + q * DMAX), param, nuc);
    else k = kern_eval_t<KIND>(kp_d2<DMAX>(xi, sp + q * DMAX), param);
    prod[q] = head ? k : prod[q] * k;
  }
}

template <int DMAX, int MN>
__device__ __forceinline__ void factor_chunk_any(int kind, double (&prod)[KP_CHUNK], const double (&xi)[DMAX],
                                                 const double* sp, double param, bool head, const double* nuc) {
  if (KP_DOT_ROUTE(MN, kind)) {
    factor_chunk_dot<DMAX, MN>(kind, prod, xi, sp, param, head);
    return;
  }
  if (MN && kind == SGP_MATERN_NU) {
    factor_chunk<DMAX, SGP_MATERN_NU>(prod, xi, sp, param, head, nuc);
    return;
  }
  switch (kind) {
    case K_SE: factor_chunk<DMAX, K_SE>(prod, xi, sp, param, head, nuc); break;
    case K_M12: factor_chunk<DMAX, K_M12>(prod, xi, sp, param, head, nuc); break;
    case K_M32: factor_chunk<DMAX, K_M32>(prod, xi, sp, param, head, nuc); break;
    case K_M52: factor_chunk<DMAX, K_M52>(prod, xi, sp, param, head, nuc); break;
    case K_WHITE: factor_chunk<DMAX, K_WHITE>(prod, xi, sp, param, head, nuc); break;
    case SGP_RQ: factor_chunk<DMAX, SGP_RQ>(prod, xi, sp, param, head, nuc); break;
    case SGP_LINEAR: factor_chunk<DMAX, SGP_LINEAR>(prod, xi, sp, param, head, nuc); break;
    case SGP_COSINE: factor_chunk<DMAX, SGP_COSINE>(prod, xi, sp, param, head, nuc); break;
    case SGP_GAMMAEXP: factor_chunk<DMAX, SGP_GAMMAEXP>(prod, xi, sp, param, head, nuc); break;
    default: factor_chunk<DMAX, K_CONST>(prod, xi, sp, param, head, nuc); break;
  }
}

// terms [0, nterms): whole chains (a term with KP_TIMES_PREV continues the chain of the nearest term before it without)
template <int DMAX, int MN>
__global__ __launch_bounds__(256) void assemble_kprod_kernel(
    double* K, long ld, long r0, long nr, long c0, long nc, const DevTerm* terms, int nterms, int lower_only,
    int accumulate, int noise_kind, double sigma2, const double* noise_diag, long tile_r_first, long tile_c_first) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  if (lower_only && gtr < gtc) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];  // [nterms][128][DMAX] column points
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;

  TileClip cl;
  if (!tile_clip(gtr, gtc, r0, nr, c0, nc, cl)) return;   // uniform over the workgroup
  const auto [cbeg, cend, rbeg, rend] = cl;
  stage_col_points<DMAX>(smem, terms, nterms, gtc, c0, cl, t);
  __syncthreads();

  const long grow = gtr * TILE + trow;
  if (grow < rbeg || grow >= rend) return;  // no further barriers below
  const long lrow = grow - r0;
  const bool diag_noise = noise_kind >= 0;
  const double nval = row_noise(noise_kind, sigma2, noise_diag, grow);

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
        factor_chunk_any<DMAX, MN>(T.kind & KP_KIND_MASK, prod, xi, &smem[(f * TILE + pbase) * DMAX], T.param, f == tm, T.nuc);
        ++f;
        if (f >= nterms || !(terms[f].kind & KP_TIMES_PREV)) break;
      }
#pragma unroll
      for (int q = 0; q < KP_CHUNK; ++q) acc[q] = fma(prod[q], cw[q], acc[q]);
      tm = f;
    }
    store_row_tail<KP_CHUNK>(K, ld, grow, gtc * TILE + pbase, cl, acc, diag_noise, nval, accumulate);
  }
}

// The terms [t, t + return value) of one launch: whole chains, as many as keep terms x DMAX <= 64 (64 KiB of column points);
// *dmax_out = that DMAX.  The first chain always fits: dspec_create refuses a chain beyond the limits.
int kprod_group(const DevTerm* h_terms, int t, int t1, int* dmax_out) {
  int cnt = 0, dmax = 1;
  while (t + cnt < t1) {
    int e = t + cnt + 1, dm = std::max(dmax, pow2ceil(h_terms[t + cnt].dim));
    while (e < t1 && (h_terms[e].kind & KP_TIMES_PREV)) dm = std::max(dm, pow2ceil(h_terms[e].dim)), ++e;
    if (cnt > 0 && (e - t) * dm > 64) break;
    cnt = e - t;
    dmax = dm;
  }
  *dmax_out = dmax;
  return cnt;
}

// The one place where a launch's (DMAX class, mode) becomes template arguments: returns f(KpInt<DM>{}, KpInt<M>{}) with
// DM = kp_dmax_class(dmax) and M = mode < NMODES (kprod_kinds_table.h: kp_mn_of_tier or kp_nk_of_tier of the terms' tier).  A
// kernel without a DMAX argument passes MAXDM = 1 and dmax = 1.  Every launcher below states its launch once, in such an f.
// (The highest mode first: the instantiations keep the order they have always had in the code object.)
template <int N>
using KpInt = std::integral_constant<int, N>;
template <int NMODES, int MAXDM = 16, class F>
static int kp_dispatch(int dmax, int mode, F f) {
#define KP_CASE(DM, M)                                                          \
  case DM * 8 + M:                                                              \
    if constexpr (DM <= MAXDM && M < NMODES) return f(KpInt<DM>{}, KpInt<M>{}); \
    break;
#define KP_ROW(DM) KP_CASE(DM, 4) KP_CASE(DM, 3) KP_CASE(DM, 2) KP_CASE(DM, 1) KP_CASE(DM, 0)
  switch (kp_dmax_class(dmax) * 8 + mode) { KP_ROW(1) KP_ROW(2) KP_ROW(4) KP_ROW(8) KP_ROW(16) }
#undef KP_ROW
#undef KP_CASE
  set_error("kprod: no kernel instantiation for this DMAX class and mode");
  return -1;
}

int launch_assemble_kprod(const AsmLaunch& L, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int dmax,
                          hipStream_t s) {
  if (L.empty() || nterms <= 0) return 0;
  if (dmax > 16 || nterms * dmax > 64) {
    set_error("assemble: a product launch beyond terms x dimension <= 64");
    return -1;
  }
  const dim3 grid((unsigned)L.r_cnt, (unsigned)L.c_cnt), block(256);
  return kp_dispatch<KP_MN_MODES>(dmax, kp_mn_of_tier(kp_chain_tier(h_terms, nterms)), [&](auto dm, auto mn) {
    constexpr int DM = decltype(dm)::value, MN = decltype(mn)::value;
    const size_t lds = (size_t)nterms * TILE * DM * sizeof(double);
    hipLaunchKernelGGL((assemble_kprod_kernel<DM, MN>), grid, block, lds, s, L.K, L.ld, L.r0, L.nr, L.c0, L.nc, d_terms, nterms,
                       ASM_TAIL(L), L.r_first, L.c_first);
    SGP_HIP(hipGetLastError());
    return 0;
  });
}

// ---- the diagonal: out[i] (+)= the sum of the chains of one launch group, in the assembly's operation order ------------
template <int MN>
__device__ __forceinline__ double kp_factor_diag(const DevTerm& T, long i) {
  const int kind = T.kind & KP_KIND_MASK;
  const double* a = T.xr + i * T.ldr;
  const double* b = T.xc + i * T.ldc;
  if (KP_DOT_ROUTE(MN, kind)) {
    const KpDot r = kp_dot_scalars_n<MN == 3>(kind, a, b, T.dim);
    return KP_DOT_EVAL(MN, kind, T.param, r);
  }
  if (kind == SGP_LINEAR) {
    double s = 0.0;
    for (int d = 0; d < T.dim; ++d) s = fma(a[d], b[d], s);
    return s + T.param;
  }
  double d2 = 0.0;
  for (int d = 0; d < T.dim; ++d) {
    const double df = a[d] - b[d];
    d2 = fma(df, df, d2);
  }
  if (kind == SGP_RQ) return rq_eval(d2, T.param);
  if (kind == SGP_COSINE) return cosine_eval(d2);
  if (kind == SGP_GAMMAEXP) return gexp_eval(d2, T.param);
  if (MN && kind == SGP_MATERN_NU) return matern_nu_eval(d2, T.param, T.nuc);
  return kern_eval(kind, d2, T.param);
}

template <int MN>
__global__ void diag_kprod_kernel(double* out, long n, const DevTerm* terms, int nterms, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  int tm = 0;
  while (tm < nterms) {
    const DevTerm H = terms[tm];
    double cw = H.coef * (H.rs ? H.rs[i] : 1.0);
    if (H.cs) cw = cw * H.cs[i];
    double prod = kp_factor_diag<MN>(H, i);
    int f = tm + 1;
    while (f < nterms && (terms[f].kind & KP_TIMES_PREV)) {
      const DevTerm T = terms[f];
      prod = prod * kp_factor_diag<MN>(T, i);
      ++f;
    }
    acc = fma(prod, cw, acc);
    tm = f;
  }
  out[i] = accumulate ? acc + out[i] : acc;
}

int launch_diag_kprod(double* out, long n, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int accumulate,
                      hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  return kp_dispatch<KP_MN_MODES, 1>(1, kp_mn_of_tier(kp_chain_tier(h_terms, nterms)), [&](auto, auto mn) {
    hipLaunchKernelGGL(diag_kprod_kernel<decltype(mn)::value>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n,
                       d_terms, nterms, accumulate);
    SGP_HIP(hipGetLastError());
    return 0;
  });
}

// ---- gradient contraction of ONE chain --------------------------------------------------------------------------------
// k, d k / d g (both inputs scaled by g, at g = 1) and d k / d param of one factor
template <int DMAX, int MN>
__device__ __forceinline__ void kp_factor_grad(int kind, double param, const double* xr, const double* sp, double& k,
                                               double& dk, double& dp, const DevTerm* term) {
  if (KP_DOT_ROUTE(MN, kind)) {
    const KpDot q = kp_dot_scalars<DMAX, MN == 3>(kind, xr, sp);
    const KpDotDerivs r = KP_DOT_DERIVS(MN, kind, param, q);
    k = r.k;
    dk = r.dk;
    dp = r.dp;
    return;
  }
  if (kind == SGP_LINEAR) {
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
  if (kind == SGP_RQ) {
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
  if (kind == SGP_COSINE || kind == SGP_GAMMAEXP || (MN && kind == SGP_MATERN_NU)) {
    const KpDerivs r = MN ? newkind_derivs_mn(kind, d2, param, kind == SGP_MATERN_NU ? term->nuc : nullptr)
                          : newkind_derivs(kind, d2, param);
    k = r.k;
    dk = r.dk;
    dp = r.dp;
    return;
  }
  kern_and_dscale(kind, d2, param, k, dk);
  dp = kind == G_CONST ? 1.0 : 0.0;
}

template <int DMAX, int MN>
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
  TileClip cl;
  const bool live_tile = tile_clip(gtr, gtc, r0, nr, c0, nc, cl);
  const auto [cbeg, cend, rbeg, rend] = cl;

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
        if (f < nf) kp_factor_grad<DMAX, MN>(kind[f], param[f], &xr[f * DMAX], &sx[(f * TILE + p) * DMAX], k[f], dk[f], dp[f], terms + f);
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

template <int DMAX, int MN>
static int launch_grad_kprod_t(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                               const DevTerm* d_terms, int nf, long trf, long tcf, long trc, long tcc, double* partials,
                               hipStream_t s) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;
  if (nf > TMAX) {
    set_error("grad: a product chain beyond factors x dimension <= 64");
    return -1;
  }
  const size_t lds = (size_t)(TMAX * TILE * DMAX + TILE) * sizeof(double);
  SGP_LDS_ATTR_ONCE((grad_kprod_kernel<DMAX, MN>), lds);
  hipLaunchKernelGGL((grad_kprod_kernel<DMAX, MN>), dim3((unsigned)trc, (unsigned)tcc), dim3(256), lds, s, Kinv, ldk, alpha, r0,
                     nr, c0, nc, d_terms, nf, trf, tcf, partials);
  SGP_HIP(hipGetLastError());
  return 0;
}

// partials: trc x tcc x 24 doubles.  out_coef / out_scale / out_param: the chain's first entry (nf each; any may be NULL)
int launch_grad_kprod(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                      const DevTerm* h_terms, const DevTerm* d_terms, int nf, int dmax, long trf, long tcf, long trc,
                      long tcc, double* partials, double* out_coef, double* out_scale, double* out_param, hipStream_t s) {
  if (nf <= 0 || trc <= 0 || tcc <= 0) return 0;
  if (nf > KP_MAXF || dmax > 16) {
    set_error("grad: a product chain beyond the limits of include/sthenomi_kprod.h");
    return -1;
  }
  const int rc = kp_dispatch<KP_MN_MODES>(dmax, kp_mn_of_tier(kp_chain_tier(h_terms, nf)), [&](auto dm, auto mn) {
    return launch_grad_kprod_t<decltype(dm)::value, decltype(mn)::value>(Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, nf, trf, tcf,
                                                                         trc, tcc, partials, s);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(grad_kprod_reduce_kernel, dim3((unsigned)(nf * 3)), dim3(256), 0, s, partials, trc * tcc, out_coef,
                     out_scale, out_param);
  SGP_HIP(hipGetLastError());
  return 0;
}


// ---- input-point and scale gradients of ONE chain ---------------------------------------------------------------------
// k and d k / d x of one factor from its row point and a column point: a distance kind has d k / d x = 2 kx (x - x') with
// kx = kappa'(d2) (kern_grad.h: kern_val_dd2; COSINE / GAMMAEXP / MATERN_NU: their _derivs above; RQ: -1/2 (1 + u)^(-alpha - 1)
// = -1/2 exp(-(alpha + 1) log1p(u)), an exact 0 -- never NaN -- where d2 overflowed, finite where only u did: rq_log1p_u),
// LINEAR has d k / d x = x' and kx stands for nothing.
// NK: 1 if the chain holds a COSINE / GAMMAEXP factor, 2 if it holds a MATERN_NU factor (and possibly those), else 0.  The call of their out-of-line routine costs the row-side kernel
// below registers at every factor (DMAX = 1: 2 waves per SIMD become 1), so chains of the older kinds run an instantiation
// without it
// NK == 3: the chain holds a NEURALNET / FBM / EXPONENTIATED factor (and possibly any other kind).  Such a factor has
// d k / d x = c1 x + c2 (x - x') + c3 x' (KpDotDerivs), c2 = 2 kx; c1 and c3 exist in that instantiation only.
// NK == 4: the chain holds a WIENER / PIECEWISE factor (and possibly any other kind): launch mode 3 of the kernels above.
// NK is the chain's tier (kprod_kinds_table.h: kp_nk_of_tier).  The mode of the scalars' route is written NK - 1 here and in the
// kernel below: kp_mn_of_tier(NK) for NK >= 1, and no route at NK == 0 either way.  Through kp_mn_of_tier the kernel's
// generated code changes, so the expression stays as it was
template <int DMAX, int NK>
__device__ __forceinline__ void kp_factor_dx(int kind, double param, const double* xr, const double* sp, double& k,
                                             double& kx, const double* nuc, double& c1, double& c3) {
  if (KP_DOT_ROUTE(NK - 1, kind)) {
    const KpDot q = kp_dot_scalars<DMAX, NK == 4>(kind, xr, sp);
    const KpDotDerivs r = KP_DOT_DERIVS(NK - 1, kind, param, q);
    k = r.k;
    kx = 0.5 * r.c2;
    c1 = r.c1;
    c3 = r.c3;
    return;
  }
  if (kind == SGP_LINEAR) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) s = fma(xr[d], sp[d], s);
    k = s + param;
    kx = 0.0;
    return;
  }
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = xr[d] - sp[d];
    d2 = fma(df, df, d2);
  }
  if (kind == SGP_RQ) {
    double u;
    const double l = rq_log1p_u(d2, param, u);
    k = exp(-param * l);
    kx = -0.5 * exp(-(param + 1.0) * l);
    return;
  }
  if (NK && (kind == SGP_COSINE || kind == SGP_GAMMAEXP || (NK >= 2 && kind == SGP_MATERN_NU))) {
    const KpDerivs r = NK >= 2 ? newkind_derivs_mn(kind, d2, param, nuc) : newkind_derivs(kind, d2, param);
    k = r.k;
    kx = r.kx;
    return;
  }
  kern_val_dd2(kind, d2, param, k, kx);
}

// Row side of one chain over one block pair, grad_inputs_kernel's tiling (grad.hip): a workgroup owns 128 rows and walks the
// column tiles, thread = one row x one half of a tile's columns, the column points of every factor in LDS, the row points and
// one accumulator per (factor, coordinate) in registers.  Per entry every factor is evaluated once (k and kx), the products
// with one factor left out come from prefix and suffix products (no division), and factor f adds
//     W_ij E^f_ij 2 kx_f (x^f_i - x'^f_j)   (distance kinds)       W_ij E^f_ij x'^f_j   (LINEAR)
// into its own accumulators.  The two column halves are combined in a fixed order through LDS (the column points' storage,
// no longer needed) and the owner adds into the gradient of each factor's row input, in factor order: no atomics.
// G as in grad_inputs_kernel: Gm[(r0 + i) * sr + (c0 + j) * sc], alpha != NULL: G = (alpha alpha' - Gm) / 2.
struct KpChainArgs {
  DevTerm t[KP_MAXF];
  double* gx[KP_MAXF];   // gradient of factor f's row input (dim x nr, packed) or NULL
};

template <int DMAX, int NK>
__global__ __launch_bounds__(256) void grad_kprod_inputs_kernel(const double* Gm, long sr, long sc, const double* alpha,
                                                                long r0, long nr, long c0, long nc, KpChainArgs C, int nf,
                                                                double scale, double* gsv /* nr, or NULL */) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* sx = smem;                         // [TMAX][128][DMAX] column points; afterwards [TMAX * DMAX][128] half sums
  double* scs = smem + TMAX * TILE * DMAX;   // [128] column scale of the head; afterwards the half sums of gsv
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  const long lrow = (long)blockIdx.x * TILE + trow;
  const bool live = lrow < nr;
  const long grow = r0 + lrow;
  double xr[TMAX * DMAX], acc[TMAX * DMAX], param[TMAX];
  int kind[TMAX];
#pragma unroll
  for (int f = 0; f < TMAX; ++f) {
    kind[f] = G_CONST;
    param[f] = 1.0;
    const bool on = live && f < nf;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      xr[f * DMAX + d] = (on && d < C.t[f].dim) ? C.t[f].xr[lrow * C.t[f].ldr + d] : 0.0;
      acc[f * DMAX + d] = 0.0;
    }
    if (f < nf) {
      kind[f] = C.t[f].kind & KP_KIND_MASK;
      param[f] = C.t[f].param;
    }
  }
  double accs = 0.0;
  const double coef = C.t[0].coef;
  const double ai = (alpha && live) ? alpha[grow] : 0.0;
  const double wrow = live ? coef * (C.t[0].rs ? C.t[0].rs[lrow] : 1.0) : 0.0;
  for (long ct = 0; ct * TILE < nc; ++ct) {
    __syncthreads();
#pragma unroll
    for (int f = 0; f < TMAX; ++f) {
      if (f >= nf) break;
      for (int idx = t; idx < TILE * DMAX; idx += 256) {
        const int p = idx / DMAX, d = idx % DMAX;
        const long lc = ct * TILE + p;
        sx[f * TILE * DMAX + idx] = (lc < nc && d < C.t[f].dim) ? C.t[f].xc[lc * C.t[f].ldc + d] : 0.0;
      }
    }
    if (t < TILE) {
      const long lc = ct * TILE + t;
      scs[t] = (lc < nc) ? (C.t[0].cs ? C.t[0].cs[lc] : 1.0) : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int p = th * 64; p < th * 64 + 64; ++p) {
        const long lc = ct * TILE + p;
        if (lc >= nc) break;
        const long gc = c0 + lc;
        const double gm = Gm[grow * sr + gc * sc];
        const double g = alpha ? 0.5 * (ai * alpha[gc] - gm) : gm;
        double k[TMAX], kx[TMAX], pre[TMAX + 1];
        double c1[NK >= 3 ? TMAX : 1], c3[NK >= 3 ? TMAX : 1];   // NEURALNET / FBM / EXPONENTIATED / WIENER: kp_factor_dx
        pre[0] = 1.0;
#pragma unroll
        for (int f = 0; f < TMAX; ++f) {
          k[f] = 1.0;
          kx[f] = 0.0;
          if (NK >= 3) c1[NK >= 3 ? f : 0] = c3[NK >= 3 ? f : 0] = 0.0;
          if (f < nf) kp_factor_dx<DMAX, NK>(kind[f], param[f], &xr[f * DMAX], &sx[(f * TILE + p) * DMAX], k[f], kx[f],
                                              NK >= 2 ? C.t[f].nuc : nullptr, c1[NK >= 3 ? f : 0], c3[NK >= 3 ? f : 0]);
          pre[f + 1] = pre[f] * k[f];
        }
        const double gcs = g * scs[p];
        accs = fma(gcs * coef, pre[TMAX], accs);
        const double w = gcs * wrow;
        double suf = 1.0;   // the product of the factors behind f
#pragma unroll
        for (int f = TMAX - 1; f >= 0; --f) {
          if (f < nf) {
            const double excl = w * (pre[f] * suf);
            const double* sp = &sx[(f * TILE + p) * DMAX];
            if (KP_DOT_ROUTE(NK - 1, kind[f])) {
              const double e1 = excl * c1[NK >= 3 ? f : 0], e2 = 2.0 * excl * kx[f], e3 = excl * c3[NK >= 3 ? f : 0];
#pragma unroll
              for (int d = 0; d < DMAX; ++d) {
                const double xv = xr[f * DMAX + d];
                acc[f * DMAX + d] = fma(e3, sp[d], fma(e2, xv - sp[d], fma(e1, xv, acc[f * DMAX + d])));
              }
            } else if (kind[f] == SGP_LINEAR) {
#pragma unroll
              for (int d = 0; d < DMAX; ++d) acc[f * DMAX + d] = fma(excl, sp[d], acc[f * DMAX + d]);
            } else {
              const double c2 = 2.0 * excl * kx[f];
#pragma unroll
              for (int d = 0; d < DMAX; ++d) acc[f * DMAX + d] = fma(c2, xr[f * DMAX + d] - sp[d], acc[f * DMAX + d]);
            }
          }
          suf = suf * k[f];
        }
      }
    }
  }
  // combine the two column halves in fixed order, then add into the inputs' gradients
  __syncthreads();
  if (th == 1) {
#pragma unroll
    for (int q = 0; q < TMAX * DMAX; ++q) sx[q * TILE + trow] = acc[q];
    scs[trow] = accs;
  }
  __syncthreads();
  if (th == 0 && live) {
#pragma unroll
    for (int f = 0; f < TMAX; ++f) {
      if (f >= nf || !C.gx[f]) continue;
      const int dim = C.t[f].dim;
      double* o = C.gx[f] + lrow * dim;
#pragma unroll
      for (int d = 0; d < DMAX; ++d)
        if (d < dim) o[d] += scale * (acc[f * DMAX + d] + sx[(f * DMAX + d) * TILE + trow]);
    }
    if (gsv) gsv[lrow] += scale * (accs + scs[trow]);
  }
}

template <int DMAX, int NK>
static int launch_grad_kprod_inputs_t(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0,
                                      long nc, const KpChainArgs& C, int nf, double scale, double* gsv, hipStream_t s) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;
  if (nf > TMAX) {
    set_error("grad: a product chain beyond factors x dimension <= 64");
    return -1;
  }
  const size_t lds = (size_t)(TMAX * TILE * DMAX + TILE) * sizeof(double);
  SGP_LDS_ATTR_ONCE((grad_kprod_inputs_kernel<DMAX, NK>), lds);
  hipLaunchKernelGGL((grad_kprod_inputs_kernel<DMAX, NK>), dim3((unsigned)((nr + TILE - 1) / TILE)), dim3(256), lds, s, Gm,
                     sr, sc, alpha, r0, nr, c0, nc, C, nf, scale, gsv);
  SGP_HIP(hipGetLastError());
  return 0;
}

// h_terms: the chain's nf factors (host copies); gx[f]: where factor f's row-input gradient goes (NULL: not asked for);
// gsv: the head's row-scale sums (NULL: not asked for).  transpose != 0: every factor is seen from its column points (the
// caller passes (sr, sc), the offsets and lengths of the transposed block itself, as for launch_grad_inputs)
int launch_grad_kprod_inputs(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                             const DevTerm* h_terms, int nf, int dmax, int transpose, double scale, double* const* gx,
                             double* gsv, hipStream_t s) {
  if (nf <= 0 || nr <= 0 || nc <= 0) return 0;
  if (nf > KP_MAXF || dmax > 16) {
    set_error("grad: a product chain beyond the limits of include/sthenomi_kprod.h");
    return -1;
  }
  KpChainArgs C;
  for (int f = 0; f < KP_MAXF; ++f) {
    C.t[f] = h_terms[f < nf ? f : 0];
    C.gx[f] = (f < nf && gx) ? gx[f] : nullptr;
    if (transpose) {
      std::swap(C.t[f].xr, C.t[f].xc);
      std::swap(C.t[f].ldr, C.t[f].ldc);
      std::swap(C.t[f].rs, C.t[f].cs);
    }
  }
  return kp_dispatch<KP_NK_MODES>(dmax, kp_nk_of_tier(kp_chain_tier(h_terms, nf)), [&](auto dm, auto nk) {
    return launch_grad_kprod_inputs_t<decltype(dm)::value, decltype(nk)::value>(Gm, sr, sc, alpha, r0, nr, c0, nc, C, nf, scale,
                                                                                gsv, s);
  });
}

// ---- the diagonal of ONE chain: sum_i w_i d var_i / d theta, var_i = coef rs_i cs_i prod_f k_f(xr^f_i, xc^f_i) -----------
// One workgroup, every point handled by exactly one thread: the per-point outputs (row / column scale, input points) are
// added by that thread, the sums over points (d / d coef of the head, d / d inscale and d / d param of every factor) are
// reduced in a fixed order.  Inputs: a distance kind gives the row input + and the column input - 2 kx (xr - xc) (they cancel
// when both are one array, which is skipped); LINEAR gives the row input xc and the column input xr, both added when they are
// one array.
struct KpDiagArgs {
  DevTerm t[KP_MAXF];
  double* gxr[KP_MAXF];
  double* gxc[KP_MAXF];
};

template <int MN>
__global__ __launch_bounds__(256) void diag_grad_kprod_kernel(const double* w, long n, KpDiagArgs C, int nf, double* out_coef,
                                                              double* out_scale, double* out_param, double* out_rs,
                                                              double* out_cs) {
  __shared__ double sh[256];
  double g_coef = 0.0, gs_acc[KP_MAXF], gp_acc[KP_MAXF];
#pragma unroll
  for (int f = 0; f < KP_MAXF; ++f) gs_acc[f] = gp_acc[f] = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    double k[KP_MAXF], dk[KP_MAXF], dp[KP_MAXF], kx[KP_MAXF], pre[KP_MAXF + 1];
    constexpr int NDOT = MN >= 2 ? KP_MAXF : 1;   // NEURALNET / FBM / EXPONENTIATED: the coefficients of KpDotDerivs
    double c1[NDOT], c1y[NDOT], c3[NDOT];
    pre[0] = 1.0;
#pragma unroll
    for (int f = 0; f < KP_MAXF; ++f) {
      k[f] = 1.0;
      dk[f] = dp[f] = kx[f] = 0.0;
      if (MN >= 2) c1[f % NDOT] = c1y[f % NDOT] = c3[f % NDOT] = 0.0;
      if (f < nf) {
        const DevTerm& T = C.t[f];
        const int kind = T.kind & KP_KIND_MASK;
        const double* a = T.xr + i * T.ldr;
        const double* b = T.xc + i * T.ldc;
        if (KP_DOT_ROUTE(MN, kind)) {
          const KpDot q = kp_dot_scalars_n<MN == 3>(kind, a, b, T.dim);
          const KpDotDerivs r = KP_DOT_DERIVS(MN, kind, T.param, q);
          k[f] = r.k;
          dk[f] = r.dk;
          dp[f] = r.dp;
          kx[f] = 0.5 * r.c2;
          c1[f % NDOT] = r.c1;
          c1y[f % NDOT] = r.c1y;
          c3[f % NDOT] = r.c3;
        } else if (kind == SGP_LINEAR) {
          double s = 0.0;
          for (int d = 0; d < T.dim; ++d) s = fma(a[d], b[d], s);
          k[f] = s + T.param;
          dk[f] = 2.0 * s;
          dp[f] = 1.0;
        } else {
          double d2 = 0.0;
          for (int d = 0; d < T.dim; ++d) {
            const double df = a[d] - b[d];
            d2 = fma(df, df, d2);
          }
          if (kind == SGP_RQ) {
            double u;
            const double l = rq_log1p_u(d2, T.param, u);
            k[f] = exp(-T.param * l);
            const double r = u < 1e300 ? u / (1.0 + u) : 1.0;
            dk[f] = -(2.0 * T.param) * r * k[f];
            dp[f] = k[f] == 0.0 ? 0.0 : k[f] * (r - l);
            kx[f] = -0.5 * exp(-(T.param + 1.0) * l);
          } else if (kind == SGP_COSINE || kind == SGP_GAMMAEXP || (MN && kind == SGP_MATERN_NU)) {
            const KpDerivs r = MN ? newkind_derivs_mn(kind, d2, T.param, kind == SGP_MATERN_NU ? T.nuc : nullptr)
                                  : newkind_derivs(kind, d2, T.param);
            k[f] = r.k;
            dk[f] = r.dk;
            kx[f] = r.kx;
            dp[f] = r.dp;
          } else {
            double kk;
            kern_and_dscale(kind, d2, T.param, k[f], dk[f]);
            kern_val_dd2(kind, d2, T.param, kk, kx[f]);
            dp[f] = kind == G_CONST ? 1.0 : 0.0;
          }
        }
      }
      pre[f + 1] = pre[f] * k[f];
    }
    const DevTerm& H = C.t[0];
    const double rsv = H.rs ? H.rs[i] : 1.0, csv = H.cs ? H.cs[i] : 1.0;
    const double wi = w[i];
    g_coef = fma(wi * rsv * csv, pre[KP_MAXF], g_coef);
    if (out_rs) out_rs[i] += wi * H.coef * csv * pre[KP_MAXF];
    if (out_cs) out_cs[i] += wi * H.coef * rsv * pre[KP_MAXF];
    const double wc = wi * rsv * csv * H.coef;
    double suf = 1.0;
    double excl[KP_MAXF];
#pragma unroll
    for (int f = KP_MAXF - 1; f >= 0; --f) {
      excl[f] = wc * (pre[f] * suf);
      if (f < nf) {
        gs_acc[f] = fma(excl[f], dk[f], gs_acc[f]);
        gp_acc[f] = fma(excl[f], dp[f], gp_acc[f]);
      }
      suf = suf * k[f];
    }
#pragma unroll
    for (int f = 0; f < KP_MAXF; ++f) {   // factor order: several factors may add into one array
      if (f >= nf || !C.gxr[f]) continue;
      const DevTerm& T = C.t[f];
      const double* a = T.xr + i * T.ldr;
      const double* b = T.xc + i * T.ldc;
      double* orow = C.gxr[f] + i * T.dim;
      double* ocol = C.gxc[f] + i * T.dim;
      if (KP_DOT_ROUTE(MN, T.kind & KP_KIND_MASK)) {
        // LINEAR's convention: the row input receives d k / d x, the column input d k / d y, both added when they are one array
        const double e1 = excl[f] * c1[f % NDOT], e1y = excl[f] * c1y[f % NDOT], e2 = 2.0 * excl[f] * kx[f],
                     e3 = excl[f] * c3[f % NDOT];
        for (int d = 0; d < T.dim; ++d) {
          const double av = a[d], bv = b[d];
          orow[d] += fma(e3, bv, fma(e2, av - bv, e1 * av));
          ocol[d] += fma(e3, av, fma(e2, bv - av, e1y * bv));
        }
      } else if ((T.kind & KP_KIND_MASK) == SGP_LINEAR) {
        for (int d = 0; d < T.dim; ++d) {
          const double av = a[d], bv = b[d];
          orow[d] += excl[f] * bv;
          ocol[d] += excl[f] * av;
        }
      } else if (ocol != orow) {
        const double c2 = 2.0 * excl[f] * kx[f];
        for (int d = 0; d < T.dim; ++d) {
          const double df = a[d] - b[d];
          orow[d] += c2 * df;
          ocol[d] -= c2 * df;
        }
      }
    }
  }
  // fixed-order tree per output
  for (int q = 0; q < 1 + 2 * KP_MAXF; ++q) {
    double v = 0.0;
    if (q == 0) v = g_coef;
#pragma unroll
    for (int f = 0; f < KP_MAXF; ++f) {
      if (q == 1 + f) v = gs_acc[f];
      if (q == 1 + KP_MAXF + f) v = gp_acc[f];
    }
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (q == 0) {
        if (out_coef) {
          out_coef[0] = sh[0];
          for (int f = 1; f < nf; ++f) out_coef[f] = 0.0;
        }
      } else if (q <= KP_MAXF) {
        if (out_scale && q - 1 < nf) out_scale[q - 1] = sh[0];
      } else if (out_param && q - 1 - KP_MAXF < nf) {
        out_param[q - 1 - KP_MAXF] = sh[0];
      }
    }
  }
}

// out_coef / out_scale / out_param: the chain's first entry (nf each, device; any may be NULL); gxr / gxc: per factor, the
// gradient arrays of its row / column input at the block's first point (both or neither; NULL arrays: not asked for);
// out_rs / out_cs: the head's row / column scale sums (NULL: not asked for)
int launch_diag_grad_kprod(const double* w, long n, const DevTerm* h_terms, int nf, double* out_coef, double* out_scale,
                           double* out_param, double* const* gxr, double* const* gxc, double* out_rs, double* out_cs,
                           hipStream_t s) {
  if (nf <= 0 || n <= 0) return 0;
  if (nf > KP_MAXF) {
    set_error("grad: a product chain beyond the limits of include/sthenomi_kprod.h");
    return -1;
  }
  KpDiagArgs C;
  for (int f = 0; f < KP_MAXF; ++f) {
    C.t[f] = h_terms[f < nf ? f : 0];
    C.gxr[f] = (f < nf && gxr) ? gxr[f] : nullptr;
    C.gxc[f] = (f < nf && gxc) ? gxc[f] : nullptr;
  }
  return kp_dispatch<KP_MN_MODES, 1>(1, kp_mn_of_tier(kp_chain_tier(h_terms, nf)), [&](auto, auto mn) {
    hipLaunchKernelGGL(diag_grad_kprod_kernel<decltype(mn)::value>, dim3(1), dim3(256), 0, s, w, n, C, nf, out_coef, out_scale,
                       out_param, out_rs, out_cs);
    SGP_HIP(hipGetLastError());
    return 0;
  });
}

}  // namespace sgp
