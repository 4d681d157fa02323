// Stencil terms: K[i, j] = coef rs_i cs_j sum_p w_p sum_q v_q k(x_i - a_p, y_j - b_q), the covariance of g(x) = sum_p w_p
// f(x - a_p) with g'(y) = sum_q v_q f(y - b_q) (include/sthenomi_stencil.h).  A plain side is the one-point stencil
// {a = 0, w = 1}: x - 0 == x and fma(1, t, 0) == t exactly, so the one-sided sum sum_q v_q k(x_i, y_j - b_q) is the same
// code, and a one-point zero-offset unit-weight stencil reproduces the plain term bit for bit.
//
// Every kernel value is the plain assembly's formula (kern_eval.h) on the shifted points: x - a and y - b first, then the
// direct sum_d ((x - a)_d - (y - b)_d)^2 in d order.  Sums are exact IEEE operations in a fixed order: the inner sum over q
// t = fma(v_q, k, t), then s = fma(w_p, t, s) over p.
//   stencil_kernel       a workgroup of 4 waves owns 64 rows (one per lane) x 4 * CC columns (CC per thread), aligned to
//                        the global index so that it lies in one 128 x 128 tile; both stencils are staged in LDS and read
//                        as wave-uniform broadcasts; a thread keeps its row point and its CC column points in registers
//                        and shares every offset / weight it reads between its CC entries;
//   diag_stencil_kernel  one thread per diagonal entry, adds every stencil term of the pair onto the plain and patch
//                        diagonal already in `out` through the same summation function, so var == diag(cov) bit for bit.
// Accumulation onto the pair's plain and patch terms: v = fma(s, w, K) with w = (coef rs_i) cs_j; a pair with nothing
// before its first stencil term is written afresh, fma(s, w, 0) (+ the noise on the diagonal).
#include "asm_frame.h"
#include "kern_eval.h"
#include "kern_grad.h"
#include <algorithm>
#include <string>

// sums of kernel values are exact IEEE adds in a fixed order: no contraction of a kernel value's last product into them
#pragma clang fp contract(off)

namespace sgp {

constexpr int ST_ROWS = 64;    // rows per workgroup: one per lane
constexpr int ST_WAVES = 4;    // column groups per workgroup, one wave each

// column points per thread: as many as the registers allow (DMAX doubles each)
template <int DMAX>
constexpr int st_cc() {
  return DMAX <= 4 ? 4 : (DMAX <= 8 ? 2 : 1);
}

// LDS image of one side's stencil: offset d of point p at o[p * DMAX + d] (zero-padded to DMAX: exact zeros in the
// distance), weight p at w[p]; q == 0 (a plain side): the one-point stencil {0, 1}.  nt >= DMAX threads take part.
template <int DMAX>
__device__ __forceinline__ void stage_stencil(double* o, double* w, const double* src, int q, int D, int t, int nt) {
  if (q == 0) {
    if (t < DMAX) o[t] = 0.0;
    if (t == 0) w[0] = 1.0;
    return;
  }
  for (int e = t; e < q * DMAX; e += nt) {
    const int p = e / DMAX, d = e - p * DMAX;
    o[e] = d < D ? src[p * D + d] : 0.0;
  }
  for (int e = t; e < q; e += nt) w[e] = src[q * D + e];
}

template <int DMAX>
__device__ __forceinline__ void load_pt(double (&v)[DMAX], const double* x, int D) {
#pragma unroll
  for (int d = 0; d < DMAX; ++d) v[d] = d < D ? x[d] : 0.0;
}

// s[c] = sum_p w_p sum_q v_q k(x - a_p, y_c - b_q), p and q in order (ro / rw: row stencil, qr points; co / cw: column
// stencil, qc points; LDS, every lane reads the same address)
template <int DMAX, int KIND, int CC>
__device__ __forceinline__ void stencil_sums(double (&s)[CC], const double (&x)[DMAX], const double (&y)[CC][DMAX],
                                             const double* ro, const double* rw, int qr, const double* co,
                                             const double* cw, int qc, int kind, double param) {
#pragma unroll
  for (int c = 0; c < CC; ++c) s[c] = 0.0;
  for (int p = 0; p < qr; ++p) {
    double xs[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xs[d] = x[d] - ro[p * DMAX + d];
    double t[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) t[c] = 0.0;
    for (int q = 0; q < qc; ++q) {
      double b[DMAX];
#pragma unroll
      for (int d = 0; d < DMAX; ++d) b[d] = co[q * DMAX + d];
      const double v = cw[q];
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          const double df = xs[d] - (y[c][d] - b[d]);
          d2 = fma(df, df, d2);
        }
        const double k = KIND >= 0 ? kern_eval_t<(KIND >= 0 ? KIND : 0)>(d2, param) : kern_eval(kind, d2, param);
        t[c] = fma(v, k, t[c]);
      }
    }
    const double wp = rw[p];
#pragma unroll
    for (int c = 0; c < CC; ++c) s[c] = fma(wp, t[c], s[c]);
  }
}

__device__ __forceinline__ double st_weight(const DevTerm& T, long lr, long lc) {
  return (T.coef * (T.rs ? T.rs[lr] : 1.0)) * (T.cs ? T.cs[lc] : 1.0);
}

template <int DMAX>
struct StencilLds {
  double ro[STENCIL_MAX_POINTS * DMAX], rw[STENCIL_MAX_POINTS], co[STENCIL_MAX_POINTS * DMAX], cw[STENCIL_MAX_POINTS];
};

// ---- the matrix -------------------------------------------------------------------------------------------------------
// rows [rlo, rhi) x cols [clo, chi) of the pair (global indices; r0 / c0: the pair's first row / column).  blockIdx.x: the
// column group of 4 CC columns, blockIdx.y: the 64 rows, both counted from the aligned group holding rlo / clo.
template <int DMAX, int KIND>
__global__ __launch_bounds__(256) void stencil_kernel(double* __restrict__ K, long ld, long r0, long c0, long rlo, long rhi,
                                                      long clo, long chi, const DevTerm* __restrict__ terms, int lower_only,
                                                      int accumulate, int noise_kind, double sigma2,
                                                      const double* __restrict__ noise_diag) {
  constexpr int CC = st_cc<DMAX>();
  constexpr int BC = ST_WAVES * CC;
  __shared__ StencilLds<DMAX> sm;
  const long rb = (rlo / ST_ROWS) * ST_ROWS + (long)blockIdx.y * ST_ROWS;
  const long cb = (clo / BC) * BC + (long)blockIdx.x * BC;
  if (lower_only && rb / TILE < cb / TILE) return;   // uniform: the group lies in one tile, above the diagonal
  const DevTerm T = terms[0];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  stage_stencil<DMAX>(sm.ro, sm.rw, T.str, T.qr, T.dim, t, 256);
  stage_stencil<DMAX>(sm.co, sm.cw, T.stc, T.qc, T.dim, t, 256);
  __syncthreads();
  const long r = rb + lane;
  const long cfirst = cb + (long)wv * CC;
  if (r < rlo || r >= rhi || cfirst >= chi || cfirst + CC <= clo) return;
  double x[DMAX], y[CC][DMAX];
  load_pt<DMAX>(x, T.xr + (r - r0) * T.ldr, T.dim);
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    const long col = cfirst + c;
    const long cl = (col >= clo && col < chi ? col : std::max(clo, cfirst)) - c0;   // (out-of-range columns read a valid
    load_pt<DMAX>(y[c], T.xc + cl * T.ldc, T.dim);                                   //  point and are not written)
  }
  double s[CC];
  stencil_sums<DMAX, KIND, CC>(s, x, y, sm.ro, sm.rw, T.qr > 0 ? T.qr : 1, sm.co, sm.cw, T.qc > 0 ? T.qc : 1, T.kind,
                               T.param);
#pragma unroll
  for (int c = 0; c < CC; ++c) {
    const long col = cfirst + c;
    if (col < clo || col >= chi) continue;
    // asm_frame.h's write_entry, written out: through the helper the D = 8 covariance measured above the parent's range
    double* p = K + r + col * ld;
    double v = fma(s[c], st_weight(T, r - r0, col - c0), accumulate ? *p : 0.0);
    if (noise_kind >= 0 && r == col) v += (noise_kind == 0) ? sigma2 : noise_diag[r];
    *p = v;
  }
}

// ---- the diagonal -----------------------------------------------------------------------------------------------------
template <int DMAX>
__global__ __launch_bounds__(256) void diag_stencil_kernel(double* out, long n, const DevTerm* __restrict__ terms,
                                                           int nterms) {
  __shared__ StencilLds<DMAX> sm;
  const int t = threadIdx.x;
  const long i = (long)blockIdx.x * 256 + t;
  const long il = i < n ? i : n - 1;     // (threads past the end take part in the staging and write nothing)
  double acc = out[il];
  for (int tm = 0; tm < nterms; ++tm) {
    const DevTerm T = terms[tm];
    __syncthreads();     // the previous term's stencils are no longer read
    stage_stencil<DMAX>(sm.ro, sm.rw, T.str, T.qr, T.dim, t, 256);
    stage_stencil<DMAX>(sm.co, sm.cw, T.stc, T.qc, T.dim, t, 256);
    __syncthreads();
    double x[DMAX], y[1][DMAX], s[1];
    load_pt<DMAX>(x, T.xr + il * T.ldr, T.dim);
    load_pt<DMAX>(y[0], T.xc + il * T.ldc, T.dim);
    stencil_sums<DMAX, -1, 1>(s, x, y, sm.ro, sm.rw, T.qr > 0 ? T.qr : 1, sm.co, sm.cw, T.qc > 0 ? T.qc : 1, T.kind,
                              T.param);
    acc = fma(s[0], st_weight(T, il, il), acc);
  }
  if (i < n) out[i] = acc;
}

// ---- launchers --------------------------------------------------------------------------------------------------------
template <int DMAX, int KIND>
static int launch_stencil_t(const AsmLaunch& L, long rlo, long rhi, long clo, long chi, const DevTerm* dterm, hipStream_t s) {
  constexpr int BC = ST_WAVES * st_cc<DMAX>();
  const long gx = (chi - 1) / BC - clo / BC + 1, gy = (rhi - 1) / ST_ROWS - rlo / ST_ROWS + 1;
  if (gy > 65535) {
    set_error("assemble: too many rows for one stencil launch");
    return -1;
  }
  hipLaunchKernelGGL((stencil_kernel<DMAX, KIND>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, L.K, L.ld, L.r0, L.c0,
                     rlo, rhi, clo, chi, dterm, ASM_TAIL(L));
  SGP_HIP(hipGetLastError());
  return 0;
}

template <int DMAX>
static int launch_stencil_kind(const AsmLaunch& L, long rlo, long rhi, long clo, long chi, int kind, const DevTerm* dterm,
                               hipStream_t s) {
#define SGP_STK(KD) return launch_stencil_t<DMAX, KD>(L, rlo, rhi, clo, chi, dterm, s)
  switch (kind) {
    case K_SE: SGP_STK(K_SE);
    case K_M12: SGP_STK(K_M12);
    case K_M32: SGP_STK(K_M32);
    case K_M52: SGP_STK(K_M52);
    default: SGP_STK(-1);   // white / constant: the run-time switch
  }
#undef SGP_STK
}

// the input dimension's instantiation: the next power of two, zero-padded
#define SGP_STENCIL_DISPATCH(D, CALL) \
  do {                                \
    if ((D) <= 1) CALL(1);            \
    else if ((D) <= 2) CALL(2);       \
    else if ((D) <= 4) CALL(4);       \
    else if ((D) <= 8) CALL(8);       \
    else CALL(16);                    \
  } while (0)

int launch_assemble_stencil(const AsmLaunch& L, const DevTerm& T, const DevTerm* dterm, hipStream_t s) {
  long rlo, rhi, clo, chi;
  if (!L.entries(rlo, rhi, clo, chi)) return 0;
  if (!(T.qr || T.qc) || T.dim < 1 || T.dim > STENCIL_MAX_DIM || T.qr > STENCIL_MAX_POINTS || T.qc > STENCIL_MAX_POINTS) {
    set_error("assemble: not a stencil term");
    return -1;
  }
#define SGP_ST_CALL(DM) return launch_stencil_kind<DM>(L, rlo, rhi, clo, chi, T.kind, dterm, s)
  SGP_STENCIL_DISPATCH(T.dim, SGP_ST_CALL);
#undef SGP_ST_CALL
  return 0;
}

int launch_diag_stencil(double* out, long n, const DevTerm* d_terms, int nterms, int max_dim, hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  if (max_dim < 1 || max_dim > STENCIL_MAX_DIM) {
    set_error("kernelmatrix_diag: bad stencil dimension");
    return -1;
  }
  const dim3 grid((unsigned)((n + 255) / 256));
#define SGP_DIAG_CALL(DM)                                                                                  \
  do {                                                                                                     \
    hipLaunchKernelGGL((diag_stencil_kernel<DM>), grid, dim3(256), 0, s, out, n, d_terms, nterms);         \
    SGP_HIP(hipGetLastError());                                                                            \
    return 0;                                                                                              \
  } while (0)
  SGP_STENCIL_DISPATCH(max_dim, SGP_DIAG_CALL);
#undef SGP_DIAG_CALL
  return 0;
}

// ======================================================================================================================
// Gradient contractions against a stencil term (include/sthenomi_stencil_grad.h).  With a cotangent G (grad.hip's two
// forms: (alpha alpha' - Kinv) / 2 when alpha is given, else the matrix itself) and, per entry, s_k = sum_pq w_p v_q k and
// s_d = sum_pq w_p v_q dk/dg |_{g=1} on the shifted points -- one kern_and_dscale evaluation per (p, q), summed in the
// assembly's order (stencil_sums_kd beside stencil_sums) --
//   grad_coef    = sum_ij G_ij rs_i cs_j s_k,        grad_inscale = sum_ij G_ij coef rs_i cs_j s_d.
//   stencil_grad_kernel         the assembly's work split (64 rows x 4 CC columns per workgroup, stencils in LDS); a thread
//                               adds its CC entries up in column order, then a wave butterfly and the four waves in wave
//                               order: one pair of partial sums per workgroup;
//   stencil_diag_grad_kernel    one thread per diagonal entry, the sums by the same device function; one pair per entry;
//   stencil_grad_reduce_kernel  partials -> the two outputs, 256 strided sums and a fixed tree (conv_grad_reduce_kernel's
//                               order);
//   stencil_points_kernel       d / d (row side's points): a workgroup owns 16 rows and walks every column of the pair; a
//                               wave's lanes are 16 rows x 4 column groups and its waves take further columns, so column
//                               j belongs to (wave, group) = (j / 4 mod NW, j mod 4); the four groups are added by two
//                               butterfly steps, the waves in wave order through LDS, and wave 0 adds the sums into the
//                               input's gradient: every output column is written by exactly one thread -- no atomics.
//                               The column side is the same kernel on the transposed cotangent with the term's sides
//                               and stencils swapped;
//   stencil_diag_points_kernel  one thread per diagonal entry: the row input gets +, the column input - the same sum.
// Nothing here depends on the launch order of other workgroups: two calls give the same bits.
// ======================================================================================================================
template <int DMAX, int CC>
__device__ __forceinline__ void stencil_sums_kd(double (&sk)[CC], double (&sd)[CC], const double (&x)[DMAX],
                                                const double (&y)[CC][DMAX], const double* ro, const double* rw, int qr,
                                                const double* co, const double* cw, int qc, int kind, double param) {
#pragma unroll
  for (int c = 0; c < CC; ++c) sk[c] = sd[c] = 0.0;
  for (int p = 0; p < qr; ++p) {
    double xs[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xs[d] = x[d] - ro[p * DMAX + d];
    double tk[CC], td[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) tk[c] = td[c] = 0.0;
    for (int q = 0; q < qc; ++q) {
      double b[DMAX];
#pragma unroll
      for (int d = 0; d < DMAX; ++d) b[d] = co[q * DMAX + d];
      const double v = cw[q];
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          const double df = xs[d] - (y[c][d] - b[d]);
          d2 = fma(df, df, d2);
        }
        double k, dk;
        kern_and_dscale(kind, d2, param, k, dk);
        tk[c] = fma(v, k, tk[c]);
        td[c] = fma(v, dk, td[c]);
      }
    }
    const double wp = rw[p];
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      sk[c] = fma(wp, tk[c], sk[c]);
      sd[c] = fma(wp, td[c], sd[c]);
    }
  }
}

// g[d] = sum_p w_p sum_q v_q 2 kappa'(d2_pq) ((x - a_p) - (y - b_q))[d], p and q in the assembly's order (kappa' = d k /
// d (d^2), kern_val_dd2: Matern-1/2 contributes 0 where a shifted pair coincides)
template <int DMAX>
__device__ __forceinline__ void stencil_point_sums(double (&g)[DMAX], const double (&x)[DMAX], const double (&y)[DMAX],
                                                   const double* ro, const double* rw, int qr, const double* co,
                                                   const double* cw, int qc, int kind, double param) {
#pragma unroll
  for (int d = 0; d < DMAX; ++d) g[d] = 0.0;
  for (int p = 0; p < qr; ++p) {
    double xs[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) xs[d] = x[d] - ro[p * DMAX + d];
    const double wp = 2.0 * rw[p];
    for (int q = 0; q < qc; ++q) {
      double df[DMAX], d2 = 0.0;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        df[d] = xs[d] - (y[d] - co[q * DMAX + d]);
        d2 = fma(df[d], df[d], d2);
      }
      double k, kx;
      kern_val_dd2(kind, d2, param, k, kx);
      const double wk = (wp * cw[q]) * kx;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) g[d] = fma(wk, df[d], g[d]);
    }
  }
}

__device__ __forceinline__ double st_cotangent(const double* Gm, long sr, long sc, const double* alpha, long r, long c) {
  const double gm = Gm[r * sr + c * sc];
  return alpha ? 0.5 * (alpha[r] * alpha[c] - gm) : gm;
}

// rows [rlo, rhi) x cols [clo, chi) of the pair, global indices, the grid counted from the aligned groups as in
// stencil_kernel; G(r, c) at Gm[r + c * ldg]
template <int DMAX>
__global__ __launch_bounds__(256) void stencil_grad_kernel(const double* __restrict__ Gm, long ldg,
                                                           const double* __restrict__ alpha, long r0, long c0, long rlo,
                                                           long rhi, long clo, long chi, const DevTerm* __restrict__ terms,
                                                           double* __restrict__ partials) {
  constexpr int CC = st_cc<DMAX>();
  constexpr int BC = ST_WAVES * CC;
  __shared__ StencilLds<DMAX> sm;
  __shared__ double red[2 * ST_WAVES];
  const long rb = (rlo / ST_ROWS) * ST_ROWS + (long)blockIdx.y * ST_ROWS;
  const long cb = (clo / BC) * BC + (long)blockIdx.x * BC;
  const DevTerm T = terms[0];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  stage_stencil<DMAX>(sm.ro, sm.rw, T.str, T.qr, T.dim, t, 256);
  stage_stencil<DMAX>(sm.co, sm.cw, T.stc, T.qc, T.dim, t, 256);
  __syncthreads();
  const long r = rb + lane;
  const long cfirst = cb + (long)wv * CC;
  double a = 0.0, b = 0.0;
  if (r >= rlo && r < rhi && cfirst < chi && cfirst + CC > clo) {
    double x[DMAX], y[CC][DMAX];
    load_pt<DMAX>(x, T.xr + (r - r0) * T.ldr, T.dim);
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      const long col = cfirst + c;
      const long cl = (col >= clo && col < chi ? col : std::max(clo, cfirst)) - c0;   // (out of range: a valid point, unused)
      load_pt<DMAX>(y[c], T.xc + cl * T.ldc, T.dim);
    }
    double sk[CC], sd[CC];
    stencil_sums_kd<DMAX, CC>(sk, sd, x, y, sm.ro, sm.rw, T.qr > 0 ? T.qr : 1, sm.co, sm.cw, T.qc > 0 ? T.qc : 1, T.kind,
                              T.param);
    const double wr = T.rs ? T.rs[r - r0] : 1.0;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      const long col = cfirst + c;
      if (col < clo || col >= chi) continue;
      const double w = (st_cotangent(Gm, 1, ldg, alpha, r, col) * wr) * (T.cs ? T.cs[col - c0] : 1.0);
      a = fma(w, sk[c], a);
      b = fma(w * T.coef, sd[c], b);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    a = a + __shfl_xor(a, m, 64);
    b = b + __shfl_xor(b, m, 64);
  }
  if (lane == 0) {
    red[wv * 2 + 0] = a;
    red[wv * 2 + 1] = b;
  }
  __syncthreads();
  if (t < 2) {
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * 2 + t] = ((red[t] + red[2 + t]) + red[4 + t]) + red[6 + t];
  }
}

// sum_i w_i d var_i / d theta of ONE stencil term of a diagonal pair: partials[2 i] / [2 i + 1] per entry
template <int DMAX>
__global__ __launch_bounds__(256) void stencil_diag_grad_kernel(const double* __restrict__ w, long n,
                                                                const DevTerm* __restrict__ terms,
                                                                double* __restrict__ partials) {
  __shared__ StencilLds<DMAX> sm;
  const DevTerm T = terms[0];
  const int t = threadIdx.x;
  const long i = (long)blockIdx.x * 256 + t;
  stage_stencil<DMAX>(sm.ro, sm.rw, T.str, T.qr, T.dim, t, 256);
  stage_stencil<DMAX>(sm.co, sm.cw, T.stc, T.qc, T.dim, t, 256);
  __syncthreads();
  if (i >= n) return;
  double x[DMAX], y[1][DMAX], sk[1], sd[1];
  load_pt<DMAX>(x, T.xr + i * T.ldr, T.dim);
  load_pt<DMAX>(y[0], T.xc + i * T.ldc, T.dim);
  stencil_sums_kd<DMAX, 1>(sk, sd, x, y, sm.ro, sm.rw, T.qr > 0 ? T.qr : 1, sm.co, sm.cw, T.qc > 0 ? T.qc : 1, T.kind,
                           T.param);
  const double ww = (w[i] * (T.rs ? T.rs[i] : 1.0)) * (T.cs ? T.cs[i] : 1.0);
  partials[2 * i] = ww * sk[0];
  partials[2 * i + 1] = (ww * T.coef) * sd[0];
}

// out_coef[0] / out_scale[0] = sum_b partials[2 b] / [2 b + 1] in a fixed order (blockIdx.x: the component)
__global__ __launch_bounds__(256) void stencil_grad_reduce_kernel(const double* __restrict__ partials, long nblocks,
                                                                  double* out_coef, double* out_scale) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long b = threadIdx.x; b < nblocks; b += 256) s += partials[b * 2 + blockIdx.x];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *(blockIdx.x ? out_scale : out_coef) = sh[0];
}

// waves per workgroup of the points kernel: as many as the registers of the dimension allow
template <int DMAX>
constexpr int st_pw() {
  return DMAX <= 4 ? 16 : (DMAX <= 8 ? 8 : 4);
}
constexpr int ST_PCG = 4;                 // column groups within a wave of the points kernel
constexpr int ST_PROWS = 64 / ST_PCG;     // ... and its rows: 16 per workgroup, so that N = 4096 fills 256 compute units

// gx[:, i] += scale sum_j G_ij coef rs_i cs_j sum_pq w_p v_q 2 kappa'(d2_pq) ((x_i - a_p) - (y_j - b_q))  (gx: dim x nr,
// packed); G(i, j) of the launch's (row point i, column point j) at Gm[(r0 + i) * sr + (c0 + j) * sc], as grad_inputs_kernel
template <int DMAX>
__global__ __launch_bounds__(64 * st_pw<DMAX>()) void stencil_points_kernel(const double* __restrict__ Gm, long sr, long sc,
                                                                            const double* __restrict__ alpha, long r0,
                                                                            long nr, long c0, long nc, DevTerm T,
                                                                            double scale, double* __restrict__ gx) {
  constexpr int NW = st_pw<DMAX>();
  __shared__ StencilLds<DMAX> sm;
  __shared__ double comb[(NW - 1) * ST_PROWS * DMAX];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int rl = lane & (ST_PROWS - 1), cg = lane / ST_PROWS;     // the lane's row and column group
  stage_stencil<DMAX>(sm.ro, sm.rw, T.str, T.qr, T.dim, t, 64 * NW);
  stage_stencil<DMAX>(sm.co, sm.cw, T.stc, T.qc, T.dim, t, 64 * NW);
  __syncthreads();
  const long lrow = (long)blockIdx.x * ST_PROWS + rl;
  const bool live = lrow < nr;
  double acc[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) acc[d] = 0.0;
  if (live) {
    double x[DMAX];
    load_pt<DMAX>(x, T.xr + lrow * T.ldr, T.dim);
    const double wrow = T.coef * (T.rs ? T.rs[lrow] : 1.0);
    const int qr = T.qr > 0 ? T.qr : 1, qc = T.qc > 0 ? T.qc : 1;
    for (long lc = wv * ST_PCG + cg; lc < nc; lc += NW * ST_PCG) {
      double y[DMAX], g[DMAX];
      load_pt<DMAX>(y, T.xc + lc * T.ldc, T.dim);
      stencil_point_sums<DMAX>(g, x, y, sm.ro, sm.rw, qr, sm.co, sm.cw, qc, T.kind, T.param);
      const double w = (st_cotangent(Gm, sr, sc, alpha, r0 + lrow, c0 + lc) * wrow) * (T.cs ? T.cs[lc] : 1.0);
#pragma unroll
      for (int d = 0; d < DMAX; ++d) acc[d] = fma(w, g[d], acc[d]);
    }
  }
  // the four column groups of a row (lanes rl, rl + 16, rl + 32, rl + 48; every lane takes part, idle rows hold zeros)
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    acc[d] = acc[d] + __shfl_xor(acc[d], ST_PROWS, 64);
    acc[d] = acc[d] + __shfl_xor(acc[d], 2 * ST_PROWS, 64);
  }
  if (wv > 0 && cg == 0) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) comb[((wv - 1) * ST_PROWS + rl) * DMAX + d] = acc[d];
  }
  __syncthreads();
  if (wv == 0 && cg == 0 && live) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      double v = acc[d];
      for (int k = 0; k < NW - 1; ++k) v = v + comb[(k * ST_PROWS + rl) * DMAX + d];
      if (d < T.dim) gx[lrow * T.dim + d] += scale * v;
    }
  }
}

// d / d (input points) of sum_i w_i var_i for ONE stencil term of a diagonal pair: gxr[:, i] += c_i g_i, gxc[:, i] -= c_i g_i
// with c_i = w_i coef rs_i cs_i and g_i the sum of stencil_point_sums at entry (i, i); either output may be NULL
template <int DMAX>
__global__ __launch_bounds__(256) void stencil_diag_points_kernel(const double* __restrict__ w, long n, DevTerm T,
                                                                  double* gxr, double* gxc) {
  __shared__ StencilLds<DMAX> sm;
  const int t = threadIdx.x;
  const long i = (long)blockIdx.x * 256 + t;
  stage_stencil<DMAX>(sm.ro, sm.rw, T.str, T.qr, T.dim, t, 256);
  stage_stencil<DMAX>(sm.co, sm.cw, T.stc, T.qc, T.dim, t, 256);
  __syncthreads();
  if (i >= n) return;
  double x[DMAX], y[DMAX], g[DMAX];
  load_pt<DMAX>(x, T.xr + i * T.ldr, T.dim);
  load_pt<DMAX>(y, T.xc + i * T.ldc, T.dim);
  stencil_point_sums<DMAX>(g, x, y, sm.ro, sm.rw, T.qr > 0 ? T.qr : 1, sm.co, sm.cw, T.qc > 0 ? T.qc : 1, T.kind, T.param);
  const double c = ((w[i] * T.coef) * (T.rs ? T.rs[i] : 1.0)) * (T.cs ? T.cs[i] : 1.0);
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    if (d >= T.dim) continue;
    if (gxr) gxr[i * T.dim + d] += c * g[d];
    if (gxc) gxc[i * T.dim + d] -= c * g[d];
  }
}

static int stencil_term_check(const DevTerm& T, const char* who) {
  if (!(T.qr || T.qc) || T.dim < 1 || T.dim > STENCIL_MAX_DIM || T.qr > STENCIL_MAX_POINTS || T.qc > STENCIL_MAX_POINTS ||
      T.qr < 0 || T.qc < 0) {
    set_error(std::string(who) + ": not a stencil term within the limits of include/sthenomi_stencil.h");
    return -1;
  }
  return 0;
}

static inline int st_bc(int dim) { return ST_WAVES * (dim <= 4 ? 4 : (dim <= 8 ? 2 : 1)); }

long grad_stencil_partials(long r0, long nr, long c0, long nc, const DevTerm& T) {
  if (nr <= 0 || nc <= 0) return 0;
  const int bc = st_bc(T.dim);
  const long gx = (c0 + nc - 1) / bc - c0 / bc + 1, gy = (r0 + nr - 1) / ST_ROWS - r0 / ST_ROWS + 1;
  return 2 * gx * gy;
}

int launch_grad_stencil(const double* Gm, long ldg, const double* alpha, long r0, long nr, long c0, long nc, const DevTerm& T,
                        const DevTerm* dterm, double* partials, double* out_coef, double* out_scale, hipStream_t s) {
  if (nr <= 0 || nc <= 0) return 0;
  if (stencil_term_check(T, "grad")) return -1;
  const int bc = st_bc(T.dim);
  const long gx = (c0 + nc - 1) / bc - c0 / bc + 1, gy = (r0 + nr - 1) / ST_ROWS - r0 / ST_ROWS + 1;
  if (gy > 65535) {
    set_error("grad: too many rows for one stencil launch");
    return -1;
  }
#define SGP_STG_CALL(DM)                                                                                               \
  hipLaunchKernelGGL((stencil_grad_kernel<DM>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, Gm, ldg, alpha, r0, c0, \
                     r0, r0 + nr, c0, c0 + nc, dterm, partials)
  SGP_STENCIL_DISPATCH(T.dim, SGP_STG_CALL);
#undef SGP_STG_CALL
  SGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(stencil_grad_reduce_kernel, dim3(2), dim3(256), 0, s, partials, gx * gy, out_coef, out_scale);
  SGP_HIP(hipGetLastError());
  return 0;
}

int launch_diag_grad_stencil(const double* w, long n, const DevTerm& T, const DevTerm* dterm, double* partials /* 2 n */,
                             double* out_coef, double* out_scale, hipStream_t s) {
  if (n <= 0) return 0;
  if (stencil_term_check(T, "kernelmatrix_diag_grad")) return -1;
  const dim3 grid((unsigned)((n + 255) / 256));
#define SGP_STD_CALL(DM) hipLaunchKernelGGL((stencil_diag_grad_kernel<DM>), grid, dim3(256), 0, s, w, n, dterm, partials)
  SGP_STENCIL_DISPATCH(T.dim, SGP_STD_CALL);
#undef SGP_STD_CALL
  SGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(stencil_grad_reduce_kernel, dim3(2), dim3(256), 0, s, partials, n, out_coef, out_scale);
  SGP_HIP(hipGetLastError());
  return 0;
}

// the term seen from its column points: sides, scales and stencils swapped
static DevTerm stencil_swapped(const DevTerm& T) {
  DevTerm U = T;
  U.xr = T.xc, U.ldr = T.ldc, U.xc = T.xr, U.ldc = T.ldr;
  U.rs = T.cs, U.cs = T.rs;
  U.qr = T.qc, U.qc = T.qr;
  U.str = T.stc, U.stc = T.str;
  return U;
}

int launch_grad_stencil_points(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                               const DevTerm& T, int transpose, double scale, double* gx, hipStream_t s) {
  if (nr <= 0 || nc <= 0 || !gx) return 0;
  if (stencil_term_check(T, "grad (points)")) return -1;
  const DevTerm U = transpose ? stencil_swapped(T) : T;
  const dim3 grid((unsigned)((nr + ST_PROWS - 1) / ST_PROWS));
#define SGP_STP_CALL(DM)                                                                                              \
  hipLaunchKernelGGL((stencil_points_kernel<DM>), grid, dim3(64 * st_pw<DM>()), 0, s, Gm, sr, sc, alpha, r0, nr, c0, nc, U, \
                     scale, gx)
  SGP_STENCIL_DISPATCH(T.dim, SGP_STP_CALL);
#undef SGP_STP_CALL
  SGP_HIP(hipGetLastError());
  return 0;
}

int launch_diag_grad_stencil_points(const double* w, long n, const DevTerm& T, double* gxr, double* gxc, hipStream_t s) {
  if (n <= 0 || (!gxr && !gxc)) return 0;
  if (stencil_term_check(T, "kernelmatrix_diag_grad (points)")) return -1;
  if (gxr == gxc) return 0;   // one input on both sides: var_i does not depend on x_i, the two contributions cancel
  const dim3 grid((unsigned)((n + 255) / 256));
#define SGP_STDP_CALL(DM) hipLaunchKernelGGL((stencil_diag_points_kernel<DM>), grid, dim3(256), 0, s, w, n, T, gxr, gxc)
  SGP_STENCIL_DISPATCH(T.dim, SGP_STDP_CALL);
#undef SGP_STDP_CALL
  SGP_HIP(hipGetLastError());
  return 0;
}

// ======================================================================================================================
// Gradients with respect to a stencil's own weights and offsets (include/sthenomi_stencil_wo.h).  For the row side of a term,
// with W_ij = G_ij coef rs_i cs_j and delta_pq = (x_i - a_p) - (y_j - b_q):
//   grad_weights[p]    =  sum_ij W_ij sum_q v_q k(d2_pq)
//   grad_offsets[:, p] = -w_p sum_ij W_ij sum_q v_q 2 kappa'(d2_pq) delta_pq
// and the column side is the same pass on the transposed cotangent with the term's sides and stencils swapped (delta changes
// its sign with the view, which gives the column side's +).  Q (1 + D) sums do not fit a thread, so the row side's stencil point
// p is the outer loop:
//   stencil_wo_kernel         a workgroup of 4 waves owns 64 rows (one per lane) x a strip of ST_WO_STRIP columns; wave w
//                             takes the strip's columns j = w, w + 4, ..., so the column point is wave-uniform and the read of
//                             G(:, j) runs along the lanes.  For each p a lane adds 1 + D sums over its columns (in column
//                             order) and all q (in order); then a 64-lane butterfly, the four waves in wave order through
//                             LDS, and one partial of 1 + DMAX doubles per (workgroup, p);
//   stencil_wo_diag_kernel    one thread per diagonal entry, the same sums at (i, i), reduced the same way per workgroup;
//   stencil_wo_reduce_kernel  one workgroup per output element: 256 strided sums over the workgroups' partials and a fixed
//                             tree (stencil_grad_reduce_kernel's order); thread 0 writes the element, the offsets times -w_p.
// Scratch: (row groups x strips) x Q x (1 + DMAX) doubles.  No atomics, nothing depends on the launch order of workgroups.
// ======================================================================================================================
constexpr int ST_WO_STRIP = 128;   // columns per workgroup: N = 4096 gives 64 x 32 workgroups

// the sums of one column point y (weight wt = W_ij) into a / g: all q in order
template <int DMAX>
__device__ __forceinline__ void stencil_wo_sums(double& a, double (&g)[DMAX], const double (&xs)[DMAX], const double (&y)[DMAX],
                                                double wt, const double* co, const double* cw, int qc, int kind,
                                                double param) {
  for (int q = 0; q < qc; ++q) {
    double df[DMAX], d2 = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      df[d] = xs[d] - (y[d] - co[q * DMAX + d]);
      d2 = fma(df[d], df[d], d2);
    }
    double k, kx;
    kern_val_dd2(kind, d2, param, k, kx);
    const double wv = wt * cw[q];
    a = fma(wv, k, a);
    const double wk = (2.0 * wv) * kx;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) g[d] = fma(wk, df[d], g[d]);
  }
}

// the workgroup's 256 values of each of the 1 + DMAX sums -> dst[0 .. DMAX]: butterfly within a wave, then the four waves in
// wave order.  red: two buffers, used in turn by consecutive calls (buf = the call's parity), so one barrier per call suffices
template <int DMAX>
__device__ __forceinline__ void stencil_wo_combine(double a, double (&g)[DMAX], double (*red)[ST_WAVES][1 + DMAX], int buf,
                                                   int t, double* dst) {
  const int lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    a = a + __shfl_xor(a, m, 64);
#pragma unroll
    for (int d = 0; d < DMAX; ++d) g[d] = g[d] + __shfl_xor(g[d], m, 64);
  }
  if (lane == 0) {
    red[buf][wv][0] = a;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) red[buf][wv][1 + d] = g[d];
  }
  __syncthreads();
  if (t < 1 + DMAX) dst[t] = ((red[buf][0][t] + red[buf][1][t]) + red[buf][2][t]) + red[buf][3][t];
}

// T: the term seen from the side whose stencil is differentiated (T.qr >= 1); G(i, j) of the launch's (row point i, column
// point j) at Gm[(r0 + i) * sr + (c0 + j) * sc], as stencil_points_kernel.  blockIdx.x: the strip, blockIdx.y: the 64 rows;
// partials[((blockIdx.y * gridDim.x + blockIdx.x) * T.qr + p) * (1 + DMAX) + e]
template <int DMAX>
__global__ __launch_bounds__(256) void stencil_wo_kernel(const double* __restrict__ Gm, long sr, long sc,
                                                         const double* __restrict__ alpha, long r0, long nr, long c0, long nc,
                                                         DevTerm T, double* __restrict__ partials) {
  __shared__ StencilLds<DMAX> sm;
  __shared__ double red[2][ST_WAVES][1 + DMAX];
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  stage_stencil<DMAX>(sm.ro, sm.rw, T.str, T.qr, T.dim, t, 256);
  stage_stencil<DMAX>(sm.co, sm.cw, T.stc, T.qc, T.dim, t, 256);
  __syncthreads();
  const int qc = T.qc > 0 ? T.qc : 1;
  const long i = (long)blockIdx.y * ST_ROWS + lane;
  const bool live = i < nr;
  const long il = live ? i : nr - 1;     // (rows past the end read a valid point and add zeros)
  const long j0 = (long)blockIdx.x * ST_WO_STRIP, j1 = std::min(nc, j0 + ST_WO_STRIP);
  double x[DMAX];
  load_pt<DMAX>(x, T.xr + il * T.ldr, T.dim);
  const double wrow = T.coef * (T.rs ? T.rs[il] : 1.0);
  double* dst = partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * T.qr * (1 + DMAX);
  for (int p = 0; p < T.qr; ++p) {
    double xs[DMAX], g[DMAX], a = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      xs[d] = x[d] - sm.ro[p * DMAX + d];
      g[d] = 0.0;
    }
    if (live) {
      for (long j = j0 + wv; j < j1; j += ST_WAVES) {
        double y[DMAX];
        load_pt<DMAX>(y, T.xc + j * T.ldc, T.dim);
        const double wt = (st_cotangent(Gm, sr, sc, alpha, r0 + i, c0 + j) * wrow) * (T.cs ? T.cs[j] : 1.0);
        stencil_wo_sums<DMAX>(a, g, xs, y, wt, sm.co, sm.cw, qc, T.kind, T.param);
      }
    }
    stencil_wo_combine<DMAX>(a, g, red, p & 1, t, dst + (long)p * (1 + DMAX));
  }
}

// the diagonal form: entries (i, i) with W_i = w_i coef rs_i cs_i; partials[(blockIdx.x * T.qr + p) * (1 + DMAX) + e]
template <int DMAX>
__global__ __launch_bounds__(256) void stencil_wo_diag_kernel(const double* __restrict__ w, long n, DevTerm T,
                                                              double* __restrict__ partials) {
  __shared__ StencilLds<DMAX> sm;
  __shared__ double red[2][ST_WAVES][1 + DMAX];
  const int t = threadIdx.x;
  stage_stencil<DMAX>(sm.ro, sm.rw, T.str, T.qr, T.dim, t, 256);
  stage_stencil<DMAX>(sm.co, sm.cw, T.stc, T.qc, T.dim, t, 256);
  __syncthreads();
  const int qc = T.qc > 0 ? T.qc : 1;
  const long i = (long)blockIdx.x * 256 + t;
  const bool live = i < n;
  const long il = live ? i : n - 1;
  double x[DMAX], y[DMAX];
  load_pt<DMAX>(x, T.xr + il * T.ldr, T.dim);
  load_pt<DMAX>(y, T.xc + il * T.ldc, T.dim);
  const double wt = live ? ((w[il] * T.coef) * (T.rs ? T.rs[il] : 1.0)) * (T.cs ? T.cs[il] : 1.0) : 0.0;
  double* dst = partials + (long)blockIdx.x * T.qr * (1 + DMAX);
  for (int p = 0; p < T.qr; ++p) {
    double xs[DMAX], g[DMAX], a = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      xs[d] = x[d] - sm.ro[p * DMAX + d];
      g[d] = 0.0;
    }
    if (live) stencil_wo_sums<DMAX>(a, g, xs, y, wt, sm.co, sm.cw, qc, T.kind, T.param);
    stencil_wo_combine<DMAX>(a, g, red, p & 1, t, dst + (long)p * (1 + DMAX));
  }
}

// blockIdx.x = p * (1 + dim) + e: e == 0 the weight of point p, e >= 1 coordinate e - 1 of its offset; st: the differentiated
// stencil (dim x q offsets, then the q weights); an output that is not asked for (NULL) is not formed
__global__ __launch_bounds__(256) void stencil_wo_reduce_kernel(const double* __restrict__ partials, long nblocks, int q, int dim,
                                                                int stride, const double* __restrict__ st, double* out_w,
                                                                double* out_o) {
  __shared__ double sh[256];
  const int p = blockIdx.x / (1 + dim), e = blockIdx.x - p * (1 + dim);
  if (e == 0 ? !out_w : !out_o) return;   // uniform
  double s = 0.0;
  for (long b = threadIdx.x; b < nblocks; b += 256) s += partials[(b * q + p) * stride + e];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (e == 0) out_w[p] = sh[0];
  else out_o[(long)p * dim + (e - 1)] = -(st[(long)q * dim + p] * sh[0]);
}

static inline int st_dmax(int dim) { return dim <= 1 ? 1 : (dim <= 2 ? 2 : (dim <= 4 ? 4 : (dim <= 8 ? 8 : 16))); }

long grad_stencil_wo_partials(long nr, long nc, const DevTerm& T, int transpose) {
  const int q = transpose ? T.qc : T.qr;
  if (nr <= 0 || nc <= 0 || q <= 0) return 0;
  return ((nr + ST_ROWS - 1) / ST_ROWS) * ((nc + ST_WO_STRIP - 1) / ST_WO_STRIP) * q * (1 + st_dmax(T.dim));
}

long diag_grad_stencil_wo_partials(long n, const DevTerm& T, int transpose) {
  const int q = transpose ? T.qc : T.qr;
  if (n <= 0 || q <= 0) return 0;
  return ((n + 255) / 256) * q * (1 + st_dmax(T.dim));
}

int launch_grad_stencil_wo(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                           const DevTerm& T, int transpose, double* partials, double* out_w, double* out_o, hipStream_t s) {
  if (nr <= 0 || nc <= 0 || (!out_w && !out_o)) return 0;
  if (stencil_term_check(T, "grad (weights and offsets)")) return -1;
  const DevTerm U = transpose ? stencil_swapped(T) : T;
  if (U.qr < 1) {
    set_error("grad (weights and offsets): plain side: it has no stencil to differentiate");
    return -1;
  }
  const long gx = (nc + ST_WO_STRIP - 1) / ST_WO_STRIP, gy = (nr + ST_ROWS - 1) / ST_ROWS;
  if (gy > 65535) {
    set_error("grad (weights and offsets): too many rows for one stencil launch");
    return -1;
  }
#define SGP_STWO_CALL(DM)                                                                                                  \
  hipLaunchKernelGGL((stencil_wo_kernel<DM>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, Gm, sr, sc, alpha, r0, nr, \
                     c0, nc, U, partials)
  SGP_STENCIL_DISPATCH(T.dim, SGP_STWO_CALL);
#undef SGP_STWO_CALL
  SGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(stencil_wo_reduce_kernel, dim3((unsigned)(U.qr * (1 + U.dim))), dim3(256), 0, s, partials, gx * gy, U.qr,
                     U.dim, 1 + st_dmax(U.dim), U.str, out_w, out_o);
  SGP_HIP(hipGetLastError());
  return 0;
}

int launch_diag_grad_stencil_wo(const double* w, long n, const DevTerm& T, int transpose, double* partials, double* out_w,
                                double* out_o, hipStream_t s) {
  if (n <= 0 || (!out_w && !out_o)) return 0;
  if (stencil_term_check(T, "kernelmatrix_diag_grad (weights and offsets)")) return -1;
  const DevTerm U = transpose ? stencil_swapped(T) : T;
  if (U.qr < 1) {
    set_error("kernelmatrix_diag_grad (weights and offsets): plain side: it has no stencil to differentiate");
    return -1;
  }
  const long gx = (n + 255) / 256;
#define SGP_STWOD_CALL(DM) \
  hipLaunchKernelGGL((stencil_wo_diag_kernel<DM>), dim3((unsigned)gx), dim3(256), 0, s, w, n, U, partials)
  SGP_STENCIL_DISPATCH(T.dim, SGP_STWOD_CALL);
#undef SGP_STWOD_CALL
  SGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(stencil_wo_reduce_kernel, dim3((unsigned)(U.qr * (1 + U.dim))), dim3(256), 0, s, partials, gx, U.qr, U.dim,
                     1 + st_dmax(U.dim), U.str, out_w, out_o);
  SGP_HIP(hipGetLastError());
  return 0;
}

}  // namespace sgp
