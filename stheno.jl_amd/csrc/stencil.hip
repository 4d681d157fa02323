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
#include "common.h"
#include "kern_eval.h"
#include <algorithm>

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
static int launch_stencil_t(double* K, long ld, long r0, long c0, long rlo, long rhi, long clo, long chi,
                            const DevTerm* dterm, int lower_only, int accumulate, int noise_kind, double sigma2,
                            const double* d_noise_diag, hipStream_t s) {
  constexpr int BC = ST_WAVES * st_cc<DMAX>();
  const long gx = (chi - 1) / BC - clo / BC + 1, gy = (rhi - 1) / ST_ROWS - rlo / ST_ROWS + 1;
  if (gy > 65535) {
    set_error("assemble: too many rows for one stencil launch");
    return -1;
  }
  hipLaunchKernelGGL((stencil_kernel<DMAX, KIND>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, K, ld, r0, c0, rlo,
                     rhi, clo, chi, dterm, lower_only, accumulate, noise_kind, sigma2, d_noise_diag);
  SGP_HIP(hipGetLastError());
  return 0;
}

template <int DMAX>
static int launch_stencil_kind(int kind, double* K, long ld, long r0, long c0, long rlo, long rhi, long clo, long chi,
                               const DevTerm* dterm, int lower_only, int accumulate, int noise_kind, double sigma2,
                               const double* d_noise_diag, hipStream_t s) {
#define SGP_STK(KD)                                                                                                       \
  return launch_stencil_t<DMAX, KD>(K, ld, r0, c0, rlo, rhi, clo, chi, dterm, lower_only, accumulate, noise_kind, sigma2, \
                                    d_noise_diag, s)
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

int launch_assemble_stencil(double* K, long ld, long r0, long nr, long c0, long nc, const DevTerm& T, const DevTerm* dterm,
                            int lower_only, int accumulate, int noise_kind, double sigma2, const double* d_noise_diag,
                            long tile_r_first, long tile_c_first, long tile_r_cnt, long tile_c_cnt, hipStream_t s) {
  if (tile_r_cnt <= 0 || tile_c_cnt <= 0) return 0;
  const long rlo = std::max(r0, tile_r_first * TILE), rhi = std::min(r0 + nr, (tile_r_first + tile_r_cnt) * TILE);
  const long clo = std::max(c0, tile_c_first * TILE), chi = std::min(c0 + nc, (tile_c_first + tile_c_cnt) * TILE);
  if (rlo >= rhi || clo >= chi) return 0;
  if (!(T.qr || T.qc) || T.dim < 1 || T.dim > STENCIL_MAX_DIM || T.qr > STENCIL_MAX_POINTS || T.qc > STENCIL_MAX_POINTS) {
    set_error("assemble: not a stencil term");
    return -1;
  }
#define SGP_ST_CALL(DM) \
  return launch_stencil_kind<DM>(T.kind, K, ld, r0, c0, rlo, rhi, clo, chi, dterm, lower_only, accumulate, noise_kind, \
                                 sigma2, d_noise_diag, s)
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

}  // namespace sgp
