// Patch (convolutional) terms: K[i, j] = coef rs_i cs_j sum_p sum_q k(patch_p(X_i), patch_q(Y_j)) when both sides are
// patched, sum_p k(patch_p(X_i), y_j) / sum_q k(x_i, patch_q(Y_j)) when one side is.  A patched side's points are raw
// images (column-major H x W, one per column); patch (pr, pc) of an image is its ph x pw window at row pr, column pc,
// flattened column-major (row index fastest), stride 1, every position used: P = (H - ph + 1) (W - pw + 1).  Positions are
// summed in the order p = pr + pc (H - ph + 1).
//
// The images are staged in LDS and the patches gathered from there (nothing of size P x image is written to HBM); the
// kernel value of every pair of patches is the plain assembly's own formula (kern_eval.h), so a geometry with patch ==
// image reproduces the plain term bit for bit.
//   conv1_kernel  one side patched: a thread owns CONV1_CC points of the plain side and sums over every patch of each of the
//                 CONV1_IMG images staged for its workgroup, sequentially in p (one patch read from LDS serves CONV1_CC
//                 kernel values);
//   conv2_kernel  both sides patched: one wave per entry, lanes take the row patches p = lane, lane + 64, ..., each lane
//                 sums over every column patch q in order, then a butterfly over the wave; four waves (entries (i, j..j+3))
//                 share the staged row image;
//   diag_conv_kernel  one wave per diagonal entry: the plain terms' diagonal (diag_plain_sum), then every patch term summed
//                 by the same functions as above, so var == diag(cov) bit for bit.
// Accumulation onto the plain terms of the pair: v = fma(s, w, K) with w = (coef rs_i) cs_j; a pair without plain terms
// is written afresh, fma(s, w, 0) (+ the noise on the diagonal) by its first patch term.
#include "common.h"
#include "kern_eval.h"
#include <algorithm>

// sums of kernel values are exact IEEE adds in a fixed order: no contraction of a kernel value's last product into them
#pragma clang fp contract(off)

namespace sgp {

constexpr int CONV1_CC = 2;     // plain-side points per thread
constexpr int CONV1_IMG = 4;    // images staged per workgroup (one-sided)
constexpr int CONV2_WAVES = 4;  // column entries per workgroup (two-sided), one wave each

struct ConvSide {
  int h;      // image height (rows); 0: this side is plain
  int np_r;   // patch positions along the rows (h - ph + 1)
  int np;     // patch positions
};

__device__ __forceinline__ ConvSide conv_side(int h, int w, int ph, int pw) {
  ConvSide c;
  c.h = h;
  c.np_r = h > 0 ? h - ph + 1 : 1;
  c.np = h > 0 ? c.np_r * (w - pw + 1) : 1;
  return c;
}

// element d = a + b ph of a patch sits at offset a + b h of the patch's first pixel
template <int DMAX>
__device__ __forceinline__ void patch_offsets(int (&off)[DMAX], int ph, int h, int D) {
#pragma unroll
  for (int d = 0; d < DMAX; ++d) off[d] = d < D ? (d % ph) + (d / ph) * h : 0;
}

template <int DMAX, bool EXACT>
__device__ __forceinline__ void load_patch(double (&v)[DMAX], const double* img, int base, const int (&off)[DMAX], int D) {
#pragma unroll
  for (int d = 0; d < DMAX; ++d) v[d] = (EXACT || d < D) ? img[base + off[d]] : 0.0;
}

template <int DMAX, bool EXACT>
__device__ __forceinline__ void load_point(double (&v)[DMAX], const double* x, int D) {
#pragma unroll
  for (int d = 0; d < DMAX; ++d) v[d] = (EXACT || d < D) ? x[d] : 0.0;
}

// the plain assembly's per-pair formula: direct sum_d (row_d - col_d)^2 in d order, then the kernel
template <int DMAX, int KIND>
__device__ __forceinline__ double pair_kernel(const double (&r)[DMAX], const double (&c)[DMAX], int kind, double param) {
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = r[d] - c[d];
    d2 = fma(df, df, d2);
  }
  return KIND >= 0 ? kern_eval_t<(KIND >= 0 ? KIND : 0)>(d2, param) : kern_eval(kind, d2, param);
}

// one side patched: s[k] += sum_p k(patch_p(img), pt[k]) in p order (patched side on the rows: row_img = true)
template <int DMAX, bool EXACT, int KIND, int CC>
__device__ __forceinline__ void conv1_sums(double (&s)[CC], const double* img, const ConvSide& g, const int (&off)[DMAX],
                                           int D, const double (&pt)[CC][DMAX], bool row_img, int kind, double param) {
  for (int pc = 0, base0 = 0; pc < g.np / g.np_r; ++pc, base0 += g.h) {
    for (int pr = 0; pr < g.np_r; ++pr) {
      double a[DMAX];
      load_patch<DMAX, EXACT>(a, img, base0 + pr, off, D);
#pragma unroll
      for (int k = 0; k < CC; ++k) {
        const double v = row_img ? pair_kernel<DMAX, KIND>(a, pt[k], kind, param) : pair_kernel<DMAX, KIND>(pt[k], a, kind, param);
        s[k] = s[k] + v;
      }
    }
  }
}

// both sides patched, one wave: the full sum, identical in every lane
template <int DMAX, bool EXACT, int KIND>
__device__ __forceinline__ double conv2_sum(const double* imr, const ConvSide& gr, const int (&offr)[DMAX], const double* imc,
                                            const ConvSide& gc, const int (&offc)[DMAX], int D, int kind, double param,
                                            int lane) {
  double s = 0.0;
  for (int p = lane; p < gr.np; p += 64) {
    double a[DMAX];
    load_patch<DMAX, EXACT>(a, imr, (p % gr.np_r) + (p / gr.np_r) * gr.h, offr, D);
    for (int qc = 0, base0 = 0; qc < gc.np / gc.np_r; ++qc, base0 += gc.h) {
#pragma unroll 2
      for (int qr = 0; qr < gc.np_r; ++qr) {
        double b[DMAX];
        load_patch<DMAX, EXACT>(b, imc, base0 + qr, offc, D);
        s = s + pair_kernel<DMAX, KIND>(a, b, kind, param);
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m, 64);
  return s;
}

__device__ __forceinline__ void stage(double* dst, const double* src, int n, int t, int nt) {
  for (int e = t; e < n; e += nt) dst[e] = src[e];
}

__device__ __forceinline__ bool entry_live(long r, long c, int lower_only) { return !lower_only || r / TILE >= c / TILE; }

__device__ __forceinline__ double entry_weight(const DevTerm& T, long lr, long lc) {
  return (T.coef * (T.rs ? T.rs[lr] : 1.0)) * (T.cs ? T.cs[lc] : 1.0);
}

__device__ __forceinline__ void write_entry(double* K, long ld, long r, long c, double s, double w, int accumulate,
                                            int noise_kind, double sigma2, const double* noise_diag) {
  double* p = K + r + c * ld;
  double v = fma(s, w, accumulate ? *p : 0.0);
  if (noise_kind >= 0 && r == c) v += (noise_kind == 0) ? sigma2 : noise_diag[r];
  *p = v;
}

// ---- one side patched -----------------------------------------------------------------------------------------------
// rows [rlo, rhi) x cols [clo, chi) of the pair (global indices; r0 / c0: the pair's first row / column).  The patched side
// ("a") runs over blockIdx.x in chunks of CONV1_IMG images, the plain side ("b") over blockIdx.y in chunks of 256 CC points.
template <int DMAX, bool EXACT, int KIND>
__global__ __launch_bounds__(256) void conv1_kernel(double* __restrict__ K, long ld, long r0, long c0, long rlo, long rhi,
                                                    long clo, long chi, const DevTerm* __restrict__ terms, int lower_only,
                                                    int accumulate, int noise_kind, double sigma2,
                                                    const double* __restrict__ noise_diag) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const DevTerm T = terms[0];
  const bool row_img = T.hr > 0;
  const int H = row_img ? T.hr : T.hc, W = row_img ? T.wr : T.wc, HW = H * W;
  const int D = T.ph * T.pw;
  const long alo = row_img ? rlo : clo, ahi = row_img ? rhi : chi, a0 = row_img ? r0 : c0;
  const long blo = row_img ? clo : rlo, bhi = row_img ? chi : rhi, b0 = row_img ? c0 : r0;
  const double* ximg = row_img ? T.xr : T.xc;
  const double* xpt = row_img ? T.xc : T.xr;
  const long ldpt = row_img ? T.ldc : T.ldr;
  const int t = threadIdx.x;
  const long a_first = alo + (long)blockIdx.x * CONV1_IMG;
  const int nimg = (int)std::min<long>(CONV1_IMG, ahi - a_first);
  for (int k = 0; k < nimg; ++k) stage(smem + k * HW, ximg + (a_first + k - a0) * (long)HW, HW, t, 256);
  __syncthreads();
  long b[CONV1_CC];
  double pt[CONV1_CC][DMAX];
#pragma unroll
  for (int k = 0; k < CONV1_CC; ++k) {
    b[k] = blo + (long)blockIdx.y * (256 * CONV1_CC) + t + 256 * k;
    const long bl = (b[k] < bhi ? b[k] : blo) - b0;        // (out-of-range points read a valid one and are not written)
    load_point<DMAX, EXACT>(pt[k], xpt + bl * ldpt, D);
  }
  if (b[0] >= bhi) return;
  const ConvSide g = conv_side(H, W, T.ph, T.pw);
  int off[DMAX];
  patch_offsets<DMAX>(off, T.ph, H, D);
  for (int k = 0; k < nimg; ++k) {
    const long a = a_first + k;
    bool any = false;
#pragma unroll
    for (int j = 0; j < CONV1_CC; ++j)
      any |= b[j] < bhi && (row_img ? entry_live(a, b[j], lower_only) : entry_live(b[j], a, lower_only));
    if (!any) continue;
    double s[CONV1_CC];
#pragma unroll
    for (int j = 0; j < CONV1_CC; ++j) s[j] = 0.0;
    conv1_sums<DMAX, EXACT, KIND, CONV1_CC>(s, smem + k * HW, g, off, D, pt, row_img, T.kind, T.param);
#pragma unroll
    for (int j = 0; j < CONV1_CC; ++j) {
      const long r = row_img ? a : b[j], c = row_img ? b[j] : a;
      if (b[j] < bhi && entry_live(r, c, lower_only))
        write_entry(K, ld, r, c, s[j], entry_weight(T, r - r0, c - c0), accumulate, noise_kind, sigma2, noise_diag);
    }
  }
}

// ---- both sides patched ---------------------------------------------------------------------------------------------
template <int DMAX, bool EXACT, int KIND>
__global__ __launch_bounds__(256) void conv2_kernel(double* __restrict__ K, long ld, long r0, long c0, long rlo, long rhi,
                                                    long clo, long chi, const DevTerm* __restrict__ terms, int lower_only,
                                                    int accumulate, int noise_kind, double sigma2,
                                                    const double* __restrict__ noise_diag) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const DevTerm T = terms[0];
  const int HWr = T.hr * T.wr, HWc = T.hc * T.wc, D = T.ph * T.pw;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long r = rlo + blockIdx.x;
  const long c_first = clo + (long)blockIdx.y * CONV2_WAVES;
  const int ncol = (int)std::min<long>(CONV2_WAVES, chi - c_first);
  if (lower_only && r / TILE < c_first / TILE) return;      // uniform: every column of the group is in a later tile
  double* imr = smem;
  stage(imr, T.xr + (r - r0) * (long)HWr, HWr, t, 256);
  for (int k = 0; k < ncol; ++k) stage(smem + HWr + k * HWc, T.xc + (c_first + k - c0) * (long)HWc, HWc, t, 256);
  __syncthreads();
  const long c = c_first + wv;
  if (wv >= ncol || !entry_live(r, c, lower_only)) return;
  const ConvSide gr = conv_side(T.hr, T.wr, T.ph, T.pw), gc = conv_side(T.hc, T.wc, T.ph, T.pw);
  int offr[DMAX], offc[DMAX];
  patch_offsets<DMAX>(offr, T.ph, T.hr, D);
  patch_offsets<DMAX>(offc, T.ph, T.hc, D);
  const double s = conv2_sum<DMAX, EXACT, KIND>(imr, gr, offr, smem + HWr + wv * HWc, gc, offc, D, T.kind, T.param, lane);
  if (lane == 0) write_entry(K, ld, r, c, s, entry_weight(T, r - r0, c - c0), accumulate, noise_kind, sigma2, noise_diag);
}

// ---- diagonal ---------------------------------------------------------------------------------------------------------
template <int DMAX, bool EXACT>
__device__ double diag_patch_term(const DevTerm& T, long i, double* smem, int lane) {
  const int HWr = T.hr * T.wr, HWc = T.hc * T.wc, D = T.ph * T.pw;
  __syncthreads();     // the previous term's images are no longer read
  if (T.hr) stage(smem, T.xr + i * (long)HWr, HWr, lane, 64);
  if (T.hc) stage(smem + HWr, T.xc + i * (long)HWc, HWc, lane, 64);
  __syncthreads();
  const ConvSide gr = conv_side(T.hr, T.wr, T.ph, T.pw), gc = conv_side(T.hc, T.wc, T.ph, T.pw);
  if (T.hr && T.hc) {
    int offr[DMAX], offc[DMAX];
    patch_offsets<DMAX>(offr, T.ph, T.hr, D);
    patch_offsets<DMAX>(offc, T.ph, T.hc, D);
    return conv2_sum<DMAX, EXACT, -1>(smem, gr, offr, smem + HWr, gc, offc, D, T.kind, T.param, lane);
  }
  // one side: every lane runs the sum of conv1_kernel's thread for this entry
  const bool row_img = T.hr > 0;
  int off[DMAX];
  patch_offsets<DMAX>(off, T.ph, row_img ? T.hr : T.hc, D);
  double pt[1][DMAX];
  load_point<DMAX, EXACT>(pt[0], row_img ? T.xc + i * T.ldc : T.xr + i * T.ldr, D);
  double s[1] = {0.0};
  conv1_sums<DMAX, EXACT, -1, 1>(s, row_img ? smem : smem + HWr, row_img ? gr : gc, off, D, pt, row_img, T.kind, T.param);
  return s[0];
}

template <int DMAX, bool EXACT>
__global__ __launch_bounds__(64) void diag_conv_kernel(double* out, long n, const DevTerm* __restrict__ terms, int nplain,
                                                       int nterms) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const long i = blockIdx.x;
  const int lane = threadIdx.x;
  double acc = diag_plain_sum(terms, nplain, i);
  for (int tm = nplain; tm < nterms; ++tm) {
    const DevTerm T = terms[tm];
    const double s = diag_patch_term<DMAX, EXACT>(T, i, smem, lane);
    acc = fma(s, entry_weight(T, i, i), acc);
  }
  if (lane == 0) out[i] = acc;
}

// ---- launchers --------------------------------------------------------------------------------------------------------
template <int DMAX, bool EXACT, int KIND>
static int launch_conv_t(double* K, long ld, long r0, long c0, long rlo, long rhi, long clo, long chi, const DevTerm& T,
                         const DevTerm* dterm, int lower_only, int accumulate, int noise_kind, double sigma2,
                         const double* d_noise_diag, hipStream_t s) {
  if (T.hr && T.hc) {
    const size_t lds = sizeof(double) * ((size_t)T.hr * T.wr + (size_t)CONV2_WAVES * T.hc * T.wc);
    SGP_LDS_ATTR_ONCE((conv2_kernel<DMAX, EXACT, KIND>), 160 * 1024);
    dim3 grid((unsigned)(rhi - rlo), (unsigned)((chi - clo + CONV2_WAVES - 1) / CONV2_WAVES));
    hipLaunchKernelGGL((conv2_kernel<DMAX, EXACT, KIND>), grid, dim3(256), lds, s, K, ld, r0, c0, rlo, rhi, clo, chi, dterm,
                       lower_only, accumulate, noise_kind, sigma2, d_noise_diag);
  } else {
    const bool row_img = T.hr > 0;
    const long na = row_img ? rhi - rlo : chi - clo, nb = row_img ? chi - clo : rhi - rlo;
    const size_t lds = sizeof(double) * (size_t)CONV1_IMG * (row_img ? T.hr * T.wr : T.hc * T.wc);
    SGP_LDS_ATTR_ONCE((conv1_kernel<DMAX, EXACT, KIND>), 160 * 1024);
    dim3 grid((unsigned)((na + CONV1_IMG - 1) / CONV1_IMG), (unsigned)((nb + 256 * CONV1_CC - 1) / (256 * CONV1_CC)));
    hipLaunchKernelGGL((conv1_kernel<DMAX, EXACT, KIND>), grid, dim3(256), lds, s, K, ld, r0, c0, rlo, rhi, clo, chi, dterm,
                       lower_only, accumulate, noise_kind, sigma2, d_noise_diag);
  }
  SGP_HIP(hipGetLastError());
  return 0;
}

template <int DMAX, bool EXACT>
static int launch_conv_kind(int kind, double* K, long ld, long r0, long c0, long rlo, long rhi, long clo, long chi,
                            const DevTerm& T, const DevTerm* dterm, int lower_only, int accumulate, int noise_kind,
                            double sigma2, const double* d_noise_diag, hipStream_t s) {
#define SGP_CONVK(KD) \
  return launch_conv_t<DMAX, EXACT, KD>(K, ld, r0, c0, rlo, rhi, clo, chi, T, dterm, lower_only, accumulate, noise_kind, \
                                        sigma2, d_noise_diag, s)
  switch (kind) {
    case K_SE: SGP_CONVK(K_SE);
    case K_M12: SGP_CONVK(K_M12);
    case K_M32: SGP_CONVK(K_M32);
    case K_M52: SGP_CONVK(K_M52);
    default: SGP_CONVK(-1);   // white / constant: the run-time switch
  }
#undef SGP_CONVK
}

// the patch dimension's instantiation: exactly 9 (3 x 3) or the next power of two with zero padding (which adds exact
// zeros to the squared distance)
#define SGP_CONV_DISPATCH(D, CALL)              \
  do {                                          \
    if ((D) == 9) CALL(9, true);                \
    else if ((D) <= 1) CALL(1, true);           \
    else if ((D) <= 2) CALL(2, false);          \
    else if ((D) <= 4) CALL(4, false);          \
    else if ((D) <= 8) CALL(8, false);          \
    else if ((D) <= 16) CALL(16, false);        \
    else if ((D) <= 32) CALL(32, false);        \
    else CALL(64, false);                       \
  } while (0)

int launch_assemble_conv(double* K, long ld, long r0, long nr, long c0, long nc, const DevTerm& T, const DevTerm* dterm,
                         int lower_only, int accumulate, int noise_kind, double sigma2, const double* d_noise_diag,
                         long tile_r_first, long tile_c_first, long tile_r_cnt, long tile_c_cnt, hipStream_t s) {
  if (tile_r_cnt <= 0 || tile_c_cnt <= 0) return 0;
  const long rlo = std::max(r0, tile_r_first * TILE), rhi = std::min(r0 + nr, (tile_r_first + tile_r_cnt) * TILE);
  const long clo = std::max(c0, tile_c_first * TILE), chi = std::min(c0 + nc, (tile_c_first + tile_c_cnt) * TILE);
  if (rlo >= rhi || clo >= chi) return 0;
  const int D = T.ph * T.pw;
  if (!(T.hr || T.hc) || D < 1 || D > CONV_MAX_PATCH) {
    set_error("assemble: not a patch term");
    return -1;
  }
#define SGP_CONV_CALL(DM, EX) \
  return launch_conv_kind<DM, EX>(T.kind, K, ld, r0, c0, rlo, rhi, clo, chi, T, dterm, lower_only, accumulate, noise_kind, \
                                  sigma2, d_noise_diag, s)
  SGP_CONV_DISPATCH(D, SGP_CONV_CALL);
#undef SGP_CONV_CALL
  return 0;
}

template <int DMAX, bool EXACT>
static int launch_diag_t(double* out, long n, const DevTerm* d_terms, int nplain, int nterms, size_t lds, hipStream_t s) {
  SGP_LDS_ATTR_ONCE((diag_conv_kernel<DMAX, EXACT>), 160 * 1024);
  hipLaunchKernelGGL((diag_conv_kernel<DMAX, EXACT>), dim3((unsigned)n), dim3(64), lds, s, out, n, d_terms, nplain, nterms);
  SGP_HIP(hipGetLastError());
  return 0;
}

int launch_diag_conv(double* out, long n, const DevTerm* d_terms, int nplain, int nterms, int max_d, int d_all,
                     int max_pixels, hipStream_t s) {
  if (n <= 0) return 0;
  const size_t lds = sizeof(double) * (size_t)std::max(1, max_pixels);
  if (max_d < 1 || max_d > CONV_MAX_PATCH) {
    set_error("kernelmatrix_diag: bad patch dimension");
    return -1;
  }
  // every patch term of the pair in one instantiation: the widest patch, zero-padded (exact zeros in the distance)
#define SGP_DIAG_CALL(DM, EX) return launch_diag_t<DM, EX>(out, n, d_terms, nplain, nterms, lds, s)
  if (d_all == 9) SGP_DIAG_CALL(9, true);
  SGP_CONV_DISPATCH(max_d == 9 ? 16 : max_d, SGP_DIAG_CALL);
#undef SGP_DIAG_CALL
  return 0;
}

}  // namespace sgp
