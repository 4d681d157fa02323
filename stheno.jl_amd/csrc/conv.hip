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
#include "asm_frame.h"
#include "kern_eval.h"
#include "kern_grad.h"
#include <algorithm>
#include <string>

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
static int launch_conv_t(const AsmLaunch& L, long rlo, long rhi, long clo, long chi, const DevTerm& T, const DevTerm* dterm,
                         hipStream_t s) {
  if (T.hr && T.hc) {
    const size_t lds = sizeof(double) * ((size_t)T.hr * T.wr + (size_t)CONV2_WAVES * T.hc * T.wc);
    SGP_LDS_ATTR_ONCE((conv2_kernel<DMAX, EXACT, KIND>), 160 * 1024);
    dim3 grid((unsigned)(rhi - rlo), (unsigned)((chi - clo + CONV2_WAVES - 1) / CONV2_WAVES));
    hipLaunchKernelGGL((conv2_kernel<DMAX, EXACT, KIND>), grid, dim3(256), lds, s, L.K, L.ld, L.r0, L.c0, rlo, rhi, clo, chi,
                       dterm, ASM_TAIL(L));
  } else {
    const bool row_img = T.hr > 0;
    const long na = row_img ? rhi - rlo : chi - clo, nb = row_img ? chi - clo : rhi - rlo;
    const size_t lds = sizeof(double) * (size_t)CONV1_IMG * (row_img ? T.hr * T.wr : T.hc * T.wc);
    SGP_LDS_ATTR_ONCE((conv1_kernel<DMAX, EXACT, KIND>), 160 * 1024);
    dim3 grid((unsigned)((na + CONV1_IMG - 1) / CONV1_IMG), (unsigned)((nb + 256 * CONV1_CC - 1) / (256 * CONV1_CC)));
    hipLaunchKernelGGL((conv1_kernel<DMAX, EXACT, KIND>), grid, dim3(256), lds, s, L.K, L.ld, L.r0, L.c0, rlo, rhi, clo, chi,
                       dterm, ASM_TAIL(L));
  }
  SGP_HIP(hipGetLastError());
  return 0;
}

template <int DMAX, bool EXACT>
static int launch_conv_kind(const AsmLaunch& L, long rlo, long rhi, long clo, long chi, const DevTerm& T, const DevTerm* dterm,
                            hipStream_t s) {
#define SGP_CONVK(KD) return launch_conv_t<DMAX, EXACT, KD>(L, rlo, rhi, clo, chi, T, dterm, s)
  switch (T.kind) {
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

int launch_assemble_conv(const AsmLaunch& L, const DevTerm& T, const DevTerm* dterm, hipStream_t s) {
  long rlo, rhi, clo, chi;
  if (!L.entries(rlo, rhi, clo, chi)) return 0;
  const int D = T.ph * T.pw;
  if (!(T.hr || T.hc) || D < 1 || D > CONV_MAX_PATCH) {
    set_error("assemble: not a patch term");
    return -1;
  }
#define SGP_CONV_CALL(DM, EX) return launch_conv_kind<DM, EX>(L, rlo, rhi, clo, chi, T, dterm, s)
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

// ======================================================================================================================
// Gradient contractions against a patch term (include/sthenomi_conv_grad.h).  With a cotangent G (grad.hip's two forms:
// (alpha alpha' - Kinv) / 2 when alpha is given, else the matrix itself) and s_k = sum_pq k, s_d = sum_pq dk/dg |_{g=1}
// of an entry -- both from one kern_and_dscale evaluation per pair of patches, summed in the assembly's order --
//   grad_coef    = sum_ij G_ij rs_i cs_j s_k,        grad_inscale = sum_ij G_ij coef rs_i cs_j s_d.
//   conv2_grad_kernel   both sides patched: a workgroup owns one row and 128 columns of the pair; its row image stays in
//                       LDS, the column images come four at a time, one wave per entry as in conv2_kernel; every wave adds
//                       its entries up in column order, the four waves are added in wave order: one partial per workgroup;
//   conv1_grad_kernel   one side patched: conv1_kernel's work split (CONV1_IMG staged images x 256 CONV1_CC plain points);
//                       a thread adds its entries up in image order, then wave butterfly + the four waves in order;
//   conv_diag_grad_kernel  one wave per diagonal entry, the sums by the same device functions; one partial per entry;
//   conv_grad_reduce_kernel  partials -> the two outputs, 256 strided sums and a fixed tree (grad_reduce_kernel's order);
//   conv1_points_kernel  d / d (plain side's points) of a one-sided term: one wave owns one plain point z_j, walks every
//                       image (staged CONV1_IMG at a time), lanes take the patches p = lane, lane + 64, ..., a butterfly
//                       per coordinate at the end: every output column is written by one wave -- no atomics.
// Nothing here depends on the launch order of other workgroups: two calls give the same bits.
// ======================================================================================================================
template <int DMAX>
__device__ __forceinline__ double pair_d2(const double (&r)[DMAX], const double (&c)[DMAX]) {
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = r[d] - c[d];
    d2 = fma(df, df, d2);
  }
  return d2;
}

__device__ __forceinline__ double cotangent(const double* Gm, long ld, const double* alpha, long r, long c) {
  return alpha ? 0.5 * (alpha[r] * alpha[c] - Gm[r + c * ld]) : Gm[r + c * ld];
}

// conv2_sum with the derivative beside the value
template <int DMAX, bool EXACT>
__device__ __forceinline__ void conv2_sum_kd(const double* imr, const ConvSide& gr, const int (&offr)[DMAX], const double* imc,
                                             const ConvSide& gc, const int (&offc)[DMAX], int D, int kind, double param,
                                             int lane, double& sk, double& sd) {
  sk = sd = 0.0;
  for (int p = lane; p < gr.np; p += 64) {
    double a[DMAX];
    load_patch<DMAX, EXACT>(a, imr, (p % gr.np_r) + (p / gr.np_r) * gr.h, offr, D);
    for (int qc = 0, base0 = 0; qc < gc.np / gc.np_r; ++qc, base0 += gc.h) {
#pragma unroll 2
      for (int qr = 0; qr < gc.np_r; ++qr) {
        double b[DMAX], k, dk;
        load_patch<DMAX, EXACT>(b, imc, base0 + qr, offc, D);
        kern_and_dscale(kind, pair_d2<DMAX>(a, b), param, k, dk);
        sk = sk + k;
        sd = sd + dk;
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sk = sk + __shfl_xor(sk, m, 64);
    sd = sd + __shfl_xor(sd, m, 64);
  }
}

// conv1_sums with the derivative beside the value (the kernels are symmetric in their arguments: no orientation)
template <int DMAX, bool EXACT, int CC>
__device__ __forceinline__ void conv1_sums_kd(double (&sk)[CC], double (&sd)[CC], const double* img, const ConvSide& g,
                                              const int (&off)[DMAX], int D, const double (&pt)[CC][DMAX], int kind,
                                              double param) {
  for (int pc = 0, base0 = 0; pc < g.np / g.np_r; ++pc, base0 += g.h) {
    for (int pr = 0; pr < g.np_r; ++pr) {
      double a[DMAX];
      load_patch<DMAX, EXACT>(a, img, base0 + pr, off, D);
#pragma unroll
      for (int k = 0; k < CC; ++k) {
        double kv, dk;
        kern_and_dscale(kind, pair_d2<DMAX>(a, pt[k]), param, kv, dk);
        sk[k] = sk[k] + kv;
        sd[k] = sd[k] + dk;
      }
    }
  }
}

// the four waves' sums (a, b), identical in every lane of a wave, added in wave order into partials[2 blk], [2 blk + 1]
__device__ __forceinline__ void block_partial(double a, double b, double* red /* 8 doubles of LDS */, double* partials, long blk,
                                              int t) {
  __syncthreads();
  if ((t & 63) == 0) {
    red[(t >> 6) * 2 + 0] = a;
    red[(t >> 6) * 2 + 1] = b;
  }
  __syncthreads();
  if (t < 2) partials[blk * 2 + t] = ((red[t] + red[2 + t]) + red[4 + t]) + red[6 + t];
}

template <int DMAX, bool EXACT>
__global__ __launch_bounds__(256) void conv2_grad_kernel(const double* __restrict__ Gm, long ldg,
                                                         const double* __restrict__ alpha, long r0, long nr, long c0,
                                                         long nc, const DevTerm* __restrict__ terms,
                                                         double* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const DevTerm T = terms[0];
  const int HWr = T.hr * T.wr, HWc = T.hc * T.wc, D = T.ph * T.pw;
  double* red = smem + HWr + CONV2_WAVES * HWc;                 // 8 doubles behind the images (all of the LDS is dynamic)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long lr = blockIdx.x;                                   // row within the pair (< nr: the grid)
  const long lc_beg = (long)blockIdx.y * TILE, lc_end = std::min<long>(nc, lc_beg + TILE);
  const ConvSide gr = conv_side(T.hr, T.wr, T.ph, T.pw), gc = conv_side(T.hc, T.wc, T.ph, T.pw);
  int offr[DMAX], offc[DMAX];
  patch_offsets<DMAX>(offr, T.ph, T.hr, D);
  patch_offsets<DMAX>(offc, T.ph, T.hc, D);
  stage(smem, T.xr + lr * (long)HWr, HWr, t, 256);
  const double wr = T.rs ? T.rs[lr] : 1.0;
  double a = 0.0, b = 0.0;
  for (long lc0 = lc_beg; lc0 < lc_end; lc0 += CONV2_WAVES) {
    const int ncol = (int)std::min<long>(CONV2_WAVES, lc_end - lc0);
    __syncthreads();     // the previous group's images are no longer read
    for (int k = 0; k < ncol; ++k) stage(smem + HWr + k * HWc, T.xc + (lc0 + k) * (long)HWc, HWc, t, 256);
    __syncthreads();
    if (wv < ncol) {
      const long lc = lc0 + wv;
      double sk, sd;
      conv2_sum_kd<DMAX, EXACT>(smem, gr, offr, smem + HWr + wv * HWc, gc, offc, D, T.kind, T.param, lane, sk, sd);
      const double w = (cotangent(Gm, ldg, alpha, r0 + lr, c0 + lc) * wr) * (T.cs ? T.cs[lc] : 1.0);
      a = fma(w, sk, a);
      b = fma(w * T.coef, sd, b);
    }
  }
  block_partial(a, b, red, partials, (long)blockIdx.y * gridDim.x + blockIdx.x, t);
}

template <int DMAX, bool EXACT>
__global__ __launch_bounds__(256) void conv1_grad_kernel(const double* __restrict__ Gm, long ldg,
                                                         const double* __restrict__ alpha, long r0, long nr, long c0,
                                                         long nc, const DevTerm* __restrict__ terms,
                                                         double* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const DevTerm T = terms[0];
  const bool row_img = T.hr > 0;
  const int H = row_img ? T.hr : T.hc, W = row_img ? T.wr : T.wc, HW = H * W;
  double* red = smem + CONV1_IMG * HW;                           // 8 doubles behind the images
  const int D = T.ph * T.pw;
  const long na = row_img ? nr : nc, nb = row_img ? nc : nr;     // images / plain points of the pair (local indices)
  const double* ximg = row_img ? T.xr : T.xc;
  const double* xpt = row_img ? T.xc : T.xr;
  const long ldpt = row_img ? T.ldc : T.ldr;
  const int t = threadIdx.x;
  const long a_first = (long)blockIdx.x * CONV1_IMG;
  const int nimg = (int)std::min<long>(CONV1_IMG, na - a_first);
  for (int k = 0; k < nimg; ++k) stage(smem + k * HW, ximg + (a_first + k) * (long)HW, HW, t, 256);
  __syncthreads();
  long bl[CONV1_CC];
  double pt[CONV1_CC][DMAX];
#pragma unroll
  for (int k = 0; k < CONV1_CC; ++k) {
    bl[k] = (long)blockIdx.y * (256 * CONV1_CC) + t + 256 * k;
    load_point<DMAX, EXACT>(pt[k], xpt + (bl[k] < nb ? bl[k] : 0) * ldpt, D);   // (out of range: a valid point, weight 0)
  }
  const ConvSide g = conv_side(H, W, T.ph, T.pw);
  int off[DMAX];
  patch_offsets<DMAX>(off, T.ph, H, D);
  double a = 0.0, b = 0.0;
  if (bl[0] < nb) {
    for (int k = 0; k < nimg; ++k) {
      const long al = a_first + k;
      double sk[CONV1_CC], sd[CONV1_CC];
#pragma unroll
      for (int j = 0; j < CONV1_CC; ++j) sk[j] = sd[j] = 0.0;
      conv1_sums_kd<DMAX, EXACT, CONV1_CC>(sk, sd, smem + k * HW, g, off, D, pt, T.kind, T.param);
#pragma unroll
      for (int j = 0; j < CONV1_CC; ++j) {
        if (bl[j] >= nb) continue;
        const long lr = row_img ? al : bl[j], lc = row_img ? bl[j] : al;
        const double w = (cotangent(Gm, ldg, alpha, r0 + lr, c0 + lc) * (T.rs ? T.rs[lr] : 1.0)) * (T.cs ? T.cs[lc] : 1.0);
        a = fma(w, sk[j], a);
        b = fma(w * T.coef, sd[j], b);
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    a = a + __shfl_xor(a, m, 64);
    b = b + __shfl_xor(b, m, 64);
  }
  block_partial(a, b, red, partials, (long)blockIdx.y * gridDim.x + blockIdx.x, t);
}

// sum_i w_i d var_i / d theta of ONE patch term of a diagonal pair: partials[2 i] / [2 i + 1] per entry
template <int DMAX, bool EXACT>
__global__ __launch_bounds__(64) void conv_diag_grad_kernel(const double* __restrict__ w, long n,
                                                            const DevTerm* __restrict__ terms,
                                                            double* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const DevTerm T = terms[0];
  const long i = blockIdx.x;
  const int lane = threadIdx.x;
  const int HWr = T.hr * T.wr, HWc = T.hc * T.wc, D = T.ph * T.pw;
  if (T.hr) stage(smem, T.xr + i * (long)HWr, HWr, lane, 64);
  if (T.hc) stage(smem + HWr, T.xc + i * (long)HWc, HWc, lane, 64);
  __syncthreads();
  const ConvSide gr = conv_side(T.hr, T.wr, T.ph, T.pw), gc = conv_side(T.hc, T.wc, T.ph, T.pw);
  double sk, sd;
  if (T.hr && T.hc) {
    int offr[DMAX], offc[DMAX];
    patch_offsets<DMAX>(offr, T.ph, T.hr, D);
    patch_offsets<DMAX>(offc, T.ph, T.hc, D);
    conv2_sum_kd<DMAX, EXACT>(smem, gr, offr, smem + HWr, gc, offc, D, T.kind, T.param, lane, sk, sd);
  } else {   // one side: every lane runs the sum of conv1_grad_kernel's thread for this entry
    const bool row_img = T.hr > 0;
    int off[DMAX];
    patch_offsets<DMAX>(off, T.ph, row_img ? T.hr : T.hc, D);
    double pt[1][DMAX], s1[1] = {0.0}, s2[1] = {0.0};
    load_point<DMAX, EXACT>(pt[0], row_img ? T.xc + i * T.ldc : T.xr + i * T.ldr, D);
    conv1_sums_kd<DMAX, EXACT, 1>(s1, s2, row_img ? smem : smem + HWr, row_img ? gr : gc, off, D, pt, T.kind, T.param);
    sk = s1[0], sd = s2[0];
  }
  if (lane == 0) {
    const double ww = (w[i] * (T.rs ? T.rs[i] : 1.0)) * (T.cs ? T.cs[i] : 1.0);
    partials[2 * i] = ww * sk;
    partials[2 * i + 1] = (ww * T.coef) * sd;
  }
}

// out_coef[0] / out_scale[0] = sum_b partials[2 b] / [2 b + 1] in a fixed order (blockIdx.x: the component)
__global__ __launch_bounds__(256) void conv_grad_reduce_kernel(const double* __restrict__ partials, long nblocks,
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

// gz[:, j] += scale sum_i G_ij coef rs_i cs_j sum_p 2 kappa'(|patch_p x_i - z_j|^2) (z_j - patch_p x_i)  (gz: D x nb, packed)
template <int DMAX, bool EXACT>
__global__ __launch_bounds__(256) void conv1_points_kernel(const double* __restrict__ Gm, long ldg,
                                                           const double* __restrict__ alpha, long r0, long nr, long c0,
                                                           long nc, const DevTerm* __restrict__ terms, double scale,
                                                           double* __restrict__ gz) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const DevTerm T = terms[0];
  const bool row_img = T.hr > 0;
  const int H = row_img ? T.hr : T.hc, W = row_img ? T.wr : T.wc, HW = H * W;
  const int D = T.ph * T.pw;
  const long na = row_img ? nr : nc, nb = row_img ? nc : nr;
  const double* ximg = row_img ? T.xr : T.xc;
  const double* xpt = row_img ? T.xc : T.xr;
  const long ldpt = row_img ? T.ldc : T.ldr;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long bl = (long)blockIdx.x * CONV2_WAVES + wv;           // this wave's plain point
  const bool live = bl < nb;
  double z[DMAX], acc[DMAX];
  load_point<DMAX, EXACT>(z, xpt + (live ? bl : 0) * ldpt, D);
#pragma unroll
  for (int d = 0; d < DMAX; ++d) acc[d] = 0.0;
  const ConvSide g = conv_side(H, W, T.ph, T.pw);
  int off[DMAX];
  patch_offsets<DMAX>(off, T.ph, H, D);
  for (long a_first = 0; a_first < na; a_first += CONV1_IMG) {
    const int nimg = (int)std::min<long>(CONV1_IMG, na - a_first);
    __syncthreads();     // the previous images are no longer read
    for (int k = 0; k < nimg; ++k) stage(smem + k * HW, ximg + (a_first + k) * (long)HW, HW, t, 256);
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < nimg; ++k) {
      const long al = a_first + k;
      const long lr = row_img ? al : bl, lc = row_img ? bl : al;
      const double w = 2.0 * cotangent(Gm, ldg, alpha, r0 + lr, c0 + lc) * entry_weight(T, lr, lc);
      for (int p = lane; p < g.np; p += 64) {
        double a[DMAX], df[DMAX], d2 = 0.0, kv, kx;
        load_patch<DMAX, EXACT>(a, smem + k * HW, (p % g.np_r) + (p / g.np_r) * g.h, off, D);
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
          df[d] = z[d] - a[d];
          d2 = fma(df[d], df[d], d2);
        }
        kern_val_dd2(T.kind, d2, T.param, kv, kx);
        const double wk = w * kx;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) acc[d] = fma(wk, df[d], acc[d]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    double v = acc[d];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    if (lane == 0 && d < D) gz[bl * D + d] += scale * v;
  }
}

static int conv_term_check(const DevTerm& T, const char* who) {
  const int D = T.ph * T.pw;
  if (!(T.hr || T.hc) || D < 1 || D > CONV_MAX_PATCH || T.hr * T.wr > CONV_MAX_PIXELS || T.hc * T.wc > CONV_MAX_PIXELS) {
    set_error(std::string(who) + ": not a patch term within the limits of include/sthenomi_conv.h");
    return -1;
  }
  return 0;
}

long grad_conv_partials(long nr, long nc, const DevTerm& T) {
  if (T.hr && T.hc) return 2 * nr * ((nc + TILE - 1) / TILE);
  const long na = T.hr ? nr : nc, nb = T.hr ? nc : nr;
  return 2 * ((na + CONV1_IMG - 1) / CONV1_IMG) * ((nb + 256 * CONV1_CC - 1) / (256 * CONV1_CC));
}

template <int DMAX, bool EXACT>
static int launch_grad_conv_t(const double* Gm, long ldg, const double* alpha, long r0, long nr, long c0, long nc,
                              const DevTerm& T, const DevTerm* dterm, double* partials, hipStream_t s) {
  if (T.hr && T.hc) {
    const size_t lds = sizeof(double) * ((size_t)T.hr * T.wr + (size_t)CONV2_WAVES * T.hc * T.wc + 8);
    SGP_LDS_ATTR_ONCE((conv2_grad_kernel<DMAX, EXACT>), 160 * 1024);
    dim3 grid((unsigned)nr, (unsigned)((nc + TILE - 1) / TILE));
    hipLaunchKernelGGL((conv2_grad_kernel<DMAX, EXACT>), grid, dim3(256), lds, s, Gm, ldg, alpha, r0, nr, c0, nc, dterm,
                       partials);
  } else {
    const bool row_img = T.hr > 0;
    const long na = row_img ? nr : nc, nb = row_img ? nc : nr;
    const size_t lds = sizeof(double) * ((size_t)CONV1_IMG * (row_img ? T.hr * T.wr : T.hc * T.wc) + 8);
    SGP_LDS_ATTR_ONCE((conv1_grad_kernel<DMAX, EXACT>), 160 * 1024);
    dim3 grid((unsigned)((na + CONV1_IMG - 1) / CONV1_IMG), (unsigned)((nb + 256 * CONV1_CC - 1) / (256 * CONV1_CC)));
    hipLaunchKernelGGL((conv1_grad_kernel<DMAX, EXACT>), grid, dim3(256), lds, s, Gm, ldg, alpha, r0, nr, c0, nc, dterm,
                       partials);
  }
  SGP_HIP(hipGetLastError());
  return 0;
}

int launch_grad_conv(const double* Gm, long ldg, const double* alpha, long r0, long nr, long c0, long nc, const DevTerm& T,
                     const DevTerm* dterm, double* partials, double* out_coef, double* out_scale, hipStream_t s) {
  if (nr <= 0 || nc <= 0) return 0;
  if (conv_term_check(T, "grad")) return -1;
  int rc = 0;
#define SGP_CONV_CALL(DM, EX) rc = launch_grad_conv_t<DM, EX>(Gm, ldg, alpha, r0, nr, c0, nc, T, dterm, partials, s)
  SGP_CONV_DISPATCH(T.ph * T.pw, SGP_CONV_CALL);
#undef SGP_CONV_CALL
  if (rc) return rc;
  hipLaunchKernelGGL(conv_grad_reduce_kernel, dim3(2), dim3(256), 0, s, partials, grad_conv_partials(nr, nc, T) / 2, out_coef,
                     out_scale);
  SGP_HIP(hipGetLastError());
  return 0;
}

template <int DMAX, bool EXACT>
static int launch_diag_grad_conv_t(const double* w, long n, const DevTerm& T, const DevTerm* dterm, double* partials,
                                   hipStream_t s) {
  const size_t lds = sizeof(double) * (size_t)std::max(1, T.hr * T.wr + T.hc * T.wc);
  SGP_LDS_ATTR_ONCE((conv_diag_grad_kernel<DMAX, EXACT>), 160 * 1024);
  hipLaunchKernelGGL((conv_diag_grad_kernel<DMAX, EXACT>), dim3((unsigned)n), dim3(64), lds, s, w, n, dterm, partials);
  SGP_HIP(hipGetLastError());
  return 0;
}

int launch_diag_grad_conv(const double* w, long n, const DevTerm& T, const DevTerm* dterm, double* partials /* 2 n */,
                          double* out_coef, double* out_scale, hipStream_t s) {
  if (n <= 0) return 0;
  if (conv_term_check(T, "kernelmatrix_diag_grad")) return -1;
  int rc = 0;
#define SGP_CONV_CALL(DM, EX) rc = launch_diag_grad_conv_t<DM, EX>(w, n, T, dterm, partials, s)
  SGP_CONV_DISPATCH(T.ph * T.pw, SGP_CONV_CALL);
#undef SGP_CONV_CALL
  if (rc) return rc;
  hipLaunchKernelGGL(conv_grad_reduce_kernel, dim3(2), dim3(256), 0, s, partials, n, out_coef, out_scale);
  SGP_HIP(hipGetLastError());
  return 0;
}

template <int DMAX, bool EXACT>
static int launch_grad_conv_points_t(const double* Gm, long ldg, const double* alpha, long r0, long nr, long c0, long nc,
                                     const DevTerm& T, const DevTerm* dterm, double scale, double* gz, hipStream_t s) {
  const bool row_img = T.hr > 0;
  const long nb = row_img ? nc : nr;
  const size_t lds = sizeof(double) * (size_t)CONV1_IMG * (row_img ? T.hr * T.wr : T.hc * T.wc);
  SGP_LDS_ATTR_ONCE((conv1_points_kernel<DMAX, EXACT>), 160 * 1024);
  hipLaunchKernelGGL((conv1_points_kernel<DMAX, EXACT>), dim3((unsigned)((nb + CONV2_WAVES - 1) / CONV2_WAVES)), dim3(256), lds,
                     s, Gm, ldg, alpha, r0, nr, c0, nc, dterm, scale, gz);
  SGP_HIP(hipGetLastError());
  return 0;
}

int launch_grad_conv_points(const double* Gm, long ldg, const double* alpha, long r0, long nr, long c0, long nc,
                            const DevTerm& T, const DevTerm* dterm, double scale, double* gz, hipStream_t s) {
  if (nr <= 0 || nc <= 0) return 0;
  if (conv_term_check(T, "grad (points)")) return -1;
  if (T.hr && T.hc) {
    set_error("grad (points): both sides of the term are patched");
    return -1;
  }
  int rc = 0;
#define SGP_CONV_CALL(DM, EX) rc = launch_grad_conv_points_t<DM, EX>(Gm, ldg, alpha, r0, nr, c0, nc, T, dterm, scale, gz, s)
  SGP_CONV_DISPATCH(T.ph * T.pw, SGP_CONV_CALL);
#undef SGP_CONV_CALL
  return rc;
}

}  // namespace sgp
