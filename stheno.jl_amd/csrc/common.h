// Internal definitions shared by the HIP translation units of libsthenomi.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>
#include <vector>

namespace sgp {

constexpr int TILE = 128;      // tile edge of every blocked kernel (rows and cols)
constexpr int MICRO = 16;      // MFMA f64 16x16x4 micro-tile edge
constexpr int LDS_LD = 144;    // LDS leading dimension for 128-row operand panels:
                               // 144 % 32 == 16 makes the (16 rows x 2 k) ds_read_b64 pattern
                               // of a 32-lane group hit 32 distinct 8-byte slots.

typedef double d4 __attribute__((ext_vector_type(4)));

// D = A(16x4) * B(4x16) + C on one wave.  Operand/result lane maps (guide section 3):
//   A-operand lane l holds A[m = l & 15][k = l >> 4]
//   B-operand lane l holds B[k = l >> 4][n = l & 15]
//   result    lane l, reg r holds D[m = (l >> 4) + 4 r][n = l & 15]
__device__ __forceinline__ d4 mfma_f64(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// 4-block form: D_b(4x4) = A_b(4x4) B_b(4x4) + C_b for b = 0..3, one f64 per lane
// (lane maps in gemm_nt.hip).  Issues every 16 cycles on gfx950 -- the full fp64 matrix rate.
__device__ __forceinline__ double mfma44_f64(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// ---- fp64 elementary functions of the covariance kernels -----------------------------------------
// The assembly kernel is fp64-VALU bound: libm's exp / sqrt / a true division
// cost it ~100 issue slots per Matern-5/2 entry.  These straight-line versions (no special-case
// branches; arguments are known to be <= 0 resp. >= 0) are accurate to ~1 ulp: tests/test_gpu_kernel_formulas.py holds
// the kernels built from them to a 60-digit table (SE within 2 ulp of the truth, subnormal results included; the
// measured maxima are in docs/04_oracle_and_parity.md).
// exp(x) for x <= 0: n = rint(x log2 e), r = x - n ln2 (two-part), degree-13 Taylor on |r| <= 0.347
// (remainder 4e-18), scaled by 2^n with v_ldexp_f64 (correct down to denormals / 0).
__device__ __forceinline__ double exp_nonpos(double x) {
  x = fmax(x, -800.0);
  const double n = __builtin_rint(x * 1.4426950408889634);
  double r = fma(n, -6.93147180369123816490e-01, x);
  r = fma(n, -1.90821492927058770002e-10, r);
  double p = 1.6059043836821613e-10;          // 1/13!
  p = fma(p, r, 2.08767569878681e-09);        // 1/12!
  p = fma(p, r, 2.505210838544172e-08);       // 1/11!
  p = fma(p, r, 2.755731922398589e-07);       // 1/10!
  p = fma(p, r, 2.7557319223985893e-06);      // 1/9!
  p = fma(p, r, 2.48015873015873e-05);        // 1/8!
  p = fma(p, r, 0.0001984126984126984);       // 1/7!
  p = fma(p, r, 0.001388888888888889);        // 1/6!
  p = fma(p, r, 0.008333333333333333);        // 1/5!
  p = fma(p, r, 0.041666666666666664);        // 1/4!
  p = fma(p, r, 0.16666666666666666);         // 1/3!
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return __builtin_ldexp(p, (int)n);
}
// sqrt(a) for a >= 0: v_rsq_f64 seed (~2^-26), one Newton step on 1/sqrt, then one Newton step on the
// root itself (quadratic: rounding-level result).  a is clamped to 1e-300 so that a == 0 needs no
// branch: the result is then 1e-150, which every kernel maps to exactly kappa(0) (1 + 1e-150 == 1).  It is clamped
// to 1e300 at the top as well: a squared distance that overflowed (a sentinel coordinate) gives rsq(inf) = 0 and with
// it inf * 0 = NaN in the Newton step, and the Matern-5/2 polynomial overflows from l = 1.3e154; at 1e150 every kernel
// is an exact 0 through exp_nonpos.  No finite argument below 1e300 changes a bit.
__device__ __forceinline__ double sqrt_nonneg(double a) {
  a = fmin(fmax(a, 1e-300), 1e300);
  double r = __builtin_amdgcn_rsq(a);
  r = r * fma(-0.5 * a, r * r, 1.5);
  double d = a * r;
  return fma(0.5 * r, fma(-d, d, a), d);
}

// device-side description of one covariance term of one block pair
struct DevTerm {
  int kind;
  int dim;
  double coef;
  double param;
  const double* xr;  // D x nr, first point of the row block
  long ldr;
  const double* xc;  // D x nc
  long ldc;
  const double* rs;  // row scale or nullptr
  const double* cs;  // col scale or nullptr
  // patch term (conv.hip): ph x pw patches, stride 1, of the images of a side with hr / hc > 0 -- that side's points are
  // column-major hr x wr (hc x wc) images, dim = ph * pw counts the patch; ph == 0: a plain term
  int ph, pw, hr, wr, hc, wc;
  // stencil term (stencil.hip): a side with qr / qc > 0 reads its points shifted by a registered stencil -- str (stc)
  // holds its offsets (dim x qr, column-major) followed by its qr weights on the device; qr == 0: that side is plain
  int qr, qc;
  // a term of the kind SGP_MATERN_NU (kprod.hip; never a stencil term, qr == 0): nuc points at the MN_COUNT numbers that
  // depend on nu alone, computed on the host when the spec is uploaded (matern_nu_constants) and laid out in the spec's block
  union {
    const double* str;
    const double* nuc;
  };
  const double* stc;
};

// the constants of one SGP_MATERN_NU term: nu = mu + n (n = 0: nu < 1/2 and mu = -nu), pi mu / sin(pi mu), Temme's Gamma_1 and
// Gamma_2, 1 / (2 Gamma^-1(1 + mu)) and 1 / (2 Gamma^-1(1 - mu)), 1/4 - mu^2, 2^(1-n) / Gamma(nu) and nu times it, sqrt(2 nu),
// and d k / d (d^2) at coincident points
enum { MN_N = 0, MN_MU, MN_FACT, MN_GAM1, MN_GAM2, MN_PH, MN_QH, MN_A1, MN_CA, MN_CK, MN_SQ, MN_KX0, MN_COUNT };
void matern_nu_constants(double nu, double* out /* MN_COUNT */);

// a patch geometry registered on a context (sgp_conv_geom).  Stencils (sgp_stencil_register) take their ids from the same
// table: an entry with st > 0 names the context's stencil st - 1 and no geometry (h == 0)
struct PatchGeom {
  int h, w, ph, pw;
  int st = 0;
};
// a stencil registered on a context (include/sthenomi_stencil.h): g(x) = sum_q w_q f(x - a_q)
struct StencilDesc {
  int dim, npoints;
  std::vector<double> host;   // offsets (dim x npoints, column-major), then the npoints weights
  double* dev = nullptr;      // the same on the context's device
};
constexpr int STENCIL_MAX_POINTS = 64;
constexpr int STENCIL_MAX_DIM = 16;
constexpr int CONV_MAX_PIXELS = 3072;   // images of at most this many pixels: five of them are staged in LDS at once
constexpr int CONV_MAX_PATCH = 64;      // ph * pw

// what an assembly launch writes into: the target matrix, the pair's rectangle, the tile window, and whether it is the pair's
// first launch (asm_frame.h)
struct AsmLaunch;

// conv.hip: patch terms of one block pair, one launch per term, onto what the pair's earlier launches wrote or, as its first
// launch, written afresh with the pair's noise; `dterm` is the device copy of `T`
int launch_assemble_conv(const AsmLaunch& L, const DevTerm& T, const DevTerm* dterm, hipStream_t s);
// out[i] (i < n) = the plain terms' diagonal (nplain of them, diag_terms_kernel's sum) followed by the patch terms
// terms[nplain, nterms), each summed as launch_assemble_conv sums entry (i, i).  max_d: the widest patch of those terms,
// d_all: their common patch dimension (0: they differ), max_pixels: the most image pixels (row + column side) of one term
int launch_diag_conv(double* out, long n, const DevTerm* d_terms, int nplain, int nterms, int max_d, int d_all,
                     int max_pixels, hipStream_t s);

// conv.hip, the gradient contractions against ONE patch term of a block pair (include/sthenomi_conv_grad.h); G as in
// launch_grad_block (alpha != nullptr: (alpha alpha' - Gm) / 2, else Gm itself), indexed globally: entry (i, j) of the pair at
// Gm[r0 + i + (c0 + j) * ldg].  out_coef[0] = sum_ij G_ij rs_i cs_j sum_pq k, out_scale[0] = sum_ij G_ij coef rs_i cs_j
// sum_pq dk/dg; `partials` holds grad_conv_partials(nr, nc, T) doubles (per-workgroup sums, reduced in a fixed order)
long grad_conv_partials(long nr, long nc, const DevTerm& T);
int launch_grad_conv(const double* Gm, long ldg, const double* alpha, long r0, long nr, long c0, long nc, const DevTerm& T,
                     const DevTerm* dterm, double* partials, double* out_coef, double* out_scale, hipStream_t s);
// ... on the diagonal: sum_i w_i d var_i / d theta of one patch term; `partials`: 2 n doubles
int launch_diag_grad_conv(const double* w, long n, const DevTerm& T, const DevTerm* dterm, double* partials, double* out_coef,
                          double* out_scale, hipStream_t s);
// ... with respect to the PLAIN side's points of a one-sided term: gz (ph pw x points, packed) += scale * the sum over the
// images and their patches; one wave owns a point (no atomics)
int launch_grad_conv_points(const double* Gm, long ldg, const double* alpha, long r0, long nr, long c0, long nc,
                            const DevTerm& T, const DevTerm* dterm, double scale, double* gz, hipStream_t s);

// stencil.hip: stencil terms of one block pair, one launch per term, arguments as launch_assemble_conv
int launch_assemble_stencil(const AsmLaunch& L, const DevTerm& T, const DevTerm* dterm, hipStream_t s);
// out[i] (i < n) = fma(s_t(i), w_t(i), out[i]) for the stencil terms t in order, s_t(i) summed as launch_assemble_stencil
// sums entry (i, i); out holds the pair's plain and patch diagonal.  max_dim: the largest input dimension of those terms
int launch_diag_stencil(double* out, long n, const DevTerm* d_terms, int nterms, int max_dim, hipStream_t s);

// stencil.hip, the gradient contractions against ONE stencil term of a block pair (include/sthenomi_stencil_grad.h); G and
// its indexing as for launch_grad_conv.  out_coef[0] = sum_ij G_ij rs_i cs_j sum_pq w_p v_q k, out_scale[0] = sum_ij G_ij
// coef rs_i cs_j sum_pq w_p v_q dk/dg; `partials` holds grad_stencil_partials(r0, nr, c0, nc, T) doubles (per-workgroup
// sums, reduced in a fixed order)
long grad_stencil_partials(long r0, long nr, long c0, long nc, const DevTerm& T);
int launch_grad_stencil(const double* Gm, long ldg, const double* alpha, long r0, long nr, long c0, long nc, const DevTerm& T,
                        const DevTerm* dterm, double* partials, double* out_coef, double* out_scale, hipStream_t s);
// ... on the diagonal: sum_i w_i d var_i / d theta of one stencil term; `partials`: 2 n doubles
int launch_diag_grad_stencil(const double* w, long n, const DevTerm& T, const DevTerm* dterm, double* partials,
                             double* out_coef, double* out_scale, hipStream_t s);
// ... with respect to the row side's points: gx (dim x nr, packed) += scale * the row-side sum, G addressed as for
// launch_grad_inputs; transpose != 0: the term seen from its column points (sides and stencils swapped; the caller passes the
// column block as (r0, nr), the row block as (c0, nc) and the strides of the transposed cotangent)
int launch_grad_stencil_points(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                               const DevTerm& T, int transpose, double scale, double* gx, hipStream_t s);
// ... on the diagonal: gxr += / gxc -= the per-entry sums (either may be NULL; gxr == gxc: the two cancel, nothing is launched)
int launch_diag_grad_stencil_points(const double* w, long n, const DevTerm& T, double* gxr, double* gxc, hipStream_t s);
// ... with respect to the weights and offsets of ONE side's stencil (include/sthenomi_stencil_wo.h): out_w[p] (npoints) and
// out_o[p * dim + d] (the layout of sgp_stencil.offsets) on the device, overwritten; either may be NULL.  G addressed and
// `transpose` as for launch_grad_stencil_points: 0 differentiates the row side's stencil, != 0 the column side's.  A plain
// side is refused.  `partials` holds grad_stencil_wo_partials(nr, nc, T, transpose) doubles (nr, nc: the launch's, after the
// swap), reduced in a fixed order
long grad_stencil_wo_partials(long nr, long nc, const DevTerm& T, int transpose);
int launch_grad_stencil_wo(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                           const DevTerm& T, int transpose, double* partials, double* out_w, double* out_o, hipStream_t s);
// ... on the diagonal: `partials` holds diag_grad_stencil_wo_partials(n, T, transpose) doubles
long diag_grad_stencil_wo_partials(long n, const DevTerm& T, int transpose);
int launch_diag_grad_stencil_wo(const double* w, long n, const DevTerm& T, int transpose, double* partials, double* out_w,
                                double* out_o, hipStream_t s);

// kprod.hip: product chains and the RQ / LINEAR kinds (include/sthenomi_kprod.h).  The terms of one launch are whole chains;
// kprod_group cuts a pair's chain terms [t, t1) into launches (returns how many terms the launch at t carries, *dmax_out = its
// DMAX) for the matrix and the diagonal alike.  Arguments of launch_assemble_kprod as launch_assemble_block.
// Every launcher takes the host copies of its terms (h_terms; where the kernel reads them from device memory, d_terms too,
// as launch_grad_conv does) and picks the kernel instantiation from their kinds: kprod_kinds_table.h
int kprod_group(const DevTerm* h_terms, int t, int t1, int* dmax_out);
int launch_assemble_kprod(const AsmLaunch& L, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int dmax,
                          hipStream_t s);
// out[i] (i < n) = (accumulate ? out[i] : 0) + the chains of one launch group, summed as launch_assemble_kprod sums entry (i, i)
int launch_diag_kprod(double* out, long n, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int accumulate,
                      hipStream_t s);
// gradient contraction of ONE chain (nf factors at d_terms): out_coef / out_scale / out_param point at the chain's first entry
// (nf each; any may be NULL); partials: tile rows x tile columns x 24 doubles
int launch_grad_kprod(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                      const DevTerm* h_terms, const DevTerm* d_terms, int nf, int dmax, long trf, long tcf, long trc,
                      long tcc, double* partials, double* out_coef, double* out_scale, double* out_param, hipStream_t s);

// input-point gradients and the head's row-scale sums of ONE chain over one block pair (kprod.hip: grad_kprod_inputs_kernel):
// h_terms the chain's nf factors (host copies), gx[f] the gradient of factor f's row input (NULL: not asked for), G addressed
// as for launch_grad_inputs; transpose != 0: every factor seen from its column points (column side of a rectangular block)
int launch_grad_kprod_inputs(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                             const DevTerm* h_terms, int nf, int dmax, int transpose, double scale, double* const* gx,
                             double* gsv, hipStream_t s);
// sum_i w_i d var_i / d theta of ONE chain on the diagonal (kprod.hip: diag_grad_kprod_kernel); every output may be NULL
int launch_diag_grad_kprod(const double* w, long n, const DevTerm* h_terms, int nf, double* out_coef, double* out_scale,
                           double* out_param, double* const* gxr, double* const* gxc, double* out_rs, double* out_cs,
                           hipStream_t s);

// deriv.hip: the derivative kinds (include/sthenomi.h: SGP_DERIV_*), a term class of its own.  A launch carries ONE group of a
// pair's derivative terms (deriv_kinds.h: deriv_group -- the same base kind, points and scale vectors), host copies at h_terms,
// device copies at d_terms.  Arguments of launch_assemble_deriv as launch_assemble_block.
int launch_assemble_deriv(const AsmLaunch& L, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, hipStream_t s);
// out[i] (i < n) = (accumulate ? out[i] : 0) + the group, summed as launch_assemble_deriv sums entry (i, i)
int launch_diag_deriv(double* out, long n, const DevTerm* h_terms, const DevTerm* d_terms, int nterms, int accumulate,
                      hipStream_t s);
// gradient contraction of one group: out_coef / out_scale point at the group's first entry (nterms each); partials:
// grad_deriv_partials(trc, tcc) doubles, reduced in a fixed order.  G as in launch_grad_block
long grad_deriv_partials(long trc, long tcc);
int launch_grad_deriv(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                      const DevTerm* h_terms, const DevTerm* d_terms, int nterms, long trf, long tcf, long trc, long tcc,
                      double* partials, double* out_coef, double* out_scale, hipStream_t s);

void set_error(const std::string& s);

#define SGP_HIP(expr)                                                                     \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      sgp::set_error(std::string(#expr) + ": " + hipGetErrorString(_e) + " at " + __FILE__ + \
                     ":" + std::to_string(__LINE__));                                     \
      return -2;                                                                          \
    }                                                                                     \
  } while (0)

// the host-side early returns of every unit: a refused argument (-1, error text set) and a failed step (its code)
#define CHECK_ARG(cond, msg)       \
  do {                             \
    if (!(cond)) {                 \
      sgp::set_error(msg);         \
      return -1;                   \
    }                              \
  } while (0)
#define CHECK_RC(expr)        \
  do {                        \
    int _rc = (expr);         \
    if (_rc != 0) return _rc; \
  } while (0)
// a refusal that names the entry point it came through
#define REFUSE_UNLESS(cond, who, msg)                     \
  do {                                                    \
    if (!(cond)) {                                        \
      sgp::set_error(std::string(who) + ": " + (msg));    \
      return -1;                                          \
    }                                                     \
  } while (0)

// Raise a kernel's dynamic-LDS limit once per device (function attributes are per device; a process
// may hold contexts on several GPUs).
#define SGP_LDS_ATTR_ONCE(func, bytes)                                                              \
  do {                                                                                             \
    static std::atomic<bool> done_[64];                                                                  \
    int dev_ = 0;                                                                                  \
    SGP_HIP(hipGetDevice(&dev_));                                                                  \
    if (dev_ >= 0 && dev_ < 64 && !done_[dev_]) {                                                  \
      SGP_HIP(hipFuncSetAttribute((const void*)(func), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  (int)(bytes)));                                                  \
      done_[dev_] = true;                                                                          \
    }                                                                                              \
  } while (0)

// ---- launchers implemented in the .hip files -------------------------------------------
// kernelmatrix.hip
int launch_assemble_block(const AsmLaunch& L, const DevTerm* d_terms, int nterms, int dmax, hipStream_t s);
int assemble_terms_per_launch(int dmax);  // how many terms one launch_assemble_block may carry (LDS)
int launch_rows_dot(const double* rows, long ld, long nrows, long nc, const double* zrow, double* sumsq,
                    double* dot, hipStream_t s);
int launch_zero_rows(double* A, long ld, long r0, long r1, long nc, hipStream_t s);
int launch_fill_pad(double* K, long ld, long N, long n_pad, long c0, long nc, long m_tot,
                    long row_lo, hipStream_t s);
int launch_border_rows(double* A, long ld, long n_pad, long N, long c0, long nc, const double* dY,
                       long ldy, long ncols, const double* d_mean, hipStream_t s);
int launch_diag_terms(double* out, long n, const DevTerm* d_terms, int nterms, hipStream_t s);
int launch_add_dense(double* K, long ld, const double* S, long lds, long N, int lower_only,
                     hipStream_t s);
int launch_add_dense_cols(double* P, long ldp, const double* S, long lds, long c0, long w, long N, hipStream_t s);
int launch_mirror_lower(double* K, long ld, long N, hipStream_t s);

// gemm_nt.hip : C = beta*C + alpha * A B'   (A: M x K, B: Nc x K, all column-major)
// tiles (tr, tc) with tr < tc + mask_off are skipped.  kcap_mode: per-tile K limited to
// (tc + 1) * 128 + kcap_off (used by L*Z products where only the lower triangle of B is valid).
int launch_gemm_nt(const double* A, long lda, const double* B, long ldb, double* C, long ldc,
                   long M, long Nc, long K, double alpha, double beta, long mask_off,
                   int kcap_mode, long kcap_off, hipStream_t s);
int launch_gemm_nt_update(const double* P, long ldp, double* C, long ldc, long M, long Nc, long K, hipStream_t s);
// the same lower update with potrf_diag of tile (0, 0) -- the next diagonal block -- fused into its workgroup
int launch_gemm_nt_potrf(const double* P, long ldp, double* C, long ldc, long M, long Nc, long K, int outer,
                         int handoff, double* d_invd, double* d_logdet_slot, int* d_info, long gcol0,
                         hipStream_t s);
// Structural zeros (round 4).  A Stheno programme with independent components has EXACT zero blocks in its covariance (no
// term connects the two processes: cross.jl gives zeros), and so has its Cholesky factor; the reference's dense LAPACK path
// multiplies them out.  capi.hip: sz_build derives the tile-level pattern of the factor (symbolic factorisation with
// fill-in) and the factorisation skips every tile product one of whose operands is structurally zero -- the skipped
// products are exact zeros, so the factor keeps its bits.  nz: one row of `words` 64-bit words per tile row of the
// bordered matrix, bit k = tile (row, k) of the factor may be non-zero.
typedef unsigned long long sz_word;
struct TileSkip {      // per launch of a lower update C -= P P': C's first tile row / column, the k tiles the panel covers
  const sz_word* nz = nullptr;
  int words = 0, tr0 = 0, tc0 = 0, kt0 = 0, kt1 = 0;
  // big launches: the live tiles of every XCD compacted to the front of its id sequence (tile_compact_kernel): cmap[x] =
  // live ids of XCD x, cmap[16 + x * cstride + pos] = the pos-th live id / 8 -- the live tiles keep the order, and with it
  // the lock-step operand sharing, of the dense enumeration
  const int* cmap = nullptr;
  int cstride = 0;
  // round 5 (the gradient's C^-1 = inv(L)' inv(L), launch_gemm_nt_uut): >= 0: pattern row need0 + tr says which tiles (tr, tc)
  // of the RESULT anyone reads -- the tiles of block pairs with terms (+ the diagonal); the others are not computed
  int need0 = -1;
};
// while set (chol_bordered's scope; per host thread), the lower updates launched on tiles of `base` skip dead tiles;
// scratch (optional, only for launches that are ordered on one stream): room for the compacted id maps
// tile0 (round 5): the global tile coordinate of base[0] -- 0 for the bordered matrix itself, c0 / 128 for a PACKED column
// panel of the sharded factorisation (its element [0] is (row c0, column c0) of the matrix), so that the launches of a
// panel's own factorisation find their tiles in the pattern too
// (scratch / scratch_ints: room for the compacted live-tile id map of a launch; stream2 / scratch2: a second map of the same
// size for the launches of that other stream -- launches of one stream are ordered, so a map per stream is enough)
// ncols: the columns of the matrix at `base` (pointers beyond base + ld * ncols are not part of it and get no pattern)
void gemm_set_structure(const double* base, long ld, const sz_word* d_nz, int words, long ncols = 0, int* scratch = nullptr,
                        long scratch_ints = 0, long tile0 = 0, hipStream_t stream2 = nullptr, int* scratch2 = nullptr);
// the panel solve X <- X inv(L_kk)' over rows of the structured matrix: 128-row tiles of X whose tile (row, k) is structurally
// zero are left alone (they hold the exact zeros the assembly wrote).  nz == nullptr: every row is solved.
struct StripSkip {
  const sz_word* nz = nullptr;
  int words = 0, tr0 = 0, kt = 0;   // tile row of X's first row, k tile of the block column
};
StripSkip strip_skip_for(const double* X, long ldx);   // from the per-thread structure record (gemm_nt.hip), or an empty one
// the fp32 instantiation (f32.hip, round 6): the same record over a float matrix; its update launches keep the dense tile
// enumeration (no compacted id maps) and skip / trim per workgroup
void gemm_set_structure_f32(const float* base, long ld, const sz_word* d_nz, int words, long ncols);
TileSkip gemm_skip_for_f32(const float* P, long ldp, const float* C, long ldc, long K);
StripSkip strip_skip_for_f32(const float* X, long ldx);
// chol_df.hip: the whole bordered factorisation (lower tiles of the n_pad columns + rows n_pad .. m_tot) in one launch of
// persistent workgroups; d_state: df_state_words(m_tot, 1) ints, d_invall: n_pad / 128 x 2048 doubles
constexpr int SGP_DF_TIMEOUT = -77;   // *info when a dependency wait inside the kernel ran into its bound
// One matrix of a launch (a batch holds up to DF_MAX_BATCH equally shaped ones: launch_chol_dataflow_batch)
constexpr int DF_MAX_BATCH = 16, DF_MAX_EXT = 2;
struct DfProb {
  double* A;        // m_tot x n_pad, column-major, lower tiles + bordered rows
  double* invall;   // n_pad / 128 x 2048 doubles: inverse 16x16 diagonal blocks of every 128-block
  double* slots;    // n_pad / 128 logdet contributions
  int* info;
};
// A factored column panel LEFT of the matrix a panel launch works on (round 6, the sharded factorisation): base points at the
// source's element (row of A's first row, first column of the source), kt0 = global tile column of that first column, kt =
// its tile columns.  Every task contracts the sources first, in the order given (k ascending).
struct DfExt {
  const double* base;
  long ld;
  int kt0, kt;
};
struct DfPanel {    // launch_chol_dataflow's optional extension: factor only the first n_fact columns (the others: update-only)
  long n_fact = 0;
  int n_ext = 0;
  DfExt ext[DF_MAX_EXT];
};
int launch_chol_dataflow(double* A, long ld, long n_pad, long m_tot, int* d_state, double* d_invall, double* d_slots,
                         int* d_info, int n_wg, double timeout_s, hipStream_t s, long long* d_stats = nullptr,
                         long long* d_cols = nullptr, int fat = 0, const sz_word* d_nz = nullptr, int nz_words = 0,
                         long gcol_base = 0, const DfPanel* px = nullptr);
int launch_chol_dataflow_batch(const DfProb* probs, int nb, long ld, long n_pad, long m_tot, int* d_state, int n_wg,
                               double timeout_s, int fat, hipStream_t s, const sz_word* d_nz = nullptr, int nz_words = 0);
long df_state_words(long m_tot, int nb);   // ints of d_state a launch needs
// A RAGGED pool (chol_df.hip: chol_pool_kernel; df_pool.h): up to DF_MAX_BATCH independent matrices of DIFFERENT shapes as one
// task pool -- every member with its own tile grid, leading dimension and (optional) structural-zero pattern
struct DfPoolMember {
  DfProb p;
  long ld;
  int T_r, T_c;           // tile rows (m_tot / 128), tile columns (n_pad / 128) of this member
  const sz_word* nz;      // its own pattern (bit k of row i = tile (i, k) may be non-zero) or nullptr: dense
  int nzw;                // words per pattern row
};
long df_pool_state_words(const DfPoolMember* mem, int nb);   // SGP_DF_STATE_WORDS + the sum of the members' tile rows
// d_order: the table df_pool_order (df_pool.h) builds for exactly these shapes, ntasks entries, final on s before the launch
int launch_chol_pool(const DfPoolMember* mem, int nb, int* d_state, const uint32_t* d_order, long ntasks, int n_wg,
                     double timeout_s, int fat, hipStream_t s);
constexpr long SGP_DF_STATE_WORDS = 16;   // state words ahead of the per-tile-row progress counters
int launch_gemm_nt_stamps(const double* P, long ldp, double* C, long ldc, long M, long Nc, long K, long long* dbg,
                          long* n_ids, hipStream_t s);   // bench: per-workgroup phase stamps of one lower update
// batched, segmented trailing update (gemm_nt.hip: gemm_nt_seg_kernel): destination panels, each with a range of source panels
constexpr int SEG_MAX_SRC = 8, SEG_MAX_DST = 16;
struct SegSrc {      // a factored column panel, packed: element (global row r, local column k) at base[(r - row0) + k * ld]
  const double* base;
  long ld, row0;
  int w;
  long k0 = -1;      // global column of the first column (a sub-panel: row0 + its offset); -1: row0.  Only the structural-
                     // zero test reads it.
};
struct SegDst {      // an owned column panel, packed: element (global row r, global column c) at C[(r - c0) + (c - c0) * ldc]
  double* C;
  long ldc, c0;
  int w, s_first, s_count;
  unsigned id0;      // (filled in by the launcher)
};
struct SegBatch {
  SegSrc src[SEG_MAX_SRC];
  SegDst dst[SEG_MAX_DST];
  int n_dst;
  long m_tot;
  const sz_word* nz = nullptr;   // structural zeros (above): a tile skips the sources all of whose k tiles are dead for it
  int nz_words = 0;
  // round 6: room for the compacted live-tile id map of a big structured launch (launches of ONE stream only: they are
  // ordered); nullptr: the dead ids leave where they stand.  cmap / cstride: filled in by the launcher.
  int* map_scratch = nullptr;
  long map_ints = 0, map_min_ids = 4096;   // (smaller launches are not worth the extra kernel; tests lower the bound)
  const int* cmap = nullptr;
  int cstride = 0;
};
int launch_gemm_nt_seg(SegBatch& b, hipStream_t s, long* n_ids = nullptr);
int launch_gemm_nt_cin(const double* A, long lda, const double* B, long ldb, const double* Cin, long ldcin,
                       double* C, long ldc, long M, long Nc, long K, double alpha, double beta,
                       hipStream_t s);
int launch_gemm_nt_lz(const double* L, long ldl, const double* Zt, long ldz, double* C, long ldc, long n,
                      long ns, double beta, hipStream_t s);
int launch_gemm_nt_lz_k(const double* L, long ldl, const double* Zt, long ldz, double* C, long ldc, long n,
                        long ns, long K, double beta, hipStream_t s);
int launch_gemm_nt_uut(const double* X, long ldx, double* C, long ldc, long n, hipStream_t s, const TileSkip* sk = nullptr);
// the same product for nb <= DF_MAX_BATCH equally sized members in ONE launch (the member is blockIdx.z): member b computes
// C[b] = X[b] X[b]' with exactly the dense tile program of launch_gemm_nt_uut (no TileSkip), so its bits are that call's
int launch_gemm_nt_uut_batch(const double* const* X, long ldx, double* const* C, long ldc, long n, int nb, hipStream_t s);
int launch_gemm_nt_splitk(const double* A, long lda, const double* B, long ldb, double* Cpart, long ldc,
                          long M, long Nc, long K, int nsplit, long part_stride, int lower_only,
                          hipStream_t s);
int launch_splitk_reduce(const double* part, long part_stride, int nsplit, double* C, long ldc, long M,
                         long Nc, double alpha, double beta, int lower_only, hipStream_t s, long K = 0, long ld_part = 0);
long splitk_sub(long M, long K);                 // further k split of the Gram product's leftover tiles (gemm_nt.hip)
long splitk_slabs(long M, long K, int nsplit);   // slabs launch_gemm_nt_splitk writes for this shape

// grad.hip
int launch_grad_block(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                      const DevTerm* d_terms, int nterms, int dmax, long trf, long tcf, long trc, long tcc,
                      double* partials, double* out_coef, double* out_scale, hipStream_t s, int accumulate = 0,
                      long clo = -(1L << 60), long chi = (1L << 60));   // accumulate into out_*; column window [clo, chi)
int launch_diag_grad(const double* w, long n, const DevTerm* d_terms, int nterms, double* out_coef,
                     double* out_scale, hipStream_t s);
int launch_diag_scale_grad(const double* w, long n, const DevTerm& T, double* out_rs, double* out_cs, hipStream_t s);
int launch_vfe_zs(const double* B, const double* Binv, const double* u, double* Z, double* S, long m,
                  hipStream_t s);
int launch_vfe_rowstats(const double* R, long ld, const double* RZ, long ldrz, const double* u,
                        const double* delta, const double* rsig, const double* var_x, long N, long m,
                        double* gy, double* gsy, hipStream_t s);
int launch_vfe_gxz(double* E, long ld, const double* delta, const double* ut, const double* rsig, long nrows,
                   long m, hipStream_t s);
int launch_grad_inputs(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                       const DevTerm& T, int dmax, double scale, double* gx, hipStream_t s, double* gsv = nullptr);
int launch_diag_grad_inputs(const double* w, long n, const DevTerm& T, double* gxr, double* gxc, hipStream_t s);
int launch_grad_border(double* A, long ld, long n_pad, long N, const double* y, const double* mean,
                       long nrows, hipStream_t s);
int launch_grad_noise(const double* Kinv, long ldk, const double* alpha, long N, int diag, double* out,
                      hipStream_t s);
int launch_grad_noise_dense(const double* Kinv, long ldk, const double* alpha, long N, double* out, hipStream_t s);
int launch_grad_noise_dense_cols(const double* Kinv, long ldk, const double* alpha, long N, long c0, long w, double* out, long ldo,
                                 hipStream_t s);

// potrf.hip
int launch_potrf_diag(double* A, long ld, double* d_invd, double* d_logdet_slot, int* d_info,
                      long gcol0, hipStream_t s);
int launch_potrf_diag_dbg(double* A, long ld, double* d_invd, double* d_logdet_slot, int* d_info, long long* dbg,
                          hipStream_t s);
int launch_panel_solve(double* X, long ldx, long rows, const double* L, long ldl, const double* inv,
                       long inv_cstride, long inv_kstride, hipStream_t s, const StripSkip* sk = nullptr, long div = 256);
// fp32 storage, fp64 arithmetic: the panel kernels of the fp32 instantiation (f32.hip)
int launch_potrf_diag_f32(float* A, long ld, double* d_invd, double* d_logdet_slot, int* d_info, long gcol0,
                          hipStream_t s);
int launch_panel_solve_f32(float* X, long ldx, long rows, const float* L, long ldl, const double* inv,
                           long inv_cstride, long inv_kstride, hipStream_t s, const StripSkip* sk = nullptr);

// reduce.hip
int launch_rowsumsq(const double* rows, long ld, long nc, long nrows, double* out, int accumulate,
                    hipStream_t s);
int launch_sum_array(const double* in, long n, double* out, hipStream_t s);
int launch_logpdf_final(const double* d_logdet, const double* d_sq, long N, long ncols,
                        double* d_out, hipStream_t s);
int launch_colsumsq_sub(const double* V, long ld, long nrows, long ncols, const double* prior,
                        double* out, double sign, hipStream_t s);
int launch_gemv_rows(const double* rows, long ld, long nrows, long nc, const double* z, long ldz,
                     const double* add, double* out, hipStream_t s, int upper_tri = 0);
// transposition + column sums in one pass (the ELBO's chunked pipeline): dst = (diag(row_scale) src)', dots[c] (+)= sum_r v delta[r],
// sq[c] (+)= sum_r v^2; scratch: transpose_colsum_scratch(nr, nc) doubles
long transpose_colsum_scratch(long nr, long nc);
int launch_transpose_colsum(const double* src, long lds, long nr, long nc, double* dst, long ldd, const double* row_scale,
                            const double* delta, double* dots, double* sq, int accumulate, double* scratch, hipStream_t s);
int launch_transpose_add(const double* src, long lds, long nr, long nc, double* dst, long ldd,
                         const double* add_vec, hipStream_t s);   // row_scale: src row r is multiplied by row_scale[r]
int launch_scale_rows(double* rows, long ld, long nrows, long nc, const double* scale,
                      hipStream_t s);

}  // namespace sgp
