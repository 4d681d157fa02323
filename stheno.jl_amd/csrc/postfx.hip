// rand / logpdf of a posterior FiniteGP f_post(x*, S*) against the kept factor (include/sthenomi_postfx.h).
//
// What a host does without these entry points: fetch cov(f_post, x*) (sgp_posterior_predict, cov_out) and mean(f_post, x*),
// add S* to the covariance itself and hand the sum back as dense noise on a zero-term spec to sgp_logpdf / sgp_rand -- two
// N*^2 transfers around the factorisation.  Here the same launches run in the same order with the N*^2 buffers left where
// they are, so the result keeps the bits of that route:
//   V (and C), m*                              the solved cross rows and the mean off them: kept.h, shared with predict
//   C*  <- K(x*, x*) - V V' (+ C C')           straight into the bordered buffer of sgp_geometry(N*, ncols or 0), lower tiles
//   C*  += S*                                  ONE add per entry of the tiles the factorisation reads, as the host's C + S*
//   identity padding, border rows (Y - m*)'    (launch_fill_pad, launch_border_rows: what build_bordered runs)
//   the bordered factorisation, dense schedule, and the tail of sgp_logpdf (launch_logpdf_final) or sgp_rand (m* + L* Z)
// The product K** - V V' runs on the lower tiles only (mask_off == 0): launch_gemm_nt enumerates fewer tiles of the same
// kernel, every tile it computes contracts k in the same order as the full product -- the factorisation never reads the others.
// Every launch is ordered on the context's stream; no kernel here waits on another workgroup.
#include "kept.h"

#include <string>

using namespace sgp;

namespace {

// K[r, c] += S*[r, c] for a scalar or diagonal S* on the tiles the factorisation reads (tile row >= tile column): the diagonal
// receives sigma2 (scalar) or diag[r], every other entry the zero the host's dense S* holds there -- sigma2 * eye(N) and
// diag(v) in NumPy -- so that each entry sees the one IEEE add of the host route, signed zeros and non-finite sigma2 included.
__global__ void add_noise_sd_kernel(double* K, long ld, long N, int diag_kind, double sigma2, const double* __restrict__ diag) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * N) return;
  const long r = idx % N, c = idx / N;
  if ((r / TILE) < (c / TILE)) return;
  const double e = r == c ? 1.0 : 0.0;
  K[r + c * ld] += diag_kind ? (r == c ? diag[r] : 0.0) : sigma2 * e;
}

int launch_add_noise_sd(double* K, long ld, long N, int noise_kind, double sigma2, const double* d_diag, hipStream_t s) {
  const long tot = N * N;
  if (tot <= 0) return 0;
  hipLaunchKernelGGL(add_noise_sd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, K, ld, N,
                     noise_kind == SGP_NOISE_DIAG ? 1 : 0, sigma2, d_diag);
  SGP_HIP(hipGetLastError());
  return 0;
}

int upload_cols(DevBuf& b, const double* h, long ldh, long nr, long nc) {
  CHECK_RC(b.alloc((size_t)nr * nc));
  SGP_HIP(hipMemcpy2D(b.p, sizeof(double) * nr, h, sizeof(double) * ldh, sizeof(double) * nr, (size_t)nc, hipMemcpyHostToDevice));
  return 0;
}

struct FxArgs {
  const char* who;
  const sgp_cov_spec *cross, *prior_ss;
  const double *mean_s, *noise, *X;   // X: Z (rand) or Y (logpdf), N* x cols
  int noise_kind;
  long ldx, cols;
  double* out;
  long ldo;
  bool rand;
};

int postfx_impl(sgp_ctx* ctx, PostRef post, const FxArgs& a) {
  CtxScope scope(ctx);
  const Kept k = post.kept();
  SpecGuard gc, gp;
  CHECK_RC(drv_dspec_create(ctx, a.cross, &gc.ds));
  CHECK_RC(drv_dspec_create(ctx, a.prior_ss, &gp.ds));
  const long Ns = gc.ds->N, cols = a.cols;
  REFUSE_UNLESS(gc.ds->M == k.n, a.who, "the columns of the cross spec are not the points the posterior was conditioned on");
  REFUSE_UNLESS(Ns >= 1, a.who, "no test points");
  REFUSE_UNLESS(gp.ds->symmetric && gp.ds->N == Ns && gp.ds->M == Ns, a.who,
                "prior_ss must be the symmetric spec of the N* test points of the cross spec");
  REFUSE_UNLESS(a.ldx >= Ns && (!a.rand || a.ldo >= Ns), a.who, "a leading dimension is smaller than the number of test points");
  REFUSE_UNLESS(a.rand || 16 + 2 * cols <= ctx->n_scal, a.who, "too many columns of Y");
  int64_t np_, mt_;
  sgp_geometry(Ns, a.rand ? 0 : cols, &np_, &mt_);
  const long n_pad = np_, m_tot = mt_;   // n_pad: the test points padded to whole tiles -- the rows of V as well
  REFUSE_UNLESS(n_pad / TILE <= ctx->n_slots, a.who, "too many test points for the logdet slot buffer");
  hipStream_t s = ctx->stream;

  DevBuf dA, dX, dnoise;
  if (a.noise_kind == SGP_NOISE_DIAG) CHECK_RC(dnoise.upload(a.noise, Ns));
  if (a.noise_kind == SGP_NOISE_DENSE) CHECK_RC(dnoise.upload(a.noise, (size_t)Ns * Ns));
  const double sigma2 = a.noise_kind == SGP_NOISE_SCALAR ? a.noise[0] : 0.0;
  CHECK_RC(upload_cols(dX, a.X, a.ldx, Ns, cols));

  // ---- V (and C), the posterior mean
  CrossRows R;
  CHECK_RC(R.solve(ctx, k, CrossSource{gc.ds, nullptr, 0, Ns, a.mean_s}, n_pad, s));
  CHECK_RC(R.mean(k, s));

  // ---- C* + S* in the bordered buffer
  CHECK_RC(dA.alloc((size_t)m_tot * n_pad));
  SGP_HIP(hipMemsetAsync(dA.p, 0, sizeof(double) * m_tot * n_pad, s));
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  CHECK_RC(drv_assemble(gp.ds, dA.p, m_tot, 0, n_pad / TILE, 0, n_pad / TILE, 0, -1, 0.0, nullptr, s));
  constexpr long LOWER = 0;   // launch_gemm_nt's mask_off: the tiles with tile row >= tile column
  CHECK_RC(launch_gemm_nt(R.V.p, n_pad, R.V.p, n_pad, dA.p, m_tot, n_pad, n_pad, k.n_pad, -1.0, 1.0, LOWER, 0, 0, s));
  if (k.L2) CHECK_RC(launch_gemm_nt(R.V2.p, n_pad, R.V2.p, n_pad, dA.p, m_tot, n_pad, n_pad, k.n_pad, 1.0, 1.0, LOWER, 0, 0, s));
  if (a.noise_kind == SGP_NOISE_DENSE)
    CHECK_RC(launch_add_dense(dA.p, m_tot, dnoise.p, Ns, Ns, 1, s));
  else
    CHECK_RC(launch_add_noise_sd(dA.p, m_tot, Ns, a.noise_kind, sigma2, dnoise.p, s));
  CHECK_RC(launch_fill_pad(dA.p, m_tot, Ns, n_pad, 0, n_pad, m_tot, 0, s));
  if (!a.rand) CHECK_RC(launch_border_rows(dA.p, m_tot, n_pad, Ns, 0, n_pad, dX.p, Ns, cols, R.mu.p, s));
  CHECK_RC(drv_chol_sub(ctx, dA.p, m_tot, n_pad, m_tot, nullptr, s));

  DevBuf dZt, dOut;
  const long s_pad = (cols + TILE - 1) / TILE * TILE;
  double* d_out = ctx->d_scal + 16 + cols;
  if (a.rand) {   // out[i, c] = m*[i] + sum_{k <= i} L*[i, k] Z[k, c]: the tail of sgp_rand
    CHECK_RC(dZt.alloc((size_t)s_pad * n_pad));
    CHECK_RC(dOut.alloc((size_t)n_pad * s_pad));
    SGP_HIP(hipMemsetAsync(dZt.p, 0, sizeof(double) * s_pad * n_pad, s));
    CHECK_RC(launch_transpose_add(dX.p, Ns, Ns, cols, dZt.p, s_pad, nullptr, s));
    CHECK_RC(drv_fill_mean_cols(dOut.p, n_pad, n_pad, s_pad, Ns, R.mu.p, s));
    CHECK_RC(launch_gemm_nt_lz(dA.p, m_tot, dZt.p, s_pad, dOut.p, n_pad, n_pad, s_pad, 1.0, s));
  } else {        // the tail of sgp_logpdf
    CHECK_RC(launch_rowsumsq(dA.p + n_pad, m_tot, Ns, cols, ctx->d_scal + 16, 0, s));
    CHECK_RC(launch_sum_array(ctx->d_slots, n_pad / TILE, ctx->d_scal, s));
    CHECK_RC(launch_logpdf_final(ctx->d_scal, ctx->d_scal + 16, Ns, cols, d_out, s));
  }
  const int info = drv_fetch_info(ctx, s);   // (drains the stream)
  if (info < 0) return -3;
  if (info > 0) {
    set_error("matrix is not positive definite; Cholesky factorization failed at leading minor " + std::to_string(info));
    return info;
  }
  if (a.rand)
    SGP_HIP(hipMemcpy2D(a.out, sizeof(double) * a.ldo, dOut.p, sizeof(double) * n_pad, sizeof(double) * Ns, (size_t)cols,
                        hipMemcpyDeviceToHost));
  else
    SGP_HIP(hipMemcpy(a.out, d_out, sizeof(double) * cols, hipMemcpyDeviceToHost));
  return 0;
}

// what every entry point checks of its arguments, then the door (kept.h) for the posterior's context
int enter(PostRef post, const FxArgs& a, const char* multi_refusal) {
  REFUSE_UNLESS(post && a.cross && a.prior_ss && a.noise && a.X && a.out, a.who, "NULL argument");
  REFUSE_UNLESS(a.noise_kind >= SGP_NOISE_SCALAR && a.noise_kind <= SGP_NOISE_DENSE, a.who, "bad noise kind");
  REFUSE_UNLESS(a.cols >= 1, a.who, a.rand ? "S must be at least 1" : "ncols must be at least 1");
  CHECK_RC(kept_door(post, true, a.who, multi_refusal));
  sgp_ctx* ctx = post.ctx();
  return drv_with_df_fallback(ctx, [&]() { return postfx_impl(ctx, post, a); });
}

int dense_entry(sgp_post* post, const FxArgs& a) {
  return enter(post, a, "a posterior of a multi-GPU context (sharded factor) is not sampled or scored on the device");
}

int sparse_entry(sgp_sparse_post* post, const FxArgs& a) {
  return enter(post, a, "a posterior of a multi-GPU context is not sampled or scored on the device");
}

}  // namespace

namespace sgp {

int drv_posterior_rand(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                       int noise_kind, const double* noise, const double* Z, int64_t ldz, int64_t S, double* out, int64_t ldo) {
  return dense_entry(post, FxArgs{"sgp_posterior_rand", cross, prior_ss, mean_s, noise, Z, noise_kind, (long)ldz, (long)S, out,
                                  (long)ldo, true});
}
int drv_posterior_logpdf(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                         int noise_kind, const double* noise, const double* Y, int64_t ldy, int64_t ncols, double* out) {
  return dense_entry(post, FxArgs{"sgp_posterior_logpdf", cross, prior_ss, mean_s, noise, Y, noise_kind, (long)ldy, (long)ncols,
                                  out, 0, false});
}
int drv_sparse_posterior_rand(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                              const double* mean_s, int noise_kind, const double* noise, const double* Z, int64_t ldz,
                              int64_t S, double* out, int64_t ldo) {
  return sparse_entry(post, FxArgs{"sgp_sparse_posterior_rand", cross, prior_ss, mean_s, noise, Z, noise_kind, (long)ldz, (long)S,
                                   out, (long)ldo, true});
}
int drv_sparse_posterior_logpdf(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                const double* mean_s, int noise_kind, const double* noise, const double* Y, int64_t ldy,
                                int64_t ncols, double* out) {
  return sparse_entry(post, FxArgs{"sgp_sparse_posterior_logpdf", cross, prior_ss, mean_s, noise, Y, noise_kind, (long)ldy,
                                   (long)ncols, out, 0, false});
}

}  // namespace sgp
