// libsthenomi_postfx.so -- the entry points of include/sthenomi_postfx.h.  Links against libsthenomi.so, whose driver does the
// work (postfx.hip: drv_posterior_rand / _logpdf and their sparse forms) on posteriors created there; this file only gives
// them their C names.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_postfx.h"

extern "C" int sgp_posterior_rand(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                                  int noise_kind, const double* noise, const double* Z, int64_t ldz, int64_t S, double* out,
                                  int64_t ldo) {
  return sgp::drv_posterior_rand(post, cross, prior_ss, mean_s, noise_kind, noise, Z, ldz, S, out, ldo);
}
extern "C" int sgp_posterior_logpdf(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                    const double* mean_s, int noise_kind, const double* noise, const double* Y, int64_t ldy,
                                    int64_t ncols, double* out) {
  return sgp::drv_posterior_logpdf(post, cross, prior_ss, mean_s, noise_kind, noise, Y, ldy, ncols, out);
}
extern "C" int sgp_sparse_posterior_rand(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                         const double* mean_s, int noise_kind, const double* noise, const double* Z,
                                         int64_t ldz, int64_t S, double* out, int64_t ldo) {
  return sgp::drv_sparse_posterior_rand(post, cross, prior_ss, mean_s, noise_kind, noise, Z, ldz, S, out, ldo);
}
extern "C" int sgp_sparse_posterior_logpdf(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                           const double* mean_s, int noise_kind, const double* noise, const double* Y,
                                           int64_t ldy, int64_t ncols, double* out) {
  return sgp::drv_sparse_posterior_logpdf(post, cross, prior_ss, mean_s, noise_kind, noise, Y, ldy, ncols, out);
}
