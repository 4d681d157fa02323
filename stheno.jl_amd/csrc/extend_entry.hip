// libsthenomi_extend.so -- the entry point of include/sthenomi_extend.h.  Links against libsthenomi.so, whose driver does the
// work (extend.hip: drv_posterior_extend) on posteriors created there; this file only gives it its C name.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_extend.h"

extern "C" int sgp_posterior_extend(sgp_post* post, const sgp_cov_spec* spec_all, const double* mean_all, int noise_kind,
                                    const double* noise, const double* y_all, int64_t n_new, int64_t reserve_n,
                                    double* alpha_out, double* logpdf_out) {
  return sgp::drv_posterior_extend(post, spec_all, mean_all, noise_kind, noise, y_all, n_new, reserve_n, alpha_out, logpdf_out);
}
