// libsthenomi_vfe_update.so -- the entry points of include/sthenomi_vfe_update.h.  Links against libsthenomi.so, whose driver
// does the work (vfe_update.hip: drv_sparse_posterior_update) on posteriors created there; this file only gives them their C names.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_vfe_update.h"

extern "C" int sgp_sparse_posterior_update(sgp_sparse_post* post, const sgp_cov_spec* xz_new, const double* var_x_new,
                                           const double* mean_x_new, int noise_kind, const double* noise_new,
                                           const double* y_new, double* elbo_out) {
  return sgp::drv_sparse_posterior_update(post, xz_new, var_x_new, mean_x_new, noise_kind, noise_new, y_new, elbo_out);
}

extern "C" int sgp_sparse_posterior_count(sgp_sparse_post* post, int64_t* n_out) {
  return sgp::drv_sparse_posterior_count(post, n_out);
}
