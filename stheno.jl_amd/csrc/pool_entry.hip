// libsthenomi_pool.so -- the entry points of include/sthenomi_pool.h.  Links against libsthenomi.so, whose driver does the
// work (capi.hip: drv_logpdf_pool, drv_logpdf_grad_pool) on contexts created there; this file only gives them their C names.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_pool.h"

extern "C" int sgp_logpdf_pool(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                               const int* noise_kinds, const double* const* noises, const double* const* ys, double* out,
                               int* infos, sgp_pool_report* report) {
  return sgp::drv_logpdf_pool(ctx, nspec, specs, means, noise_kinds, noises, ys, out, infos, report);
}

extern "C" int sgp_logpdf_grad_pool(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                                    const int* noise_kinds, const double* const* noises, const double* const* ys,
                                    double* logpdf_out, double* const* grad_y, double* const* grad_mean,
                                    double* const* grad_noise, double* const* grad_coef, double* const* grad_inscale,
                                    int* infos, sgp_pool_report* report) {
  return sgp::drv_logpdf_grad_pool(ctx, nspec, specs, means, noise_kinds, noises, ys, logpdf_out, grad_y, grad_mean,
                                   grad_noise, grad_coef, grad_inscale, infos, report);
}
