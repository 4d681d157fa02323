// libsthenomi_batch.so -- the entry point of include/sthenomi_batch.h.  Links against libsthenomi.so, whose driver does the
// work (capi.hip: drv_logpdf_grad_batch) on contexts created there; this file only gives it its C name.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_batch.h"

extern "C" int sgp_logpdf_grad_batch(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                                     int noise_kind, const double* const* noises, const double* const* ys, double* logpdf_out,
                                     double* const* grad_y, double* const* grad_mean, double* const* grad_noise,
                                     double* const* grad_coef, double* const* grad_inscale, int* infos) {
  return sgp::drv_logpdf_grad_batch(ctx, nspec, specs, means, noise_kind, noises, ys, logpdf_out, grad_y, grad_mean,
                                    grad_noise, grad_coef, grad_inscale, infos);
}
