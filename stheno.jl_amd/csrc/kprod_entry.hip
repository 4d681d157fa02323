// libsthenomi_kprod.so -- the entry point of include/sthenomi_kprod.h.  Links against libsthenomi.so, which validates and
// assembles product chains (capi.hip: dspec_create, kprod.hip) and contracts their gradient; this file only gives the
// parameter gradient its C name: it fills the core's record (ctx.h), sets the chain leave and calls the door (driver.h).
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_kprod.h"

extern "C" int sgp_logpdf_grad_param(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                                     const double* noise, const double* y, double* logpdf_out, double* grad_y,
                                     double* grad_mean, double* grad_noise, double* grad_coef, double* grad_inscale,
                                     double* grad_param) {
  sgp::LogpdfGradArgs a = sgp::logpdf_grad_args(spec, mean, noise_kind, noise, y, logpdf_out, grad_y, grad_mean, grad_noise,
                                                grad_coef, grad_inscale);
  a.grad_param = grad_param, a.leave.kprod = true;
  return sgp::drv_logpdf_grad(ctx, a);
}
