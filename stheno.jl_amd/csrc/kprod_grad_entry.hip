// libsthenomi_kprod_grad.so -- the entry points of include/sthenomi_kprod_grad.h.  Links against libsthenomi.so, whose driver
// carries product chains through the gradient cores (capi.hip: logpdf_grad_core, diag_grad_core, elbo_grad_core; kernels in
// kprod.hip); this file only gives the superset family its C names: each fills its core's record (ctx.h), sets the chain
// leave and calls the core's door (driver.h).
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_kprod_grad.h"

extern "C" int sgp_logpdf_grad_param_xs(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                                        const double* noise, const double* y, double* logpdf_out, double* grad_y,
                                        double* grad_mean, double* grad_noise, double* grad_coef, double* grad_inscale,
                                        double* grad_param, double* const* grad_inputs, double* const* grad_rowscale) {
  sgp::LogpdfGradArgs a = sgp::logpdf_grad_args(spec, mean, noise_kind, noise, y, logpdf_out, grad_y, grad_mean, grad_noise,
                                                grad_coef, grad_inscale);
  a.grad_param = grad_param, a.grad_inputs = grad_inputs, a.grad_rowscale = grad_rowscale, a.leave.kprod = true;
  return sgp::drv_logpdf_grad(ctx, a);
}

extern "C" int sgp_kernelmatrix_diag_grad_param(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w, double* grad_coef,
                                                double* grad_inscale, double* grad_param, double* const* grad_inputs,
                                                double* const* grad_rowscale, double* const* grad_colscale) {
  sgp::DiagGradArgs a;
  a.spec = spec, a.w = w, a.grad_coef = grad_coef, a.grad_inscale = grad_inscale, a.grad_param = grad_param;
  a.grad_inputs = grad_inputs, a.grad_rowscale = grad_rowscale, a.grad_colscale = grad_colscale, a.leave.kprod = true;
  return sgp::drv_diag_grad(ctx, a);
}

extern "C" int sgp_elbo_grad_param(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                                   const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                                   const double* z_noise, const double* y, double* elbo_out, double* grad_y,
                                   double* grad_mean, double* grad_noise, double* grad_var_x, double* grad_z_noise,
                                   double* grad_coef_zz, double* grad_inscale_zz, double* grad_param_zz,
                                   double* grad_coef_xz, double* grad_inscale_xz, double* grad_param_xz,
                                   double* const* grad_inputs_zz, double* const* grad_inputs_xz,
                                   double* const* grad_rowscale_zz, double* const* grad_rowscale_xz,
                                   double* const* grad_colscale_xz) {
  sgp::ElboGradArgs a = sgp::elbo_grad_args(zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, elbo_out,
                                            grad_y, grad_mean, grad_noise, grad_var_x, grad_z_noise, grad_coef_zz,
                                            grad_inscale_zz, grad_coef_xz, grad_inscale_xz);
  a.grad_param_zz = grad_param_zz, a.grad_param_xz = grad_param_xz;
  a.grad_inputs_zz = grad_inputs_zz, a.grad_inputs_xz = grad_inputs_xz, a.grad_rowscale_zz = grad_rowscale_zz;
  a.grad_rowscale_xz = grad_rowscale_xz, a.grad_colscale_xz = grad_colscale_xz, a.leave.kprod = true;
  return sgp::elbo_grad_entry(ctx, a);
}
