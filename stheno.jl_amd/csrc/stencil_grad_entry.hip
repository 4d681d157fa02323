// libsthenomi_stencil_grad.so -- the entry points of include/sthenomi_stencil_grad.h.  Links against libsthenomi.so, whose
// driver carries stencil terms through the gradient cores (capi.hip: logpdf_grad_core, diag_grad_core, elbo_grad_core; kernels
// in stencil.hip); this file only gives the three their C names: each fills its core's record (ctx.h), sets the leaves the
// family carries and calls the core's door (driver.h).
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_stencil_grad.h"

extern "C" int sgp_logpdf_grad_stencil(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                                       const double* noise, const double* y, double* logpdf_out, double* grad_y,
                                       double* grad_mean, double* grad_noise, double* grad_coef, double* grad_inscale,
                                       double* const* grad_inputs) {
  sgp::LogpdfGradArgs a = sgp::logpdf_grad_args(spec, mean, noise_kind, noise, y, logpdf_out, grad_y, grad_mean, grad_noise,
                                                grad_coef, grad_inscale);
  a.grad_inputs = grad_inputs, a.leave.patch = a.leave.stencil = true;
  return sgp::drv_logpdf_grad(ctx, a);
}

extern "C" int sgp_kernelmatrix_diag_grad_stencil(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w, double* grad_coef,
                                                  double* grad_inscale, double* const* grad_inputs) {
  if (!(grad_coef && grad_inscale)) {
    sgp::set_error("sgp_kernelmatrix_diag_grad_stencil: NULL argument");
    return -1;
  }
  sgp::DiagGradArgs a;
  a.spec = spec, a.w = w, a.grad_coef = grad_coef, a.grad_inscale = grad_inscale, a.grad_inputs = grad_inputs;
  a.leave.kprod = a.leave.patch = a.leave.stencil = true;
  return sgp::drv_diag_grad(ctx, a);
}

extern "C" int sgp_elbo_grad_stencil(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                                     const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                                     const double* z_noise, const double* y, double* elbo_out, double* grad_y,
                                     double* grad_mean, double* grad_noise, double* grad_var_x, double* grad_z_noise,
                                     double* grad_coef_zz, double* grad_inscale_zz, double* grad_coef_xz,
                                     double* grad_inscale_xz, double* const* grad_inputs_zz,
                                     double* const* grad_inputs_xz) {
  sgp::ElboGradArgs a = sgp::elbo_grad_args(zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, elbo_out,
                                            grad_y, grad_mean, grad_noise, grad_var_x, grad_z_noise, grad_coef_zz,
                                            grad_inscale_zz, grad_coef_xz, grad_inscale_xz);
  a.grad_inputs_zz = grad_inputs_zz, a.grad_inputs_xz = grad_inputs_xz, a.leave.patch = a.leave.stencil = true;
  return sgp::elbo_grad_entry(ctx, a);
}
