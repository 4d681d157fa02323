// libsthenomi_stencil_wo.so -- the entry points of include/sthenomi_stencil_wo.h.  Links against libsthenomi.so, whose driver
// contracts a stencil's weights and offsets at the stencil terms of the gradient cores (capi.hip: logpdf_grad_core,
// diag_grad_core, elbo_grad_core; kernels in stencil.hip); this file only gives the three their C names.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_stencil_wo.h"

extern "C" int sgp_logpdf_grad_stencil_wo(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                                          const double* noise, const double* y, double* logpdf_out, double* grad_y,
                                          double* grad_mean, double* grad_noise, double* grad_coef, double* grad_inscale,
                                          double* const* grad_inputs, double* const* grad_weights,
                                          double* const* grad_offsets) {
  return sgp::drv_logpdf_grad_stencil_wo(ctx, spec, mean, noise_kind, noise, y, logpdf_out, grad_y, grad_mean, grad_noise,
                                         grad_coef, grad_inscale, grad_inputs, grad_weights, grad_offsets);
}

extern "C" int sgp_kernelmatrix_diag_grad_stencil_wo(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w,
                                                     double* grad_coef, double* grad_inscale, double* const* grad_inputs,
                                                     double* const* grad_weights, double* const* grad_offsets) {
  return sgp::drv_diag_grad_stencil_wo(ctx, spec, w, grad_coef, grad_inscale, grad_inputs, grad_weights, grad_offsets);
}

extern "C" int sgp_elbo_grad_stencil_wo(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                                        const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                                        const double* z_noise, const double* y, double* elbo_out, double* grad_y,
                                        double* grad_mean, double* grad_noise, double* grad_var_x, double* grad_z_noise,
                                        double* grad_coef_zz, double* grad_inscale_zz, double* grad_coef_xz,
                                        double* grad_inscale_xz, double* const* grad_inputs_zz,
                                        double* const* grad_inputs_xz, double* const* grad_weights_zz,
                                        double* const* grad_offsets_zz, double* const* grad_weights_xz,
                                        double* const* grad_offsets_xz) {
  sgp::ElboGradArgs a;
  a.zz = zz, a.xz = xz, a.var_x = var_x, a.mean_x = mean_x, a.noise_kind = noise_kind, a.noise_x = noise_x;
  a.z_noise_kind = z_noise_kind, a.z_noise = z_noise, a.y = y, a.elbo_out = elbo_out, a.grad_y = grad_y;
  a.grad_mean = grad_mean, a.grad_noise = grad_noise, a.grad_var_x = grad_var_x, a.grad_z_noise = grad_z_noise;
  a.grad_coef_zz = grad_coef_zz, a.grad_inscale_zz = grad_inscale_zz, a.grad_coef_xz = grad_coef_xz;
  a.grad_inscale_xz = grad_inscale_xz, a.grad_inputs_zz = grad_inputs_zz, a.grad_inputs_xz = grad_inputs_xz;
  a.grad_weights_zz = grad_weights_zz, a.grad_offsets_zz = grad_offsets_zz;
  a.grad_weights_xz = grad_weights_xz, a.grad_offsets_xz = grad_offsets_xz;
  a.patch_ok = a.stencil_ok = true;
  return sgp::drv_elbo_grad_stencil_wo(ctx, a);
}
