// libsthenomi_predgrad.so -- the entry points of include/sthenomi_predgrad.h.  Links against libsthenomi.so, whose driver does
// the work (predgrad.hip: drv_posterior_predict_grad_x and its sparse form) on posteriors created there; this file only gives
// them their C names.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_predgrad.h"

extern "C" int sgp_posterior_predict_grad_x(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                            const double* mean_s, double* mean_out, double* var_out,
                                            double* const* grad_mean_inputs, double* const* grad_var_inputs,
                                            double* const* grad_var_prior_inputs) {
  return sgp::drv_posterior_predict_grad_x(post, cross, prior_ss, mean_s, mean_out, var_out, grad_mean_inputs, grad_var_inputs,
                                           grad_var_prior_inputs);
}
extern "C" int sgp_sparse_posterior_predict_grad_x(sgp_sparse_post* post, const sgp_cov_spec* cross,
                                                   const sgp_cov_spec* prior_ss, const double* mean_s, double* mean_out,
                                                   double* var_out, double* const* grad_mean_inputs,
                                                   double* const* grad_var_inputs, double* const* grad_var_prior_inputs) {
  return sgp::drv_sparse_posterior_predict_grad_x(post, cross, prior_ss, mean_s, mean_out, var_out, grad_mean_inputs,
                                                  grad_var_inputs, grad_var_prior_inputs);
}
