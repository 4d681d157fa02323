// The per-pair formulas of the additive kinds (additive.hip), beside kern_eval.h, deriv_eval.h and gibbs_eval.h: one
// definition for the matrix kernel, the diagonal kernel and both gradient kernels, so that var == diag(cov) bit for bit.
//
// A coordinate: u = x_d - y_d, s = u u, z = kappa_base(s) in [0, 1], kx = kappa'(s) = d z / d s (<= 0).
//   SE          z = exp(-s / 2)                      kx = -z / 2
//   Matern-1/2  z = exp(-r), r = sqrt(s)             kx = -z / (2 r), 0 at s == 0 (not differentiable there: subgradient 0)
//   Matern-3/2  z = (1 + l) exp(-l), l = sqrt(3 s)   kx = -(3 / 2) exp(-l)
//   Matern-5/2  z = (1 + l + l^2 / 3) exp(-l), l = sqrt(5 s)     kx = -(5 / 6) (1 + l) exp(-l)
// u == 0 gives z == 1 exactly (sqrt_nonneg(0) = 1e-150, 1 + 1e-150 == 1, exp_nonpos(-1e-150) == 1); an exponential that
// underflowed gives z == 0 exactly (the polynomial in front of it stays finite: sqrt_nonneg clamps its argument).
//
// The elementary symmetric polynomials e_0 .. e_R of z_0 .. z_{D-1}: e = (1, 0, .., 0); for every d in ascending order, for k
// from the top down to 1: e_k = fma(z_d, e_{k-1}, e_k) (esp_step).  The step runs over all RMAX >= R entries of the table: an
// entry above min(d + 1, R) adds fma(z_d, 0, 0) == 0, so the bits of e_1 .. e_R are those of the recurrence that stops there.
#pragma once
#include "additive_kinds.h"
#include "common.h"

namespace sgp {

// (s is clamped to 1e300: a difference that overflowed its square gives z == 0 and kx == 0, not inf * 0)
template <int BASE>
__device__ __forceinline__ void additive_z(double s, double& z, double& kx) {
  s = fmin(s, 1e300);
  if (BASE == SGP_SE) {
    z = exp_nonpos(-0.5 * s);
    kx = -0.5 * z;
  } else if (BASE == SGP_MATERN12) {
    const double r = sqrt_nonneg(s);
    z = exp_nonpos(-r);
    kx = s > 0.0 ? -0.5 * z / r : 0.0;
  } else if (BASE == SGP_MATERN32) {
    const double l = 1.7320508075688772 * sqrt_nonneg(s);
    const double E = exp_nonpos(-l);
    z = (1.0 + l) * E;
    kx = -1.5 * E;
  } else {
    const double l = 2.23606797749979 * sqrt_nonneg(s);
    const double E = exp_nonpos(-l);
    z = fma(l, fma(l, 0.3333333333333333, 1.0), 1.0) * E;
    kx = -0.8333333333333334 * ((1.0 + l) * E);
  }
}
template <int BASE>
__device__ __forceinline__ double additive_z(double u) {
  double z, kx;
  additive_z<BASE>(u * u, z, kx);
  return z;
}

// The table steps are written as compile-time recursions, not loops: every index is a constant before any optimisation runs,
// so the tables are registers in every instantiation (a loop the optimiser unrolls late leaves them in scratch).
// e[0 .. RMAX]: one coordinate enters the table (e[0] stays 1), k from RMAX down to 1
template <int RMAX, int K = RMAX>
__device__ __forceinline__ void esp_step(double (&e)[RMAX + 1], double z) {
  e[K] = fma(z, e[K - 1], e[K]);
  if constexpr (K > 1) esp_step<RMAX, K - 1>(e, z);
}
// the same with the tangent de of the table for dz = v (forward mode; the tangent first: it reads the table before the step)
template <int RMAX, int K = RMAX>
__device__ __forceinline__ void esp_step_tangent(double (&e)[RMAX + 1], double (&de)[RMAX + 1], double z, double v) {
  de[K] = fma(z, de[K - 1], fma(v, e[K - 1], de[K]));
  e[K] = fma(z, e[K - 1], e[K]);
  if constexpr (K > 1) esp_step_tangent<RMAX, K - 1>(e, de, z, v);
}
// e[r] for a runtime r in 1 .. RMAX without indexing the registers
template <int RMAX, int K = RMAX>
__device__ __forceinline__ double esp_pick(const double (&e)[RMAX + 1], int r) {
  if constexpr (K == 1) return e[1];
  else return r == K ? e[K] : esp_pick<RMAX, K - 1>(e, r);
}
// e = (1, 0, .., 0) (fill: 0 for a tangent or a sum)
template <int RMAX, int K = RMAX>
__device__ __forceinline__ void esp_init(double (&e)[RMAX + 1], double first = 1.0) {
  e[K] = K == 0 ? first : 0.0;
  if constexpr (K > 0) esp_init<RMAX, K - 1>(e, first);
}

}  // namespace sgp
