// The per-pair formulas of the blur kind (blur.hip), beside kern_eval.h and gibbs_eval.h: one definition for the matrix kernel
// in both of its modes, the diagonal kernel and both gradient kernels, so that var == diag(cov) bit for bit and the one-sided
// mode gives the bits of the two-sided one.
//
// A point is (mu, s): D locations and D variances.  Per coordinate, with u = mu - mu':
//   q = 1 + (s + s')            symmetric in the two sides; a side without variance adds an exact 0
//   w = 1 / q                   a true division, the same operation wherever it is taken (per pair, or per point in staging)
//   t = fma(u w, u, t)          d ascending; with w == 1 this is the plain kernels' squared distance
//   P = P q                     d ascending, from 1
// and once per pair E = exp_nonpos(-t / 2) (the SE kernel's call), rn = blur_rnorm(P), k = rn E.  Padding coordinates hold
// u = 0 and s = s' = 0: q = w = 1, t and P keep their bits.  E == 0 marks the pair dead: its value and gradients are exact 0.
#pragma once
#include "common.h"

namespace sgp {

__device__ __forceinline__ double blur_q(double s, double sp) { return 1.0 + (s + sp); }

// P^(-1/2) for P >= 1: v_rsq_f64 seed, one Newton step on the reciprocal root, one residual correction (rounding level).
// P == 1 is selected, not computed: zero variances give exactly 1.  A product that overflowed is clamped (rsq(inf) = 0 would
// put inf * 0 into the Newton step)
__device__ __forceinline__ double blur_rnorm(double P) {
  const double a = fmin(P, 1e300);
  double r = __builtin_amdgcn_rsq(a);
  r = r * fma(-0.5 * a, r * r, 1.5);
  const double e = fma(-(a * r), r, 1.0);
  r = fma(0.5 * r, e, r);
  return P == 1.0 ? 1.0 : r;
}

// one coordinate of a pair whose w comes ready (the one-sided mode): the plain kernels' distance step with one more multiply
__device__ __forceinline__ double blur_step(double u, double w, double t) { return fma(u * w, u, t); }

// rn E, an exact 0 where the exponential underflowed
__device__ __forceinline__ double blur_value(double t, double rn) {
  const double E = exp_nonpos(-0.5 * t);
  return E == 0.0 ? 0.0 : rn * E;
}

// the pair (x, s) against (y, sp) over D coordinates, every step as above (the diagonal kernel; the matrix and gradient kernels
// run the same steps over registers and LDS)
__device__ __forceinline__ double blur_pair(const double* x, const double* s, const double* y, const double* sp, int D) {
  double t = 0.0, P = 1.0;
  for (int d = 0; d < D; ++d) {
    const double q = blur_q(s[d], sp[d]);
    t = blur_step(x[d] - y[d], 1.0 / q, t);
    P *= q;
  }
  return blur_value(t, blur_rnorm(P));
}

}  // namespace sgp
