// The arc-cosine kinds' per-pair arithmetic (include/sthenomi.h: SGP_NNGP, SGP_NTK), in ONE place: the matrix, diagonal and
// gradient kernels of arccos.hip all run these steps, so a pair has the same bits wherever it is evaluated.
//
// A depth-L ReLU network with weight variance 2 keeps norms, so K = n_x n_y T(c_0), c_0 the cosine of the angle between the
// points and T = c_L (NNGP) or t_L (NTK) by
//   c_{l+1} = kappa_1(c_l),   t_{l+1} = c_{l+1} + t_l kappa_0(c_l),   t_0 = c_0,
//   kappa_0(c) = 1 - acos(c) / pi,   kappa_1(c) = (sqrt(1 - c^2) + (pi - acos c) c) / pi.
// The recursion is carried in the HALF ANGLE h = theta / 2, never in c: near-parallel points have 1 - c below 2^-53, where
// acos(c) has lost half its digits, and the NTK needs exactly that angle through kappa_0.
//   h_0 = atan2(|xh - yh|, |xh + yh|)                      xh, yh the unit vectors, formed once per point
//   s   = 2 sin^2 h - (sin 2h - 2h cos 2h) / pi            the deficit 1 - c_{l+1};  sin 2h = 2 sin h cos h, cos 2h = 1 - 2 sin^2 h
//   h'  = asin(sqrt(s / 2))
// The cancellation in sin - theta cos costs an absolute error of order 2^-53 theta in s, which is what h' can bear.  Every
// step is symmetric in the two points.  A bit-equal pair has h = 0 and then s = 0, c = 1, kappa_0 = 1 exactly at every layer.
#pragma once
#include "../../include/sthenomi.h"
#include <hip/hip_runtime.h>

namespace sgp {

constexpr double ARCCOS_INV_PI = 0.31830988618379067154;

// the norm of a point (d ascending) -- and its unit vector is x_d / n per coordinate, exact zeros for a point of norm 0
__device__ __forceinline__ double arccos_norm(const double* x, int D) {
  double q = 0.0;
  for (int d = 0; d < D; ++d) q = fma(x[d], x[d], q);
  return sqrt(q);
}
__device__ __forceinline__ double arccos_unit(double x, double n) { return n > 0.0 ? x / n : 0.0; }

// one coordinate of |xh - yh|^2 and |xh + yh|^2
__device__ __forceinline__ void arccos_step(double xh, double yh, double& a2, double& b2) {
  const double m = xh - yh, p = xh + yh;
  a2 = fma(m, m, a2);
  b2 = fma(p, p, b2);
}
__device__ __forceinline__ double arccos_half_angle(double a2, double b2) { return atan2(sqrt(a2), sqrt(b2)); }

// what one layer leaves besides the next half angle
struct ArccosLayer {
  double A;    // 1 - cos theta of the angle the layer STARTED from (2 sin^2 h)
  double B;    // 1 + cos theta of that angle (2 cos^2 h)
  double st;   // sin theta of that angle
  double k0;   // kappa_0 there
  double c;    // c_{l+1}
};
// h (theta_l / 2) -> theta_{l+1} / 2
__device__ __forceinline__ ArccosLayer arccos_layer(double& h) {
  ArccosLayer y;
  double sh, ch;
  sincos(h, &sh, &ch);
  const double th = 2.0 * h;
  y.A = 2.0 * sh * sh;
  y.B = 2.0 * ch * ch;
  y.st = 2.0 * sh * ch;
  const double w = fma(-th, 1.0 - y.A, y.st);        // sin theta - theta cos theta
  const double s = fmax(fma(-w, ARCCOS_INV_PI, y.A), 0.0);
  y.k0 = fma(-th, ARCCOS_INV_PI, 1.0);
  y.c = 1.0 - s;
  h = asin(fmin(sqrt(0.5 * s), 1.0));
  return y;
}

// one pair of the diagonal kernel (and the statement of the whole evaluation): sum_t T_t w_t over the group's terms, whose
// depths do not decrease (arccos_kinds.h: arccos_group); w_t = (coef_t rs) cs.  Term: DevTerm's fields
template <class Term>
__device__ __forceinline__ double arccos_pair_sum(const double* x, const double* y, int D, const Term* terms, int nterms,
                                                  double rs, double cs) {
  const double nx = arccos_norm(x, D), ny = arccos_norm(y, D);
  double a2 = 0.0, b2 = 0.0;
  for (int d = 0; d < D; ++d) arccos_step(arccos_unit(x[d], nx), arccos_unit(y[d], ny), a2, b2);
  double h = arccos_half_angle(a2, b2), t = 0.0, acc = 0.0;
  const double nn = nx * ny;
  const int L = (int)terms[nterms - 1].param;
  int tm = 0;
  for (int l = 0; l < L; ++l) {
    const ArccosLayer y1 = arccos_layer(h);
    if (l == 0) t = 1.0 - y1.A;   // t_0 = c_0
    t = fma(t, y1.k0, y1.c);
    for (; tm < nterms && (int)terms[tm].param == l + 1; ++tm)
      acc = fma(nn * ((terms[tm].kind & 0xff) == SGP_NTK ? t : y1.c), (terms[tm].coef * rs) * cs, acc);
  }
  return acc;
}

}  // namespace sgp
