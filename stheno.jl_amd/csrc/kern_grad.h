// k and d k / d g (input scale, at g = 1) of the six leaf kinds from the squared distance: the formulas of the gradient
// contractions, shared by grad.hip (terms) and kprod.hip (the factors of a product chain): one definition.
#pragma once
#include "common.h"

namespace sgp {

enum { G_SE = 0, G_M12 = 1, G_M32 = 2, G_M52 = 3, G_WHITE = 4, G_CONST = 5 };

// d2 is clamped to 1e150: every kernel and derivative is an exact 0 long before, and a squared distance that overflowed
// would make them inf * 0 = NaN
__device__ __forceinline__ void kern_and_dscale(int kind, double d2, double param, double& k, double& dk) {
  d2 = fmin(d2, 1e150);
  switch (kind) {
    case G_SE:
      k = exp(-0.5 * d2);
      dk = -d2 * k;
      return;
    case G_M12: {
      double d = sqrt(d2);
      k = exp(-d);
      dk = -d * k;
      return;
    }
    case G_M32: {
      double l = 1.7320508075688772 * sqrt(d2);
      double e = exp(-l);
      k = (1.0 + l) * e;
      dk = -3.0 * d2 * e;
      return;
    }
    case G_M52: {
      double l = 2.23606797749979 * sqrt(d2);
      double e = exp(-l);
      k = (1.0 + l + l * l / 3.0) * e;
      dk = -(5.0 * d2 / 3.0) * (1.0 + l) * e;
      return;
    }
    case G_WHITE:
      k = d2 == 0.0 ? 1.0 : 0.0;
      dk = 0.0;
      return;
    default:
      k = param;
      dk = 0.0;
  }
}


// k and kappa' = d k / d (d^2) of the distance kinds, for the gradient with respect to the points (d k / d x =
// 2 kappa' (x - x')): one exponential for both.  Matern-1/2 is not differentiable at coincident points: subgradient 0
__device__ __forceinline__ void kern_val_dd2(int kind, double d2, double param, double& k, double& kx) {
  d2 = fmin(d2, 1e150);
  switch (kind) {
    case G_SE:
      k = exp(-0.5 * d2);
      kx = -0.5 * k;
      return;
    case G_M12: {
      double d = sqrt(d2);
      k = exp(-d);
      kx = d > 0.0 ? -0.5 * k / d : 0.0;
      return;
    }
    case G_M32: {
      double l = 1.7320508075688772 * sqrt(d2);
      double e = exp(-l);
      k = (1.0 + l) * e;
      kx = -1.5 * e;
      return;
    }
    case G_M52: {
      double l = 2.23606797749979 * sqrt(d2);
      double e = exp(-l);
      k = (1.0 + l + l * l / 3.0) * e;
      kx = -(5.0 / 6.0) * (1.0 + l) * e;
      return;
    }
    case G_WHITE:
      k = d2 == 0.0 ? 1.0 : 0.0;
      kx = 0.0;
      return;
    default:
      k = param;
      kx = 0.0;
  }
}

}  // namespace sgp
