// The per-pair formulas of the derivative kinds (deriv.hip), beside kern_eval.h / kern_grad.h: one definition for the matrix
// kernel, the diagonal kernel and the gradient contraction, so that var == diag(cov) bit for bit.
//
// k = kappa(s), s = |u|^2, u = x - y.  With A = 2 kappa'(s) and B = -4 kappa''(s) a term (a, b) of include/sthenomi.h is
//   (p+1, 0)    A u_p            (0, q+1)   -(A u_q)            (p+1, q+1)   B u_p u_q - A delta_pq
// and its input-scale derivative u . grad_u of that, with GA = 4 s kappa'' + 2 kappa', GB = -8 s kappa''' - 8 kappa'',
// GC = -4 s kappa'':
//   (p+1, 0)    GA u_p           (0, q+1)   -(GA u_q)           (p+1, q+1)   GB u_p u_q + GC delta_pq
// In closed form, E the kind's exponential, r = sqrt(s), l = sqrt(3) r resp. sqrt(5) r:
//   SE          A = -E                   B = -E                    GA = E (s - 1)              GB = E (s - 2)                  GC = -E s
//   Matern-3/2  A = -3 E                 B = -3 sqrt3 E / r        GA = 3 E (l - 1)            GB = 3 sqrt3 E (l - 1) / r      GC = -3 sqrt3 E r
//   Matern-5/2  A = -(5/3) (1 + l) E     B = -(25/3) E             GA = (5/3) E (5 s - 1 - l)  GB = (25/3) E (l - 2)           GC = -(25/3) E s
// Matern-3/2 alone divides: 1 / r is formed from the reciprocal square root (never as a quotient), is exactly 0 at s == 0
// (the products u_p / r are then 0, and the entry is -A delta_pq = 3 delta_pq), and below s = 1e-290, where s has lost its
// bits to underflow, r and 1 / r come from the squared distance of the points scaled by 2^480.
// An exponential that underflowed to 0 -- far points, an overflowed s -- marks the pair dead: every term is an exact 0.
#pragma once
#include "common.h"
#include "kern_eval.h"

namespace sgp {

constexpr double DERIV_TINY_S = 1e-290;            // Matern-3/2: below it the caller hands in the rescaled squared distance
constexpr double DERIV_UP = 0x1p480, DERIV_DOWN = 0x1p-480;

struct DerivPair {
  double A, B;   // value coefficients
  bool dead;     // E == 0: the pair's entries are exact zeros
};
struct DerivPairGrad {
  double GA, GB, GC;
};

// r and 1 / r of Matern-3/2.  sr: s, or with up != 0 the squared distance of the points scaled by DERIV_UP
__device__ __forceinline__ void deriv_r_rinv(double sr, bool up, double& r, double& rinv) {
  const double a = fmin(fmax(sr, 1e-300), 1e300);
  double y = __builtin_amdgcn_rsq(a);
  y = y * fma(-0.5 * a, y * y, 1.5);
  y = y * fma(-0.5 * a, y * y, 1.5);
  const double d = a * y;
  r = fma(0.5 * y, fma(-d, d, a), d);
  if (up) r *= DERIV_DOWN, y *= DERIV_UP;
  const bool zero = sr == 0.0;
  r = zero ? 0.0 : r;
  rinv = zero ? 0.0 : y;
}

// BASE: K_SE, K_M32 or K_M52.  WITH_GRAD: the input-scale coefficients too (the value kernels leave them out)
template <int BASE, bool WITH_GRAD>
__device__ __forceinline__ DerivPair deriv_pair(double s, double sr, bool up, DerivPairGrad* g) {
  DerivPair o;
  if (BASE == K_SE) {
    const double E = exp_nonpos(-0.5 * s);
    o.A = -E, o.B = -E, o.dead = E == 0.0;
    if (WITH_GRAD) g->GA = E * (s - 1.0), g->GB = E * (s - 2.0), g->GC = -(E * s);
  } else if (BASE == K_M32) {
    double r, rinv;
    deriv_r_rinv(sr, up, r, rinv);
    const double l = 1.7320508075688772 * r;
    const double E = exp_nonpos(-l);
    const double E3 = 3.0 * E, Eq = 5.196152422706632 * E;   // 3 sqrt(3) E
    o.A = -E3, o.B = -(Eq * rinv), o.dead = E == 0.0;
    if (WITH_GRAD) g->GA = E3 * (l - 1.0), g->GB = (Eq * (l - 1.0)) * rinv, g->GC = -(Eq * r);
  } else {
    const double l = 2.23606797749979 * sqrt_nonneg(s);
    const double E = exp_nonpos(-l);
    const double E53 = 1.6666666666666667 * E, E253 = 8.333333333333334 * E;
    o.A = -((1.0 + l) * E53), o.B = -E253, o.dead = E == 0.0;
    if (WITH_GRAD) g->GA = E53 * (fma(5.0, s, -1.0) - l), g->GB = E253 * (l - 2.0), g->GC = -(E253 * s);
  }
  return o;
}

// one term's entry from the pair's coefficients: (ca, cb, cd) = (A, B, -A) for the value, (GA, GB, GC) for the input-scale
// derivative.  a, b: the term's sides (0: not differentiated), up = u_(a-1), uq = u_(b-1) (anything where the side is 0)
__device__ __forceinline__ double deriv_entry(int a, int b, double ca, double cb, double cd, double up, double uq, bool dead) {
  double v;
  if (b == 0) v = ca * up;
  else if (a == 0) v = -(ca * uq);
  else v = fma(cb * up, uq, a == b ? cd : 0.0);
  return dead ? 0.0 : v;
}

}  // namespace sgp
