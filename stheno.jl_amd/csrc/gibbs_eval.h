// The per-pair formulas of the Gibbs kind (gibbs.hip), beside kern_eval.h and deriv_eval.h: one definition for the matrix
// kernel, the diagonal kernel and both gradient kernels, so that var == diag(cov) bit for bit.
//
// A point is (x, l): D location coordinates and its lengthscale; l2 = l * l is formed ONCE per point (staging), never per pair.
// With s = |x - y|^2, q = lx2 + ly2 and ONE reciprocal rq = 1 / q:
//   t = s rq                      the exponent, E = exp_nonpos(-t)
//   c = 2 lx ly rq                corrected by one fma step (c += (2 lx ly - q c) rq), so that lx == ly gives exactly 1
//   h = sqrt(c)                   c^(p/2) = h multiplied p times, p a wave-uniform integer of the term
//   k_p = h^p E                   the term's entry is fma(k_p, (coef rs_i) cs_j, acc)
// A pair that coincides in location and lengthscale: s = 0, q = 2 lx2 and 2 lx ly = 2 fl(lx lx) are the same number, c == 1,
// h == 1 (selected, not computed), E == 1: the entry is exactly (coef rs_i) cs_j.  E == 0 marks the pair dead: every term is
// an exact 0, whatever rq and c hold (Inf, NaN from an overflowed s or q).
// Range: l in [2^-500, 2^500] keeps l2 and q normal numbers.
#pragma once
#include "common.h"

namespace sgp {

struct GibbsPair {
  double h, E;   // sqrt(c), the exponential
  double t, rq;  // s / q and 1 / q: the gradient kernels' coefficients
  bool dead;     // E == 0: the pair's entries are exact zeros
};

__device__ __forceinline__ GibbsPair gibbs_pair(double s, double lx, double lx2, double ly, double ly2) {
  GibbsPair o;
  const double q = lx2 + ly2;
  o.rq = 1.0 / q;
  o.t = s * o.rq;
  const double num = (2.0 * lx) * ly;
  double c = num * o.rq;
  c = fma(fma(-q, c, num), o.rq, c);
  c = fmin(c, 1.0);
  o.h = c == 1.0 ? 1.0 : sqrt_nonneg(c);
  o.E = exp_nonpos(-o.t);
  o.dead = o.E == 0.0;
  return o;
}

// h^p E for p >= 1, the product taken left to right
__device__ __forceinline__ double gibbs_value(const GibbsPair& P, int p) {
  double v = P.h;
  for (int m = 1; m < p; ++m) v *= P.h;
  v *= P.E;
  return P.dead ? 0.0 : v;
}

// d / d lx (the row side's lengthscale) of a group's sum A = sum_t coef_t k_t, with Bh = sum_t coef_t (p_t / 2) k_t:
//   sum_t coef_t k_t (p_t / 2 (1 / lx - 2 lx rq) + 2 t lx rq) = Bh (1 / lx - 2 lx rq) + A 2 t lx rq.     rlx: 1 / lx
__device__ __forceinline__ double gibbs_dl(const GibbsPair& P, double A, double Bh, double lx, double rlx) {
  const double lr = lx * P.rq;
  return fma(Bh, fma(-2.0, lr, rlx), A * (2.0 * (P.t * lr)));
}

}  // namespace sgp
