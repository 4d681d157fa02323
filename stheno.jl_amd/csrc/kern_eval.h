// The per-pair kernel formulas of the fp64 assembly, shared by the plain assembly (kernelmatrix.hip) and the patch
// assembly (conv.hip): one definition, so that a patch term whose patch is the whole image reproduces the plain term bit
// for bit, and the diagonal kernels sum exactly as the matrix kernels do.
#pragma once
#include "common.h"

namespace sgp {

enum { K_SE = 0, K_M12 = 1, K_M32 = 2, K_M52 = 3, K_WHITE = 4, K_CONST = 5 };

template <int KIND>
__device__ __forceinline__ double kern_eval_t(double d2, double param) {
  if (KIND == K_SE) return exp_nonpos(-0.5 * d2);
  if (KIND == K_M12) return exp_nonpos(-sqrt_nonneg(d2));
  if (KIND == K_M32) {
    double l = 1.7320508075688772 * sqrt_nonneg(d2);
    return (1.0 + l) * exp_nonpos(-l);
  }
  if (KIND == K_M52) {
    double l = 2.23606797749979 * sqrt_nonneg(d2);
    return fma(l, fma(l, 0.3333333333333333, 1.0), 1.0) * exp_nonpos(-l);   // 1 + l + l^2 / 3
  }
  if (KIND == K_WHITE) return d2 == 0.0 ? 1.0 : 0.0;
  return param;
}

__device__ __forceinline__ double kern_eval(int kind, double d2, double param) {
  switch (kind) {
    case K_SE: return kern_eval_t<K_SE>(d2, param);
    case K_M12: return kern_eval_t<K_M12>(d2, param);
    case K_M32: return kern_eval_t<K_M32>(d2, param);
    case K_M52: return kern_eval_t<K_M52>(d2, param);
    case K_WHITE: return kern_eval_t<K_WHITE>(d2, param);
    default: return param;
  }
}

// diag of the plain terms of a block: sum_t coef rs[i] cs[i] k(xr_i, xc_i), in the operation order of the assembly
// kernels, so var(f, x) == diag(cov(f, x)) bit for bit
__device__ __forceinline__ double diag_plain_sum(const DevTerm* terms, int nterms, long i) {
  double acc = 0.0;
  for (int tm = 0; tm < nterms; ++tm) {
    const DevTerm T = terms[tm];
    double d2 = 0.0;
    for (int d = 0; d < T.dim; ++d) {
      double df = T.xr[i * T.ldr + d] - T.xc[i * T.ldc + d];
      d2 = fma(df, df, d2);
    }
    double cw = T.coef * (T.rs ? T.rs[i] : 1.0);
    if (T.cs) cw = cw * T.cs[i];
    acc = fma(kern_eval(T.kind, d2, T.param), cw, acc);
  }
  return acc;
}

}  // namespace sgp
