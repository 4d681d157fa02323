// The blur kind (blur.hip; include/sthenomi.h: SGP_BLUR_SE) in a table of its own: the code, what the input dimension and the
// variance rows may be, the text a spec that breaks a rule is refused with, and which terms of a pair share a launch.
// Host-only plain C++17 like gibbs_kinds.h; no other table knows the code: capi.hip asks this one too.
#pragma once
#include "../../include/sthenomi.h"

namespace sgp {

constexpr int BLUR_MAX_DIM = 16;   // dimension of the points a term reads: D locations, then D variances

// `code`: a kind code without its flags
constexpr bool blur_kind_known(int code) { return code == SGP_BLUR_SE; }

constexpr const char* BLUR_REFUSAL_DIM =
    "spec: SGP_BLUR_SE (blur): the points must have an even dimension 2 D in 2 .. 16 (D location coordinates, then the D "
    "variances of the footprint at the point)";
constexpr const char* BLUR_REFUSAL_CHAIN =
    "spec: a blur term takes no SGP_KIND_TIMES_PREV, on it or on its successor (no products with a blur factor)";
constexpr const char* BLUR_REFUSAL_RESERVED = "spec: a blur term must have reserved == 0 (no patch or stencil sides)";
constexpr const char* BLUR_REFUSAL_MULTI = "spec: blur terms are not supported on a multi-GPU context";
constexpr const char* BLUR_REFUSAL_VARIANCE =
    "spec: SGP_BLUR_SE (blur): the variance rows of an input must hold finite values >= 0";

// the DMAX a kernel is instantiated with for points of dimension dim = 2 D: 1, 2, 4 or 8
constexpr int blur_dmax_class(int dim) {
  int p = 1;
  while (2 * p < dim) p <<= 1;
  return p;
}

// nullptr: points of this dimension are ones a blur term takes; else the refusal
inline const char* blur_dim_refusal(long dim) {
  return (dim < 2 || dim > BLUR_MAX_DIM || (dim & 1)) ? BLUR_REFUSAL_DIM : nullptr;
}

// the variance rows of one input (host, dim x n, leading dimension ld): 0 = one of them is negative, NaN or infinite;
// 1 = all are fine; 2 = all are exactly 0 (the side is a plain evaluation: blur.hip's one-sided mode)
inline int blur_variance_scan(const double* x, long ld, long dim, long n) {
  bool zero = true;
  for (long j = 0; j < n; ++j)
    for (long d = dim / 2; d < dim; ++d) {
      const double s = x[j * ld + d];
      if (!(s >= 0.0) || s > 1.7976931348623157e308) return 0;
      zero = zero && s == 0.0;
    }
  return zero ? 2 : 1;
}

// Terms [t, t1) of one pair's blur segment: how many, from t on, form one launch group -- the same points and scale vectors,
// so that the exponential and the normaliser are evaluated once per point pair for all of them; the terms of a group differ
// in coef alone.  Term: DevTerm's fields
template <class Term>
int blur_group(const Term* terms, int t, int t1) {
  int e = t + 1;
  while (e < t1 && terms[e].kind == terms[t].kind && terms[e].xr == terms[t].xr && terms[e].xc == terms[t].xc &&
         terms[e].rs == terms[t].rs && terms[e].cs == terms[t].cs && terms[e].dim == terms[t].dim)
    ++e;
  return e - t;
}

}  // namespace sgp
