// The Gibbs kind (gibbs.hip; include/sthenomi.h: SGP_GIBBS) in a table of its own: the code, what param and the input dimension
// may be, the text a spec that breaks a rule is refused with, and which terms of a pair share a launch.  Host-only plain C++17
// like deriv_kinds.h; neither kprod_kinds_table.h nor deriv_kinds.h knows the code: capi.hip asks this table too.
#pragma once
#include "../../include/sthenomi.h"

namespace sgp {

constexpr int GIBBS_MAX_DIM = 16;   // dimension of the points a term reads: D location coordinates and the lengthscale
constexpr int GIBBS_MAX_POWER = 16;

// `code`: a kind code without its flags
constexpr bool gibbs_kind_known(int code) { return code == SGP_GIBBS; }

constexpr const char* GIBBS_REFUSAL_PARAM =
    "spec: SGP_GIBBS (Gibbs kernel): param must be an integer p in 1 .. 16 (the normaliser is (2 lx ly / (lx^2 + ly^2))^(p/2))";
constexpr const char* GIBBS_REFUSAL_DIM =
    "spec: SGP_GIBBS (Gibbs kernel): the points must have dimension D + 1 in 2 .. 16 (D location coordinates, then the "
    "lengthscale at the point)";
constexpr const char* GIBBS_REFUSAL_CHAIN =
    "spec: a Gibbs term takes no SGP_KIND_TIMES_PREV, on it or on its successor (no products with a Gibbs factor)";
constexpr const char* GIBBS_REFUSAL_RESERVED = "spec: a Gibbs term must have reserved == 0 (no patch or stencil sides)";
constexpr const char* GIBBS_REFUSAL_MULTI = "spec: Gibbs terms are not supported on a multi-GPU context";

// the DMAX a kernel is instantiated with for points of dimension dim in 2 .. GIBBS_MAX_DIM: 2, 4, 8 or 16
constexpr int gibbs_dmax_class(int dim) {
  int p = 2;
  while (p < dim) p <<= 1;
  return p;
}

// nullptr: (param, dim) is one a Gibbs term takes (NaN fails the first comparison); else the refusal
inline const char* gibbs_param_refusal(double param, long dim) {
  if (dim < 2 || dim > GIBBS_MAX_DIM) return GIBBS_REFUSAL_DIM;
  if (!(param >= 1.0 && param <= (double)GIBBS_MAX_POWER) || param != (double)(int)param) return GIBBS_REFUSAL_PARAM;
  return nullptr;
}

// Terms [t, t1) of one pair's Gibbs segment: how many, from t on, form one launch group -- the same points and scale vectors,
// so that the reciprocal, the square root and the exponential are evaluated once per point pair for all of them; the terms
// of a group differ in (coef, param).  Term: DevTerm's fields
template <class Term>
int gibbs_group(const Term* terms, int t, int t1) {
  int e = t + 1;
  while (e < t1 && terms[e].kind == terms[t].kind && terms[e].xr == terms[t].xr && terms[e].xc == terms[t].xc &&
         terms[e].rs == terms[t].rs && terms[e].cs == terms[t].cs && terms[e].dim == terms[t].dim)
    ++e;
  return e - t;
}

}  // namespace sgp
