// The additive kinds (additive.hip; include/sthenomi.h: SGP_ADDITIVE_*) in a table of their own: the codes, what param and the
// input dimension may be, the text a spec that breaks a rule is refused with, and which terms of a pair share a launch.
// Host-only plain C++17 like deriv_kinds.h and gibbs_kinds.h; no other table knows the codes: capi.hip asks this one too.
#pragma once
#include "../../include/sthenomi.h"

namespace sgp {

constexpr int ADDITIVE_MAX_DIM = 16;    // dimension of the points a term reads
constexpr int ADDITIVE_MAX_ORDER = 8;   // the largest order r of the elementary symmetric polynomial

// `code`: a kind code without its flags
constexpr bool additive_kind_known(int code) { return code >= SGP_ADDITIVE_SE && code <= SGP_ADDITIVE_MATERN52; }
constexpr int additive_base(int code) { return code - SGP_ADDITIVE_SE; }   // SGP_SE .. SGP_MATERN52

constexpr const char* ADDITIVE_REFUSAL_PARAM =
    "spec: SGP_ADDITIVE (additive kernel): param must be an integer order r in 1 .. min(D, 8), D the dimension of the points";
constexpr const char* ADDITIVE_REFUSAL_DIM = "spec: SGP_ADDITIVE (additive kernel): the points must have dimension 1 .. 16";
constexpr const char* ADDITIVE_REFUSAL_CHAIN =
    "spec: an additive term takes no SGP_KIND_TIMES_PREV, on it or on its successor (no products with an additive factor)";
constexpr const char* ADDITIVE_REFUSAL_RESERVED = "spec: an additive term must have reserved == 0 (no patch or stencil sides)";
constexpr const char* ADDITIVE_REFUSAL_MULTI = "spec: additive terms are not supported on a multi-GPU context";

// the order class a kernel is instantiated with for a largest order R in 1 .. ADDITIVE_MAX_ORDER: 2, 4 or 8
constexpr int additive_rmax_class(int R) { return R <= 2 ? 2 : R <= 4 ? 4 : 8; }

// nullptr: (param, dim) is one an additive term takes (NaN fails the first comparison); else the refusal
inline const char* additive_param_refusal(double param, long dim) {
  if (dim < 1 || dim > ADDITIVE_MAX_DIM) return ADDITIVE_REFUSAL_DIM;
  const long top = dim < ADDITIVE_MAX_ORDER ? dim : ADDITIVE_MAX_ORDER;
  if (!(param >= 1.0 && param <= (double)top) || param != (double)(int)param) return ADDITIVE_REFUSAL_PARAM;
  return nullptr;
}

// Terms [t, t1) of one pair's additive segment: how many, from t on, form one launch group -- the same kind, points and scale
// vectors, so that the D base kernels and the recurrence are evaluated once per point pair for all of them; the terms of a
// group differ in (coef, param).  Term: DevTerm's fields
template <class Term>
int additive_group(const Term* terms, int t, int t1) {
  int e = t + 1;
  while (e < t1 && terms[e].kind == terms[t].kind && terms[e].xr == terms[t].xr && terms[e].xc == terms[t].xc &&
         terms[e].rs == terms[t].rs && terms[e].cs == terms[t].cs && terms[e].dim == terms[t].dim)
    ++e;
  return e - t;
}
// the largest order of a group
template <class Term>
int additive_group_order(const Term* terms, int nterms) {
  int R = 1;
  for (int t = 0; t < nterms; ++t)
    if ((int)terms[t].param > R) R = (int)terms[t].param;
  return R;
}

}  // namespace sgp
