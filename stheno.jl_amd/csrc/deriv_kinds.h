// The derivative kinds (deriv.hip; include/sthenomi.h: SGP_DERIV_SE, SGP_DERIV_MATERN32, SGP_DERIV_MATERN52) in ONE table of
// their own: which codes exist, the base kind of each, how param = 17 a + b names the differentiated coordinates, and the
// text a spec that breaks a rule is refused with.  Host-only plain C++17 like kprod_kinds_table.h, which does not know
// these codes: capi.hip asks this table first.
#pragma once
#include "../../include/sthenomi.h"

namespace sgp {

constexpr int DERIV_MAX_DIM = 16;   // input dimension of a derivative term, and with it a, b <= 16
constexpr int DERIV_PARAM_BASE = DERIV_MAX_DIM + 1;

struct DerivKind {
  int code, base;   // base: the plain kind whose kappa is differentiated
};
constexpr DerivKind DERIV_KINDS[] = {
    {SGP_DERIV_SE, SGP_SE},
    {SGP_DERIV_MATERN32, SGP_MATERN32},
    {SGP_DERIV_MATERN52, SGP_MATERN52},
};
// `code`: a kind code without its flags
constexpr bool deriv_kind_known(int code) {
  for (const DerivKind& r : DERIV_KINDS)
    if (r.code == code) return true;
  return false;
}
constexpr int deriv_base(int code) { return code - SGP_DERIV_SE; }
static_assert(deriv_base(SGP_DERIV_MATERN32) == SGP_MATERN32 && deriv_base(SGP_DERIV_MATERN52) == SGP_MATERN52 &&
                  !deriv_kind_known(SGP_DERIV_SE + SGP_MATERN12),
              "a derivative kind is 32 + its base kind; Matern-1/2 has none");

constexpr const char* DERIV_REFUSAL_PARAM =
    "spec: SGP_DERIV: param must be an integer 17 a + b with a and b in 0 .. 16, not both 0 (a - 1, b - 1: the differentiated "
    "coordinate of the row, column side; 0: that side is not differentiated)";
constexpr const char* DERIV_REFUSAL_COORD = "spec: SGP_DERIV: a differentiated coordinate must be < the input dimension";
constexpr const char* DERIV_REFUSAL_DIM = "spec: SGP_DERIV: the input dimension of a derivative term must be <= 16";
constexpr const char* DERIV_REFUSAL_CHAIN =
    "spec: a derivative term takes no SGP_KIND_TIMES_PREV, on it or on its successor (no products of differentiated kernels)";
constexpr const char* DERIV_REFUSAL_RESERVED =
    "spec: a derivative term must have reserved == 0 (no patch or stencil sides)";
constexpr const char* DERIV_REFUSAL_MULTI = "spec: derivative terms are not supported on a multi-GPU context";

// the DMAX a kernel is instantiated with for an input dimension dim <= DERIV_MAX_DIM: 1, 2, 4, 8 or 16
constexpr int deriv_dmax_class(int dim) {
  int p = 1;
  while (p < dim) p <<= 1;
  return p;
}

// a, b of a param that passed deriv_param_refusal
constexpr int deriv_a(double param) { return (int)param / DERIV_PARAM_BASE; }
constexpr int deriv_b(double param) { return (int)param % DERIV_PARAM_BASE; }

// nullptr: (param, dim) is one a derivative term takes (NaN fails the first comparison); else the refusal
inline const char* deriv_param_refusal(double param, long dim) {
  if (dim > DERIV_MAX_DIM) return DERIV_REFUSAL_DIM;
  if (!(param >= 1.0 && param <= (double)(DERIV_PARAM_BASE * DERIV_PARAM_BASE - 1)) || param != (double)(int)param)
    return DERIV_REFUSAL_PARAM;
  if (deriv_a(param) > dim || deriv_b(param) > dim) return DERIV_REFUSAL_COORD;
  return nullptr;
}

// Terms [t, t1) of one pair's derivative segment: how many, from t on, form one launch group -- the same base kind, inputs
// and scale vectors, so that exp, kappa' and kappa'' are evaluated once per point pair for all of them.  Term: DevTerm's fields
template <class Term>
int deriv_group(const Term* terms, int t, int t1) {
  int e = t + 1;
  while (e < t1 && terms[e].kind == terms[t].kind && terms[e].xr == terms[t].xr && terms[e].xc == terms[t].xc &&
         terms[e].rs == terms[t].rs && terms[e].cs == terms[t].cs && terms[e].dim == terms[t].dim)
    ++e;
  return e - t;
}

}  // namespace sgp
