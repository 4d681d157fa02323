// The arc-cosine kinds (arccos.hip; include/sthenomi.h: SGP_NNGP, SGP_NTK) in a table of their own: the codes, what param and
// the input dimension may be, the text a spec that breaks a rule is refused with, and which terms of a pair share a launch.
// Host-only plain C++17 like additive_kinds.h and blur_kinds.h; no other table knows the codes: capi.hip asks this one too.
#pragma once
#include "../../include/sthenomi.h"

namespace sgp {

constexpr int ARCCOS_MAX_DIM = 16;     // dimension of the points a term reads
constexpr int ARCCOS_MAX_DEPTH = 16;   // the largest number L of hidden ReLU layers

// `code`: a kind code without its flags
constexpr bool arccos_kind_known(int code) { return code == SGP_NNGP || code == SGP_NTK; }

constexpr const char* ARCCOS_REFUSAL_PARAM =
    "spec: SGP_NNGP / SGP_NTK (arc-cosine): param must be an integer number of hidden layers L in 1 .. 16";
constexpr const char* ARCCOS_REFUSAL_DIM = "spec: SGP_NNGP / SGP_NTK (arc-cosine): the points must have dimension 1 .. 16";
constexpr const char* ARCCOS_REFUSAL_CHAIN =
    "spec: an arc-cosine term takes no SGP_KIND_TIMES_PREV, on it or on its successor (no products with an arc-cosine factor)";
constexpr const char* ARCCOS_REFUSAL_RESERVED = "spec: an arc-cosine term must have reserved == 0 (no patch or stencil sides)";
constexpr const char* ARCCOS_REFUSAL_MULTI = "spec: arc-cosine terms are not supported on a multi-GPU context";

// the DMAX a kernel is instantiated with for points of dimension dim: 2, 4, 8 or 16
constexpr int arccos_dmax_class(int dim) { return dim <= 2 ? 2 : dim <= 4 ? 4 : dim <= 8 ? 8 : 16; }

// nullptr: (param, dim) is one an arc-cosine term takes (NaN fails the first comparison); else the refusal
inline const char* arccos_param_refusal(double param, long dim) {
  if (dim < 1 || dim > ARCCOS_MAX_DIM) return ARCCOS_REFUSAL_DIM;
  if (!(param >= 1.0 && param <= (double)ARCCOS_MAX_DEPTH) || param != (double)(int)param) return ARCCOS_REFUSAL_PARAM;
  return nullptr;
}

// Terms [t, t1) of one pair's arc-cosine segment: how many, from t on, form one launch group -- the same points, scale vectors
// and dimension, and depths that do not decrease, so that ONE layer recursion per point pair, run to the group's last depth,
// hands every term its c_L or t_L on the way and the terms add up in the caller's order.  The terms of a group differ in
// (kind, coef, param): NNGP and NTK terms share a group.  Term: DevTerm's fields
template <class Term>
int arccos_group(const Term* terms, int t, int t1) {
  int e = t + 1;
  while (e < t1 && terms[e].xr == terms[t].xr && terms[e].xc == terms[t].xc && terms[e].rs == terms[t].rs &&
         terms[e].cs == terms[t].cs && terms[e].dim == terms[t].dim && terms[e].param >= terms[e - 1].param)
    ++e;
  return e - t;
}
}  // namespace sgp
