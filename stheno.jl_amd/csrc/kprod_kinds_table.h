// The kinds of the product path (kprod.hip), in ONE table: which codes exist, the register tier of each, its parameter rule
// and the text a spec that breaks the rule is refused with.  Host-only plain C++17: nothing of HIP is included, so the
// table is checked by a g++ program of its own (tests/kprod_kinds_host.cpp).  capi.hip validates specs with it, kprod.hip's
// launchers pick their kernel instantiation with it.  The codes are those of the public headers: there is no second enum.
// A new kind is one row here plus its math in kprod_kinds.h.
#pragma once
#include "../../include/sthenomi_kprod.h"

namespace sgp {

constexpr int KP_KIND_MASK = 0xff, KP_TIMES_PREV = SGP_KIND_TIMES_PREV;

// Tier: the register class of a kind.  The product kernels are instantiated per tier, so that a chain runs the code it ran
// before the kinds of the higher tiers existed (docs/03_kernels.md section 3.2e); a higher tier's instantiation is a
// superset of the lower ones' -- the same bits, only slower -- so a chain's tier is the largest of its factors'.
//   0  the old kinds            1  COSINE, GAMMAEXP (out-of-line cospi / sinpi / pow)       2  MATERN_NU (the Bessel routine)
//   3  NEURALNET, FBM, EXPONENTIATED (kinds of x'y, x'x, y'y)                               4  WIENER, PIECEWISE0 .. 3
struct KpKind {
  int code, tier;
  bool (*param_ok)(double);   // nullptr: every param is taken
  const char* refusal;        // what dspec_create reports where param_ok says no
};
constexpr bool kp_piecewise_j_ok(double p) { return p >= 1.0 && p <= (double)SGP_PIECEWISE_J_MAX && p == (double)(int)p; }
constexpr const char* KP_PIECEWISE_REFUSAL = "spec: SGP_PIECEWISE (product path): param = j must be an integer in [1, 64]";
constexpr KpKind KP_KINDS[] = {
    {SGP_SE, 0, nullptr, nullptr},
    {SGP_MATERN12, 0, nullptr, nullptr},
    {SGP_MATERN32, 0, nullptr, nullptr},
    {SGP_MATERN52, 0, nullptr, nullptr},
    {SGP_WHITE, 0, nullptr, nullptr},
    {SGP_CONST, 0, nullptr, nullptr},
    {SGP_RQ, 0, [](double p) { return p > 0.0 && p < 1e300; }, "spec: SGP_RQ (product path): param = alpha must be > 0 and finite"},
    {SGP_LINEAR, 0, [](double p) { return p >= 0.0 && p < 1e300; },
     "spec: SGP_LINEAR (product path): param = c must be >= 0 and finite"},
    {SGP_WIENER, 4, [](double p) { return p == 0.0 || p == 1.0 || p == 2.0 || p == 3.0; },
     "spec: SGP_WIENER (product path): param = i must be exactly 0, 1, 2 or 3"},
    {SGP_PIECEWISE0, 4, kp_piecewise_j_ok, KP_PIECEWISE_REFUSAL},
    {SGP_PIECEWISE1, 4, kp_piecewise_j_ok, KP_PIECEWISE_REFUSAL},
    {SGP_PIECEWISE2, 4, kp_piecewise_j_ok, KP_PIECEWISE_REFUSAL},
    {SGP_PIECEWISE3, 4, kp_piecewise_j_ok, KP_PIECEWISE_REFUSAL},
    {SGP_COSINE, 1, nullptr, nullptr},
    {SGP_GAMMAEXP, 1, [](double p) { return p > 0.0 && p <= 2.0; },
     "spec: SGP_GAMMAEXP (product path): param = gamma must be in (0, 2]"},
    {SGP_MATERN_NU, 2, [](double p) { return p > 0.0 && p <= SGP_MATERN_NU_MAX; },
     "spec: SGP_MATERN_NU (product path): param = nu must be finite and in (0, 32]"},
    {SGP_NEURALNET, 3, nullptr, nullptr},
    {SGP_FBM, 3, [](double p) { return p > 0.0 && p <= 1.0; },
     "spec: SGP_FBM (product path): param = h must be finite and in (0, 1]"},
    {SGP_EXPONENTIATED, 3, nullptr, nullptr},
};

// the row of `code` (a kind code without its flags), nullptr: no such kind
constexpr const KpKind* kp_kind(int code) {
  for (const KpKind& r : KP_KINDS)
    if (r.code == code) return &r;
  return nullptr;
}
constexpr bool kp_kind_known(int code) { return kp_kind(code) != nullptr; }
constexpr int kp_tier(int code) {
  const KpKind* r = kp_kind(code);
  return r ? r->tier : 0;
}
// nullptr: `param` is one the kind takes (a rule is written so that NaN fails it); else the refusal
inline const char* kp_param_refusal(int code, double param) {
  const KpKind* r = kp_kind(code);
  return r && r->param_ok && !r->param_ok(param) ? r->refusal : nullptr;
}

// the tier of a chain (or of the chains of one launch): terms[i].kind is a code, possibly with KP_TIMES_PREV
template <class Term>
int kp_chain_tier(const Term* terms, int n) {
  int tier = 0;
  for (int i = 0; i < n; ++i) {
    const int t = kp_tier(terms[i].kind & KP_KIND_MASK);
    if (t > tier) tier = t;
  }
  return tier;
}
// The template argument a kernel is launched with.  grad_kprod_inputs_kernel<DMAX, NK> tells every tier apart; the other
// four kernels (<DMAX, MN> / <MN>) call the tier-1 kinds' routine from their tier-0 code, so tiers 0 and 1 share MN = 0.
constexpr int kp_nk_of_tier(int tier) { return tier; }
constexpr int kp_mn_of_tier(int tier) { return tier > 1 ? tier - 1 : 0; }
constexpr int KP_NK_MODES = 5, KP_MN_MODES = 4;

constexpr int pow2ceil(int d) {
  int p = 1;
  while (p < d) p <<= 1;
  return p;
}
// the DMAX a kernel is instantiated with for a largest factor dimension dmax <= SGP_KPROD_MAX_DIM: 1, 2, 4, 8 or 16
constexpr int kp_dmax_class(int dmax) { return pow2ceil(dmax) < 16 ? pow2ceil(dmax) : 16; }

// ---- what the device code asks of a kind code: range tests by name --------------------------------------------------------
// The kernels test a runtime code, so these are comparisons, not table look-ups; the static_assert below holds each to the
// table over every code.
// tier 4: WIENER and the PIECEWISE kinds
constexpr bool kp_is_wiener_or_piecewise(int code) { return code >= SGP_WIENER && code <= SGP_PIECEWISE3; }
// tier 3: NEURALNET, FBM, EXPONENTIATED, kinds of the scalars (x'y, x'x, y'y)
constexpr int KP_FIRST_DOT_KIND = SGP_NEURALNET;
constexpr bool kp_is_dot_kind(int code) { return code >= KP_FIRST_DOT_KIND; }
// Among the kinds of tiers 3 and 4 -- the only ones the scalar route of a mode-3 kernel sees -- the tier-4 ones are those below
// SGP_COSINE.  ONE comparison where kp_is_wiener_or_piecewise makes two: kp_dot_scalars had this form when the kernels'
// generated code was frozen, and keeps it.
constexpr int KP_FIRST_CODE_ABOVE_TIER4 = SGP_COSINE;
constexpr bool kp_scalar_route_kind_is_tier4(int code) { return code < KP_FIRST_CODE_ABOVE_TIER4; }

constexpr bool kp_predicates_match_table() {
  for (int c = 0; c < 256; ++c) {
    if (!kp_kind_known(c)) continue;
    if (kp_is_wiener_or_piecewise(c) != (kp_tier(c) == 4) || kp_is_dot_kind(c) != (kp_tier(c) == 3)) return false;
    if (kp_tier(c) >= 3 && kp_scalar_route_kind_is_tier4(c) != (kp_tier(c) == 4)) return false;
  }
  return true;
}
static_assert(kp_predicates_match_table(), "a range test above no longer says what the table says");

}  // namespace sgp
