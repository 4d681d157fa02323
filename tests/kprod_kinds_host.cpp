// Host-side check of the kind table of the product path (stheno.jl_amd/csrc/kprod_kinds_table.h; compiled by g++ in
// tests/test_kprod_kinds_host.py -- no GPU involved).  Every expected value below is written out, none is computed by the
// header under test:
//   * which of the codes 0 .. 255 are kinds, and the tier of each;
//   * the (DMAX class, MN, NK) a launcher instantiates its kernel with, for dmax = 1 .. 16 and chains of one kind each and five
//     mixed ones -- the values of the rules the launchers had before the table (kprod_mode and the nk ladder).  A chain of old
//     kinds sent to a higher mode's instantiation computes the same bits, only slower: no value test sees that, this one does;
//   * the parameter rule of every kind at its edges and at NaN, with the exact text of each refusal.
// The first output line lists the known codes (tests/test_kprod_kinds_host.py holds the constants of lib.py against it).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include "../stheno.jl_amd/csrc/kprod_kinds_table.h"

using namespace sgp;

static long failures = 0, cases = 0;
#define CHECK(c, ...)                      \
  do {                                     \
    ++cases;                               \
    if (!(c)) {                            \
      if (failures < 20) {                 \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");                 \
      }                                    \
      ++failures;                          \
    }                                      \
  } while (0)

struct Term {
  int kind;   // as DevTerm's: a code, continuations with SGP_KIND_TIMES_PREV
};

// code -> tier, -1: no kind
static int expected_tier(int c) {
  switch (c) {
    case 0: case 1: case 2: case 3: case 4: case 5: case 6: case 7: return 0;
    case 16: case 17: return 1;
    case 20: return 2;
    case 24: case 25: case 26: return 3;
    case 10: case 11: case 12: case 13: case 14: return 4;
    default: return -1;
  }
}

struct Chain {
  const char* name;
  int n;
  int kind[2];
  int mn, nk;   // kprod_mode of the chain; the nk ladder of launch_grad_kprod_inputs
};
static const Chain CHAINS[] = {
    {"SE", 1, {0, 0}, 0, 0},          {"MATERN12", 1, {1, 0}, 0, 0},   {"MATERN32", 1, {2, 0}, 0, 0},
    {"MATERN52", 1, {3, 0}, 0, 0},    {"WHITE", 1, {4, 0}, 0, 0},      {"CONST", 1, {5, 0}, 0, 0},
    {"RQ", 1, {6, 0}, 0, 0},          {"LINEAR", 1, {7, 0}, 0, 0},     {"WIENER", 1, {10, 0}, 3, 4},
    {"PIECEWISE0", 1, {11, 0}, 3, 4}, {"PIECEWISE1", 1, {12, 0}, 3, 4}, {"PIECEWISE2", 1, {13, 0}, 3, 4},
    {"PIECEWISE3", 1, {14, 0}, 3, 4}, {"COSINE", 1, {16, 0}, 0, 1},    {"GAMMAEXP", 1, {17, 0}, 0, 1},
    {"MATERN_NU", 1, {20, 0}, 1, 2},  {"NEURALNET", 1, {24, 0}, 2, 3}, {"FBM", 1, {25, 0}, 2, 3},
    {"EXPONENTIATED", 1, {26, 0}, 2, 3},
    {"SE * COSINE", 2, {0, 16}, 0, 1},
    {"MATERN_NU * GAMMAEXP", 2, {20, 17}, 1, 2},
    {"FBM * MATERN_NU", 2, {25, 20}, 2, 3},
    {"WIENER * NEURALNET", 2, {10, 24}, 3, 4},
    {"PIECEWISE3 * SE", 2, {14, 0}, 3, 4},
};
static const int DMAX_CLASS[17] = {0, 1, 2, 4, 4, 8, 8, 8, 8, 16, 16, 16, 16, 16, 16, 16, 16};   // [dmax], dmax = 1 .. 16

static const char* const RQ_MSG = "spec: SGP_RQ (product path): param = alpha must be > 0 and finite";
static const char* const GAMMAEXP_MSG = "spec: SGP_GAMMAEXP (product path): param = gamma must be in (0, 2]";
static const char* const MATERN_NU_MSG = "spec: SGP_MATERN_NU (product path): param = nu must be finite and in (0, 32]";
static const char* const FBM_MSG = "spec: SGP_FBM (product path): param = h must be finite and in (0, 1]";
static const char* const WIENER_MSG = "spec: SGP_WIENER (product path): param = i must be exactly 0, 1, 2 or 3";
static const char* const PIECEWISE_MSG = "spec: SGP_PIECEWISE (product path): param = j must be an integer in [1, 64]";
static const char* const LINEAR_MSG = "spec: SGP_LINEAR (product path): param = c must be >= 0 and finite";

static void refused(int code, double p, const char* msg) {
  const char* r = kp_param_refusal(code, p);
  CHECK(r && std::strcmp(r, msg) == 0, "kind %d, param %.17g: expected the refusal \"%s\", got %s", code, p, msg, r ? r : "none");
}
static void accepted(int code, double p) {
  const char* r = kp_param_refusal(code, p);
  CHECK(!r, "kind %d, param %.17g: refused (\"%s\")", code, p, r);
}

int main() {
  std::printf("known");
  for (int c = 0; c < 256; ++c)
    if (kp_kind_known(c)) std::printf(" %d", c);
  std::printf("\n");

  for (int c = 0; c < 256; ++c) {
    CHECK(kp_kind_known(c) == (expected_tier(c) >= 0), "kp_kind_known(%d)", c);
    if (expected_tier(c) >= 0) CHECK(kp_tier(c) == expected_tier(c), "kp_tier(%d) = %d", c, kp_tier(c));
  }

  for (const Chain& ch : CHAINS) {
    Term t[2] = {{ch.kind[0]}, {ch.kind[1] | SGP_KIND_TIMES_PREV}};
    for (int order = 0; order < ch.n; ++order) {   // a chain's tier does not depend on which factor is the head
      if (order) t[0].kind = ch.kind[1], t[1].kind = ch.kind[0] | SGP_KIND_TIMES_PREV;
      const int tier = kp_chain_tier(t, ch.n);
      CHECK(tier == ch.nk, "%s: chain tier %d", ch.name, tier);
      for (int dmax = 1; dmax <= 16; ++dmax) {
        CHECK(kp_dmax_class(dmax) == DMAX_CLASS[dmax], "kp_dmax_class(%d) = %d", dmax, kp_dmax_class(dmax));
        CHECK(kp_mn_of_tier(tier) == ch.mn, "%s, dmax %d: MN = %d", ch.name, dmax, kp_mn_of_tier(tier));
        CHECK(kp_nk_of_tier(tier) == ch.nk, "%s, dmax %d: NK = %d", ch.name, dmax, kp_nk_of_tier(tier));
      }
    }
  }
  CHECK(KP_MN_MODES == 4 && KP_NK_MODES == 5, "the number of modes");

  const double nan = std::numeric_limits<double>::quiet_NaN();
  refused(6, 0.0, RQ_MSG), refused(6, 1e300, RQ_MSG), accepted(6, 1e-300), refused(6, nan, RQ_MSG);
  refused(17, 0.0, GAMMAEXP_MSG), refused(17, 2.0000000000000004, GAMMAEXP_MSG), accepted(17, 2.0), refused(17, nan, GAMMAEXP_MSG);
  refused(20, 0.0, MATERN_NU_MSG), refused(20, 32.000000000000007, MATERN_NU_MSG), accepted(20, 32.0);
  refused(20, nan, MATERN_NU_MSG);
  refused(25, 0.0, FBM_MSG), refused(25, 1.0000000000000002, FBM_MSG), accepted(25, 1.0), refused(25, nan, FBM_MSG);
  refused(10, 0.5, WIENER_MSG), refused(10, 4.0, WIENER_MSG), accepted(10, -0.0), refused(10, nan, WIENER_MSG);
  for (int i = 0; i <= 3; ++i) accepted(10, (double)i);
  for (int c = 11; c <= 14; ++c) {
    refused(c, 0.0, PIECEWISE_MSG), refused(c, 1.5, PIECEWISE_MSG), refused(c, 65.0, PIECEWISE_MSG), refused(c, nan, PIECEWISE_MSG);
    accepted(c, 1.0), accepted(c, 64.0);
  }
  refused(7, -1e-300, LINEAR_MSG), refused(7, 1e300, LINEAR_MSG), accepted(7, 0.0), refused(7, nan, LINEAR_MSG);
  // the kinds without a rule take every param, NaN included, as before the table; so does a code that is no kind
  const int no_rule[] = {0, 1, 2, 3, 4, 5, 16, 24, 26, 8, 15, 255};
  for (int c : no_rule) accepted(c, nan), accepted(c, -1.0), accepted(c, 0.0);

  std::printf("cases %ld failures %ld\n", cases, failures);
  return failures ? 1 : 0;
}
