// Host-side check of the pair-segment record (stheno.jl_amd/csrc/spec_segments.h; compiled by g++ in
// tests/test_spec_segments_host.py -- no GPU involved).  Hand-written term_ptr and count arrays, as dspec_create fills them,
// for eight pairs; every expected boundary below is written out, none is computed by the header under test:
//   pair 0  empty                          pair 4  stencil terms only (2)
//   pair 1  plain terms only (3)           pair 5  chain terms only (one chain of 2)
//   pair 2  patch terms only (2)           pair 6  all four classes: 2 plain, 1 patch, 3 stencil, 2 chain terms
//   pair 3  empty again, between classes   pair 7  1 plain term and two chains of lengths 1 and 3
// and chain_end / chain_dmax on the chains of pairs 5 and 7.
#include <cstdio>
#include "../stheno.jl_amd/csrc/spec_segments.h"

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
  int kind, dim;   // as DevTerm's: a code, continuations with SGP_KIND_TIMES_PREV; the input dimension
};

int main() {
  //                         pair:  0  1  2  3  4  5  6   7
  const int term_ptr[9] = {0, 0, 3, 5, 5, 7, 9, 17, 22};
  const int nplain[8] = {0, 3, 0, 0, 0, 0, 2, 1};
  const int npatch[8] = {0, 0, 2, 0, 0, 0, 1, 0};
  const int nkprod[8] = {0, 0, 0, 0, 0, 2, 2, 4};
  const PairSegs want[8] = {
      {0, 0, 0, 0, 0},        // empty
      {0, 3, 3, 3, 3},        // plain [0, 3)
      {3, 3, 5, 5, 5},        // patch [3, 5)
      {5, 5, 5, 5, 5},        // empty
      {5, 5, 5, 7, 7},        // stencil [5, 7)
      {7, 7, 7, 7, 9},        // chains [7, 9)
      {9, 11, 12, 15, 17},    // plain [9, 11) | patch [11, 12) | stencil [12, 15) | chains [15, 17)
      {17, 18, 18, 18, 22},   // plain [17, 18) | chains [18, 22)
  };
  for (int p = 0; p < 8; ++p) {
    const PairSegs g = pair_segments(term_ptr, nplain, npatch, nkprod, p);
    CHECK(g.t0 == want[p].t0, "pair %d: t0 = %d, expected %d", p, g.t0, want[p].t0);
    CHECK(g.tp == want[p].tp, "pair %d: tp = %d, expected %d", p, g.tp, want[p].tp);
    CHECK(g.ts == want[p].ts, "pair %d: ts = %d, expected %d", p, g.ts, want[p].ts);
    CHECK(g.tk == want[p].tk, "pair %d: tk = %d, expected %d", p, g.tk, want[p].tk);
    CHECK(g.t1 == want[p].t1, "pair %d: t1 = %d, expected %d", p, g.t1, want[p].t1);
    CHECK(g.t0 <= g.tp && g.tp <= g.ts && g.ts <= g.tk && g.tk <= g.t1, "pair %d: boundaries out of order", p);
  }
  // the terms the chain questions read: positions 7 .. 8 (pair 5), 15 .. 16 (pair 6) and 17 .. 21 (pair 7); the rest plain SE, D = 2
  const int P = SGP_KIND_TIMES_PREV;
  Term terms[22];
  for (Term& t : terms) t = {SGP_SE, 2};
  terms[7] = {SGP_SE, 3}, terms[8] = {SGP_MATERN32 | P, 1};                     // one chain of 2: dims 3, 1 -> DMAX 4
  terms[15] = {SGP_RQ, 1}, terms[16] = {SGP_LINEAR, 16};                        // two chains of 1: DMAX 1 and 16
  terms[17] = {SGP_SE, 9};                                                      // the plain term of pair 7: not part of a chain
  terms[18] = {SGP_LINEAR, 5};                                                  // a chain of 1: DMAX 8
  terms[19] = {SGP_SE, 1}, terms[20] = {SGP_MATERN52 | P, 2}, terms[21] = {SGP_RQ | P, 6};   // a chain of 3: dims 1, 2, 6 -> DMAX 8
  CHECK(chain_end(terms, 7, 9) == 9, "pair 5: the chain at 7 ends at %d, expected 9", chain_end(terms, 7, 9));
  CHECK(chain_dmax(terms, 7, 9) == 4, "pair 5: DMAX %d, expected 4", chain_dmax(terms, 7, 9));
  CHECK(chain_end(terms, 15, 17) == 16, "pair 6: the chain at 15 ends at %d, expected 16", chain_end(terms, 15, 17));
  CHECK(chain_dmax(terms, 15, 16) == 1, "pair 6: DMAX %d, expected 1", chain_dmax(terms, 15, 16));
  CHECK(chain_end(terms, 16, 17) == 17, "pair 6: the chain at 16 ends at %d, expected 17", chain_end(terms, 16, 17));
  CHECK(chain_dmax(terms, 16, 17) == 16, "pair 6: DMAX %d, expected 16", chain_dmax(terms, 16, 17));
  CHECK(chain_end(terms, 18, 22) == 19, "pair 7: the chain at 18 ends at %d, expected 19", chain_end(terms, 18, 22));
  CHECK(chain_dmax(terms, 18, 19) == 8, "pair 7: DMAX %d, expected 8", chain_dmax(terms, 18, 19));
  CHECK(chain_end(terms, 19, 22) == 22, "pair 7: the chain at 19 ends at %d, expected 22", chain_end(terms, 19, 22));
  CHECK(chain_dmax(terms, 19, 22) == 8, "pair 7: DMAX %d, expected 8", chain_dmax(terms, 19, 22));
  // a chain never runs past the end of its pair, whatever follows it in the table
  CHECK(chain_end(terms, 19, 21) == 21, "a chain cut at its pair's end: %d, expected 21", chain_end(terms, 19, 21));
  // walking pair 7's chains as the drivers do visits exactly the two heads
  int heads = 0, at[2] = {-1, -1};
  const PairSegs g7 = pair_segments(term_ptr, nplain, npatch, nkprod, 7);
  for (int t = g7.tk; t < g7.t1; t = chain_end(terms, t, g7.t1)) {
    if (heads < 2) at[heads] = t;
    ++heads;
  }
  CHECK(heads == 2 && at[0] == 18 && at[1] == 19, "pair 7: %d chain heads at %d, %d, expected 2 at 18, 19", heads, at[0], at[1]);
  std::printf("cases %ld failures %ld\n", cases, failures);
  return failures ? 1 : 0;
}
