// Which terms of a block pair are what, in ONE place.  dspec_create (capi.hip) sorts every pair's terms by class with a stable
// pass -- plain | patch (conv.hip) | stencil (stencil.hip) | derivative (deriv.hip) | product chains (kprod.hip) -- and always
// fills the count arrays read here, whatever classes the spec has.  Host-only plain C++17: nothing of HIP is included, so the
// boundaries are checked by a g++ program of their own (tests/spec_segments_host.cpp).  A new term class is one boundary here.
#pragma once
#include "kprod_kinds_table.h"

namespace sgp {

// device positions of pair p's terms: plain [t0, tp) | patch [tp, ts) | stencil [ts, td) | derivative [td, tk) | chains [tk, t1)
struct PairSegs {
  int t0, tp, ts, tk, t1;
  int td = -1;   // filled by pair_segments; == tk where the pair has no derivative terms
};
// term_ptr: CSR over the pairs; nplain / npatch / nderiv / nkprod: per pair, the plain, patch, derivative and chain terms (the
// rest are stencil terms)
inline PairSegs pair_segments(const int* term_ptr, const int* nplain, const int* npatch, const int* nderiv, const int* nkprod,
                              int p) {
  PairSegs g;
  g.t0 = term_ptr[p];
  g.tp = g.t0 + nplain[p];
  g.ts = g.tp + npatch[p];
  g.t1 = term_ptr[p + 1];
  g.tk = g.t1 - nkprod[p];
  g.td = g.tk - (nderiv ? nderiv[p] : 0);
  return g;
}
// a spec without derivative terms
inline PairSegs pair_segments(const int* term_ptr, const int* nplain, const int* npatch, const int* nkprod, int p) {
  return pair_segments(term_ptr, nplain, npatch, nullptr, nkprod, p);
}

// the chain whose head sits at device position t of a pair that ends at t1: one past its last factor (terms[i].kind is a code,
// continuations with KP_TIMES_PREV), and the DMAX of its factors [t, e) (terms[i].dim)
template <class Term>
int chain_end(const Term* terms, int t, int t1) {
  int e = t + 1;
  while (e < t1 && (terms[e].kind & KP_TIMES_PREV)) ++e;
  return e;
}
template <class Term>
int chain_dmax(const Term* terms, int t, int e) {
  int dm = 1;
  for (int f = t; f < e; ++f)
    if (pow2ceil(terms[f].dim) > dm) dm = pow2ceil(terms[f].dim);
  return dm;
}

}  // namespace sgp
