// Which terms of a block pair are what, in ONE place.  dspec_create (capi.hip) sorts every pair's terms by class with a stable
// pass -- plain | patch (conv.hip) | stencil (stencil.hip) | derivative (deriv.hip) | Gibbs (gibbs.hip) | additive
// (additive.hip) | blur (blur.hip) | arc-cosine (arccos.hip) | product chains (kprod.hip) -- and always
// fills the count arrays read here, whatever classes the spec has.  Host-only plain C++17: nothing of HIP is included, so the
// boundaries are checked by a g++ program of their own (tests/spec_segments_host.cpp).  A new term class is one boundary here.
#pragma once
#include "kprod_kinds_table.h"

namespace sgp {

// device positions of pair p's terms: plain [t0, tp) | patch [tp, ts) | stencil [ts, td) | derivative [td, tg) | Gibbs [tg, ta) |
// additive [ta, tb) | blur [tb, tn) | arc-cosine [tn, tk) | chains [tk, t1)
struct PairSegs {
  int t0, tp, ts, tk, t1;
  int td = -1;   // filled by pair_segments; == tg where the pair has no derivative terms
  int tg = -1;   // filled by pair_segments; == ta where the pair has no Gibbs terms
  int ta = -1;   // filled by pair_segments; == tb where the pair has no additive terms
  int tb = -1;   // filled by pair_segments; == tn where the pair has no blur terms
  int tn = -1;   // filled by pair_segments; == tk where the pair has no arc-cosine terms
};
// term_ptr: CSR over the pairs; nplain / npatch / nderiv / ngibbs / nadditive / nblur / narccos / nkprod: per pair, the plain,
// patch, derivative, Gibbs, additive, blur, arc-cosine and chain terms (the rest are stencil terms)
inline PairSegs pair_segments(const int* term_ptr, const int* nplain, const int* npatch, const int* nderiv, const int* ngibbs,
                              const int* nadditive, const int* nblur, const int* narccos, const int* nkprod, int p) {
  PairSegs g;
  g.t0 = term_ptr[p];
  g.tp = g.t0 + nplain[p];
  g.ts = g.tp + npatch[p];
  g.t1 = term_ptr[p + 1];
  g.tk = g.t1 - nkprod[p];
  g.tn = g.tk - (narccos ? narccos[p] : 0);
  g.tb = g.tn - (nblur ? nblur[p] : 0);
  g.ta = g.tb - (nadditive ? nadditive[p] : 0);
  g.tg = g.ta - (ngibbs ? ngibbs[p] : 0);
  g.td = g.tg - (nderiv ? nderiv[p] : 0);
  return g;
}
// a spec without arc-cosine terms; without blur terms; without additive terms; without Gibbs terms; without derivative terms
// either
inline PairSegs pair_segments(const int* term_ptr, const int* nplain, const int* npatch, const int* nderiv, const int* ngibbs,
                              const int* nadditive, const int* nblur, const int* nkprod, int p) {
  return pair_segments(term_ptr, nplain, npatch, nderiv, ngibbs, nadditive, nblur, nullptr, nkprod, p);
}
inline PairSegs pair_segments(const int* term_ptr, const int* nplain, const int* npatch, const int* nderiv, const int* ngibbs,
                              const int* nadditive, const int* nkprod, int p) {
  return pair_segments(term_ptr, nplain, npatch, nderiv, ngibbs, nadditive, nullptr, nullptr, nkprod, p);
}
inline PairSegs pair_segments(const int* term_ptr, const int* nplain, const int* npatch, const int* nderiv, const int* ngibbs,
                              const int* nkprod, int p) {
  return pair_segments(term_ptr, nplain, npatch, nderiv, ngibbs, nullptr, nullptr, nullptr, nkprod, p);
}
inline PairSegs pair_segments(const int* term_ptr, const int* nplain, const int* npatch, const int* nderiv, const int* nkprod,
                              int p) {
  return pair_segments(term_ptr, nplain, npatch, nderiv, nullptr, nullptr, nullptr, nullptr, nkprod, p);
}
inline PairSegs pair_segments(const int* term_ptr, const int* nplain, const int* npatch, const int* nkprod, int p) {
  return pair_segments(term_ptr, nplain, npatch, nullptr, nullptr, nullptr, nullptr, nullptr, nkprod, p);
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
