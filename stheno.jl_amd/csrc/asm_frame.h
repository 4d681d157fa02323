// The frame of every covariance-assembly kernel (kernelmatrix.hip, kprod.hip, deriv.hip, conv.hip, stencil.hip): what a launch
// writes into, how a 128 x 128 tile is clipped to its block pair, and how finished values reach the matrix.  Three decisions
// are stated here (two kernels keep a written-out copy of their store, for reasons given at the copy: assemble_block2_kernel
// that of pair_rows / store_pair_tail, stencil_kernel that of write_entry -- a change to either is made in both places):
//   * the clip of a tile to its pair (tile_clip; the gradient contractions of grad.hip, kprod.hip and deriv.hip use it too);
//   * Sigma_y enters with the FIRST launch of a pair, which overwrites; every later launch accumulates (AsmLaunch::first);
//   * how a chunk of values is stored (store_row_tail, store_pair_tail, write_entry).
// The kernels keep scalar arguments (the kernarg layout is what it was); a launcher unpacks the record at its launch.
// No helper reorders a floating-point operation: the results are the bits of the written-out code these replace.
#pragma once
#include "common.h"
#include <algorithm>
#include <climits>

namespace sgp {

// ---- host: what a launch writes into ------------------------------------------------------------------------------------
struct AsmLaunch {
  // the target: element (r, c) (global indices) at K[r + c * ld]; lower_only: tiles with tile row < tile column are skipped;
  // Sigma_y = sigma2 I (noise_kind 0) or diag(noise_diag) (1, indexed globally), none (-1)
  double* K;
  long ld;
  int lower_only, noise_kind;
  double sigma2;
  const double* noise_diag;
  // the pair's rectangle (global indices); diag: a diagonal block of a symmetric matrix, the only place Sigma_y lands
  long r0, nr, c0, nc;
  bool diag;
  // the window of global tiles this launch covers
  long r_first, c_first, r_cnt, c_cnt;
  // the pair's first launch: it overwrites and carries Sigma_y; every later one adds onto it and carries none
  bool first;

  int accumulate() const { return first ? 0 : 1; }
  int noise() const { return first && diag ? noise_kind : -1; }
  bool empty() const { return r_cnt <= 0 || c_cnt <= 0; }
  // the entries of the pair inside the window (conv.hip, stencil.hip: kernels that do not walk tiles); false: none
  bool entries(long& rlo, long& rhi, long& clo, long& chi) const {
    rlo = std::max(r0, r_first * TILE), rhi = std::min(r0 + nr, (r_first + r_cnt) * TILE);
    clo = std::max(c0, c_first * TILE), chi = std::min(c0 + nc, (c_first + c_cnt) * TILE);
    return !empty() && rlo < rhi && clo < chi;
  }
};
// the kernels' scalar arguments behind the terms, in kernarg order
#define ASM_TAIL(L) (L).lower_only, (L).accumulate(), (L).noise(), (L).sigma2, (L).noise_diag

// ---- device: the tile clipped to its pair -------------------------------------------------------------------------------
struct TileClip {
  long cbeg, cend, rbeg, rend;
};
// columns [cbeg, cend) x rows [rbeg, rend) of global tile (gtr, gtc) that lie in the pair (and, for the sharded gradient, in
// the column window [clo, chi)); false: none.  The result is uniform over the workgroup, so `if (!tile_clip(...)) return;` may
// stand before a barrier.
__device__ __forceinline__ bool tile_clip(long gtr, long gtc, long r0, long nr, long c0, long nc, TileClip& cl,
                                          long clo = LONG_MIN, long chi = LONG_MAX) {
  cl.cbeg = gtc * TILE, cl.cend = cl.cbeg + TILE;
  if (cl.cbeg < c0) cl.cbeg = c0;
  if (cl.cend > c0 + nc) cl.cend = c0 + nc;
  if (cl.cbeg < clo) cl.cbeg = clo;
  if (cl.cend > chi) cl.cend = chi;
  cl.rbeg = gtr * TILE, cl.rend = cl.rbeg + TILE;
  if (cl.rbeg < r0) cl.rbeg = r0;
  if (cl.rend > r0 + nr) cl.rend = r0 + nr;
  return cl.cbeg < cl.cend && cl.rbeg < cl.rend;
}

// ---- device: staging -----------------------------------------------------------------------------------------------------
// one-row kernels: the tile's 128 column points of every term, smem[(tm * 128 + p) * DMAX + d], p relative to gtc * 128;
// zeros past the term's dimension and outside the clip
template <int DMAX>
__device__ __forceinline__ void stage_col_points(double* smem, const DevTerm* terms, int nterms, long gtc, long c0,
                                                 const TileClip& cl, int t) {
  for (int tm = 0; tm < nterms; ++tm) {
    const DevTerm T = terms[tm];
    const int D = T.dim;
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long gc = gtc * TILE + p;
      double v = 0.0;
      if (d < D && gc >= cl.cbeg && gc < cl.cend) v = T.xc[(gc - c0) * T.ldc + d];
      smem[(tm * TILE + p) * DMAX + d] = v;
    }
  }
}

// two-row kernels, one term: s = [128][DMAX] column points | [DMAX][128] row points | rw[128] | cw[128], with
// rw = rcoef * row scale and cw = column scale (1 without one), zeros outside the clip
template <int DMAX>
__device__ __forceinline__ void stage_pair_points(double* s, const DevTerm& T, double rcoef, long gtr, long gtc, long r0,
                                                  long c0, const TileClip& cl, int t) {
  const int D = T.dim;
  double* sr = s + TILE * DMAX;
  for (int idx = t; idx < TILE * DMAX; idx += 256) {
    const int p = idx / DMAX, d = idx % DMAX;
    const long gc = gtc * TILE + p, gr = gtr * TILE + p;
    s[idx] = (d < D && gc >= cl.cbeg && gc < cl.cend) ? T.xc[(gc - c0) * T.ldc + d] : 0.0;
    sr[d * TILE + p] = (d < D && gr >= cl.rbeg && gr < cl.rend) ? T.xr[(gr - r0) * T.ldr + d] : 0.0;  // [d][row]
  }
  if (t < TILE) {
    const long gr = gtr * TILE + t;
    sr[TILE * DMAX + t] = (gr >= cl.rbeg && gr < cl.rend) ? rcoef * (T.rs ? T.rs[gr - r0] : 1.0) : 0.0;
  } else {
    const int p = t - TILE;
    const long gc = gtc * TILE + p;
    sr[TILE * DMAX + TILE + p] = (gc >= cl.cbeg && gc < cl.cend) ? (T.cs ? T.cs[gc - c0] : 1.0) : 0.0;
  }
}

// ---- device: the store tails ----------------------------------------------------------------------------------------------
// one row per thread: the Sigma_y entry of row `grow` (added where gc == grow)
__device__ __forceinline__ double row_noise(int noise_kind, double sigma2, const double* noise_diag, long grow) {
  double nval = 0.0;
  if (noise_kind >= 0) nval = (noise_kind == 0) ? sigma2 : noise_diag[grow];
  return nval;
}
__device__ __forceinline__ void store_row_entry(double* K, long ld, long grow, long gc, double v, bool diag_noise,
                                                double nval, int accumulate) {
  if (diag_noise && gc == grow) v += nval;
  double* p = K + grow + gc * ld;
  if (accumulate) v += *p;
  *p = v;
}
// acc[q] -> K[grow, gc0 + q] for the columns inside the clip
template <int NC>
__device__ __forceinline__ void store_row_tail(double* K, long ld, long grow, long gc0, const TileClip& cl,
                                               const double (&acc)[NC], bool diag_noise, double nval, int accumulate) {
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const long gc = gc0 + q;
    if (gc >= cl.cbeg && gc < cl.cend) store_row_entry(K, ld, grow, gc, acc[q], diag_noise, nval, accumulate);
  }
}

// two rows per thread: rows g0 = gtr * 128 + 2 lane and g1 = g0 + 1
struct PairRows {
  long g0, g1;
  bool ok0, ok1;     // the row lies in the clip
  bool diag_noise;   // only tiles on the diagonal carry Sigma_y entries
  double nv0, nv1;
  bool full;         // interior tile: all 128 x 128 entries belong to the block pair, and 16-byte stores are aligned
};
__device__ __forceinline__ PairRows pair_rows(const double* K, long ld, long gtr, long gtc, int lane, const TileClip& cl,
                                              int accumulate, int noise_kind, double sigma2, const double* noise_diag) {
  PairRows R;
  R.g0 = gtr * TILE + 2 * lane, R.g1 = R.g0 + 1;
  R.ok0 = R.g0 >= cl.rbeg && R.g0 < cl.rend, R.ok1 = R.g1 >= cl.rbeg && R.g1 < cl.rend;
  R.diag_noise = noise_kind >= 0 && gtr == gtc;
  R.nv0 = R.nv1 = 0.0;
  if (R.diag_noise) {
    R.nv0 = (noise_kind == 0) ? sigma2 : (R.ok0 ? noise_diag[R.g0] : 0.0);
    R.nv1 = (noise_kind == 0) ? sigma2 : (R.ok1 ? noise_diag[R.g1] : 0.0);
  }
  R.full = (cl.cend - cl.cbeg == TILE) && (cl.rend - cl.rbeg == TILE) && !accumulate &&
           ((((unsigned long long)(K + R.g0)) & 15ull) == 0) && ((ld & 1) == 0);
  return R;
}
// (acc0[q], acc1[q]) -> K[g0 .. g1, gc0 + q]
template <int NC>
__device__ __forceinline__ void store_pair_tail(double* K, long ld, long gc0, const TileClip& cl, const PairRows& R,
                                                const double (&acc0)[NC], const double (&acc1)[NC], int accumulate) {
  if (R.full && !R.diag_noise) {
    double* kp = K + R.g0 + gc0 * ld;
#pragma unroll
    for (int q = 0; q < NC; ++q) *reinterpret_cast<double2*>(kp + q * ld) = make_double2(acc0[q], acc1[q]);
  } else if (R.full) {
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const long gc = gc0 + q;
      double v0 = acc0[q], v1 = acc1[q];
      if (gc == R.g0) v0 += R.nv0;
      if (gc == R.g1) v1 += R.nv1;
      *reinterpret_cast<double2*>(K + R.g0 + gc * ld) = make_double2(v0, v1);
    }
  } else {
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const long gc = gc0 + q;
      if (gc >= cl.cbeg && gc < cl.cend) {
        double v0 = acc0[q], v1 = acc1[q];
        if (R.diag_noise && gc == R.g0) v0 += R.nv0;
        if (R.diag_noise && gc == R.g1) v1 += R.nv1;
        double* p = K + R.g0 + gc * ld;
        if (R.ok0) p[0] = accumulate ? p[0] + v0 : v0;
        if (R.ok1) p[1] = accumulate ? p[1] + v1 : v1;
      }
    }
  }
}

// one entry per thread (conv.hip; stencil.hip keeps these lines written out, see there): K[r, c] = fma(s, w, what the pair's earlier launches wrote) (+ Sigma_y)
__device__ __forceinline__ void write_entry(double* K, long ld, long r, long c, double s, double w, int accumulate,
                                            int noise_kind, double sigma2, const double* noise_diag) {
  double* p = K + r + c * ld;
  double v = fma(s, w, accumulate ? *p : 0.0);
  if (noise_kind >= 0 && r == c) v += (noise_kind == 0) ? sigma2 : noise_diag[r];
  *p = v;
}

}  // namespace sgp
