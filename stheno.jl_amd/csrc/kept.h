// The read side of a kept posterior: what every way of asking one something starts with.  Not part of the ABI.
//
//   V   <- K(x*, x) L1^-T                  zero fill, assembly (or a copy of the caller's matrix), row_trsm against the kept factor
//   V2  <- V L2^-T                         the sparse (VFE) posterior only: B' = V against Lz, C' = V2 = B' Le^-T
//   m*  <- mean_s + (V2 or V) z            launch_gemv_rows against the solved border row
//   v*  <- k** - |V|^2 (+ |V2|^2)          the prior diagonal, then launch_colsumsq_sub once per buffer
// sgp_posterior_predict, _predict_explicit and sgp_sparse_posterior_predict (capi.hip), rand / logpdf of a posterior FiniteGP
// (postfx.hip) and the prediction gradients (predgrad.hip) all issue these launches, in this order, from here -- which is
// why their means and variances agree to the bit.  No kernels of its own: kept.hip calls the drv_ doors of driver.h.
#pragma once
#include "ctx.h"
#include "driver.h"

namespace sgp {

// the kept factor(s) a posterior answers from: V = K(x*, .) L1^-T over n_pad columns of which n are points; the sparse
// posterior solves V once more against L2 (C = B Le^-T), takes its mean from C and adds C C' back; z: the solved border row
struct Kept {
  const double *L1 = nullptr, *w1 = nullptr, *L2 = nullptr, *w2 = nullptr, *z = nullptr;
  long ld1 = 0, ld2 = 0, ldz = 0, n = 0, n_pad = 0;
};
// Which posterior a reader was handed, exact or sparse.  kept() reads the factor pointers and sizes and is called with the
// context held (CtxScope): update_posterior replaces the buffers and changes the sizes under that lock.
struct PostRef {
  const sgp_post* dense = nullptr;
  const sgp_sparse_post* sparse = nullptr;
  PostRef(const sgp_post* p) : dense(p) {}
  PostRef(const sgp_sparse_post* p) : sparse(p) {}
  explicit operator bool() const { return dense || sparse; }
  sgp_ctx* ctx() const { return dense ? dense->ctx : sparse->ctx; }
  long ctx_serial() const { return dense ? dense->ctx_serial : sparse->ctx_serial; }
  bool sharded() const { return dense && dense->mp; }   // the factor lies on the ranks of a multi-GPU context (multi.hip)
  Kept kept() const;
};

// The door of every reader, before it takes the context: its arguments are there (`args`: the caller's own pointers) and the
// posterior's context is alive.  multi_refusal, in the reader's own words: refuse a sharded factor, and with any_multi_ctx
// every posterior of a multi-GPU context; nullptr: the reader takes such posteriors.  Errors read "<who>: <text>".
int kept_door(PostRef p, bool args, const char* who, const char* multi_refusal = nullptr, bool any_multi_ctx = true);

// where the rows K(x*, x) come from: assembled in place from a cross spec, or copied from an Ns x kept.n host matrix
struct CrossSource {
  const sgp_dspec* spec = nullptr;
  const double* host = nullptr;
  long ld = 0;                      // leading dimension of host
  long Ns = 0;
  const double* mean_s = nullptr;   // host, Ns values: the prior mean at x* (nullptr: zero)
};

// the solved cross rows of one call, rows_pad x kept.n_pad each, and what is read off them
struct CrossRows {
  DevBuf V, V2, mean_s, mu, prior, var;
  long Ns = 0, ns_pad = 0;
  int solve(sgp_ctx* ctx, const Kept& k, const CrossSource& src, long rows_pad, hipStream_t s);
  int mean(const Kept& k, hipStream_t s);   // -> mu, from V2 where the posterior has a second factor
  // -> var; the prior diagonal from prior_ss, or Ns uploaded values where there is no spec
  int variance(sgp_ctx* ctx, const Kept& k, const sgp_dspec* prior_ss, const double* prior_var_host, hipStream_t s);
};

}  // namespace sgp
