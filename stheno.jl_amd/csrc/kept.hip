// The shared launches of every read of a kept posterior (kept.h).  No kernels here.
#include "kept.h"

namespace sgp {

Kept PostRef::kept() const {
  Kept k;
  if (dense) {
    k.L1 = dense->dA;
    k.ld1 = dense->ld;
    k.w1 = dense->d_wall;
    k.z = dense->dA + dense->n_pad;
    k.ldz = dense->ld;
    k.n = dense->N;
    k.n_pad = dense->n_pad;
  } else {
    k.L1 = sparse->dLz;
    k.ld1 = sparse->m_pad;
    k.w1 = sparse->d_wz;
    k.L2 = sparse->dG;
    k.ld2 = sparse->ldg;
    k.w2 = sparse->d_wg;
    k.z = sparse->dG + sparse->m_pad;
    k.ldz = sparse->ldg;
    k.n = sparse->M;
    k.n_pad = sparse->m_pad;
  }
  return k;
}

int kept_door(PostRef p, bool args, const char* who, const char* multi_refusal, bool any_multi_ctx) {
  REFUSE_UNLESS(p && args, who, "NULL argument");
  REFUSE_UNLESS(drv_ctx_is_live(p.ctx(), p.ctx_serial()), who, "the context this posterior was created on has been destroyed");
  REFUSE_UNLESS(!multi_refusal || !(p.sharded() || (any_multi_ctx && p.ctx()->multi)), who, multi_refusal);
  return 0;
}

int CrossRows::solve(sgp_ctx* ctx, const Kept& k, const CrossSource& src, long rows_pad, hipStream_t s) {
  Ns = src.Ns;
  ns_pad = rows_pad;
  const size_t bytes = sizeof(double) * ns_pad * k.n_pad;
  CHECK_RC(V.alloc((size_t)ns_pad * k.n_pad));
  if (k.L2) CHECK_RC(V2.alloc((size_t)ns_pad * k.n_pad));
  if (src.mean_s) CHECK_RC(mean_s.upload(src.mean_s, Ns));
  SGP_HIP(hipMemsetAsync(V.p, 0, bytes, s));
  if (src.spec)
    CHECK_RC(drv_assemble(src.spec, V.p, ns_pad, 0, ns_pad / TILE, 0, k.n_pad / TILE, 0, -1, 0.0, nullptr, s));
  else
    SGP_HIP(hipMemcpy2DAsync(V.p, sizeof(double) * ns_pad, src.host, sizeof(double) * src.ld, sizeof(double) * Ns, (size_t)k.n,
                             hipMemcpyHostToDevice, s));
  CHECK_RC(drv_row_trsm(ctx, V.p, ns_pad, ns_pad, k.L1, k.ld1, k.w1, k.n_pad, s));
  if (k.L2) {
    SGP_HIP(hipMemcpyAsync(V2.p, V.p, bytes, hipMemcpyDeviceToDevice, s));
    CHECK_RC(drv_row_trsm(ctx, V2.p, ns_pad, ns_pad, k.L2, k.ld2, k.w2, k.n_pad, s));
  }
  return 0;
}

int CrossRows::mean(const Kept& k, hipStream_t s) {
  CHECK_RC(mu.alloc(Ns));
  return launch_gemv_rows(k.L2 ? V2.p : V.p, ns_pad, Ns, k.n, k.z, k.ldz, mean_s.p, mu.p, s);
}

int CrossRows::variance(sgp_ctx* ctx, const Kept& k, const sgp_dspec* prior_ss, const double* prior_var_host, hipStream_t s) {
  if (prior_ss)
    CHECK_RC(prior.alloc(Ns));
  else
    CHECK_RC(prior.upload(prior_var_host, Ns));
  CHECK_RC(var.alloc(Ns));
  if (prior_ss) CHECK_RC(drv_diag_of_spec(ctx, prior_ss, prior.p, s));
  CHECK_RC(launch_colsumsq_sub(V.p, ns_pad, Ns, k.n, prior.p, var.p, -1.0, s));
  if (k.L2) CHECK_RC(launch_colsumsq_sub(V2.p, ns_pad, Ns, k.n, var.p, var.p, +1.0, s));
  return 0;
}

}  // namespace sgp
