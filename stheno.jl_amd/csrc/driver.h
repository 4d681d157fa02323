// Internal entry points of the single-GPU driver (capi.hip) used by the multi-GPU driver (multi.hip): the same
// routines the C-ABI entry points are built from, without locking (the caller serialises: one host thread per
// multi-GPU call) and on an explicit stream.  Not part of the ABI.
#pragma once
#include "ctx.h"
#include "../../include/sthenomi_pool.h"

namespace sgp {

// K(rows, cols) of `ds` restricted to the global tile window, element (r, c) at Kv[r + c * ld]
int drv_assemble(const sgp_dspec* ds, double* Kv, long ld, long tile_r_lo, long tile_r_hi, long tile_c_lo,
                 long tile_c_hi, int lower_only, int noise_kind, double sigma2, const double* d_noise_diag,
                 hipStream_t s);
// Factor a PACKED column panel (w columns over m rows, element [0] = (row g0, column g0) of the matrix); keeps the panel's
// inverse 16x16 diagonal blocks (INVD_STRIDE doubles per 128-block) in d_invstore (may be NULL) -- what later solves against
// the factor need -- and adds the logdet contribution of the factored columns to *d_logdet.
// df != 0: one launch of the dataflow kernel on the panel (the hybrid schedule, round 6), with the optional extension px: only
// the first px->n_fact columns are factored (the others updated with them), external source panels applied first.
// lean != 0: the two-workgroups-per-CU instantiation of that kernel (ranks sharing one GPU).
// d_nz / nz_words: the factor's tile pattern (structural zeros), read at the panel's offset g0 / 128; NULL: dense.
int drv_panel_factor(sgp_ctx* ctx, double* P, long ld, long m, long w, long g0, double* d_logdet, int* d_info,
                     double* d_invstore, hipStream_t s, int df = 0, const sgp::sz_word* d_nz = nullptr, int nz_words = 0,
                     const sgp::DfPanel* px = nullptr, int lean = 0);
// R <- R L^-T for nrows (multiple of 128) rows against an n x n lower factor with its kept inverse blocks
int drv_row_trsm(sgp_ctx* ctx, double* R, long ldr, long nrows, const double* L, long ldl, const double* d_invall,
                 long n, hipStream_t s);
// back substitution over the 128-blocks k_first, k_first - 128, ..., k_last of alpha = L^-T z:
// element (r, c) of the factor at Lv[r + c * ld] (virtual base), inverse blocks of 128-block b at
// wall_v + b * INVD_STRIDE; d_z / d_alpha are indexed globally, rows up to n_end are read.
int drv_back_substitute(const double* Lv, long ld, const double* wall_v, long k_first, long k_last, long n_end,
                        double* d_z, double* d_alpha, hipStream_t s);
// the columns [c, c + w) of a row block whose columns left of c are solved and applied (row_trsm's in-block part)
int drv_row_trsm_block(double* R, long ldr, long nrows, const double* L, long ldl, const double* d_invall, long c, long w,
                       hipStream_t s);
// the bordered factorisation (capi.hip: chol_bordered, dense) of the sub-matrix whose element (0, 0) is A[0]: n_cols columns
// over m_rows rows; d_wall (offset by the caller) receives the inverse diagonal blocks, ctx->d_slots[0 .. n_cols / 128) the
// logdet contributions, *ctx->d_info the failing minor counted from the sub-matrix's first column
int drv_chol_sub(sgp_ctx* ctx, double* A, long ld, long n_cols, long m_rows, double* d_wall, hipStream_t s);
int drv_fetch_info(sgp_ctx* ctx, hipStream_t s);   // *ctx->d_info after draining s (notes a dataflow time-out on ctx)
bool drv_ctx_is_live(const sgp_ctx* ctx, long serial);
// run() once more on the launch-based schedule when it came back with a dataflow time-out (capi.hip: with_df_fallback)
int drv_with_df_fallback(sgp_ctx* ctx, const std::function<int()>& run);
// update_posterior (include/sthenomi_extend.h: sgp_posterior_extend, forwarded from libsthenomi_extend.so) -- extend.hip
int drv_posterior_extend(sgp_post* post, const sgp_cov_spec* spec_all, const double* mean_all, int noise_kind,
                         const double* noise, const double* y_all, int64_t n_new, int64_t reserve_n, double* alpha_out,
                         double* logpdf_out);
// times the row solve of `tile_rows` 128-row tiles against the kept factor by one schedule (sthenomi_extend_bench.h: sgp_bench_extend_row_solve)
int drv_extend_row_solve_ms(sgp_post* post, int64_t tile_rows, int schedule, int reps, double* ms_out);
// rand / logpdf of a posterior FiniteGP against the kept factor (include/sthenomi_postfx.h, forwarded from
// libsthenomi_postfx.so) -- postfx.hip; Z / Y: N* x cols with leading dimension ldin, rand's result N* x cols with ldo
int drv_posterior_rand(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                       int noise_kind, const double* noise, const double* Z, int64_t ldz, int64_t S, double* out, int64_t ldo);
int drv_posterior_logpdf(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                         int noise_kind, const double* noise, const double* Y, int64_t ldy, int64_t ncols, double* out);
int drv_sparse_posterior_rand(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                              const double* mean_s, int noise_kind, const double* noise, const double* Z, int64_t ldz,
                              int64_t S, double* out, int64_t ldo);
int drv_sparse_posterior_logpdf(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                const double* mean_s, int noise_kind, const double* noise, const double* Y, int64_t ldy,
                                int64_t ncols, double* out);
// posterior mean and variance with their gradients with respect to the test points (include/sthenomi_predgrad.h, forwarded
// from libsthenomi_predgrad.so) -- predgrad.hip
int drv_posterior_predict_grad_x(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                                 double* mean_out, double* var_out, double* const* grad_mean_inputs,
                                 double* const* grad_var_inputs, double* const* grad_var_prior_inputs);
int drv_sparse_posterior_predict_grad_x(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                        const double* mean_s, double* mean_out, double* var_out,
                                        double* const* grad_mean_inputs, double* const* grad_var_inputs,
                                        double* const* grad_var_prior_inputs);
// The gradient front doors: one per core of capi.hip, taking the core's argument record (ctx.h).  The C entry points of every
// family -- capi.hip's own and those of libsthenomi_kprod / _kprod_grad / _conv_grad / _stencil_grad / _stencil_wo.so -- fill
// a record, set the leave their family carries and call the door; each takes the context itself.
int drv_logpdf_grad(sgp_ctx* ctx, const LogpdfGradArgs& a);   // logpdf_grad_core, with the dataflow time-out fallback
int drv_diag_grad(sgp_ctx* ctx, const DiagGradArgs& a);       // diag_grad_core
// the leave checks, then the data-sharded call on a multi-GPU context (multi.hip) or drv_elbo_grad below on one GPU
int elbo_grad_entry(sgp_ctx* ctx, const ElboGradArgs& a);
int drv_diag_of_spec(sgp_ctx* ctx, const sgp_dspec* ds, double* d_out, hipStream_t s);
int drv_dspec_create(sgp_ctx* ctx, const sgp_cov_spec* sp, sgp_dspec** out);   // caller holds the context
// register a patch geometry on ctx (include/sthenomi_conv.h: sgp_conv_geom, whose C entry point in libsthenomi_conv.so
// forwards here); takes the context itself; an equal geometry registered before keeps its id
int drv_conv_geom(sgp_ctx* ctx, int h, int w, int ph, int pw, int32_t* id_out);
// register a stencil on ctx (include/sthenomi_stencil.h: sgp_stencil_register, forwarded from libsthenomi_stencil.so); ids
// share the table of sgp_conv_geom; a bitwise-equal stencil registered before keeps its id
int drv_stencil_register(sgp_ctx* ctx, int dim, int npoints, const double* offsets, const double* weights, int32_t* id_out);
void drv_dspec_free(sgp_dspec* ds);
// a device spec that lives as long as the call that created it
struct SpecGuard {
  sgp_dspec* ds = nullptr;
  ~SpecGuard() {
    if (ds) drv_dspec_free(ds);
  }
};
long drv_invd_stride();
// structural zeros (common.h; capi.hip: sz_pattern / sz_upload): rank 0's context computes the tile pattern of the factor
// (host), every rank uploads it; *words = 0 / *d_nz = nullptr: dense
int drv_sz_pattern(sgp_ctx* ctx, const sgp_dspec* ds, int noise_kind, long n_pad, long m_tot, int* words);
int drv_sz_upload(sgp_ctx* ctx, const sgp_ctx* from, int words, hipStream_t s, const sgp::sz_word** d_nz);
// executed tile products per tile column of the factor, from the host spec (empty: structurally dense) -- own_table.h
int drv_sz_col_work(const sgp_ctx* ctx, const sgp_cov_spec* sp, int noise_kind, long n_pad, long m_tot,
                    std::vector<double>& col_work);
double drv_sz_live_fraction(const sgp_ctx* ctx, int words, long c0, long w, long m_tot, long kt0, long kt1);
// dst[i] = src[i * stride], i < n
int drv_copy_strided(const double* src, long stride, long n, double* dst, hipStream_t s);
// C[r + c * ldc] += a * S[r + c * lds], nr x nc
int drv_axpy_block(double* C, long ldc, const double* S, long lds, long nr, long nc, double a, hipStream_t s);
// dst[i + c * ld] = mean[i] (i < N) else 0
int drv_fill_mean_cols(double* dst, long ld, long nrows, long ncols, long N, const double* mean, hipStream_t s);
// logpdf + gradient of nspec independent models (include/sthenomi_batch.h: sgp_logpdf_grad_batch, whose C entry point in
// libsthenomi_batch.so forwards here); takes the context itself, with the dataflow time-out fallback
int drv_logpdf_grad_batch(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means, int noise_kind,
                          const double* const* noises, const double* const* ys, double* logpdf_out, double* const* grad_y,
                          double* const* grad_mean, double* const* grad_noise, double* const* grad_coef,
                          double* const* grad_inscale, int* infos);
// logpdf / logpdf + gradient of nspec independent models of DIFFERENT sizes and noise kinds (include/sthenomi_pool.h, whose C
// entry points in libsthenomi_pool.so forward here): the poolable members are factored by ragged launches of the dataflow
// kernel (chol_df.hip: chol_pool_kernel), the others run through their own calls; with the dataflow time-out fallback
int drv_logpdf_pool(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                    const int* noise_kinds, const double* const* noises, const double* const* ys, double* out, int* infos,
                    sgp_pool_report* report);
int drv_logpdf_grad_pool(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                         const int* noise_kinds, const double* const* noises, const double* const* ys, double* logpdf_out,
                         double* const* grad_y, double* const* grad_mean, double* const* grad_noise,
                         double* const* grad_coef, double* const* grad_inscale, int* infos, sgp_pool_report* report);
// sparse-ELBO partial sums of a slice of the data / the final factorisation (see sgp_dev_elbo_partial / _finish);
// keep != 0: the M x M factors stay in the caller's buffers (sparse posterior)
long drv_vfe_part_len(long m_pad);
// takes the context itself (CtxScope inside): d_part receives the partial sums of the slice; dLz / d_wz (optional) keep
// the factor of K(z,z) + Sigma_z and its inverse diagonal blocks
int drv_vfe_partial(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                    const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind, const double* z_noise,
                    const double* y, double* dLz, double* d_wz, double* d_part, long part_len);
// ELBO + gradient on `ctx` (takes the context itself); shard == nullptr: the whole call, with the dataflow fallback
int drv_elbo_grad(sgp_ctx* ctx, const ElboGradArgs& a, const ElboGradShard* shard);
// h6: the six ELBO terms (see vfe_pipeline); d_wg (optional) keeps the inverse diagonal blocks of chol(A A' + I)
int drv_vfe_finish(sgp_ctx* ctx, long M, double* d_part, double* d_wg, double* h6);
// the row-chunk loop of the sparse pipeline in append mode (capi.hip: VfeRows): the rows of `dx` -- y, mean, var and noise
// are host vectors of dx->N values -- are solved against the kept dLz / d_wz of M inducing points and their sums are ADDED
// to the part d_part (the accumulate flags are on from the first chunk; the four scalars are added to the kept ones).
// The caller holds the context; stage slots as vfe_rows_partial: 0 buffers, 1 assembly, 2 row solve, 3 transpose + column
// sums, 4 Gram, 5 the scalars' sum
int drv_vfe_rows_append(sgp_ctx* ctx, const sgp_dspec* dx, long M, const double* var_x, const double* mean_x, int noise_kind,
                        const double* noise_x, const double* y, const double* dLz, const double* d_wz, double* d_part,
                        StageTimer& tm);
// sgp_sparse_posterior_update / _count (include/sthenomi_vfe_update.h, forwarded from libsthenomi_vfe_update.so) -- vfe_update.hip
int drv_sparse_posterior_update(sgp_sparse_post* post, const sgp_cov_spec* xz_new, const double* var_x_new,
                                const double* mean_x_new, int noise_kind, const double* noise_new, const double* y_new,
                                double* elbo_out);
int drv_sparse_posterior_count(sgp_sparse_post* post, int64_t* n_out);

}  // namespace sgp
