/* sthenomi_postfx.h -- rand and logpdf of a posterior FiniteGP against the kept factor, exported by libsthenomi_postfx.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h), in a header and a library of its own like sthenomi_extend.h:
 * libsthenomi.so keeps exporting exactly the product header.  libsthenomi_postfx.so links against libsthenomi.so and works
 * on the contexts, posteriors and error state created there (sgp_ctx_create, sgp_posterior_create,
 * sgp_sparse_posterior_create, sgp_last_error, ...); a host that wants these calls loads both.  Plain C like the product
 * header.
 *
 * What they are for: `rand(rng, f_post(x*, S*), S)` and `logpdf(f_post(x*, S*), y*)` of AbstractGPs.  Without them a host
 * fetches the N* x N* posterior covariance (sgp_posterior_predict, cov_out), adds S* itself and hands the sum back as dense
 * noise on a zero-term spec to sgp_rand / sgp_logpdf: two N*^2 transfers around the factorisation.  Here the posterior
 * covariance is formed, bordered and factored where the kept factor lives; only x*, S*, Y / Z and the result cross.
 *
 * The values are, bit for bit, those of that route: the same kernels in the same order -- the row solve against the kept
 * factor, the mean product, K** - V'V (+ C'C for the sparse posterior) on the lower tiles, ONE add of S*_ij per entry, the
 * bordered dense-schedule factorisation and the tails of sgp_logpdf / sgp_rand.
 *
 * Arguments shared by the four entry points
 *   cross, prior_ss, mean_s : as in sgp_posterior_predict / sgp_sparse_posterior_predict -- K(x*, x) (K(x*, z) for the sparse
 *                             posterior), K(x*, x*) (symmetric; required) and the prior mean at the N* points x* (NULL == zeros).
 *   noise_kind / noise      : S* at the N* test points as in sgp_logpdf -- SGP_NOISE_SCALAR (one value), SGP_NOISE_DIAG (N*
 *                             values) or SGP_NOISE_DENSE (N* x N* column-major, leading dimension N*; its lower tiles are read).
 *   rand   : Z is N* x S (leading dimension ldz >= N*), S >= 1; out (N* x S, ldo >= N*) = mean* + L* Z.
 *   logpdf : Y is N* x ncols (ldy >= N*), ncols >= 1; out[c] = logpdf(f_post(x*, S*), Y[:, c]).
 * rc 0; > 0: the LAPACK info of a posterior covariance + S* that is not positive definite (first failing leading minor);
 * < 0: refused, sgp_last_error() names the entry point -- a NULL argument, a destroyed context, a posterior of a multi-GPU
 * context (its factor is sharded), sizes that do not match the posterior or each other.  The posterior is only read: after
 * any return it answers exactly as before. */
#ifndef STHENOMI_POSTFX_H
#define STHENOMI_POSTFX_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

int sgp_posterior_rand(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                       int noise_kind, const double* noise, const double* Z, int64_t ldz, int64_t S, double* out,
                       int64_t ldo);
int sgp_posterior_logpdf(sgp_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss, const double* mean_s,
                         int noise_kind, const double* noise, const double* Y, int64_t ldy, int64_t ncols, double* out);
int sgp_sparse_posterior_rand(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                              const double* mean_s, int noise_kind, const double* noise, const double* Z, int64_t ldz,
                              int64_t S, double* out, int64_t ldo);
int sgp_sparse_posterior_logpdf(sgp_sparse_post* post, const sgp_cov_spec* cross, const sgp_cov_spec* prior_ss,
                                const double* mean_s, int noise_kind, const double* noise, const double* Y, int64_t ldy,
                                int64_t ncols, double* out);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_POSTFX_H */
