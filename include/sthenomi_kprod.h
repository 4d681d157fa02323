/* sthenomi_kprod.h -- product chains of kernels, the RationalQuadratic, Linear, Cosine, GammaExponential and general-nu
 * Matern kinds, and the
 * gradient of logpdf with respect to kernel parameters, through libsthenomi_kprod.so.
 *
 * An extension of the drop-in boundary (include/sthenomi.h), in a header and a library of its own, as
 * include/sthenomi_stencil.h is: the product header's entry points are a fixed table.  libsthenomi_kprod.so links against
 * libsthenomi.so and works on the contexts, specs and error state created there.  Plain C like the product header.
 *
 * KernelFunctions' KernelProduct (`k1 * k2`, which Stheno re-exports) multiplies kernels entry by entry.  A term of a
 * sgp_cov_spec stands for coef rs_i k(x_i, x'_j) cs_j; a CHAIN of terms stands for
 *     coef_head rs_i cs_j  prod_f k_f(x^f_i, x'^f_j)
 * Encoding (constants in include/sthenomi.h):
 *   - SGP_KIND_TIMES_PREV (0x100) or-ed into sgp_term.kind marks a continuation: inside one block pair's CSR range it
 *     multiplies the chain begun by the nearest preceding term without the flag, the head;
 *   - every factor names its own row_input / col_input (the factors of one product read differently scaled or transformed
 *     views of the points); the two inputs of a factor have one dimension;
 *   - a continuation has coef == 1.0, NULL row_scale / col_scale and reserved == 0, and is never the first term of a pair;
 *   - the head of a chain, and any term of the kinds SGP_RQ / SGP_LINEAR / SGP_COSINE / SGP_GAMMAEXP / SGP_MATERN_NU / SGP_NEURALNET /
 *     SGP_FBM / SGP_EXPONENTIATED / SGP_WIENER / SGP_PIECEWISE0 .. 3 (a chain of length one), has reserved == 0: there are no products with patch or stencil sides.
 * Kinds that exist on this path only (codes 6, 7, 10 .. 14, 16, 17, 20, 24, 25, 26; 8, 9, 15, 18, 19, 21 .. 23 and 27 and above
 * are refused as unknown):
 *   SGP_RQ        param = alpha > 0:  (1 + d^2 / (2 alpha))^-alpha       (RationalQuadraticKernel)
 *   SGP_LINEAR    param = c >= 0:     x'y + c                            (LinearKernel; PolynomialKernel(n, c) is a chain of
 *                                                                         n such factors)
 *   SGP_COSINE    param ignored:      cos(pi d), d = sqrt(d^2)           (CosineKernel; SE x Cosine is the Gabor kernel, sums of
 *                                                                         SE x Cosine over 1-D projections the spectral mixtures)
 *   SGP_GAMMAEXP  param = gamma, finite and in (0, 2]:  exp(-d^gamma) = exp(-(d^2)^(gamma / 2))
 *                                                                        (GammaExponentialKernel, KernelFunctions >= 0.9: Euclidean
 *                                                                         d; gamma = 1 is ExponentialKernel, gamma = 2 is
 *                                                                         SEKernel o ScaleTransform(sqrt 2))
 *   SGP_MATERN_NU param = nu, finite and in (0, SGP_MATERN_NU_MAX]:  2^(1-nu) / Gamma(nu) x^nu K_nu(x), x = sqrt(2 nu) d
 *                                                                        (MaternKernel(nu): Euclidean d, as in KernelFunctions and
 *                                                                         scikit-learn; nu = 1/2, 3/2, 5/2 are SGP_MATERN12 / 32 /
 *                                                                         52, which stay the faster closed forms)
 *   SGP_NEURALNET param ignored:     asin(x'y / sqrt((1 + x'x)(1 + y'y)))       (NeuralNetworkKernel, Williams' arcsine kernel)
 *   SGP_FBM       param = h, finite and in (0, 1]:  (|x|^2h + |y|^2h - |x - y|^2h) / 2
 *                                                                        (FBMKernel: fractional Brownian motion; h = 1/2 is the
 *                                                                         Wiener process on the half line, h = 1 is x'y)
 *   SGP_EXPONENTIATED param ignored: exp(x'y)                            (ExponentiatedKernel)
 * The last three are not functions of the distance: they are functions of s = x'y, a = x'x, b = y'y, formed by one fma chain
 * each in the same order (s == a == b bit for bit where x == y), and of d^2 = |x - y|^2 formed from direct differences, never
 * as a + b - 2 s.  SGP_NEURALNET is evaluated as atan2(s, R) with R^2 = (1 + a)(1 + b) - s^2 = 1 + a + b + sum_{i<j} (x_i y_j -
 * x_j y_i)^2 (Lagrange's identity: a sum of squares, D (D - 1) / 2 products, empty and exact at D = 1): asin of a ratio near 1,
 * and a b - s^2 as a difference, lose several 1e5 units of 2^-53 on nearly parallel points at large norms.  SGP_FBM: a power term
 * whose base (a, b or d^2) is exactly 0 contributes exactly 0 to the value and to every derivative -- d / dh included
 * (0^h log 0 := 0), and h < 1/2, where the true point derivative diverges: the subgradient rule GammaExponential and Matern-1/2
 * have at coincident points.  So FBM is exactly a^h on the diagonal and exactly 0 against the origin.
 * Range: finite results for |x|^2, |y|^2 <= 1e300 (SGP_NEURALNET, SGP_FBM) and x'y <= 709 (SGP_EXPONENTIATED); SGP_NEURALNET is
 * ACCURATE only while (1 + x'x)(1 + y'y) is representable (norms up to about 1e77): beyond it the squares of Lagrange's sum
 * overflow, R is +inf and the kernel and its derivatives come out as 0 -- finite, and wrong (parallel points at norm 1e150 give 0
 * where the kernel is pi / 2).  Scale such inputs first.  An overflowed
 * exp is +inf, and the factorisation then reports "not positive definite" like any other such matrix.  Beyond the range the
 * results are inf or NaN; nothing faults.  Error models: tests/dotkinds_truth.py.
 *   SGP_WIENER    param = i, exactly 0, 1, 2 or 3:  the i-times integrated Wiener process (WienerKernel{i}); with X = |x|,
 *                 Y = |y|, m = min(X, Y), M = max(X, Y), d = |x - y|:
 *                     i = 0  m          i = 1  m^3 / 3 + m^2 d / 2          i = 2  m^5 / 20 + m^3 d (X + Y - m / 2) / 12
 *                     i = 3  m^7 / 252 + m^4 d (5 M^2 + 2 X Y + 3 m^2) / 720
 *   SGP_PIECEWISE0 .. SGP_PIECEWISE3 (the code carries the degree q)  param = j, an integer in [1, SGP_PIECEWISE_J_MAX]:
 *                 max(1 - r, 0)^(j + q) p_q(r), r = d   (PiecewisePolynomialKernel{q}(dim), Rasmussen & Williams eq. 4.21; the
 *                 host passes j = floor(dim / 2) + q + 1, the library knows nothing of dim)
 *                     p_0 = 1    p_1 = 1 + (j + 1) r    p_2 = 1 + (j + 2) r + (j^2 + 4 j + 3) / 3 r^2
 *                     p_3 = 1 + (j + 3) r + (6 j^2 + 36 j + 45) / 15 r^2 + (j^3 + 9 j^2 + 23 j + 15) / 15 r^3
 * SGP_WIENER is a kind of the scalars above: X^2 = a, Y^2 = b and d^2 from direct differences (never a + b - 2 s), the three
 * square roots correctly rounded; only +, x, / by constants, min and max follow, every term is positive.  Rules at the ends:
 * the kernel is symmetric bit for bit (min / max and the commutative X + Y and X Y); exactly 0 against the origin; on the
 * diagonal d = 0 exactly and k is the single first term.  Point derivatives in the coefficient form of the kinds of x'y,
 * d k / d x = c1 x + c2 (x - y) (c3 = 0): dX / dx = x / X and 0 at X = 0, dd / dx = (x - y) / d and 0 at d = 0; at a tie X == Y,
 * which includes every diagonal entry, dm (and dM) goes half to each side, x / (2 X) and y / (2 Y): with LINEAR's diagonal
 * convention this gives the true d k(x, x) / dx, the rule SGP_FBM follows at h = 1/2.  d k / d g = (2 i + 1) k (homogeneous),
 * d k / d param = 0 (i is discrete).  Finite while m^(2 i + 1) and the products with d and M^2 are representable.  i >= 1 is
 * not known to be positive definite beyond the half line.
 * SGP_PIECEWISE: exactly 1 at d^2 == 0; exactly 0 with every derivative exactly 0 for r >= 1 and for an overflowed d^2 (the
 * only kind whose exact zeros come from the data).  The power is taken by square-and-multiply on 1 - r (exact for r >= 1/2),
 * not pow.  d k / d (d^2) = k'(r) / (2 r) with k'(r) = -r (1 - r)^(j+q-1) pt_q(r) for q >= 1 (pt_1 = (j + 1)(j + 2),
 * pt_2 = (j + 3)(j + 4) / 3 (1 + (j + 1) r), pt_3 a quadratic: stheno.jl_amd/csrc/kprod.hip), a power times a polynomial and
 * never a quotient by r; q = 0: -j (1 - r)^(j-1) / (2 r), and 0 at r = 0, the subgradient Matern-1/2 has there.
 * d k / d g = 2 d^2 d k / d (d^2), d k / d param = 0.  A param outside these sets, not integer-valued, NaN or inf is refused
 * at upload by name, as SGP_FBM's.  Error models: tests/wienerpp_truth.py.
 * General-nu Matern has no library call to lean on: K_nu is evaluated in fp64 by Temme's series (x <= 2) or Steed's second
 * continued fraction (x > 2) at the order mu = nu - n in [-1/2, 1/2), followed by n - 1 steps of the upward recurrence, on
 * quantities scaled by the power of x and by e^x so that nothing overflows or underflows before the last product; what depends
 * on nu alone (Temme's coefficients, the normalisation) is computed once per term when the spec is uploaded.  The cap on nu
 * bounds the recurrence's trip count.  The relative error is at most (128 + 4 x + 3 n) 2^-53, n = floor(nu + 1/2)
 * (tests/matern_nu_truth.py derives the constants; docs/03_kernels.md section 3.2e has the measured maxima).  nu is held fixed:
 * d k / d nu is not formed and grad_param of such a term is 0.
 * Cosine is evaluated with cospi / sinpi (exact argument reduction: the only error that grows with d is the square root's half
 * ulp, pi d |sin pi d| units of 2^-53) and is the one factor that changes sign and passes through zero.  Rules at the ends:
 *   d^2 == 0      all three kinds are exactly 1.  d k / d (d^2) of general-nu Matern is -nu / (2 (nu - 1)) for nu > 1 and, where
 *                 it diverges (nu <= 1), 0, the same subgradient.  Of the other two:  d k / d (d^2) of Cosine takes its limit -pi^2 / 2 (by a branch, not 0 / 0); that of
 *                 GammaExponential, which diverges for gamma < 2, is taken as 0 -- the subgradient Matern-1/2 has there -- and
 *                 d k / d gamma as its limit 0.
 *   d^2 == +inf   (an overflowed squared distance) Cosine is exactly 1 with derivatives exactly 0 (every double >= 2^53 is an
 *                 even integer, and cospi(inf) would be NaN): an underflowed SE times a Cosine is an exact 0, never NaN.
 *                 GammaExponential is exactly 0 there and wherever exp(-d^gamma) underflows, and then so are its derivatives;
 *                 the same holds for general-nu Matern (an underflowed SE times it is an exact 0).
 * Limits, from the assembly and contraction kernels' 64 KiB of column points in LDS and their registers
 * (stheno.jl_amd/csrc/kprod.hip): at most SGP_KPROD_MAX_FACTORS factors in a chain, factor input dimension at most
 * SGP_KPROD_MAX_DIM, and factors x (the chain's largest factor dimension rounded up to a power of two) <= 64 -- 8 factors up
 * to dimension 8, 4 at dimension 9 .. 16.  A spec beyond them, or with a malformed chain, fails wherever it is uploaded
 * (every entry point; sgp_dspec_create) with rc < 0 and a message naming "product".
 *
 * Chains and terms of the new kinds run on every fp64 operator of a single-GPU context: sgp_kernelmatrix / _diag,
 * sgp_logpdf (_batch, sgp_logpdf_pool), sgp_rand, the posterior and its extension, sgp_elbo and the sparse posterior, and
 * sgp_logpdf_grad, whose outputs keep one entry per element of spec->terms: for a chain with head h
 *     grad_coef[h]       = sum_ij G_ij rs_i cs_j prod_f k_f        grad_coef[continuation] = 0
 *     grad_inscale[f]    = sum_ij G_ij coef_h rs_i cs_j (prod_{f' != f} k_f') d k_f(g x, g x') / dg at g = 1
 * (LINEAR: 2 x'y;  RQ: -d^2 (1 + d^2 / (2 alpha))^(-alpha - 1);  COSINE: -pi d sin(pi d);  GAMMAEXP: -gamma d^gamma k;
 * MATERN_NU: -C x^(nu+1) K_(nu-1)(x), C = 2^(1-nu) / Gamma(nu);  NEURALNET: s (1 / (1 + a) + 1 / (1 + b)) / R;  FBM: 2 h k;
 * EXPONENTIATED: 2 s k;  WIENER: (2 i + 1) k;  PIECEWISE: 2 d^2 d k / d (d^2)).  With
 * respect to the points a distance kind contributes 2 kappa' (x - x'), kappa' = d k / d (d^2): COSINE -pi sin(pi d) / (2 d),
 * GAMMAEXP -(gamma / 2) d^gamma k / d^2, MATERN_NU -(nu / x) C x^nu K_(nu-1)(x).  The kinds of x'y contribute
 * d k / d x (row point; the column point's is the same with x and y exchanged):  LINEAR y;  NEURALNET (y - s x / (1 + a)) / R;
 * FBM h a^(h-1) x - h (d^2)^(h-1) (x - y);  EXPONENTIATED k y.  On the diagonal (sgp_kernelmatrix_diag_grad_param) they follow
 * LINEAR's convention: the row input receives d k / d x, the column input d k / d y, both added when the two are one array.
 * The gradients with respect to the points the factors read,
 * to function-valued scales and everything behind the ELBO come from the superset family of include/sthenomi_kprod_grad.h
 * (sgp_logpdf_grad_param_xs, sgp_kernelmatrix_diag_grad_param, sgp_elbo_grad_param; libsthenomi_kprod_grad.so).  The entry points of include/sthenomi.h
 * for those gradients keep refusing chains with rc < 0 and a message naming "product" and the function to call instead:
 * sgp_logpdf_grad_x / _xs, every sgp_elbo_grad*, sgp_kernelmatrix_diag_grad*.  What still refuses outright, each a pull request
 * of its own: sgp_logpdf_grad_batch, sgp_logpdf_grad_pool, the fp32 entry points (sgp_*_f32), every multi-GPU context, and
 * products with patch or stencil sides. */
#ifndef STHENOMI_KPROD_H
#define STHENOMI_KPROD_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGP_KPROD_MAX_FACTORS 8
#define SGP_KPROD_MAX_DIM 16
#define SGP_MATERN_NU_MAX 32.0
#define SGP_PIECEWISE_J_MAX 64

/* Values of sgp_term.kind that exist on this path only and are declared here (the others: the enum of include/sthenomi.h) */
enum {
  SGP_WIENER = 10,     /* WienerKernel{i}: the i-times integrated Wiener process of |x|, |y|, |x - y|; param = i in {0, 1, 2, 3} */
  SGP_PIECEWISE0 = 11, /* PiecewisePolynomialKernel{q}(dim): max(1 - d, 0)^(j + q) p_q(d), q = code - 11; param = j, an integer */
  SGP_PIECEWISE1 = 12, /*   in [1, SGP_PIECEWISE_J_MAX]; the host passes j = floor(dim / 2) + q + 1                              */
  SGP_PIECEWISE2 = 13,
  SGP_PIECEWISE3 = 14
};

/* sgp_logpdf_grad plus the gradient with respect to the kernel parameters: grad_param (may be NULL, like every output) has
 * one entry per element of spec->terms,
 *     grad_param[t] = sum_ij G_ij coef_h rs_i cs_j (prod_{f' != t} k_f') d k_t / d param
 * with d k / d param = k (u / (1 + u) - log1p(u)), u = d^2 / (2 alpha), for SGP_RQ; d k / d gamma = -k d^gamma log(d^2) / 2 for
 * SGP_GAMMAEXP; d k / d h = (a^h log a + b^h log b - (d^2)^h log d^2) / 2 for SGP_FBM; 1 for SGP_LINEAR and SGP_CONST; 0 for the kinds without a parameter (SGP_COSINE, SGP_NEURALNET and SGP_EXPONENTIATED among them), for
 * SGP_MATERN_NU, whose nu is held fixed, and for SGP_WIENER and SGP_PIECEWISE0 .. 3, whose i and j are discrete.  Plain terms (outside any chain) get their entries too.  Every other output is bit for bit what
 * sgp_logpdf_grad returns for the same arguments.  Any spec sgp_logpdf_grad takes, on a single-GPU context: a multi-GPU
 * context refuses this entry point (rc < 0) whatever the spec holds, product chains or not. */
int sgp_logpdf_grad_param(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind, const double* noise,
                          const double* y, double* logpdf_out, double* grad_y, double* grad_mean, double* grad_noise,
                          double* grad_coef, double* grad_inscale, double* grad_param);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_KPROD_H */
