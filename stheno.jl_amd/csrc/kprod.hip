// Product chains (include/sthenomi_kprod.h): covariance terms that multiply several leaf kernels, each on its own view of
// the points, and the kinds that exist only here: RationalQuadratic, Linear, Cosine, GammaExponential, general-nu Matern and
// the kinds of x'y: NeuralNetwork, FBM, Exponentiated, and Wiener (|x|, |y|, |x - y|) and the compactly supported
// PiecewisePolynomial kinds.
//     chain value (i, j) = coef_head rs_i cs_j  prod_f k_f(x^f_i, x'^f_j)
// KernelFunctions' KernelProduct [EXT] (`k1 * k2`, reached through src/Stheno.jl:4-6); the locally periodic kernel of the
// Mauna-Loa models and the sums of products of the neural-kernel-network example are such chains.
//
// Assembly: the plain assembly's one-row tiling (kernelmatrix.hip: assemble_block_kernel) -- 128 x 128 tiles on the global
// tile grid, 256 threads, thread = one row x 64 columns, the 128 column points of EVERY factor staged in LDS point-major
// and read as wave-uniform broadcasts, the factor's row point in registers while its 8-column chunk is evaluated.  Per entry
// the same fma chain over direct differences as the plain kernels (LINEAR: the same chain over products), the old kinds'
// values from kern_eval.h's kern_eval_t (one definition: `k * ConstantKernel(1)` reproduces `k` bit for bit), the factors
// multiplied in chain order, then acc = fma(prod, cw, acc) with cw formed as the plain term forms it.
// One launch carries whole chains: as many as fit 64 KiB of LDS (terms x DMAX <= 64, DMAX = the largest factor dimension
// rounded up to a power of two); a pair with more takes several launches, each adding onto the last.  kprod_group decides
// the cut for the matrix and the diagonal alike, so var(f, x) == diag(cov(f, x)) bit for bit.
//
// Gradient: one contraction kernel with grad_block_kernel's tiling and fixed-order reductions (grad.hip), one chain per
// launch: d / d coef of the head, d / d input scale and d / d param of every factor, the products with one factor left out
// formed from prefix and suffix products (never a division: a factor that is exactly 0 -- WHITE off the diagonal, an
// underflowed SE -- gives exact zeros for itself and finite values for the others).
#include "common.h"
#include "kern_eval.h"
#include "kern_grad.h"
#include <algorithm>

namespace sgp {

enum { K_RQ = 6, K_LINEAR = 7, K_WIENER = 10, K_PP0 = 11, K_PP3 = 14, K_COSINE = 16, K_GAMMAEXP = 17, K_MATERN_NU = 20, K_NEURALNET = 24, K_FBM = 25,
       K_EXPONENTIATED = 26 };
constexpr int KP_KIND_MASK = 0xff, KP_TIMES_PREV = 0x100;   // sthenomi.h: SGP_KIND_TIMES_PREV
constexpr int KP_MAXF = 8;                                  // sthenomi_kprod.h: SGP_KPROD_MAX_FACTORS
constexpr int KP_CHUNK = 8;                                 // columns per accumulator chunk

// RationalQuadratic (1 + d2 / (2 alpha))^-alpha = exp(-alpha log1p(d2 / (2 alpha))): exactly 1 at d2 == 0 (log1p(0) = 0,
// exp_nonpos(-0) = 1), exactly 0 -- never NaN -- where d2 overflowed (log1p(inf) = inf, exp_nonpos clamps its argument)
// A finite d2 whose u = d2 / (2 alpha) overflows (alpha < 1/2, points 1e154 apart) takes log(d2) - log(2 alpha) instead: with
// a small alpha the kernel is nowhere near 0 there.
__device__ __forceinline__ double rq_log1p_u(double d2, double alpha, double& u) {
  u = d2 / (2.0 * alpha);
  double l = log1p(u);
  if (u > 1.7e308 && d2 <= 1.7976931348623157e308) l = log(d2) - log(2.0 * alpha);
  return l;
}
__device__ __forceinline__ double rq_eval(double d2, double alpha) {
  double u;
  return exp_nonpos(-alpha * rq_log1p_u(d2, alpha, u));
}

// Cosine cos(pi d), d = sqrt(d2): cospi / sinpi reduce their argument exactly, so the only error that grows with d is the half
// ulp of the square root (pi d |sin pi d| units of 2^-53).  An overflowed d2 gives exactly 1 and exact-zero derivatives: every
// double >= 2^53 is an even integer, so 1 is the limit, while cospi(inf) is NaN.  No 1e150 clamp: the factor never decays.
// dk = d k / d g = -pi d sin(pi d); kx = d k / d (d2) = -pi sin(pi d) / (2 d), at d == 0 its limit -pi^2 / 2 by a branch.
// Both kinds are kept out of line (cospi, sinpi, pow and log are long routines: inlined into the per-kind switches they cost
// the assembly kernels a wave of occupancy and put the contractions' old kinds into scratch); values come back in registers.
constexpr double KP_PI = 3.14159265358979323846, KP_DBL_MAX = 1.7976931348623157e308;
struct KpDerivs {
  double k, dk, kx, dp;
};
__device__ __noinline__ double cosine_eval(double d2) { return d2 > KP_DBL_MAX ? 1.0 : cospi(sqrt(d2)); }
__device__ __forceinline__ KpDerivs cosine_derivs(double d2) {
  KpDerivs r = {1.0, 0.0, 0.0, 0.0};
  if (d2 > KP_DBL_MAX) return r;
  const double d = sqrt(d2), sn = sinpi(d);
  r.k = cospi(d);
  r.dk = -(KP_PI * d) * sn;
  r.kx = d > 0.0 ? -KP_PI * sn / (2.0 * d) : -0.5 * KP_PI * KP_PI;
  return r;
}

// GammaExponential exp(-d^gamma) = exp(-a), a = pow(d2, gamma / 2): a = 0 and k = 1 exactly at d2 == 0, a = inf and k = 0
// exactly -- never NaN -- where d2 overflowed (exp_nonpos clamps its argument).  pow, not exp(h log d2): the latter's error
// grows with a |log d2|.  dk = d k / d g = -gamma a k; kx = d k / d (d2) = -(gamma / 2) a k / d2 (0 at coincident points, the
// subgradient kern_val_dd2 uses for Matern-1/2); dp = d k / d gamma = -k a log(d2) / 2 (0 at d2 == 0, its limit).  Where k is
// an exact 0 every derivative is an exact 0, as for RQ.
__device__ __noinline__ double gexp_eval(double d2, double gamma) { return exp_nonpos(-pow(d2, 0.5 * gamma)); }
__device__ __forceinline__ KpDerivs gexp_derivs(double d2, double gamma) {
  const double a = pow(d2, 0.5 * gamma);
  KpDerivs r = {exp_nonpos(-a), 0.0, 0.0, 0.0};
  if (r.k == 0.0 || !(d2 > 0.0)) return r;
  const double ak = a * r.k;
  r.dk = -gamma * ak;
  r.kx = -(0.5 * gamma) * ak / d2;
  r.dp = -0.5 * (ak * log(d2));   // (the halving last: exact, where ak is subnormal too)
  return r;
}

// General-nu Matern  k = C x^nu K_nu(x),  x = sqrt(2 nu) d,  C = 2^(1-nu) / Gamma(nu)  (param = nu in (0, SGP_MATERN_NU_MAX]).
// nu = mu + n, n = floor(nu + 1/2) >= 1, mu in [-1/2, 1/2); nu < 1/2 takes mu = -nu, n = 0 (K is even in its order: the pair
// (K_mu, K_(mu+1)) is then (K_nu, K_(nu-1)), the value and what the derivative needs, without a cancelling downward step).
// Everything is carried as  Q_j = (x / 2)^mu x^j K_(mu+j)(x)  (times e^x beyond x = 2): K_(mu+j) ~ x^-(mu+j) at small x and
// ~ e^-x at large x, Q_j does neither, so nothing overflows or underflows before the last product.
//   x <= 2   Temme's series for K_mu and K_(mu+1) (N. M. Temme, J. Comput. Phys. 19 (1975) 324), each term times (x / 2)^mu:
//            the powers (2 / x)^(+-mu) of the textbook form become 1 and E = (x / 2)^(2 mu), taken with pow -- as
//            exp(2 mu log(x / 2)) its error would grow with |log x|; sinh(e) / e log(2 / x) becomes (1 - E) / (2 mu), or
//            expm1(g) / g log(2 / x), g = 2 mu log(x / 2), where |g| < 1 (mu -> 0)
//   x > 2    Steed's second continued fraction (the same paper; Thompson & Barnett 1987) for e^x K_mu and the ratio
//            K_(mu+1) / K_mu, with b d - 1 written as -a d d' (no cancellation); at mu = -1/2 it is the closed form
//   then     Q_(j+1) = x^2 Q_(j-1) + 2 (mu + j) Q_j, j = 1 .. n - 1: positive terms, 2 (mu + j) = 2 (nu - (n - j)) exact
//   k = ca Q_n [e^-x],  kx = d k / d (d2) = -nu ca Q_(n-1) [e^-x]  (d / dx x^nu K_nu = -x^nu K_(nu-1), dx / d(d2) = nu / x),
//   dk = d k / d g = 2 d2 kx;   nu < 1/2:  k = ca Q_0 / E,  kx = -nu ca Q_1 / (E x^2).   dp = 0: nu is held fixed.
// e^-x is applied once, through exp_nonpos; beyond x = 600 as e^-600 e^-(x - 600) (x - 600 is exact), since e^-x is subnormal
// from 708 on while its product with x^nu still is a normal number.  What depends on nu alone comes from the host
// (matern_nu_constants below, uploaded with the spec: DevTerm::nuc).  Ends, each a branch:
//   d2 == 0             k = 1, dk = 0, kx = -nu / (2 (nu - 1)) for nu > 1 and 0 for nu <= 1 (it diverges: the subgradient)
//   x >= 1000 (or inf)  k < 2^-1076 for every nu <= 32: k and every derivative exactly 0, as wherever k rounds to 0
// Error model and measured maxima: tests/matern_nu_truth.py, docs/03_kernels.md section 3.2e.
constexpr double MN_E600 = 2.6503965530043108e-261, MN_EPS = 1.1102230246251565e-16;
constexpr int MN_TEMME_MAXIT = 30, MN_CF2_MAXIT = 200;   // (13 and 79 are the most any argument takes)
__device__ __noinline__ KpDerivs matern_nu_derivs(double d2, double nu, const double* __restrict__ c) {
  KpDerivs r = {1.0, 0.0, c[MN_KX0], 0.0};
  if (!(d2 > 0.0)) return r;
  r.k = r.kx = 0.0;
  const double x = c[MN_SQ] * sqrt(d2);
  if (!(x < 1000.0)) return r;
  const double mu = c[MN_MU];
  const int n = (int)c[MN_N];
  double qa, qb, E;   // Q_0, Q_1, (x / 2)^(2 mu)
  if (x <= 2.0) {
    const double xh = 0.5 * x, dl = -log(xh), mu2 = mu * mu;
    E = pow(xh, 2.0 * mu);
    const double g = -(2.0 * mu) * dl;
    double t2;
    if (fabs(g) < 1.0) t2 = (g != 0.0 ? expm1(g) / g : 1.0) * dl;
    else t2 = (1.0 - E) / (2.0 * mu);
    double ff = c[MN_FACT] * (c[MN_GAM1] * (0.5 * (1.0 + E)) + c[MN_GAM2] * t2);
    double p = c[MN_PH], q = c[MN_QH] * E;
    double s0 = ff, s1 = p, cc = 1.0;
    const double dd = xh * xh;
    for (int i = 1; i <= MN_TEMME_MAXIT; ++i) {
      const double di = (double)i;
      ff = (di * ff + p + q) / (di * di - mu2);
      cc = cc * (dd / di);
      p = p / (di - mu);
      q = q / (di + mu);
      const double de0 = cc * ff, de1 = cc * (p - di * ff);
      s0 += de0;
      s1 += de1;
      if (fabs(de0) < fabs(s0) * MN_EPS && fabs(de1) < fabs(s1) * MN_EPS) break;
    }
    qa = s0;
    qb = 2.0 * s1;
  } else {
    const double a1 = c[MN_A1];
    double b = 2.0 * (1.0 + x), d = 1.0 / b, h = d, delh = d, q1 = 0.0, q2 = 1.0, q = a1, cc = a1, a = -a1;
    double s = 1.0 + q * delh;
    if (a1 != 0.0) {
      for (int i = 2; i <= MN_CF2_MAXIT; ++i) {
        a = a - 2.0 * (double)(i - 1);
        cc = -a * cc / (double)i;
        const double qn = (q1 - b * q2) / a;
        q1 = q2;
        q2 = qn;
        q = q + cc * qn;
        b = b + 2.0;
        const double dn = 1.0 / (b + a * d);
        delh = (-a * d * dn) * delh;
        d = dn;
        h += delh;
        const double dels = q * delh;
        s += dels;
        if (fabs(dels) < fabs(s) * MN_EPS) break;
      }
    }
    h = a1 * h;
    const double w = pow(0.5 * x, mu);
    qa = w * (sqrt(1.5707963267948966 / x) / s);
    qb = qa * (mu + x + 0.5 - h);
    E = w * w;
  }
  double tk, tx;
  if (n == 0) {
    tk = c[MN_CA] * (qa / E);
    tx = c[MN_CK] * ((qb / (x * E)) / x);
  } else {
    const double x2 = x * x;
    for (int j = 1; j < n; ++j) {
      const double qn = x2 * qa + (2.0 * (nu - (double)(n - j))) * qb;
      qa = qb;
      qb = qn;
    }
    tk = c[MN_CA] * qb;
    tx = c[MN_CK] * qa;
  }
  if (x > 2.0) {
    double xe = x;
    if (x > 600.0) {
      tk *= MN_E600;
      tx *= MN_E600;
      xe = x - 600.0;
    }
    const double ex = exp_nonpos(-xe);
    tk *= ex;
    tx *= ex;
  }
  r.k = fmin(tk, 1.0);
  if (r.k == 0.0) return r;
  r.kx = -tx;
  r.dk = 2.0 * d2 * r.kx;
  return r;
}
__device__ __forceinline__ double matern_nu_eval(double d2, double nu, const double* c) { return matern_nu_derivs(d2, nu, c).k; }

// 1 / Gamma(1 + z) = sum_k a_k z^k (Abramowitz & Stegun 6.1.34): Gamma_2 = (1 / Gamma(1 - mu) + 1 / Gamma(1 + mu)) / 2 is its
// even part at mu, Gamma_1 = (1 / Gamma(1 - mu) - 1 / Gamma(1 + mu)) / (2 mu) minus its odd part over mu: no cancellation at
// small mu.  |mu| <= 1/2: 28 coefficients leave 1e-27.  Evaluated in long double, rounded once.
void matern_nu_constants(double nu, double* out) {
  static const long double a[28] = {
      1.0L, 0.57721566490153286061L, -0.65587807152025388108L, -0.042002635034095235529L, 0.1665386113822914895L,
      -0.042197734555544336748L, -0.0096219715278769735621L, 0.0072189432466630995424L, -0.0011651675918590651121L,
      -0.00021524167411495097282L, 0.00012805028238811618615L, -0.000020134854780788238656L, -1.2504934821426706573e-6L,
      1.1330272319816958824e-6L, -2.0563384169776071035e-7L, 6.1160951044814158179e-9L, 5.0020076444692229301e-9L,
      -1.1812745704870201446e-9L, 1.0434267116911005105e-10L, 7.782263439905071254e-12L, -3.6968056186422057082e-12L,
      5.100370287454475979e-13L, -2.0583260535665067832e-14L, -5.3481225394230179824e-15L, 1.2267786282382607902e-15L,
      -1.1812593016974587695e-16L, 1.1866922547516003326e-18L, 1.4123806553180317816e-18L};
  const int n = nu < 0.5 ? 0 : (int)floor(nu + 0.5);
  const long double mu = n == 0 ? -(long double)nu : (long double)nu - n, m2 = mu * mu;
  long double g1 = 0.0L, g2 = 0.0L;
  for (int j = 13; j >= 0; --j) {
    g2 = g2 * m2 + a[2 * j];
    g1 = g1 * m2 - a[2 * j + 1];
  }
  const long double pi = 3.14159265358979323846264338327950288L;
  const long double ca = ldexpl(1.0L, 1 - n) / tgammal((long double)nu);
  out[MN_N] = (double)n;
  out[MN_MU] = (double)mu;
  out[MN_FACT] = mu == 0.0L ? 1.0 : (double)(pi * mu / sinl(pi * mu));
  out[MN_GAM1] = (double)g1;
  out[MN_GAM2] = (double)g2;
  out[MN_PH] = (double)(0.5L / (g2 - mu * g1));
  out[MN_QH] = (double)(0.5L / (g2 + mu * g1));
  out[MN_A1] = (double)((0.5L - mu) * (0.5L + mu));
  out[MN_CA] = (double)ca;
  out[MN_CK] = (double)((long double)nu * ca);
  out[MN_SQ] = (double)sqrtl(2.0L * (long double)nu);
  out[MN_KX0] = nu > 1.0 ? (double)(-(long double)nu / (2.0L * ((long double)nu - 1.0L))) : 0.0;
}

// PiecewisePolynomial (codes 11 .. 14, q = code - 11; param = j, an integer in [1, 64]: the host passes floor(dim / 2) + q + 1):
//     k = max(1 - r, 0)^(j + q) p_q(r),  r = sqrt(d2)      (Rasmussen & Williams eq. 4.21)
//   p_0 = 1,  p_1 = 1 + (j + 1) r,  p_2 = 1 + (j + 2) r + (j + 1)(j + 3) / 3 r^2,
//   p_3 = 1 + (j + 3) r + (6 j^2 + 36 j + 45) / 15 r^2 + (j + 1)(j + 3)(j + 5) / 15 r^3
// The power is taken by square-and-multiply on t = 1 - r (exact for r >= 1/2), never pow.  k' = -r t^(j+q-1) pt_q(r) for q >= 1:
//   pt_1 = (j + 1)(j + 2),  pt_2 = (j + 3)(j + 4) / 3 (1 + (j + 1) r),
//   pt_3 = A0 + A1 r + A2 r^2,  n = j + 3, c2 and c3 the coefficients of r^2 and r^3 in p_3:
//          A0 = n^2 + n - 2 c2,  A1 = (n + 2) c2 - 3 c3,  A2 = (n + 3) c3   (integer numerators over 15: exact before one division)
// so kx = d k / d (d2) = k' / (2 r) = -t^(j+q-1) pt_q / 2 is a power times a polynomial, never a quotient by r; q = 0 has
// kx = -j t^(j-1) / (2 r), and 0 at r == 0 (the subgradient Matern-1/2 has there).  dk = d k / d g = 2 d2 kx, dp = 0.
// Ends: exactly 1 at d2 == 0 (t = 1, p = 1); exactly 0 with every derivative exactly 0 for r >= 1, an overflowed or NaN d2.
__device__ __forceinline__ double pp_pow(double t, int e) {
  double pw = 1.0;
  for (; e > 0; e >>= 1) {
    if (e & 1) pw *= t;
    t *= t;
  }
  return pw;
}
__device__ __noinline__ KpDerivs pp_derivs(int q, double d2, double j) {
#pragma clang fp contract(off)
  KpDerivs o = {0.0, 0.0, 0.0, 0.0};
  const double r = sqrt(d2);
  if (!(r < 1.0)) return o;
  const double t = 1.0 - r;
  const double pw = pp_pow(t, (int)j + q - 1);   // t^(j+q-1); j + q - 1 >= 0
  double p = 1.0, pt = 0.0;
  if (q == 1) {
    p = 1.0 + (j + 1.0) * r;
    pt = (j + 1.0) * (j + 2.0);
  } else if (q == 2) {
    p = 1.0 + r * ((j + 2.0) + ((j + 1.0) * (j + 3.0) / 3.0) * r);
    pt = ((j + 3.0) * (j + 4.0) / 3.0) * (1.0 + (j + 1.0) * r);
  } else if (q == 3) {
    const double n = j + 3.0, n2 = 6.0 * j * j + 36.0 * j + 45.0, n3 = (j + 1.0) * (j + 3.0) * (j + 5.0);
    p = 1.0 + r * (n + r * (n2 / 15.0 + (n3 / 15.0) * r));
    const double a0 = (15.0 * (n * n + n) - 2.0 * n2) / 15.0, a1 = ((n + 2.0) * n2 - 3.0 * n3) / 15.0,
                 a2 = (n + 3.0) * n3 / 15.0;
    pt = a0 + r * (a1 + a2 * r);
  }
  o.k = (pw * t) * p;
  if (q == 0) o.kx = r > 0.0 ? -(j * pw) / (2.0 * r) : 0.0;
  else o.kx = -0.5 * (pw * pt);
  o.dk = 2.0 * d2 * o.kx;
  return o;
}
__device__ __noinline__ double pp_eval(int q, double d2, double j) { return pp_derivs(q, d2, j).k; }

// one call site per factor in the contractions: the two kinds behind one out-of-line routine
__device__ __noinline__ KpDerivs newkind_derivs(int kind, double d2, double param) {
  return kind == K_COSINE ? cosine_derivs(d2) : gexp_derivs(d2, param);
}
// MN: the launch mode (kprod_mode below: 0, 1 with a MATERN_NU factor, 2 with a NEURALNET / FBM / EXPONENTIATED factor); this
// paragraph is about modes 0 and 1.  The Bessel routine's registers count against every kernel that
// can call it (the assembly: 3 waves per SIMD become 2; the contractions go to scratch), so every kernel below is instantiated
// with and without it, and chains without the kind run what they ran before it existed (docs/03_kernels.md section 3.2e).
// With MN the three kinds sit behind one call site (nuc: MATERN_NU only)
__device__ __noinline__ KpDerivs newkind_derivs_mn(int kind, double d2, double param, const double* nuc) {
  if (kind == K_MATERN_NU) return matern_nu_derivs(d2, param, nuc);
  return kind == K_COSINE ? cosine_derivs(d2) : gexp_derivs(d2, param);
}

template <int DMAX>
__device__ __forceinline__ double kp_d2(const double (&xi)[DMAX], const double* sp) {
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = xi[d] - sp[d];
    d2 = fma(df, df, d2);
  }
  return d2;
}
template <int DMAX>
__device__ __forceinline__ double kp_dot(const double (&xi)[DMAX], const double* sp) {
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) s = fma(xi[d], sp[d], s);
  return s;
}

// ---- NEURALNET, FBM, EXPONENTIATED: kinds of the scalars s = x'y, a = x'x, b = y'y (and e, below) ----------------------------
// s, a and b share kp_dot's fma order, so s == a == b bit for bit where x == y; every sum is symmetric in (x, y) bit for bit.
//   e = d2 (FBM): |x - y|^2 from direct differences, kp_d2's chain -- never a + b - 2 s
//   e = L  (NEURALNET): Lagrange's sum  sum_{i<j} (x_i y_j - x_j y_i)^2 = a b - s^2, i outer, j inner.  A sum of squares: no
//       cancellation against a b (nearly parallel points at large norms lose everything in a b - s^2).  The two products are
//       rounded separately (no contraction), so exchanging x and y negates every term exactly; L = 0 exactly where x == y
//       and at D = 1.  R^2 = (1 + a)(1 + b) - s^2 = ((a + b) + 1) + L.
//   NEURALNET      k = asin(s / sqrt((1 + a)(1 + b))) = atan2(s, R): |k| < pi / 2 always, no argument near 1 to lose
//   FBM            k = ((a^h + b^h) - d2^h) / 2.  pow(0, h) = 0: a power term whose base is exactly 0 contributes exactly 0 to
//                  the value and to every derivative (0^h log 0 := 0 and, for h < 1, 0^(h - 1) := 0: the subgradient rule of
//                  GAMMAEXP and Matern-1/2 at coincident points).  So k = a^h exactly where x == y, 0 exactly against the origin
//   EXPONENTIATED  k = exp(s); beyond s = 709.78 it is +inf (the factorisation then reports "not positive definite")
// Derivatives (KpDotDerivs): dk = d k / d g (both inputs scaled by g, at g = 1), dp = d k / d param, and the point derivatives
//     d k / d x = c1 x + c2 (x - y) + c3 y,      d k / d y = c1y y + c2 (y - x) + c3 x
//   NEURALNET      dk = s (1 / (1 + a) + 1 / (1 + b)) / R,  c1 = -s / ((1 + a) R),  c1y = -s / ((1 + b) R),  c3 = 1 / R
//   FBM            dk = 2 h k,  dp = ((a^h log a + b^h log b) - d2^h log d2) / 2,  c1 = h a^h / a,  c1y = h b^h / b,
//                  c2 = -h d2^h / d2  (kept on x - y: folded into the coefficients of x and y it would cancel at close points)
//   EXPONENTIATED  dk = 2 s k,  c3 = k
// Range: finite for a, b <= 1e300 (NEURALNET, FBM) and s <= 709 (EXPONENTIATED); beyond it inf or NaN, never a fault.  NEURALNET
// is accurate only while (1 + a)(1 + b) is representable: beyond it L overflows, R = inf and k and its derivatives are 0.
// Out of line, one body each: the matrix and the diagonal get the same bits from the same scalars.
struct KpDot {
  double s, a, b, e;
};
struct KpDotDerivs {
  double k, dk, dp, c1, c1y, c2, c3;
};
__device__ __forceinline__ double kp_cross(double xi, double yj, double xj, double yi) {
#pragma clang fp contract(off)
  const double p = xi * yj, q = xj * yi;
  return p - q;
}
// dim <= DMAX coordinates are read (the assembly pads its points with zeros up to DMAX: they add exact zeros)
// W: the caller is a mode-3 instantiation (WIENER, PIECEWISE: e = d2 as FBM's)
template <int DMAX, bool W = false>
__device__ __forceinline__ KpDot kp_dot_scalars(int kind, const double* x, const double* y) {
  KpDot r = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    r.s = fma(x[d], y[d], r.s);
    r.a = fma(x[d], x[d], r.a);
    r.b = fma(y[d], y[d], r.b);
  }
  if (kind == K_FBM || (W && kind < K_COSINE)) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      const double df = x[d] - y[d];
      r.e = fma(df, df, r.e);
    }
  } else if (kind == K_NEURALNET) {
#pragma unroll
    for (int i = 0; i < DMAX; ++i)
#pragma unroll
      for (int j = i + 1; j < DMAX; ++j) {
        const double c = kp_cross(x[i], y[j], x[j], y[i]);
        r.e = fma(c, c, r.e);
      }
  }
  return r;
}
template <bool W = false>
__device__ __forceinline__ KpDot kp_dot_scalars_n(int kind, const double* x, const double* y, int dim) {
  KpDot r = {0.0, 0.0, 0.0, 0.0};
  for (int d = 0; d < dim; ++d) {
    r.s = fma(x[d], y[d], r.s);
    r.a = fma(x[d], x[d], r.a);
    r.b = fma(y[d], y[d], r.b);
  }
  if (kind == K_FBM || (W && kind < K_COSINE)) {
    for (int d = 0; d < dim; ++d) {
      const double df = x[d] - y[d];
      r.e = fma(df, df, r.e);
    }
  } else if (kind == K_NEURALNET) {
    for (int i = 0; i < dim; ++i)
      for (int j = i + 1; j < dim; ++j) {
        const double c = kp_cross(x[i], y[j], x[j], y[i]);
        r.e = fma(c, c, r.e);
      }
  }
  return r;
}
__device__ __noinline__ double dotkind_eval(int kind, double h, double s, double a, double b, double e) {
  if (kind == K_EXPONENTIATED) return exp(s);
  if (kind == K_FBM) return 0.5 * ((pow(a, h) + pow(b, h)) - pow(e, h));
  return atan2(s, sqrt(((a + b) + 1.0) + e));
}
__device__ __noinline__ KpDotDerivs dotkind_derivs(int kind, double h, double s, double a, double b, double e) {
  KpDotDerivs r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (kind == K_EXPONENTIATED) {
    r.k = exp(s);
    r.dk = 2.0 * s * r.k;
    r.c3 = r.k;
    return r;
  }
  if (kind == K_FBM) {
    const double pa = pow(a, h), pb = pow(b, h), pd = pow(e, h);
    r.k = 0.5 * ((pa + pb) - pd);
    r.dk = 2.0 * h * r.k;
    const double la = a > 0.0 ? pa * log(a) : 0.0, lb = b > 0.0 ? pb * log(b) : 0.0, ld = e > 0.0 ? pd * log(e) : 0.0;
    r.dp = 0.5 * ((la + lb) - ld);
    r.c1 = a > 0.0 ? h * pa / a : 0.0;
    r.c1y = b > 0.0 ? h * pb / b : 0.0;
    r.c2 = e > 0.0 ? -(h * pd / e) : 0.0;
    return r;
  }
  const double R = sqrt(((a + b) + 1.0) + e), ia = 1.0 / (1.0 + a), ib = 1.0 / (1.0 + b);
  r.k = atan2(s, R);
  r.dk = s * (ia + ib) / R;
  r.c1 = -(s * ia) / R;
  r.c1y = -(s * ib) / R;
  r.c3 = 1.0 / R;
  return r;
}
// WIENER (code 10, param = i in {0, 1, 2, 3}): the i-times integrated Wiener process on X = |x| = sqrt(a), Y = |y| = sqrt(b),
// d = |x - y| = sqrt(e) (e from direct differences, as FBM's), m = min(X, Y), M = max(X, Y):
//     i = 0  m        i = 1  m^3 / 3 + m^2 d / 2        i = 2  m^5 / 20 + m^3 d (X + Y - m / 2) / 12
//     i = 3  m^7 / 252 + m^4 d (5 M^2 + 2 X Y + 3 m^2) / 720
// Every term is positive, the square roots are correctly rounded, min / max, X + Y and X Y are symmetric bit for bit: so is k.
// m = 0 against the origin gives exactly 0; d = 0 exactly on the diagonal leaves the single first term.
// Derivatives: k is a function of (m, M, S = X + Y, P = X Y, d); with wx = d m / d X = 1, 0 or -- at a tie X == Y, which
// includes the diagonal -- 1/2 (the rule FBM follows at h = 1/2), wy = 1 - wx, d M / d X = wy:
//     kX = wx km + wy kM + kS + kP Y,   kY = wy km + wx kM + kS + kP X
//     d k / d x = c1 x + c2 (x - y),  c1 = kX / X (0 at X == 0),  c2 = kd / d (0 at d == 0),  c3 = 0;  c1y = kY / Y
//     dk = d k / d g = (2 i + 1) k (homogeneous),  dp = 0 (i is discrete)
struct KpWiener {
  double k, km, kM, kS, kP, kd;
};
__device__ __forceinline__ KpWiener wiener_parts(int i, double X, double Y, double d) {
#pragma clang fp contract(off)
  KpWiener o = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double m = fmin(X, Y), M = fmax(X, Y), m2 = m * m;
  if (i == 0) {
    o.k = m;
    o.km = 1.0;
  } else if (i == 1) {
    o.k = m2 * m / 3.0 + m2 * d * 0.5;
    o.km = m2 + m * d;
    o.kd = 0.5 * m2;
  } else if (i == 2) {
    const double m3 = m2 * m, S = X + Y, T = S - 0.5 * m;
    o.k = m3 * m2 / 20.0 + m3 * d * T / 12.0;
    o.km = m2 * m2 / 4.0 + m2 * d * (3.0 * S - 2.0 * m) / 12.0;
    o.kS = m3 * d / 12.0;
    o.kd = m3 * T / 12.0;
  } else {
    const double m3 = m2 * m, m4 = m2 * m2, Q = (5.0 * (M * M) + 2.0 * (X * Y)) + 3.0 * m2;
    o.k = m4 * m3 / 252.0 + m4 * d * Q / 720.0;
    o.km = (m4 * m2 / 36.0 + m3 * d * Q / 180.0) + m4 * m * d / 120.0;
    o.kM = m4 * d * M / 72.0;
    o.kP = m4 * d / 360.0;
    o.kd = m4 * Q / 720.0;
  }
  return o;
}
__device__ __noinline__ double wiener_eval(double p, double a, double b, double e) {
  return wiener_parts((int)p, sqrt(a), sqrt(b), sqrt(e)).k;
}
__device__ __noinline__ KpDotDerivs wiener_derivs(double p, double a, double b, double e) {
#pragma clang fp contract(off)
  KpDotDerivs r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double X = sqrt(a), Y = sqrt(b), d = sqrt(e);
  const KpWiener w = wiener_parts((int)p, X, Y, d);
  const double wx = X < Y ? 1.0 : (X > Y ? 0.0 : 0.5), wy = 1.0 - wx;
  const double kX = ((wx * w.km + wy * w.kM) + w.kS) + w.kP * Y, kY = ((wy * w.km + wx * w.kM) + w.kS) + w.kP * X;
  r.k = w.k;
  r.dk = (2.0 * p + 1.0) * w.k;
  r.c1 = X > 0.0 ? kX / X : 0.0;
  r.c1y = Y > 0.0 ? kY / Y : 0.0;
  r.c2 = d > 0.0 ? w.kd / d : 0.0;
  return r;
}
// mode 3 (below): WIENER, PIECEWISE and the three kinds above behind one call site each.  A PIECEWISE kind goes the same way
// with e = d2, c2 = 2 kx and c1 = c3 = 0
__device__ __noinline__ double dotkind_eval_w(int kind, double h, double s, double a, double b, double e) {
  if (kind >= K_NEURALNET) return dotkind_eval(kind, h, s, a, b, e);
  if (kind == K_WIENER) return wiener_eval(h, a, b, e);
  return pp_eval(kind - K_PP0, e, h);
}
__device__ __noinline__ KpDotDerivs dotkind_derivs_w(int kind, double h, double s, double a, double b, double e) {
  if (kind >= K_NEURALNET) return dotkind_derivs(kind, h, s, a, b, e);
  if (kind == K_WIENER) return wiener_derivs(h, a, b, e);
  const KpDerivs q = pp_derivs(kind - K_PP0, e, h);
  KpDotDerivs r = {q.k, q.dk, 0.0, 0.0, 0.0, 2.0 * q.kx, 0.0};
  return r;
}
// The launch mode of every kernel below (the template argument MN): 0 the chains hold none of MATERN_NU and the kinds
// above, 1 they hold MATERN_NU and none of those, 2 they hold one of NEURALNET / FBM / EXPONENTIATED (and possibly MATERN_NU)
// and none of WIENER / PIECEWISE, 3 they hold a WIENER or PIECEWISE factor (and possibly any other kind).  Modes 0 to 2
// are what ran before WIENER and PIECEWISE existed: the compiler reports the registers, scratch and LDS they had
// (tools/kprod_resources.py; docs/03_kernels.md section 3.2e)
__host__ __device__ __forceinline__ bool kp_is_wpp(int kind) { return kind >= K_WIENER && kind <= K_PP3; }
int kprod_mode(const DevTerm* h_terms, int n) {
  int mode = 0;
  for (int t = 0; t < n; ++t) {
    const int kind = h_terms[t].kind & KP_KIND_MASK;
    if (kp_is_wpp(kind)) return 3;
    if (kind >= K_NEURALNET) mode = 2;
    else if (kind == K_MATERN_NU && mode < 2) mode = 1;
  }
  return mode;
}
// Whether `kind` takes the route of the scalars (s, a, b, e) in launch mode MN, and that route's two calls.  Written so that a
// mode-2 instantiation is, once the constant conditions are folded, the very code it was before mode 3 existed
#define KP_DOT_ROUTE(MN, kind) ((MN) == 3 ? ((kind) >= K_NEURALNET || kp_is_wpp(kind)) : ((MN) == 2 && (kind) >= K_NEURALNET))
#define KP_DOT_EVAL(MN, kind, h, r) \
  ((MN) == 3 ? dotkind_eval_w(kind, h, (r).s, (r).a, (r).b, (r).e) : dotkind_eval(kind, h, (r).s, (r).a, (r).b, (r).e))
#define KP_DOT_DERIVS(MN, kind, h, r) \
  ((MN) == 3 ? dotkind_derivs_w(kind, h, (r).s, (r).a, (r).b, (r).e) : dotkind_derivs(kind, h, (r).s, (r).a, (r).b, (r).e))

// one factor of one of the three kinds over a chunk of columns
template <int DMAX, int MN>
__device__ __forceinline__ void factor_chunk_dot(int kind, double (&prod)[KP_CHUNK], const double (&xi)[DMAX], const double* sp,
                                                 double param, bool head) {
#pragma unroll
  for (int q = 0; q < KP_CHUNK; ++q) {
    const KpDot r = kp_dot_scalars<DMAX, MN == 3>(kind, xi, sp + q * DMAX);
    const double k = KP_DOT_EVAL(MN, kind, param, r);
    prod[q] = head ? k : prod[q] * k;
  }
}

// one factor over a chunk of columns: prod = k (the head) or prod * k (a continuation).  KIND is a template argument so that
// each case is straight-line code over the KP_CHUNK independent entries, as in the plain assembly
template <int DMAX, int KIND>
__device__ __forceinline__ void factor_chunk(double (&prod)[KP_CHUNK], const double (&xi)[DMAX], const double* sp,
                                             double param, bool head, const double* nuc) {
#pragma unroll
  for (int q = 0; q < KP_CHUNK; ++q) {
    double k;
    if (KIND == K_LINEAR) k = kp_dot<DMAX>(xi, sp + q * DMAX) + param;
    else if (KIND == K_RQ) k = rq_eval(kp_d2<DMAX>(xi, sp + q * DMAX), param);
    else if (KIND == K_COSINE) k = cosine_eval(kp_d2<DMAX>(xi, sp + q * DMAX));
    else if (KIND == K_GAMMAEXP) k = gexp_eval(kp_d2<DMAX>(xi, sp + q * DMAX), param);
    else if (KIND == K_MATERN_NU) k = matern_nu_eval(kp_d2<DMAX>(xi, sp + q * DMAX), param, nuc);
    else k = kern_eval_t<KIND>(kp_d2<DMAX>(xi, sp + q * DMAX), param);
    prod[q] = head ? k : prod[q] * k;
  }
}

template <int DMAX, int MN>
__device__ __forceinline__ void factor_chunk_any(int kind, double (&prod)[KP_CHUNK], const double (&xi)[DMAX],
                                                 const double* sp, double param, bool head, const double* nuc) {
  if (KP_DOT_ROUTE(MN, kind)) {
    factor_chunk_dot<DMAX, MN>(kind, prod, xi, sp, param, head);
    return;
  }
  if (MN && kind == K_MATERN_NU) {
    factor_chunk<DMAX, K_MATERN_NU>(prod, xi, sp, param, head, nuc);
    return;
  }
  switch (kind) {
    case K_SE: factor_chunk<DMAX, K_SE>(prod, xi, sp, param, head, nuc); break;
    case K_M12: factor_chunk<DMAX, K_M12>(prod, xi, sp, param, head, nuc); break;
    case K_M32: factor_chunk<DMAX, K_M32>(prod, xi, sp, param, head, nuc); break;
    case K_M52: factor_chunk<DMAX, K_M52>(prod, xi, sp, param, head, nuc); break;
    case K_WHITE: factor_chunk<DMAX, K_WHITE>(prod, xi, sp, param, head, nuc); break;
    case K_RQ: factor_chunk<DMAX, K_RQ>(prod, xi, sp, param, head, nuc); break;
    case K_LINEAR: factor_chunk<DMAX, K_LINEAR>(prod, xi, sp, param, head, nuc); break;
    case K_COSINE: factor_chunk<DMAX, K_COSINE>(prod, xi, sp, param, head, nuc); break;
    case K_GAMMAEXP: factor_chunk<DMAX, K_GAMMAEXP>(prod, xi, sp, param, head, nuc); break;
    default: factor_chunk<DMAX, K_CONST>(prod, xi, sp, param, head, nuc); break;
  }
}

// terms [0, nterms): whole chains (a term with KP_TIMES_PREV continues the chain of the nearest term before it without)
template <int DMAX, int MN>
__global__ __launch_bounds__(256) void assemble_kprod_kernel(
    double* K, long ld, long r0, long nr, long c0, long nc, const DevTerm* terms, int nterms, int lower_only,
    int accumulate, int noise_kind, double sigma2, const double* noise_diag, long tile_r_first, long tile_c_first) {
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  if (lower_only && gtr < gtc) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];  // [nterms][128][DMAX] column points
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;

  long cbeg = gtc * TILE, cend = cbeg + TILE;
  if (cbeg < c0) cbeg = c0;
  if (cend > c0 + nc) cend = c0 + nc;
  long rbeg = gtr * TILE, rend = rbeg + TILE;
  if (rbeg < r0) rbeg = r0;
  if (rend > r0 + nr) rend = r0 + nr;
  if (cbeg >= cend || rbeg >= rend) return;   // uniform over the workgroup

  for (int tm = 0; tm < nterms; ++tm) {
    const DevTerm T = terms[tm];
    const int D = T.dim;
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long gc = gtc * TILE + p;
      double v = 0.0;
      if (d < D && gc >= cbeg && gc < cend) v = T.xc[(gc - c0) * T.ldc + d];
      smem[(tm * TILE + p) * DMAX + d] = v;
    }
  }
  __syncthreads();

  const long grow = gtr * TILE + trow;
  if (grow < rbeg || grow >= rend) return;  // no further barriers below
  const long lrow = grow - r0;
  const bool diag_noise = noise_kind >= 0;
  double nval = 0.0;
  if (diag_noise) nval = (noise_kind == 0) ? sigma2 : noise_diag[grow];

  for (int jc = 0; jc < 64; jc += KP_CHUNK) {
    const int pbase = th * 64 + jc;  // point index within the tile
    if (gtc * TILE + pbase >= cend) break;
    double acc[KP_CHUNK];
#pragma unroll
    for (int q = 0; q < KP_CHUNK; ++q) acc[q] = 0.0;
    int tm = 0;
    while (tm < nterms) {
      const DevTerm H = terms[tm];   // the head of a chain: its coefficient and scales
      const double rsv = H.coef * (H.rs ? H.rs[lrow] : 1.0);
      double cw[KP_CHUNK], prod[KP_CHUNK];
#pragma unroll
      for (int q = 0; q < KP_CHUNK; ++q) {
        const long gc = gtc * TILE + pbase + q;
        cw[q] = rsv;
        if (H.cs) cw[q] = (gc >= cbeg && gc < cend) ? rsv * H.cs[gc - c0] : 0.0;
        prod[q] = 0.0;
      }
      int f = tm;
      for (;;) {
        const DevTerm T = terms[f];
        double xi[DMAX];
        {
          const double* xr = T.xr + lrow * T.ldr;
#pragma unroll
          for (int d = 0; d < DMAX; ++d) xi[d] = (d < T.dim) ? xr[d] : 0.0;
        }
        factor_chunk_any<DMAX, MN>(T.kind & KP_KIND_MASK, prod, xi, &smem[(f * TILE + pbase) * DMAX], T.param, f == tm, T.nuc);
        ++f;
        if (f >= nterms || !(terms[f].kind & KP_TIMES_PREV)) break;
      }
#pragma unroll
      for (int q = 0; q < KP_CHUNK; ++q) acc[q] = fma(prod[q], cw[q], acc[q]);
      tm = f;
    }
#pragma unroll
    for (int q = 0; q < KP_CHUNK; ++q) {
      const long gc = gtc * TILE + pbase + q;
      if (gc >= cbeg && gc < cend) {
        double v = acc[q];
        if (diag_noise && gc == grow) v += nval;
        double* p = K + grow + gc * ld;
        if (accumulate) v += *p;
        *p = v;
      }
    }
  }
}

static int pow2ceil_kp(int d) {
  int p = 1;
  while (p < d) p <<= 1;
  return p;
}

// The terms [t, t + return value) of one launch: whole chains, as many as keep terms x DMAX <= 64 (64 KiB of column points);
// *dmax_out = that DMAX.  The first chain always fits: dspec_create refuses a chain beyond the limits.
int kprod_group(const DevTerm* h_terms, int t, int t1, int* dmax_out) {
  int cnt = 0, dmax = 1;
  while (t + cnt < t1) {
    int e = t + cnt + 1, dm = std::max(dmax, pow2ceil_kp(h_terms[t + cnt].dim));
    while (e < t1 && (h_terms[e].kind & KP_TIMES_PREV)) dm = std::max(dm, pow2ceil_kp(h_terms[e].dim)), ++e;
    if (cnt > 0 && (e - t) * dm > 64) break;
    cnt = e - t;
    dmax = dm;
  }
  *dmax_out = dmax;
  return cnt;
}

int launch_assemble_kprod(double* K, long ld, long r0, long nr, long c0, long nc, const DevTerm* d_terms, int nterms,
                          int dmax, int mn, int lower_only, int accumulate, int noise_kind, double sigma2,
                          const double* d_noise_diag, long tile_r_first, long tile_c_first, long tile_r_cnt,
                          long tile_c_cnt, hipStream_t s) {
  if (tile_r_cnt <= 0 || tile_c_cnt <= 0 || nterms <= 0) return 0;
  if (dmax > 16 || nterms * dmax > 64) {
    set_error("assemble: a product launch beyond terms x dimension <= 64");
    return -1;
  }
  const dim3 grid((unsigned)tile_r_cnt, (unsigned)tile_c_cnt), block(256);
#define SGP_KP(DM)                                                                                                     \
  do {                                                                                                                 \
    const size_t lds = (size_t)nterms * TILE * DM * sizeof(double);                                                    \
    if (mn == 3)                                                                                                       \
      hipLaunchKernelGGL((assemble_kprod_kernel<DM, 3>), grid, block, lds, s, K, ld, r0, nr, c0, nc, d_terms, nterms,  \
                         lower_only, accumulate, noise_kind, sigma2, d_noise_diag, tile_r_first, tile_c_first);        \
    else if (mn == 2)                                                                                                  \
      hipLaunchKernelGGL((assemble_kprod_kernel<DM, 2>), grid, block, lds, s, K, ld, r0, nr, c0, nc, d_terms, nterms,  \
                         lower_only, accumulate, noise_kind, sigma2, d_noise_diag, tile_r_first, tile_c_first);        \
    else if (mn)                                                                                                       \
      hipLaunchKernelGGL((assemble_kprod_kernel<DM, 1>), grid, block, lds, s, K, ld, r0, nr, c0, nc, d_terms, nterms,  \
                         lower_only, accumulate, noise_kind, sigma2, d_noise_diag, tile_r_first, tile_c_first);        \
    else                                                                                                               \
      hipLaunchKernelGGL((assemble_kprod_kernel<DM, 0>), grid, block, lds, s, K, ld, r0, nr, c0, nc, d_terms,          \
                         nterms, lower_only, accumulate, noise_kind, sigma2, d_noise_diag, tile_r_first, tile_c_first); \
  } while (0)
  if (dmax <= 1) SGP_KP(1);
  else if (dmax <= 2) SGP_KP(2);
  else if (dmax <= 4) SGP_KP(4);
  else if (dmax <= 8) SGP_KP(8);
  else SGP_KP(16);
#undef SGP_KP
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---- the diagonal: out[i] (+)= the sum of the chains of one launch group, in the assembly's operation order ------------
template <int MN>
__device__ __forceinline__ double kp_factor_diag(const DevTerm& T, long i) {
  const int kind = T.kind & KP_KIND_MASK;
  const double* a = T.xr + i * T.ldr;
  const double* b = T.xc + i * T.ldc;
  if (KP_DOT_ROUTE(MN, kind)) {
    const KpDot r = kp_dot_scalars_n<MN == 3>(kind, a, b, T.dim);
    return KP_DOT_EVAL(MN, kind, T.param, r);
  }
  if (kind == K_LINEAR) {
    double s = 0.0;
    for (int d = 0; d < T.dim; ++d) s = fma(a[d], b[d], s);
    return s + T.param;
  }
  double d2 = 0.0;
  for (int d = 0; d < T.dim; ++d) {
    const double df = a[d] - b[d];
    d2 = fma(df, df, d2);
  }
  if (kind == K_RQ) return rq_eval(d2, T.param);
  if (kind == K_COSINE) return cosine_eval(d2);
  if (kind == K_GAMMAEXP) return gexp_eval(d2, T.param);
  if (MN && kind == K_MATERN_NU) return matern_nu_eval(d2, T.param, T.nuc);
  return kern_eval(kind, d2, T.param);
}

template <int MN>
__global__ void diag_kprod_kernel(double* out, long n, const DevTerm* terms, int nterms, int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  int tm = 0;
  while (tm < nterms) {
    const DevTerm H = terms[tm];
    double cw = H.coef * (H.rs ? H.rs[i] : 1.0);
    if (H.cs) cw = cw * H.cs[i];
    double prod = kp_factor_diag<MN>(H, i);
    int f = tm + 1;
    while (f < nterms && (terms[f].kind & KP_TIMES_PREV)) {
      const DevTerm T = terms[f];
      prod = prod * kp_factor_diag<MN>(T, i);
      ++f;
    }
    acc = fma(prod, cw, acc);
    tm = f;
  }
  out[i] = accumulate ? acc + out[i] : acc;
}

int launch_diag_kprod(double* out, long n, const DevTerm* d_terms, int nterms, int mn, int accumulate, hipStream_t s) {
  if (n <= 0 || nterms <= 0) return 0;
  if (mn == 3)
    hipLaunchKernelGGL(diag_kprod_kernel<3>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms,
                       accumulate);
  else if (mn == 2)
    hipLaunchKernelGGL(diag_kprod_kernel<2>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms,
                       accumulate);
  else if (mn)
    hipLaunchKernelGGL(diag_kprod_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms,
                       accumulate);
  else
    hipLaunchKernelGGL(diag_kprod_kernel<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, d_terms, nterms,
                       accumulate);
  SGP_HIP(hipGetLastError());
  return 0;
}

// ---- gradient contraction of ONE chain --------------------------------------------------------------------------------
// k, d k / d g (both inputs scaled by g, at g = 1) and d k / d param of one factor
template <int DMAX, int MN>
__device__ __forceinline__ void kp_factor_grad(int kind, double param, const double* xr, const double* sp, double& k,
                                               double& dk, double& dp, const DevTerm* term) {
  if (KP_DOT_ROUTE(MN, kind)) {
    const KpDot q = kp_dot_scalars<DMAX, MN == 3>(kind, xr, sp);
    const KpDotDerivs r = KP_DOT_DERIVS(MN, kind, param, q);
    k = r.k;
    dk = r.dk;
    dp = r.dp;
    return;
  }
  if (kind == K_LINEAR) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) s = fma(xr[d], sp[d], s);
    k = s + param;
    dk = 2.0 * s;
    dp = 1.0;
    return;
  }
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = xr[d] - sp[d];
    d2 = fma(df, df, d2);
  }
  if (kind == K_RQ) {
    // no clamp of d2 here: with a small alpha the kernel is far from 0 at d2 = 1e150.  An overflowed d2 gives u = l = inf,
    // k = 0 and, with r = u / (1 + u) taken as its limit 1, exact zeros for both derivatives
    double u;
    const double l = rq_log1p_u(d2, param, u);
    k = exp(-param * l);
    const double r = u < 1e300 ? u / (1.0 + u) : 1.0;
    dk = -(2.0 * param) * r * k;      // -d2 (1 + u)^(-alpha - 1), d2 = 2 alpha u
    dp = k == 0.0 ? 0.0 : k * (r - l);
    return;
  }
  if (kind == K_COSINE || kind == K_GAMMAEXP || (MN && kind == K_MATERN_NU)) {
    const KpDerivs r = MN ? newkind_derivs_mn(kind, d2, param, kind == K_MATERN_NU ? term->nuc : nullptr)
                          : newkind_derivs(kind, d2, param);
    k = r.k;
    dk = r.dk;
    dp = r.dp;
    return;
  }
  kern_and_dscale(kind, d2, param, k, dk);
  dp = kind == G_CONST ? 1.0 : 0.0;
}

template <int DMAX, int MN>
__global__ __launch_bounds__(256) void grad_kprod_kernel(const double* Kinv, long ldk, const double* alpha, long r0, long nr,
                                                         long c0, long nc, const DevTerm* terms, int nf,
                                                         long tile_r_first, long tile_c_first,
                                                         double* partials /*[blocks][KP_MAXF][3]*/) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;   // factors x DMAX <= 64: the spec's limit
  const long gtr = tile_r_first + blockIdx.x;
  const long gtc = tile_c_first + blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* sx = smem;                         // [TMAX][128][DMAX] column points
  double* scs = smem + TMAX * TILE * DMAX;   // [128] column scale of the head
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  long cbeg = gtc * TILE, cend = cbeg + TILE;
  if (cbeg < c0) cbeg = c0;
  if (cend > c0 + nc) cend = c0 + nc;
  long rbeg = gtr * TILE, rend = rbeg + TILE;
  if (rbeg < r0) rbeg = r0;
  if (rend > r0 + nr) rend = r0 + nr;
  const bool live_tile = cbeg < cend && rbeg < rend;

  for (int f = 0; f < nf; ++f) {
    const DevTerm T = terms[f];
    for (int idx = t; idx < TILE * DMAX; idx += 256) {
      const int p = idx / DMAX, d = idx % DMAX;
      const long gc = gtc * TILE + p;
      double v = 0.0;
      if (live_tile && d < T.dim && gc >= cbeg && gc < cend) v = T.xc[(gc - c0) * T.ldc + d];
      sx[(f * TILE + p) * DMAX + d] = v;
    }
  }
  if (t < TILE) {
    const DevTerm H = terms[0];
    const long gc = gtc * TILE + t;
    scs[t] = (live_tile && H.cs && gc >= cbeg && gc < cend) ? H.cs[gc - c0] : 1.0;
  }
  __syncthreads();

  double g_coef = 0.0, gs_acc[TMAX], gp_acc[TMAX];
#pragma unroll
  for (int f = 0; f < TMAX; ++f) gs_acc[f] = gp_acc[f] = 0.0;

  const long grow = gtr * TILE + trow;
  if (live_tile && grow >= rbeg && grow < rend) {
    const long lrow = grow - r0;
    const double ai = alpha ? alpha[grow] : 0.0;
    double xr[TMAX * DMAX], param[TMAX];
    int kind[TMAX];
#pragma unroll
    for (int f = 0; f < TMAX; ++f) {
      kind[f] = G_CONST;
      param[f] = 1.0;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) xr[f * DMAX + d] = 0.0;
      if (f < nf) {
        const DevTerm T = terms[f];
        kind[f] = T.kind & KP_KIND_MASK;
        param[f] = T.param;
        const double* xp = T.xr + lrow * T.ldr;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) xr[f * DMAX + d] = (d < T.dim) ? xp[d] : 0.0;
      }
    }
    const DevTerm H = terms[0];
    const double rsv = H.rs ? H.rs[lrow] : 1.0, coef = H.coef;
    const int pbeg = th * 64;
    const long gcol0 = gtc * TILE;
    for (int p = pbeg; p < pbeg + 64; ++p) {
      const long gc = gcol0 + p;
      if (gc < cbeg || gc >= cend) continue;
      const double g = alpha ? 0.5 * (ai * alpha[gc] - Kinv[grow + gc * ldk]) : Kinv[grow + gc * ldk];
      double k[TMAX], dk[TMAX], dp[TMAX], pre[TMAX + 1];
      pre[0] = 1.0;
#pragma unroll
      for (int f = 0; f < TMAX; ++f) {
        k[f] = 1.0;
        dk[f] = dp[f] = 0.0;
        if (f < nf) kp_factor_grad<DMAX, MN>(kind[f], param[f], &xr[f * DMAX], &sx[(f * TILE + p) * DMAX], k[f], dk[f], dp[f], terms + f);
        pre[f + 1] = pre[f] * k[f];
      }
      const double w = g * rsv * scs[p];
      g_coef = fma(w, pre[TMAX], g_coef);
      const double wc = w * coef;
      double suf = 1.0;   // the product of the factors behind f
#pragma unroll
      for (int f = TMAX - 1; f >= 0; --f) {
        if (f < nf) {
          const double excl = wc * (pre[f] * suf);
          gs_acc[f] = fma(excl, dk[f], gs_acc[f]);
          gp_acc[f] = fma(excl, dp[f], gp_acc[f]);
        }
        suf = suf * k[f];
      }
    }
  }
  // block reduction (fixed order): wave shuffle, then 4 partials through LDS
  __syncthreads();
  double* red = smem;  // reuse: [4 waves][KP_MAXF][3]
#pragma unroll
  for (int f = 0; f < KP_MAXF; ++f) {
    double a = (f == 0) ? g_coef : 0.0, b = 0.0, c = 0.0;
    if (f < TMAX) b = gs_acc[f < TMAX ? f : 0], c = gp_acc[f < TMAX ? f : 0];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off, 64);
      b += __shfl_xor(b, off, 64);
      c += __shfl_xor(c, off, 64);
    }
    if ((t & 63) == 0) {
      red[((t >> 6) * KP_MAXF + f) * 3 + 0] = a;
      red[((t >> 6) * KP_MAXF + f) * 3 + 1] = b;
      red[((t >> 6) * KP_MAXF + f) * 3 + 2] = c;
    }
  }
  __syncthreads();
  if (t < KP_MAXF * 3) {
    double s = 0.0;
    for (int wv = 0; wv < 4; ++wv) s += red[wv * KP_MAXF * 3 + t];
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    partials[blk * KP_MAXF * 3 + t] = s;
  }
}

// out_*[f] = sum_b partials[b][f][c]: one workgroup per output, 256 strided partial sums combined by a fixed tree.  The
// continuations' d / d coef is 0 by definition; out_param may be NULL
__global__ __launch_bounds__(256) void grad_kprod_reduce_kernel(const double* partials, long nblocks, double* out_coef,
                                                                double* out_scale, double* out_param) {
  __shared__ double sh[256];
  const int idx = blockIdx.x;  // factor * 3 + component
  double s = 0.0;
  for (long b = threadIdx.x; b < nblocks; b += 256) s += partials[b * KP_MAXF * 3 + idx];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int f = idx / 3, c = idx % 3;
    if (c == 0 && out_coef) out_coef[f] = f == 0 ? sh[0] : 0.0;
    if (c == 1 && out_scale) out_scale[f] = sh[0];
    if (c == 2 && out_param) out_param[f] = sh[0];
  }
}

template <int DMAX, int MN>
static int launch_grad_kprod_t(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                               const DevTerm* d_terms, int nf, long trf, long tcf, long trc, long tcc, double* partials,
                               hipStream_t s) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;
  if (nf > TMAX) {
    set_error("grad: a product chain beyond factors x dimension <= 64");
    return -1;
  }
  const size_t lds = (size_t)(TMAX * TILE * DMAX + TILE) * sizeof(double);
  SGP_LDS_ATTR_ONCE((grad_kprod_kernel<DMAX, MN>), lds);
  hipLaunchKernelGGL((grad_kprod_kernel<DMAX, MN>), dim3((unsigned)trc, (unsigned)tcc), dim3(256), lds, s, Kinv, ldk, alpha, r0,
                     nr, c0, nc, d_terms, nf, trf, tcf, partials);
  SGP_HIP(hipGetLastError());
  return 0;
}

// partials: trc x tcc x 24 doubles.  out_coef / out_scale / out_param: the chain's first entry (nf each; any may be NULL)
int launch_grad_kprod(const double* Kinv, long ldk, const double* alpha, long r0, long nr, long c0, long nc,
                      const DevTerm* d_terms, int nf, int dmax, int mn, long trf, long tcf, long trc, long tcc,
                      double* partials, double* out_coef, double* out_scale, double* out_param, hipStream_t s) {
  if (nf <= 0 || trc <= 0 || tcc <= 0) return 0;
  if (nf > KP_MAXF || dmax > 16) {
    set_error("grad: a product chain beyond the limits of include/sthenomi_kprod.h");
    return -1;
  }
  int rc;
#define SGP_KG(DM)                                                                                                     \
  rc = mn == 3 ? launch_grad_kprod_t<DM, 3>(Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, nf, trf, tcf, trc, tcc, partials, s) \
       : mn == 2 ? launch_grad_kprod_t<DM, 2>(Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, nf, trf, tcf, trc, tcc, partials, s) \
       : mn    ? launch_grad_kprod_t<DM, 1>(Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, nf, trf, tcf, trc, tcc, partials, s) \
               : launch_grad_kprod_t<DM, 0>(Kinv, ldk, alpha, r0, nr, c0, nc, d_terms, nf, trf, tcf, trc, tcc, partials, s)
  if (dmax <= 1) SGP_KG(1);
  else if (dmax <= 2) SGP_KG(2);
  else if (dmax <= 4) SGP_KG(4);
  else if (dmax <= 8) SGP_KG(8);
  else SGP_KG(16);
#undef SGP_KG
  if (rc) return rc;
  hipLaunchKernelGGL(grad_kprod_reduce_kernel, dim3((unsigned)(nf * 3)), dim3(256), 0, s, partials, trc * tcc, out_coef,
                     out_scale, out_param);
  SGP_HIP(hipGetLastError());
  return 0;
}


// ---- input-point and scale gradients of ONE chain ---------------------------------------------------------------------
// k and d k / d x of one factor from its row point and a column point: a distance kind has d k / d x = 2 kx (x - x') with
// kx = kappa'(d2) (kern_grad.h: kern_val_dd2; COSINE / GAMMAEXP / MATERN_NU: their _derivs above; RQ: -1/2 (1 + u)^(-alpha - 1)
// = -1/2 exp(-(alpha + 1) log1p(u)), an exact 0 -- never NaN -- where d2 overflowed, finite where only u did: rq_log1p_u),
// LINEAR has d k / d x = x' and kx stands for nothing.
// NK: 1 if the chain holds a COSINE / GAMMAEXP factor, 2 if it holds a MATERN_NU factor (and possibly those), else 0.  The call of their out-of-line routine costs the row-side kernel
// below registers at every factor (DMAX = 1: 2 waves per SIMD become 1), so chains of the older kinds run an instantiation
// without it
// NK == 3: the chain holds a NEURALNET / FBM / EXPONENTIATED factor (and possibly any other kind).  Such a factor has
// d k / d x = c1 x + c2 (x - x') + c3 x' (KpDotDerivs), c2 = 2 kx; c1 and c3 exist in that instantiation only.
// NK == 4: the chain holds a WIENER / PIECEWISE factor (and possibly any other kind): launch mode 3 of the kernels above.
template <int DMAX, int NK>
__device__ __forceinline__ void kp_factor_dx(int kind, double param, const double* xr, const double* sp, double& k,
                                             double& kx, const double* nuc, double& c1, double& c3) {
  if (KP_DOT_ROUTE(NK - 1, kind)) {
    const KpDot q = kp_dot_scalars<DMAX, NK == 4>(kind, xr, sp);
    const KpDotDerivs r = KP_DOT_DERIVS(NK - 1, kind, param, q);
    k = r.k;
    kx = 0.5 * r.c2;
    c1 = r.c1;
    c3 = r.c3;
    return;
  }
  if (kind == K_LINEAR) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) s = fma(xr[d], sp[d], s);
    k = s + param;
    kx = 0.0;
    return;
  }
  double d2 = 0.0;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    const double df = xr[d] - sp[d];
    d2 = fma(df, df, d2);
  }
  if (kind == K_RQ) {
    double u;
    const double l = rq_log1p_u(d2, param, u);
    k = exp(-param * l);
    kx = -0.5 * exp(-(param + 1.0) * l);
    return;
  }
  if (NK && (kind == K_COSINE || kind == K_GAMMAEXP || (NK >= 2 && kind == K_MATERN_NU))) {
    const KpDerivs r = NK >= 2 ? newkind_derivs_mn(kind, d2, param, nuc) : newkind_derivs(kind, d2, param);
    k = r.k;
    kx = r.kx;
    return;
  }
  kern_val_dd2(kind, d2, param, k, kx);
}

// Row side of one chain over one block pair, grad_inputs_kernel's tiling (grad.hip): a workgroup owns 128 rows and walks the
// column tiles, thread = one row x one half of a tile's columns, the column points of every factor in LDS, the row points and
// one accumulator per (factor, coordinate) in registers.  Per entry every factor is evaluated once (k and kx), the products
// with one factor left out come from prefix and suffix products (no division), and factor f adds
//     W_ij E^f_ij 2 kx_f (x^f_i - x'^f_j)   (distance kinds)       W_ij E^f_ij x'^f_j   (LINEAR)
// into its own accumulators.  The two column halves are combined in a fixed order through LDS (the column points' storage,
// no longer needed) and the owner adds into the gradient of each factor's row input, in factor order: no atomics.
// G as in grad_inputs_kernel: Gm[(r0 + i) * sr + (c0 + j) * sc], alpha != NULL: G = (alpha alpha' - Gm) / 2.
struct KpChainArgs {
  DevTerm t[KP_MAXF];
  double* gx[KP_MAXF];   // gradient of factor f's row input (dim x nr, packed) or NULL
};

template <int DMAX, int NK>
__global__ __launch_bounds__(256) void grad_kprod_inputs_kernel(const double* Gm, long sr, long sc, const double* alpha,
                                                                long r0, long nr, long c0, long nc, KpChainArgs C, int nf,
                                                                double scale, double* gsv /* nr, or NULL */) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* sx = smem;                         // [TMAX][128][DMAX] column points; afterwards [TMAX * DMAX][128] half sums
  double* scs = smem + TMAX * TILE * DMAX;   // [128] column scale of the head; afterwards the half sums of gsv
  const int t = threadIdx.x;
  const int trow = t & 127, th = t >> 7;
  const long lrow = (long)blockIdx.x * TILE + trow;
  const bool live = lrow < nr;
  const long grow = r0 + lrow;
  double xr[TMAX * DMAX], acc[TMAX * DMAX], param[TMAX];
  int kind[TMAX];
#pragma unroll
  for (int f = 0; f < TMAX; ++f) {
    kind[f] = G_CONST;
    param[f] = 1.0;
    const bool on = live && f < nf;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      xr[f * DMAX + d] = (on && d < C.t[f].dim) ? C.t[f].xr[lrow * C.t[f].ldr + d] : 0.0;
      acc[f * DMAX + d] = 0.0;
    }
    if (f < nf) {
      kind[f] = C.t[f].kind & KP_KIND_MASK;
      param[f] = C.t[f].param;
    }
  }
  double accs = 0.0;
  const double coef = C.t[0].coef;
  const double ai = (alpha && live) ? alpha[grow] : 0.0;
  const double wrow = live ? coef * (C.t[0].rs ? C.t[0].rs[lrow] : 1.0) : 0.0;
  for (long ct = 0; ct * TILE < nc; ++ct) {
    __syncthreads();
#pragma unroll
    for (int f = 0; f < TMAX; ++f) {
      if (f >= nf) break;
      for (int idx = t; idx < TILE * DMAX; idx += 256) {
        const int p = idx / DMAX, d = idx % DMAX;
        const long lc = ct * TILE + p;
        sx[f * TILE * DMAX + idx] = (lc < nc && d < C.t[f].dim) ? C.t[f].xc[lc * C.t[f].ldc + d] : 0.0;
      }
    }
    if (t < TILE) {
      const long lc = ct * TILE + t;
      scs[t] = (lc < nc) ? (C.t[0].cs ? C.t[0].cs[lc] : 1.0) : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int p = th * 64; p < th * 64 + 64; ++p) {
        const long lc = ct * TILE + p;
        if (lc >= nc) break;
        const long gc = c0 + lc;
        const double gm = Gm[grow * sr + gc * sc];
        const double g = alpha ? 0.5 * (ai * alpha[gc] - gm) : gm;
        double k[TMAX], kx[TMAX], pre[TMAX + 1];
        double c1[NK >= 3 ? TMAX : 1], c3[NK >= 3 ? TMAX : 1];   // NEURALNET / FBM / EXPONENTIATED / WIENER: kp_factor_dx
        pre[0] = 1.0;
#pragma unroll
        for (int f = 0; f < TMAX; ++f) {
          k[f] = 1.0;
          kx[f] = 0.0;
          if (NK >= 3) c1[NK >= 3 ? f : 0] = c3[NK >= 3 ? f : 0] = 0.0;
          if (f < nf) kp_factor_dx<DMAX, NK>(kind[f], param[f], &xr[f * DMAX], &sx[(f * TILE + p) * DMAX], k[f], kx[f],
                                              NK >= 2 ? C.t[f].nuc : nullptr, c1[NK >= 3 ? f : 0], c3[NK >= 3 ? f : 0]);
          pre[f + 1] = pre[f] * k[f];
        }
        const double gcs = g * scs[p];
        accs = fma(gcs * coef, pre[TMAX], accs);
        const double w = gcs * wrow;
        double suf = 1.0;   // the product of the factors behind f
#pragma unroll
        for (int f = TMAX - 1; f >= 0; --f) {
          if (f < nf) {
            const double excl = w * (pre[f] * suf);
            const double* sp = &sx[(f * TILE + p) * DMAX];
            if (KP_DOT_ROUTE(NK - 1, kind[f])) {
              const double e1 = excl * c1[NK >= 3 ? f : 0], e2 = 2.0 * excl * kx[f], e3 = excl * c3[NK >= 3 ? f : 0];
#pragma unroll
              for (int d = 0; d < DMAX; ++d) {
                const double xv = xr[f * DMAX + d];
                acc[f * DMAX + d] = fma(e3, sp[d], fma(e2, xv - sp[d], fma(e1, xv, acc[f * DMAX + d])));
              }
            } else if (kind[f] == K_LINEAR) {
#pragma unroll
              for (int d = 0; d < DMAX; ++d) acc[f * DMAX + d] = fma(excl, sp[d], acc[f * DMAX + d]);
            } else {
              const double c2 = 2.0 * excl * kx[f];
#pragma unroll
              for (int d = 0; d < DMAX; ++d) acc[f * DMAX + d] = fma(c2, xr[f * DMAX + d] - sp[d], acc[f * DMAX + d]);
            }
          }
          suf = suf * k[f];
        }
      }
    }
  }
  // combine the two column halves in fixed order, then add into the inputs' gradients
  __syncthreads();
  if (th == 1) {
#pragma unroll
    for (int q = 0; q < TMAX * DMAX; ++q) sx[q * TILE + trow] = acc[q];
    scs[trow] = accs;
  }
  __syncthreads();
  if (th == 0 && live) {
#pragma unroll
    for (int f = 0; f < TMAX; ++f) {
      if (f >= nf || !C.gx[f]) continue;
      const int dim = C.t[f].dim;
      double* o = C.gx[f] + lrow * dim;
#pragma unroll
      for (int d = 0; d < DMAX; ++d)
        if (d < dim) o[d] += scale * (acc[f * DMAX + d] + sx[(f * DMAX + d) * TILE + trow]);
    }
    if (gsv) gsv[lrow] += scale * (accs + scs[trow]);
  }
}

template <int DMAX, int NK>
static int launch_grad_kprod_inputs_t(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0,
                                      long nc, const KpChainArgs& C, int nf, double scale, double* gsv, hipStream_t s) {
  constexpr int TMAX = (64 / DMAX < KP_MAXF) ? 64 / DMAX : KP_MAXF;
  if (nf > TMAX) {
    set_error("grad: a product chain beyond factors x dimension <= 64");
    return -1;
  }
  const size_t lds = (size_t)(TMAX * TILE * DMAX + TILE) * sizeof(double);
  SGP_LDS_ATTR_ONCE((grad_kprod_inputs_kernel<DMAX, NK>), lds);
  hipLaunchKernelGGL((grad_kprod_inputs_kernel<DMAX, NK>), dim3((unsigned)((nr + TILE - 1) / TILE)), dim3(256), lds, s, Gm,
                     sr, sc, alpha, r0, nr, c0, nc, C, nf, scale, gsv);
  SGP_HIP(hipGetLastError());
  return 0;
}

// h_terms: the chain's nf factors (host copies); gx[f]: where factor f's row-input gradient goes (NULL: not asked for);
// gsv: the head's row-scale sums (NULL: not asked for).  transpose != 0: every factor is seen from its column points (the
// caller passes (sr, sc), the offsets and lengths of the transposed block itself, as for launch_grad_inputs)
int launch_grad_kprod_inputs(const double* Gm, long sr, long sc, const double* alpha, long r0, long nr, long c0, long nc,
                             const DevTerm* h_terms, int nf, int dmax, int transpose, double scale, double* const* gx,
                             double* gsv, hipStream_t s) {
  if (nf <= 0 || nr <= 0 || nc <= 0) return 0;
  if (nf > KP_MAXF || dmax > 16) {
    set_error("grad: a product chain beyond the limits of include/sthenomi_kprod.h");
    return -1;
  }
  KpChainArgs C;
  for (int f = 0; f < KP_MAXF; ++f) {
    C.t[f] = h_terms[f < nf ? f : 0];
    C.gx[f] = (f < nf && gx) ? gx[f] : nullptr;
    if (transpose) {
      std::swap(C.t[f].xr, C.t[f].xc);
      std::swap(C.t[f].ldr, C.t[f].ldc);
      std::swap(C.t[f].rs, C.t[f].cs);
    }
  }
  int rc;
  int nk = 0;
  for (int f = 0; f < nf; ++f) {
    const int kind = h_terms[f].kind & KP_KIND_MASK;
    nk = std::max(nk, kp_is_wpp(kind) ? 4 : kind >= K_NEURALNET ? 3 : kind == K_MATERN_NU ? 2 : (kind == K_COSINE || kind == K_GAMMAEXP) ? 1 : 0);
  }
#define SGP_KI(DM)                                                                                                     \
  rc = nk == 4 ? launch_grad_kprod_inputs_t<DM, 4>(Gm, sr, sc, alpha, r0, nr, c0, nc, C, nf, scale, gsv, s)            \
       : nk == 3 ? launch_grad_kprod_inputs_t<DM, 3>(Gm, sr, sc, alpha, r0, nr, c0, nc, C, nf, scale, gsv, s)          \
       : nk == 2 ? launch_grad_kprod_inputs_t<DM, 2>(Gm, sr, sc, alpha, r0, nr, c0, nc, C, nf, scale, gsv, s)          \
       : nk    ? launch_grad_kprod_inputs_t<DM, 1>(Gm, sr, sc, alpha, r0, nr, c0, nc, C, nf, scale, gsv, s)            \
               : launch_grad_kprod_inputs_t<DM, 0>(Gm, sr, sc, alpha, r0, nr, c0, nc, C, nf, scale, gsv, s)
  if (dmax <= 1) SGP_KI(1);
  else if (dmax <= 2) SGP_KI(2);
  else if (dmax <= 4) SGP_KI(4);
  else if (dmax <= 8) SGP_KI(8);
  else SGP_KI(16);
#undef SGP_KI
  return rc;
}

// ---- the diagonal of ONE chain: sum_i w_i d var_i / d theta, var_i = coef rs_i cs_i prod_f k_f(xr^f_i, xc^f_i) -----------
// One workgroup, every point handled by exactly one thread: the per-point outputs (row / column scale, input points) are
// added by that thread, the sums over points (d / d coef of the head, d / d inscale and d / d param of every factor) are
// reduced in a fixed order.  Inputs: a distance kind gives the row input + and the column input - 2 kx (xr - xc) (they cancel
// when both are one array, which is skipped); LINEAR gives the row input xc and the column input xr, both added when they are
// one array.
struct KpDiagArgs {
  DevTerm t[KP_MAXF];
  double* gxr[KP_MAXF];
  double* gxc[KP_MAXF];
};

template <int MN>
__global__ __launch_bounds__(256) void diag_grad_kprod_kernel(const double* w, long n, KpDiagArgs C, int nf, double* out_coef,
                                                              double* out_scale, double* out_param, double* out_rs,
                                                              double* out_cs) {
  __shared__ double sh[256];
  double g_coef = 0.0, gs_acc[KP_MAXF], gp_acc[KP_MAXF];
#pragma unroll
  for (int f = 0; f < KP_MAXF; ++f) gs_acc[f] = gp_acc[f] = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    double k[KP_MAXF], dk[KP_MAXF], dp[KP_MAXF], kx[KP_MAXF], pre[KP_MAXF + 1];
    constexpr int NDOT = MN >= 2 ? KP_MAXF : 1;   // NEURALNET / FBM / EXPONENTIATED: the coefficients of KpDotDerivs
    double c1[NDOT], c1y[NDOT], c3[NDOT];
    pre[0] = 1.0;
#pragma unroll
    for (int f = 0; f < KP_MAXF; ++f) {
      k[f] = 1.0;
      dk[f] = dp[f] = kx[f] = 0.0;
      if (MN >= 2) c1[f % NDOT] = c1y[f % NDOT] = c3[f % NDOT] = 0.0;
      if (f < nf) {
        const DevTerm& T = C.t[f];
        const int kind = T.kind & KP_KIND_MASK;
        const double* a = T.xr + i * T.ldr;
        const double* b = T.xc + i * T.ldc;
        if (KP_DOT_ROUTE(MN, kind)) {
          const KpDot q = kp_dot_scalars_n<MN == 3>(kind, a, b, T.dim);
          const KpDotDerivs r = KP_DOT_DERIVS(MN, kind, T.param, q);
          k[f] = r.k;
          dk[f] = r.dk;
          dp[f] = r.dp;
          kx[f] = 0.5 * r.c2;
          c1[f % NDOT] = r.c1;
          c1y[f % NDOT] = r.c1y;
          c3[f % NDOT] = r.c3;
        } else if (kind == K_LINEAR) {
          double s = 0.0;
          for (int d = 0; d < T.dim; ++d) s = fma(a[d], b[d], s);
          k[f] = s + T.param;
          dk[f] = 2.0 * s;
          dp[f] = 1.0;
        } else {
          double d2 = 0.0;
          for (int d = 0; d < T.dim; ++d) {
            const double df = a[d] - b[d];
            d2 = fma(df, df, d2);
          }
          if (kind == K_RQ) {
            double u;
            const double l = rq_log1p_u(d2, T.param, u);
            k[f] = exp(-T.param * l);
            const double r = u < 1e300 ? u / (1.0 + u) : 1.0;
            dk[f] = -(2.0 * T.param) * r * k[f];
            dp[f] = k[f] == 0.0 ? 0.0 : k[f] * (r - l);
            kx[f] = -0.5 * exp(-(T.param + 1.0) * l);
          } else if (kind == K_COSINE || kind == K_GAMMAEXP || (MN && kind == K_MATERN_NU)) {
            const KpDerivs r = MN ? newkind_derivs_mn(kind, d2, T.param, kind == K_MATERN_NU ? T.nuc : nullptr)
                                  : newkind_derivs(kind, d2, T.param);
            k[f] = r.k;
            dk[f] = r.dk;
            kx[f] = r.kx;
            dp[f] = r.dp;
          } else {
            double kk;
            kern_and_dscale(kind, d2, T.param, k[f], dk[f]);
            kern_val_dd2(kind, d2, T.param, kk, kx[f]);
            dp[f] = kind == G_CONST ? 1.0 : 0.0;
          }
        }
      }
      pre[f + 1] = pre[f] * k[f];
    }
    const DevTerm& H = C.t[0];
    const double rsv = H.rs ? H.rs[i] : 1.0, csv = H.cs ? H.cs[i] : 1.0;
    const double wi = w[i];
    g_coef = fma(wi * rsv * csv, pre[KP_MAXF], g_coef);
    if (out_rs) out_rs[i] += wi * H.coef * csv * pre[KP_MAXF];
    if (out_cs) out_cs[i] += wi * H.coef * rsv * pre[KP_MAXF];
    const double wc = wi * rsv * csv * H.coef;
    double suf = 1.0;
    double excl[KP_MAXF];
#pragma unroll
    for (int f = KP_MAXF - 1; f >= 0; --f) {
      excl[f] = wc * (pre[f] * suf);
      if (f < nf) {
        gs_acc[f] = fma(excl[f], dk[f], gs_acc[f]);
        gp_acc[f] = fma(excl[f], dp[f], gp_acc[f]);
      }
      suf = suf * k[f];
    }
#pragma unroll
    for (int f = 0; f < KP_MAXF; ++f) {   // factor order: several factors may add into one array
      if (f >= nf || !C.gxr[f]) continue;
      const DevTerm& T = C.t[f];
      const double* a = T.xr + i * T.ldr;
      const double* b = T.xc + i * T.ldc;
      double* orow = C.gxr[f] + i * T.dim;
      double* ocol = C.gxc[f] + i * T.dim;
      if (KP_DOT_ROUTE(MN, T.kind & KP_KIND_MASK)) {
        // LINEAR's convention: the row input receives d k / d x, the column input d k / d y, both added when they are one array
        const double e1 = excl[f] * c1[f % NDOT], e1y = excl[f] * c1y[f % NDOT], e2 = 2.0 * excl[f] * kx[f],
                     e3 = excl[f] * c3[f % NDOT];
        for (int d = 0; d < T.dim; ++d) {
          const double av = a[d], bv = b[d];
          orow[d] += fma(e3, bv, fma(e2, av - bv, e1 * av));
          ocol[d] += fma(e3, av, fma(e2, bv - av, e1y * bv));
        }
      } else if ((T.kind & KP_KIND_MASK) == K_LINEAR) {
        for (int d = 0; d < T.dim; ++d) {
          const double av = a[d], bv = b[d];
          orow[d] += excl[f] * bv;
          ocol[d] += excl[f] * av;
        }
      } else if (ocol != orow) {
        const double c2 = 2.0 * excl[f] * kx[f];
        for (int d = 0; d < T.dim; ++d) {
          const double df = a[d] - b[d];
          orow[d] += c2 * df;
          ocol[d] -= c2 * df;
        }
      }
    }
  }
  // fixed-order tree per output
  for (int q = 0; q < 1 + 2 * KP_MAXF; ++q) {
    double v = 0.0;
    if (q == 0) v = g_coef;
#pragma unroll
    for (int f = 0; f < KP_MAXF; ++f) {
      if (q == 1 + f) v = gs_acc[f];
      if (q == 1 + KP_MAXF + f) v = gp_acc[f];
    }
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (q == 0) {
        if (out_coef) {
          out_coef[0] = sh[0];
          for (int f = 1; f < nf; ++f) out_coef[f] = 0.0;
        }
      } else if (q <= KP_MAXF) {
        if (out_scale && q - 1 < nf) out_scale[q - 1] = sh[0];
      } else if (out_param && q - 1 - KP_MAXF < nf) {
        out_param[q - 1 - KP_MAXF] = sh[0];
      }
    }
  }
}

// out_coef / out_scale / out_param: the chain's first entry (nf each, device; any may be NULL); gxr / gxc: per factor, the
// gradient arrays of its row / column input at the block's first point (both or neither; NULL arrays: not asked for);
// out_rs / out_cs: the head's row / column scale sums (NULL: not asked for)
int launch_diag_grad_kprod(const double* w, long n, const DevTerm* h_terms, int nf, double* out_coef, double* out_scale,
                           double* out_param, double* const* gxr, double* const* gxc, double* out_rs, double* out_cs,
                           hipStream_t s) {
  if (nf <= 0 || n <= 0) return 0;
  if (nf > KP_MAXF) {
    set_error("grad: a product chain beyond the limits of include/sthenomi_kprod.h");
    return -1;
  }
  KpDiagArgs C;
  for (int f = 0; f < KP_MAXF; ++f) {
    C.t[f] = h_terms[f < nf ? f : 0];
    C.gxr[f] = (f < nf && gxr) ? gxr[f] : nullptr;
    C.gxc[f] = (f < nf && gxc) ? gxc[f] : nullptr;
  }
  const int mode = kprod_mode(h_terms, nf);
  if (mode == 3)
    hipLaunchKernelGGL(diag_grad_kprod_kernel<3>, dim3(1), dim3(256), 0, s, w, n, C, nf, out_coef, out_scale, out_param,
                       out_rs, out_cs);
  else if (mode == 2)
    hipLaunchKernelGGL(diag_grad_kprod_kernel<2>, dim3(1), dim3(256), 0, s, w, n, C, nf, out_coef, out_scale, out_param,
                       out_rs, out_cs);
  else if (mode)
    hipLaunchKernelGGL(diag_grad_kprod_kernel<1>, dim3(1), dim3(256), 0, s, w, n, C, nf, out_coef, out_scale, out_param,
                       out_rs, out_cs);
  else
    hipLaunchKernelGGL(diag_grad_kprod_kernel<0>, dim3(1), dim3(256), 0, s, w, n, C, nf, out_coef, out_scale, out_param,
                       out_rs, out_cs);
  SGP_HIP(hipGetLastError());
  return 0;
}

}  // namespace sgp
