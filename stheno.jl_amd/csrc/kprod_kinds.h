// The per-kind device math of the product path: values and derivatives of the kinds that exist only there (RQ, COSINE, GAMMAEXP,
// MATERN_NU, the PIECEWISE kinds, NEURALNET / FBM / EXPONENTIATED and WIENER) and the out-of-line routines that put several
// kinds behind one call site.  Included by kprod.hip ALONE, inside namespace sgp and after its headers: this is a part of that
// file kept apart, not a header of its own.  What a kind is to the host -- code, tier, parameter rule -- is in
// kprod_kinds_table.h.  The kernels that call these routines sit at their register limits: definitions keep their order,
// their inlining attributes and their contraction pragmas.

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
  return kind == SGP_COSINE ? cosine_derivs(d2) : gexp_derivs(d2, param);
}
// MN: the launch mode (kprod.hip: 0, 1 with a MATERN_NU factor, 2 with a NEURALNET / FBM / EXPONENTIATED factor); this
// paragraph is about modes 0 and 1.  The Bessel routine's registers count against every kernel that
// can call it (the assembly: 3 waves per SIMD become 2; the contractions go to scratch), so every kernel below is instantiated
// with and without it, and chains without the kind run what they ran before it existed (docs/03_kernels.md section 3.2e).
// With MN the three kinds sit behind one call site (nuc: MATERN_NU only)
__device__ __noinline__ KpDerivs newkind_derivs_mn(int kind, double d2, double param, const double* nuc) {
  if (kind == SGP_MATERN_NU) return matern_nu_derivs(d2, param, nuc);
  return kind == SGP_COSINE ? cosine_derivs(d2) : gexp_derivs(d2, param);
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
  if (kind == SGP_FBM || (W && kp_scalar_route_kind_is_tier4(kind))) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      const double df = x[d] - y[d];
      r.e = fma(df, df, r.e);
    }
  } else if (kind == SGP_NEURALNET) {
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
  if (kind == SGP_FBM || (W && kp_scalar_route_kind_is_tier4(kind))) {
    for (int d = 0; d < dim; ++d) {
      const double df = x[d] - y[d];
      r.e = fma(df, df, r.e);
    }
  } else if (kind == SGP_NEURALNET) {
    for (int i = 0; i < dim; ++i)
      for (int j = i + 1; j < dim; ++j) {
        const double c = kp_cross(x[i], y[j], x[j], y[i]);
        r.e = fma(c, c, r.e);
      }
  }
  return r;
}
__device__ __noinline__ double dotkind_eval(int kind, double h, double s, double a, double b, double e) {
  if (kind == SGP_EXPONENTIATED) return exp(s);
  if (kind == SGP_FBM) return 0.5 * ((pow(a, h) + pow(b, h)) - pow(e, h));
  return atan2(s, sqrt(((a + b) + 1.0) + e));
}
__device__ __noinline__ KpDotDerivs dotkind_derivs(int kind, double h, double s, double a, double b, double e) {
  KpDotDerivs r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (kind == SGP_EXPONENTIATED) {
    r.k = exp(s);
    r.dk = 2.0 * s * r.k;
    r.c3 = r.k;
    return r;
  }
  if (kind == SGP_FBM) {
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
  if (kp_is_dot_kind(kind)) return dotkind_eval(kind, h, s, a, b, e);
  if (kind == SGP_WIENER) return wiener_eval(h, a, b, e);
  return pp_eval(kind - SGP_PIECEWISE0, e, h);
}
__device__ __noinline__ KpDotDerivs dotkind_derivs_w(int kind, double h, double s, double a, double b, double e) {
  if (kp_is_dot_kind(kind)) return dotkind_derivs(kind, h, s, a, b, e);
  if (kind == SGP_WIENER) return wiener_derivs(h, a, b, e);
  const KpDerivs q = pp_derivs(kind - SGP_PIECEWISE0, e, h);
  KpDotDerivs r = {q.k, q.dk, 0.0, 0.0, 0.0, 2.0 * q.kx, 0.0};
  return r;
}
