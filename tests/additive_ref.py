"""The additive kinds (include/sthenomi.h: SGP_ADDITIVE_*) written directly in long double, the error model of
docs/03_kernels.md 3.2h, and the float64 restatement of csrc/additive_eval.h.  TEST INFRASTRUCTURE ONLY, shared by
tests/test_gpu_additive.py and tests/test_additive_on_numpy.py.

Units of 2^-53, one per rounding.  A coordinate z_d = kappa(u_d^2) with exponent magnitude x (SE s / 2, Matern c |u|) is right
to U_z = A x + B: u 1, s = u u 3; SE: the exponent 3, exp 4 (2 ulp): (3, 4).  Matern: the root 1.5 + 2, Matern-1/2 (3.5, 4);
l = c r adds the constant and a product: 5.5; Matern-3/2 adds 1 + l (6.5) and the product: (5.5, 11.5); Matern-5/2 the
polynomial (l^2 / 3: 13, one fma more: 14) and the product: (5.5, 19).  An entry: every product of r coordinates r max U_z,
one rounding per coordinate step of the recurrence (D), (coef rs) cs 2, the fma 1, one spare: r max_d U_z + D + 4, the maximum
over the coordinates that are alive (x <= 700; beyond 800 z_d is an exact 0).  A gradient sum: R max U_z + 3 D + 16 (the
tangent's or the skip-one table's steps, kappa', the products in front) in units of the sum of its absolute addends."""
import itertools

import numpy as np

LD, EPS, TINY = np.longdouble, 2.0 ** -53, 2.0 ** -1070
SCALE = {0: None, 1: 1.0, 2: np.sqrt(LD(3)), 3: np.sqrt(LD(5))}      # base kind (SGP_SE .. SGP_MATERN52) -> c of l = c |u|
UZ = {0: (3.0, 4.0), 1: (3.5, 4.0), 2: (5.5, 11.5), 3: (5.5, 19.0)}


def coords(base, X, Y, dtype=LD):
    """(z, kappa' = dz / ds, u, x) per coordinate and pair, (D, n, m) each"""
    u = np.asarray(X, dtype=dtype)[:, :, None] - np.asarray(Y, dtype=dtype)[:, None, :]
    s, one = u * u, dtype(1)
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        if base == 0:
            x = s / 2
            z = np.exp(-x)
            return z, -z / 2, u, x
        x = dtype(SCALE[base]) * np.abs(u)
        E = np.exp(-x)
        if base == 1:
            return E, np.where(s > 0, -E / (2 * np.where(s > 0, np.abs(u), one)), 0), u, x
        if base == 2:
            return (1 + x) * E, -E * 3 / 2, u, x
        return (1 + x + x * x / 3) * E, -(1 + x) * E * 5 / 6, u, x


def esp(z, R, skip=None):
    """[e_0 .. e_R] of z (D, ...) by the recurrence, coordinate `skip` left out"""
    e = [np.ones(z.shape[1:], dtype=z.dtype)] + [np.zeros(z.shape[1:], dtype=z.dtype) for _ in range(R)]
    for d in range(z.shape[0]):
        if d != skip:
            for k in range(R, 0, -1):
                e[k] = z[d] * e[k - 1] + e[k]
    return e


def esp_brute(z, r):
    return sum(np.prod([z[d] for d in c], axis=0) for c in itertools.combinations(range(z.shape[0]), r))


def units(base, x, r):
    """r max_d U_z + D + 4 per pair, the maximum over the live coordinates (x: coords(...)[3])"""
    a, b = UZ[base]
    xl = np.where(x <= 700, x, 0).astype(np.float64)
    return r * (a * xl.max(0) + b) + x.shape[0] + 4


def points(D, n, seed, far=2000.0):
    """n points in [-1, 1]^D; from 8 on: 1 == 0 (coincident), 2 shares the first half of 0's coordinates, 3 is far in
    coordinate 0, 4 far in all, and the last point coincides with the middle one (across a tile edge from 129 on)"""
    Z = np.asfortranarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (D, n)))
    if n >= 8:
        Z[:, 1] = Z[:, 0]
        Z[:(D + 1) // 2, 2] = Z[:(D + 1) // 2, 0]
        Z[0, 3] = far
        Z[:, 4] = far
        Z[:, n - 1] = Z[:, n // 2]
    return Z
