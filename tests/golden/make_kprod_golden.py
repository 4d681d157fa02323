"""Generate tests/golden/sklearn_kprod.json: a scikit-learn GaussianProcessRegressor (Rasmussen & Williams Alg. 2.1, an
implementation independent of this repository) with a kernel built from products,
    4 RBF(1.5) ExpSineSquared(1.2, 0.9) + 0.7 RationalQuadratic(0.8, alpha = 1.3) + 0.1 DotProduct(0.5)^2 + White(0.1)
on N = 150 points of a 1-D input, uniform in [-3, 3]: the locally periodic kernel of the Mauna-Loa models, a
rational-quadratic term and a polynomial.  In this package's terms
    4 SE o (1 / 1.5) * PeriodicKernel(r = 0.6) o (1 / 0.9) + 0.7 RQ(1.3) o (1 / 0.8) + 0.1 PolynomialKernel(2, 0.25), noise 0.1.
The targets y are this generator's own (the issue that asked for this golden fixed x and the kernel, not y), so the log
marginal likelihood stored here, -73.72, is not the -716.36 quoted there.
Stored (arrays as little-endian float64 in base64): x, y, every tenth row of the kernel matrix without the White term (the
log marginal likelihood holds all of it to account), its condition number with the White term, the log marginal likelihood.

    python tests/golden/make_kprod_golden.py      (needs scikit-learn)
"""
import base64
import json
import os

import numpy as np
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, DotProduct, ExpSineSquared, RationalQuadratic, WhiteKernel


def main():
    rng = np.random.default_rng(20240611)
    n = 150
    x = np.sort(rng.uniform(-3.0, 3.0, n))
    y = np.sin(2.0 * x) * np.exp(-0.1 * x * x) + 0.3 * x + 0.3 * rng.standard_normal(n)
    signal = (ConstantKernel(4.0) * RBF(1.5) * ExpSineSquared(1.2, 0.9) + ConstantKernel(0.7) * RationalQuadratic(0.8, 1.3) +
              ConstantKernel(0.1) * DotProduct(0.5) ** 2)
    kernel = signal + WhiteKernel(0.1)
    gpr = GaussianProcessRegressor(kernel=kernel, optimizer=None, alpha=0.0).fit(x[:, None], y)
    K = signal(x[:, None])
    pack = lambda a: base64.b64encode(np.ascontiguousarray(a, dtype="<f8").tobytes()).decode("ascii")      # noqa: E731
    out = {"n": n, "x": pack(x), "y": pack(y), "noise": 0.1, "K_rows": list(range(0, n, 10)), "K": pack(K[::10]),
           "cond": float(np.linalg.cond(K + 0.1 * np.eye(n))),
           "lml": float(gpr.log_marginal_likelihood(gpr.kernel_.theta))}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sklearn_kprod.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes; lml", out["lml"], "cond", out["cond"])


if __name__ == "__main__":
    main()
