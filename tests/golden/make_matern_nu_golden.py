"""Generate tests/golden/sklearn_matern_nu.json: scikit-learn GaussianProcessRegressors (Rasmussen & Williams Alg. 2.1, an
implementation independent of this repository, its Matern through scipy.special.kv) with the two kernels
    1.7 Matern(length_scale = 0.9, nu = 0.8)        0.6 Matern(length_scale = 1.4, nu = 1.9)
on N = 40 points of a 2-D input, uniform in [-2, 2]^2, observation noise 0.1 (the regressor's alpha), and 7 prediction points.
In this package's terms  1.7 with_lengthscale(GeneralMaternKernel(0.8), 0.9)  and  0.6 with_lengthscale(GeneralMaternKernel(1.9), 1.4).
Stored (arrays as little-endian float64 in base64): x (2 x 40, column-major points), y, xs (2 x 7), and per model the kernel
matrix K (40 x 40, without the noise), the log marginal likelihood, the predictive mean and the predictive variance of the
latent function at xs.

    python tests/golden/make_matern_nu_golden.py      (needs scikit-learn)
"""
import base64
import json
import os

import numpy as np
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import ConstantKernel, Matern

MODELS = ((1.7, 0.9, 0.8), (0.6, 1.4, 1.9))      # (variance, length scale, nu)


def main():
    rng = np.random.default_rng(20240921)
    n, noise = 40, 0.1
    X = rng.uniform(-2.0, 2.0, (n, 2))
    Xs = rng.uniform(-2.2, 2.2, (7, 2))
    y = np.sin(1.5 * X[:, 0]) * np.cos(X[:, 1]) + 0.3 * rng.standard_normal(n)
    pack = lambda a: base64.b64encode(np.ascontiguousarray(a, dtype="<f8").tobytes()).decode("ascii")      # noqa: E731
    out = {"n": n, "noise": noise, "x": pack(X), "y": pack(y), "xs": pack(Xs), "models": []}
    for var, ell, nu in MODELS:
        kernel = ConstantKernel(var) * Matern(length_scale=ell, nu=nu)
        gpr = GaussianProcessRegressor(kernel=kernel, optimizer=None, alpha=noise).fit(X, y)
        mean, std = gpr.predict(Xs, return_std=True)
        out["models"].append({"variance": var, "length_scale": ell, "nu": nu, "K": pack(kernel(X)),
                              "lml": float(gpr.log_marginal_likelihood(gpr.kernel_.theta)), "mean": pack(mean),
                              "var": pack(std ** 2)})
        print(f"nu = {nu}: lml {out['models'][-1]['lml']}")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sklearn_matern_nu.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
