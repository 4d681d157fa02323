"""grad_truth's outputs on a hand-written problem, long double and float64, every output: what tests/golden/grad_truth_pin.npz
holds (written by tests/golden/make_grad_truth_pin.py with the module as it was before logpdf_grad / elbo_grad learned to
take another spec's `dense`, `diag_of` and `contract`: tests/kprod_grad_truth.py).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import grad_truth as T

COEFS = (0.5, 0.4, 0.3, 0.2)


def _hand_spec(A, B, sym, rs=None, cs=None):
    terms = [(0, 0, kind, 0, 1, COEFS[kind], 0.0, rs if kind == 1 else None, cs if kind in (1, 2) else None)
             for kind in range(4)]
    terms.append((0, 0, T.CONST, 0, 1, 0.15, 0.7, None, None))
    return dict(terms=terms, inputs=[A, B], row_len=[A.shape[1]], col_len=[B.shape[1]], symmetric=sym)


def _flat(prefix, R, out):
    for key, v in R.items():
        if isinstance(v, dict):
            _flat(f"{prefix}.{key}", v, out)
        elif isinstance(v, (list, tuple)):
            for k, a in enumerate(v):
                if a is not None:
                    out[f"{prefix}.{key}.{k}"] = np.ascontiguousarray(a)
        elif v is not None and not isinstance(v, (int, bool)):
            out[f"{prefix}.{key}"] = np.ascontiguousarray(v)


def grad_truth_pin():
    rng = np.random.default_rng(73)
    D, n, m = 2, 14, 6
    X, Z = (rng.standard_normal((D, k)) for k in (n, m))
    y, mean = rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    noise = 0.05 + 0.25 * rng.random(n)
    sc = 1.0 + 0.3 * np.sin(X.sum(0))
    scz = 1.0 + 0.3 * np.sin(Z.sum(0))
    w = rng.standard_normal(n)
    out = {}
    for tag, dt in (("ld", T.require_extended()), ("f64", np.float64)):
        runs = {"lp": T.logpdf_grad(_hand_spec(X, X, True, sc, sc), T.NOISE_DIAG, noise, mean, y, dt, inputs=True, scales=True),
                "lps": T.logpdf_grad(_hand_spec(X, X, True), T.NOISE_SCALAR, 0.1, mean, y, dt),
                "elbo": T.elbo_grad(_hand_spec(Z, Z, True, scz, scz), _hand_spec(X, Z, False, sc, scz), _hand_spec(X, X, True, sc, sc),
                                    T.NOISE_DIAG, noise, T.NOISE_SCALAR, 1e-2, mean, y, dt, inputs=True),
                "diag": T.diag_grad(_hand_spec(X, X, True, sc, sc), w, dt)}
        for name, R in runs.items():
            _flat(f"{tag}.{name}", R, out)
    # a long double as two float64 (value and remainder: 106 bits hold its 64), so that no padding byte is compared
    pin = {}
    for k, v in out.items():
        v = np.asarray(v)
        if v.dtype == bool:
            pin[k] = v
            continue
        hi = v.astype(np.float64)
        pin[k] = np.stack([hi, (v - hi.astype(v.dtype)).astype(np.float64)])
    return pin
