"""The NumPy mirror of the NeuralNetwork, FBM and Exponentiated kinds (tests/dotkinds_np.py, the library's formulation)
against the 60-digit table under the error models of tests/dotkinds_truth.py, without a GPU: the check that the models are
satisfiable, and that the table tells the library's NEURALNET formulation from the textbook one."""
import numpy as np
import pytest

import dotkinds_np as dk
import dotkinds_truth as dt
from stheno_jl_amd import lib as L

CODE = {"nn": L.NEURALNET, "fbm": L.FBM, "exp": L.EXPONENTIATED}


def mirror(kind, g):
    """the mirror's k, dg, dp, dx, dy on the group's pairs (pair i: column i of X with column i of Y)"""
    out = {n: np.zeros(g.n) for n in ("k", "dg", "dp")}
    out["dx"], out["dy"] = np.zeros((g.D, g.n)), np.zeros((g.D, g.n))
    for i in range(g.n):
        x, y = g.X[:, i:i + 1], g.Y[:, i:i + 1]
        r = dk.derivs(CODE[kind], x, y, g.h if g.h is not None else 0.0)
        out["k"][i], out["dg"][i], out["dp"][i] = (np.asarray(r[n]).reshape(-1)[0] for n in ("k", "dk", "dp"))
        dX, dY = dk.point_derivs(CODE[kind], x, y, g.h if g.h is not None else 0.0)
        out["dx"][:, i], out["dy"][:, i] = dX[:, 0, 0], dY[:, 0, 0]
    return out


def _groups():
    T = dt.load()
    return [(key, D) for key in T for D in T[key]]


@pytest.mark.parametrize("key,D", _groups(), ids=lambda v: str(v).replace(" ", ""))
def test_mirror_stays_within_the_model(key, D):
    g = dt.load()[key][D]
    kind = key if isinstance(key, str) else key[0]
    got, tol = mirror(kind, g), dt.tolerances(kind, g)
    print(f"\n{key} D={D} ({g.n} pairs): largest error as a fraction of the bound: " +
          ", ".join(f"{n} {dt.worst(got[n], g.truth[n], tol[n]):.3f}" for n in ("k", "dg", "dp", "dx", "dy")))
    for n in ("k", "dg", "dp", "dx", "dy"):
        bad = dt.violations(got[n], g.truth[n], tol[n])
        assert bad.size == 0, (key, D, n, bad[:6], np.ravel(got[n])[bad[:6]], np.ravel(g.truth[n])[bad[:6]], np.ravel(tol[n])[bad[:6]])


def test_table_covers_the_grid():
    T = dt.load()
    assert sorted(T["nn"]) == [1, 2, 3, 8, 16]
    for D, g in T["nn"].items():
        cats = set(g.cat)
        assert {"random", "parallel", "antiparallel", "equal", "origin", "onecoord"} <= cats, (D, cats)
        norms = np.sqrt(np.sum(g.X ** 2, 0))
        assert norms[norms > 0].min() <= 1e-7 and norms.max() >= 1e5
        eq = g.is_cat("equal")
        assert np.array_equal(g.X[:, eq], g.Y[:, eq])
    s = np.concatenate([np.sum(g.X * g.Y, 0) for g in T["exp"].values()])
    assert s.min() < -699.0 and s.max() > 699.0 and np.all(np.abs(s) <= 709.0)


@pytest.mark.parametrize("h", dt.HS)
def test_fbm_zero_base_rule_is_exact(h):
    """exactly a^h on the diagonal, exactly 0 against the origin, with exact-zero derivative terms"""
    for D, g in dt.load()[("fbm", h)].items():
        got = mirror("fbm", g)
        eq, org = g.is_cat("equal"), g.is_cat("origin")
        a = np.sum(g.X * g.X, 0)
        assert np.array_equal(got["k"][eq], dk._pow0(dk.scalars(g.X[:, eq], g.X[:, eq])[1][:, 0], h)), D
        assert np.all(got["k"][org] == 0.0) and np.all(g.truth["k"][org] == 0.0) and np.all(got["dg"][org] == 0.0)
        assert not any(np.any(np.isnan(v)) for v in got.values())
        both = org & (a == 0.0) & (np.sum(g.Y * g.Y, 0) == 0.0)
        assert np.all(got["dp"][both] == 0.0) and np.all(got["dx"][:, both] == 0.0)


def test_textbook_asin_fails_the_model_on_nearly_parallel_points():
    """the table tells the two formulations apart: asin(s / sqrt((1 + a)(1 + b))) breaks the NEURALNET bound on the nearly
    parallel rows at large norms, at every D > 1, and the library's formulation does not"""
    failed = 0
    for D, g in dt.load()["nn"].items():
        tol = dt.tolerances("nn", g)["k"]
        text = np.array([dk.neuralnet_textbook(g.X[:, i:i + 1], g.Y[:, i:i + 1])[0, 0] for i in range(g.n)])
        par = g.is_cat("parallel") | g.is_cat("equal") | g.is_cat("antiparallel")
        big = np.sqrt(np.sum(g.X ** 2, 0)) >= 1e3
        bad = dt.violations(text, g.truth["k"], tol)
        assert len(set(bad) & set(np.flatnonzero(par & big))) >= 1, (D, dt.worst(text[par & big], g.truth["k"][par & big], tol[par & big]))
        failed += bad.size
    print(f"\ntextbook asin: {failed} nearly parallel pairs beyond the bound")
