"""Gradients with respect to a stencil's weights and offsets without a GPU: the truth (tests/stencil_wo_truth.py) against
long-double central differences of its own value, the float64 yardstick of every case and the floors recorded from it, the
host chain from the library's stencils back to the model's stencil nodes (logpdf_and_gradient_stencil /
elbo_and_gradient_stencil with stencils=True over the NumPy double tests/stencil_wo_np.py) against central differences of
P.logpdf / P.elbo, the refusals of the host, and the extension header include/sthenomi_stencil_wo.h (plain C, exactly what
libsthenomi_stencil_wo.so exports and lib.py types; libsthenomi_stencil_grad.so keeps its three names).

`python tests/test_stencil_wo_on_numpy.py` prints the float64 figures of every case and family: the lists recorded in
stencil_wo_truth.MEASURED_FLOAT64."""
import os
import subprocess

import numpy as np
import pytest

if __name__ == "__main__":
    import conftest  # noqa: F401  (registers the product package, as under pytest)

import grad_truth as T
import stencil_grad_truth as ST
import stencil_wo_np
import stencil_wo_truth as WT
import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the truth against central differences of its own value ---------------------------------------------------------------
@pytest.mark.parametrize("diagonal", [False, True], ids=["matrix", "diagonal"])
@pytest.mark.parametrize("kind", [T.SE, T.MATERN32, T.MATERN52], ids=["se", "m32", "m52"])
def test_truth_against_long_double_central_differences(kind, diagonal):
    """value = sum_ij W_ij sum_pq w_p v_q k(d2_pq), differenced in every weight and every offset coordinate of both sides
    with h = 2^-20 in long double: the error model is h^2 (third derivative) plus eps_longdouble / h, both far below 1e-8 of
    the output's absolute-sum scale"""
    dt = T.require_extended()
    rng = np.random.default_rng(21 + kind)
    D, nr, nc = 2, 6, 6 if diagonal else 4
    X, Y = rng.standard_normal((D, nr)), rng.standard_normal((D, nc))
    rst = (0.4 * rng.standard_normal((D, 3)), rng.standard_normal(3))
    cst = (0.4 * rng.standard_normal((D, 2)), rng.standard_normal(2))
    Wm = rng.standard_normal(nr if diagonal else (nr, nc)).astype(dt)
    h = dt(2.0) ** -20

    def value(rs, cs):
        return WT.term_sums(kind, 1.0, X, Y, rs, cs, Wm, dt, diagonal=diagonal, shift_dt=dt)[0]

    _, sides = WT.term_sums(kind, 1.0, X, Y, rst, cst, Wm, dt, diagonal=diagonal, shift_dt=dt)
    worst = 0.0
    for side, st in enumerate((rst, cst)):
        A, w = st[0].astype(dt), st[1].astype(dt)
        for key, arr in (("w", w), ("o", A)):
            for idx in np.ndindex(arr.shape):
                ap, an = arr.copy(), arr.copy()
                ap[idx] += h
                an[idx] -= h
                sts = [list(rst), list(cst)]
                sts[side] = [A, w]
                sp, sn = [list(s) for s in sts], [list(s) for s in sts]
                sp[side][0 if key == "o" else 1], sn[side][0 if key == "o" else 1] = ap, an
                fd = (value(tuple(sp[0]), tuple(sp[1])) - value(tuple(sn[0]), tuple(sn[1]))) / (2 * h)
                got, scale = sides[side][key][idx], sides[side]["S_" + key][idx]
                worst = max(worst, float(abs(got - fd) / scale))
    print(f"kind {kind}, {'diagonal' if diagonal else 'matrix'}: truth and central difference differ by {worst:.2e} of the scale")
    assert worst <= 1e-8


# ---- 2. the yardstick and the floors --------------------------------------------------------------------------------------
def _figures(case, monkeypatch):
    """e_float64 of a case, family by family: the float64 runs of the truth code against its long-double run.  The specs
    come from the host mirror running on the NumPy double; the double's numbers are not looked at."""
    stencil_wo_np.install(monkeypatch)
    figs = {}
    if case.family == "lp":
        F, fx, y = case.build()
        spec = P.build_spec(F, fx.x)[0]
        R, *R64 = WT.logpdf_runs(case, spec, fx, y)
        figs["wo.lp.weights"], figs["wo.lp.offsets"] = WT.yardstick(R, R64)
    else:
        F, fz, fx, y = case.build()
        g = P.elbo_and_gradient_stencil(P.VFE(fz), fx, y)
        specs = g["_specs"]
        spec = specs["xx"]
        R, *R64 = WT.elbo_runs(case, specs, fz, fx, y, P.finite_gp._kernelmatrix_diag(spec))
        e = [WT.yardstick(R[k], [r[k] for r in R64]) for k in ("zz", "xz")]
        figs["wo.elbo.weights"], figs["wo.elbo.offsets"] = max(v[0] for v in e), max(v[1] for v in e)
    Rd, Rd64 = WT.diag_runs(case, spec, WT.diag_weights(case, spec.N))
    figs["wo.diag.weights"], figs["wo.diag.offsets"] = WT.yardstick(Rd, [Rd64])
    return figs


@pytest.mark.parametrize("case", WT.WO_CASES, ids=repr)
def test_float64_run_is_inside_its_bound(case, monkeypatch):
    for fam, e in _figures(case, monkeypatch).items():
        assert np.isfinite(e)
        assert e <= T.SELF_MARGIN * max(e, WT.FLOORS[fam]), (case.id, fam, e)
        # the recorded figure is this run's (to the printed digit and the last bits)
        assert any(abs(e - v) <= 0.05 + 0.25 * v for v in WT.MEASURED_FLOAT64[fam]), (case.id, fam, e)


def test_floors_are_the_medians_of_the_recorded_float64_figures():
    assert set(WT.FLOORS) == set(WT.MEASURED_FLOAT64) == set(WT.FAMILIES)
    for fam, vals in WT.MEASURED_FLOAT64.items():
        assert len(vals) == len(WT.LP_CASES if ".lp." in fam else WT.ELBO_CASES if ".elbo." in fam else WT.WO_CASES)
        assert WT.FLOORS[fam] == float(np.median(vals)), fam


def test_the_case_list_is_the_stencil_gradient_one_plus_the_kernels_own():
    assert WT.WO_CASES[:len(ST.CASES)] == ST.CASES and len(WT.EXTRA) == 2
    strips, wide = WT.EXTRA
    assert max(n for _, n in strips.blocks) == 150 and sum(n for _, n in strips.blocks) <= 300     # 2 strips of 128, 3 x 64 rows
    (Ag, _), (Ah, _) = wide.stencils()
    assert (Ag.shape[1], Ah.shape[1]) == (64, 1)


# ---- 3. the host chain over the double, against central differences -------------------------------------------------------
H = 1e-4
S2 = 0.15
A0, W0 = np.array([[0.0, 0.1, -0.25], [0.0, -0.05, 0.1]]), np.array([-0.6, 1.0, -0.3])
B0, V0 = np.array([[0.05, -0.1], [0.2, 0.0]]), np.array([0.7, 0.5])
LMAT = np.array([[0.8, 0.3], [-0.2, 1.1]])


def _f(GP):
    return GP(1.3 * P.with_lengthscale(P.Matern52Kernel(), 0.9))


def m_direct(GP, st):
    g = P.stencil(_f(GP), *st["a"])
    return {"g": g}, {"a": g}


def m_stretch(GP, st):
    f = _f(GP)
    g1, g2 = P.stencil(P.stretch(f, 0.7), *st["a"]), P.stencil(P.stretch(f, LMAT), *st["b"])
    return {"g": g1, "h": g2}, {"a": g1, "b": g2}


def m_select(GP, st):
    g = P.stencil(P.select(_f(GP), [1]), *st["a"])
    return {"g": g}, {"a": g}


def m_nested(GP, st):
    inner = P.stencil(_f(GP), *st["b"])
    g = P.stencil(P.stretch(inner, 0.7), *st["a"])
    return {"g": g}, {"a": g, "b": inner}


def m_twice(GP, st):
    f = _f(GP)
    s = P.stencil(f, *st["a"])
    u = GP(0.4 * P.SEKernel())
    return {"g": s + 2 * (0.5 * s + u)}, {"a": s}


def m_sum_kernel(GP, st):
    f = GP(1.3 * P.with_lengthscale(P.SEKernel(), 0.9) + 0.4 * P.with_lengthscale(P.Matern52Kernel(), 1.3))
    g = P.stencil(f, *st["a"])
    return {"g": g}, {"a": g}


MODELS = {
    "direct": (m_direct, ["g"]), "stretch": (m_stretch, ["g", "h"]), "select": (m_select, ["g"]),
    "nested": (m_nested, ["g"]), "twice": (m_twice, ["g"]), "sum-kernel": (m_sum_kernel, ["g"]),
    "two-blocks": (m_direct, ["g", "g"]),
}
ST0 = {"a": (A0, W0), "b": (B0, V0)}


def _build(builder, st):
    nodes = {}

    def build(GP):
        procs, found = builder(GP, st)
        nodes.update(found)
        return procs
    return P.gppp(build), nodes


def _rounding(value, kappa):
    """what the rounding of the four values of a difference below can put into it: the differences are Richardson-extrapolated,
    (4 D(H) - D(2 H)) / 3 with D the central difference, so the values enter with the weights 4/3 and 1/6 over H: at most
    2 err(f) / H, and a value that comes out of solves with a matrix of condition number kappa carries err(f) = eps kappa |f|"""
    return 2.0 * 2.0 ** -52 * kappa * abs(value) / H


def _check_chain(value_of, nodes_of, g, rounding):
    """every entry of every node's d_offsets / d_weights against the extrapolated central difference of value_of(stencils).
    The tolerance of an entry is the difference's own error: 2 * rounding, plus the size of the extrapolation's correction
    |D* - D(H)| -- the H^2 term it removed, which stands (generously) for the H^4 term it left.  Both come from the reference
    side alone.  Returns the largest error / tolerance."""
    used = sorted(nodes_of)
    by_id = {id(e["node"]): e for e in g["stencils"]}
    assert sorted(by_id) == sorted(id(nodes_of[k]) for k in used) and len(g["stencils"]) == len(used)
    need = 0.0
    for name in used:
        e = by_id[id(nodes_of[name])]
        A, w = ST0[name]
        assert e["d_offsets"].shape == A.shape and e["d_weights"].shape == w.shape
        for key, arr, got in (("o", A, e["d_offsets"]), ("w", w, e["d_weights"])):
            for idx in np.ndindex(arr.shape):
                vals = []
                for step in (+H, -H, +2 * H, -2 * H):
                    a2 = arr.copy()
                    a2[idx] += step
                    vals.append(value_of(dict(ST0, **{name: (a2, w) if key == "o" else (A, a2)})))
                d1, d2 = (vals[0] - vals[1]) / (2 * H), (vals[2] - vals[3]) / (4 * H)
                fd = (4.0 * d1 - d2) / 3.0
                need = max(need, abs(got[idx] - fd) / (2 * rounding + abs(fd - d1)))
    return need


@pytest.mark.parametrize("name", sorted(MODELS))
def test_host_chain_matches_central_differences_of_logpdf(name, monkeypatch):
    stencil_wo_np.install(monkeypatch)
    builder, blocks = MODELS[name]
    rng = np.random.default_rng(40 + len(name))
    Xs = [np.asfortranarray(rng.standard_normal((2, n))) for n in (7, 5)[:len(blocks)]]
    y = rng.standard_normal(sum(X.shape[1] for X in Xs))

    def fx_of(st):
        F, nodes = _build(builder, st)
        xs = [P.GPPPInput(b, P.ColVecs(X)) for b, X in zip(blocks, Xs)]
        return F(xs[0] if len(xs) == 1 else P.BlockData(xs), S2), nodes

    fx, nodes = fx_of(ST0)
    g = P.logpdf_and_gradient_stencil(fx, y, inputs=True, stencils=True)
    plain = P.logpdf_and_gradient_stencil(fx, y, inputs=True)
    assert "stencils" not in plain and g["logpdf"] == plain["logpdf"] and np.array_equal(g["x"][0], plain["x"][0])
    assert all(np.array_equal(p, q) for p, q in zip(g["_raw"], plain["_raw"]))
    assert abs(g["logpdf"] - P.logpdf(fx, y)) <= 1e-12 * abs(g["logpdf"])
    for r in g["terms"]:
        if r.get("row_stencil") is not None:
            assert r["d_row_weights"].shape == r["row_stencil"][1].shape and r["d_row_offsets"].shape == r["row_stencil"][0].shape
        elif r.get("col_stencil") is not None:
            assert r["d_row_weights"] is None and r["d_row_offsets"] is None and r["d_col_weights"] is not None
        else:
            assert "d_row_weights" not in r
    # the condition number of K + s2 I is at most 1 + trace(K) / s2
    kappa = 1.0 + P.finite_gp._kernelmatrix_diag(g["_spec"]).sum() / S2
    need = _check_chain(lambda st: P.logpdf(fx_of(st)[0], y), nodes, g, _rounding(g["logpdf"], kappa))
    print(f"{name}: offsets and weights of {len(nodes)} node(s) are at {need:.3f} of the difference's own error (kappa <= {kappa:.0f})")
    assert need <= 1.0


@pytest.mark.parametrize("zname", ["f", "g"])
def test_host_chain_matches_central_differences_of_the_elbo(zname, monkeypatch):
    """data at g = stencil(stretch(f, 0.7), A, w), inducing points at f, then at g itself: the node is read by K(z,z) (z in
    g), K(x,z) and diag K(x,x)"""
    stencil_wo_np.install(monkeypatch)
    rng = np.random.default_rng(50)
    X, Z = np.asfortranarray(rng.standard_normal((2, 8))), np.asfortranarray(rng.standard_normal((2, 3)))
    y = rng.standard_normal(8)

    def builder(GP, st):
        f = _f(GP)
        g = P.stencil(P.stretch(f, 0.7), *st["a"])
        return {"f": f, "g": g}, {"a": g}

    def pair_of(st):
        F, nodes = _build(builder, st)
        return P.VFE(F(P.GPPPInput(zname, P.ColVecs(Z)), 1e-3)), F(P.GPPPInput("g", P.ColVecs(X)), S2), nodes

    vfe, fx, nodes = pair_of(ST0)
    g = P.elbo_and_gradient_stencil(vfe, fx, y, inputs=True, stencils=True)
    plain = P.elbo_and_gradient_stencil(vfe, fx, y, inputs=True)
    assert "stencils" not in plain and g["elbo"] == plain["elbo"]
    assert all(np.array_equal(p, q) for k in ("zz", "xz", "xx") for p, q in zip(g["_raw"][k], plain["_raw"][k]))
    assert g["xz_terms"][0]["d_row_weights"].shape == (3,) and g["xz_terms"][0]["d_row_offsets"].shape == (2, 3)
    assert (g["xz_terms"][0]["d_col_weights"] is None) == (zname == "f")
    # two solves: with Kzz + 1e-3 I (condition number at most 1 + trace / 1e-3) and with A A' + I (at most 1 + trace(Kxx) / s2)
    kappa = ((1.0 + P.finite_gp._kernelmatrix_diag(g["_specs"]["zz"]).sum() / 1e-3) *
             (1.0 + P.finite_gp._kernelmatrix_diag(g["_specs"]["xx"]).sum() / S2))
    need = _check_chain(lambda st: P.elbo(*pair_of(st)[:2], y), nodes, g, _rounding(g["elbo"], kappa))
    print(f"elbo, z in {zname}: offsets and weights are at {need:.3f} of the difference's own error (kappa <= {kappa:.0f})")
    assert need <= 1.0


# ---- 4. the keyword off, and the refusals of the host --------------------------------------------------------------------------
def test_without_the_keyword_the_old_entry_points_are_called(monkeypatch):
    ctx = stencil_wo_np.install(monkeypatch)

    def boom(*a):
        raise AssertionError("stencils=False must not reach libsthenomi_stencil_wo.so")
    for name in P.lib.stencil_wo_symbols():
        monkeypatch.setattr(ctx.lib, name, boom, raising=False)
    F, nodes = _build(m_direct, ST0)
    rng = np.random.default_rng(3)
    fx = F(P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 6))))), S2)
    z = F(P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 3))))), 1e-3)
    y = rng.standard_normal(6)
    g = P.logpdf_and_gradient_stencil(fx, y)
    assert sorted(g) == sorted(["logpdf", "y", "mean", "noise", "terms", "inputs", "x", "scales", "_raw", "_rowscale", "_spec"])
    assert not any(k.startswith("d_row_") or k.startswith("d_col_") for r in g["terms"] for k in r)
    assert "stencils" not in P.elbo_and_gradient_stencil(P.VFE(z), fx, y)
    with pytest.raises(AssertionError, match="must not reach"):
        P.logpdf_and_gradient_stencil(fx, y, stencils=True)


def test_refusals_of_the_host(monkeypatch):
    ctx = stencil_wo_np.install(monkeypatch)
    rng = np.random.default_rng(5)
    x = P.GPPPInput("g", P.ColVecs(np.asfortranarray(rng.standard_normal((2, 5)))))
    y = rng.standard_normal(5)
    # a multi-GPU context
    F, _ = _build(m_direct, ST0)
    ctx.is_multi = True
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        P.logpdf_and_gradient_stencil(F(x, S2), y, stencils=True)
    ctx.is_multi = False
    # two stencil views that cancel exactly: the term is gone, their stencils' gradient is not
    gone = P.gppp(lambda GP: (lambda f: {"g": P.stencil(f, A0, W0) - P.stencil(f, A0, W0) + f})(_f(GP)))
    assert P.logpdf_and_gradient_stencil(gone(x, S2), y)["logpdf"] < 0          # (fine without the keyword)
    with pytest.raises(NotImplementedError, match="cancel exactly"):
        P.logpdf_and_gradient_stencil(gone(x, S2), y, stencils=True)
    # a model without stencil nodes: an empty list
    plain = P.gppp(lambda GP: {"g": _f(GP)})
    assert P.logpdf_and_gradient_stencil(plain(x, S2), y, stencils=True)["stencils"] == []
    # the double, as the library: a non-NULL entry for a plain side
    F2 = P.gppp(lambda GP: (lambda f: {"f": f, "g": P.stencil(f, A0, W0)})(_f(GP)))
    spec = P.build_spec(F2, x, None, P.GPPPInput("f", x.x))[0]
    d = P.lib.dptr
    bufs = [np.zeros(3), np.zeros(3), np.zeros((3, 2)), np.zeros((3, 2))]
    tab = lambda a, b: (P.lib.C.POINTER(P.lib.C.c_double) * 2)(d(a), d(b))       # noqa: E731
    rc = ctx.lib.sgp_kernelmatrix_diag_grad_stencil_wo(ctx.handle, spec.ref(), d(np.ones(5)), d(np.zeros(1)), d(np.zeros(1)),
                                                       None, tab(bufs[0], bufs[1]), None)
    assert rc < 0 and "plain side" in ctx.lib.sgp_last_error().decode()
    rc = ctx.lib.sgp_kernelmatrix_diag_grad_stencil_wo(ctx.handle, spec.ref(), d(np.ones(5)), d(np.zeros(1)), d(np.zeros(1)),
                                                       None, tab(bufs[0], None), tab(bufs[2], None))
    assert rc == 0 and np.any(bufs[0]) and np.any(bufs[2]) and not np.any(bufs[1])


# ---- 5. the extension header -------------------------------------------------------------------------------------------------
def test_stencil_wo_header_is_plain_c(tmp_path):
    src = tmp_path / "stencil_wo_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include "sthenomi_stencil_wo.h"
int main(void) {
  int (*a)(sgp_ctx*, const sgp_cov_spec*, const double*, int, const double*, const double*, double*, double*, double*,
           double*, double*, double*, double* const*, double* const*, double* const*) = &sgp_logpdf_grad_stencil_wo;
  int (*b)(sgp_ctx*, const sgp_cov_spec*, const double*, double*, double*, double* const*, double* const*, double* const*) =
      &sgp_kernelmatrix_diag_grad_stencil_wo;
  printf("%d %d %d\n", (int)sizeof(a), (int)sizeof(b), (int)sizeof(&sgp_elbo_grad_stencil_wo));
  return 0;
}
''')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "stencil_wo_consumer.o")])


def test_stencil_wo_library_exports_exactly_its_header():
    syms = _symbols_of("sthenomi_stencil_wo.h")
    assert syms == ["sgp_elbo_grad_stencil_wo", "sgp_kernelmatrix_diag_grad_stencil_wo", "sgp_logpdf_grad_stencil_wo"]
    assert syms == P.lib.stencil_wo_symbols()
    assert _c_exports(P.lib.STENCIL_WO_LIB_PATH) == syms
    # libsthenomi_stencil_grad.so keeps exporting exactly its three names
    assert _c_exports(P.lib.STENCIL_GRAD_LIB_PATH) == ["sgp_elbo_grad_stencil", "sgp_kernelmatrix_diag_grad_stencil",
                                                       "sgp_logpdf_grad_stencil"] == P.lib.stencil_grad_symbols()
    others = [P.lib.LIB_PATH, P.lib.CONV_LIB_PATH, P.lib.CONV_GRAD_LIB_PATH, P.lib.STENCIL_LIB_PATH, P.lib.STENCIL_GRAD_LIB_PATH,
              P.lib.KPROD_LIB_PATH, P.lib.KPROD_GRAD_LIB_PATH, P.lib.BATCH_LIB_PATH, P.lib.POOL_LIB_PATH, P.lib.EXTEND_LIB_PATH,
              P.lib.POSTFX_LIB_PATH, P.lib.VFE_UPDATE_LIB_PATH, P.lib.BENCH_LIB_PATH]
    for path in others:
        assert not set(syms) & set(_c_exports(path)), path
    for header in ("sthenomi.h", "sthenomi_stencil.h", "sthenomi_stencil_grad.h", "sthenomi_conv_grad.h", "sthenomi_kprod_grad.h"):
        assert not set(syms) & set(_symbols_of(header))
    # the signatures lib.py types: the _stencil ones plus the tables
    for name, extra in (("sgp_logpdf_grad_stencil", 2), ("sgp_kernelmatrix_diag_grad_stencil", 2), ("sgp_elbo_grad_stencil", 4)):
        old, new = P.lib._SIGS_STENCIL_GRAD[name][1], P.lib._SIGS_STENCIL_WO[name + "_wo"][1]
        assert new[:len(old)] == old and new[len(old):] == [P.lib._DD] * extra


if __name__ == "__main__":          # the measurement behind stencil_wo_truth.FLOORS / MEASURED_FLOAT64
    import pprint
    import time

    class _MP:
        def __init__(self):
            self.undo = []

        def setattr(self, obj, name, value):
            self.undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)

        def close(self):
            for obj, name, value in reversed(self.undo):
                setattr(obj, name, value)

    lists = {}
    for c in WT.WO_CASES:
        mp, t0 = _MP(), time.time()
        figs = _figures(c, mp)
        mp.close()
        for fam, e in figs.items():
            lists.setdefault(fam, []).append(round(e, 1))
            print(f"{c.id:22s} {fam:20s} {e:10.1f}", flush=True)
        print(f"{c.id:22s} truth and yardstick: {time.time() - t0:.1f} s", flush=True)
    lists = {k: sorted(v) for k, v in lists.items()}
    print("MEASURED_FLOAT64 = ", end="")
    pprint.pprint(lists, width=120, compact=True)
    print("FLOORS = ", end="")
    pprint.pprint({k: float(np.median(v)) for k, v in lists.items()}, width=120)
