"""The gradient kernels of chains that hold the NeuralNetwork, FBM and Exponentiated kinds (csrc/kprod.hip: the mode-2
instantiations of grad_kprod_kernel and grad_kprod_inputs_kernel) against an extended-precision truth
(tests/dotkinds_grad_truth.py), through the host mirror (P.logpdf_and_gradient_param, P.elbo_and_gradient_param with
inputs=True).

Each case asserts the value, y, mean, noise, every term's d_coef / d_inscale / d_param and every entry of every input
gradient.  Errors are counted in eps = 2^-53 times a scale taken from the truth; the bound of a case and output family is
MARGIN * max(e_float64 of the case, the family's floor), e_float64 the larger of the column-order and the blocked-order float64
run of the same restatement and the floors the medians written down in that module: both come from the reference, never from
the device."""
import numpy as np
import pytest

import dotkinds_grad_truth as DG
import kprod_grad_truth as KT
import stheno_jl_amd as P
from test_gpu_kprod_grad_truth import _elbo_outputs, _finite, _logpdf_outputs

pytestmark = pytest.mark.gpu


def hold(case, dev, f64):
    """every family's figure inside MARGIN * max(float64 figure, floor); figures printed first"""
    for fam in sorted(dev):
        print(f"{case[0]:18s} {fam:16s} device {dev[fam]:10.1f}  float64 {f64[fam]:10.1f}  floor {DG.FLOORS[fam]:8.1f}")
    bad = {fam: (dev[fam], f64[fam]) for fam in dev if not dev[fam] <= DG.MARGIN * max(f64[fam], DG.FLOORS[fam])}
    assert not bad, (case[0], bad)


@pytest.mark.parametrize("case", [c for c in DG.CASES if c[1] == "lp"], ids=lambda c: c[0])
def test_logpdf_gradient_against_truth(case):
    F, x, _, noise, y = DG.problem(case)
    g = P.logpdf_and_gradient_param(F(x, noise), y, inputs=True, scales=True)
    R = DG.truth(case)[0]
    out = _logpdf_outputs(g)
    assert g["_spec"].has_kprod and g["_spec"].n_terms == len(R["d_coef"])
    _finite([out["value"], out["y"], out["mean"], out["noise"], out["d_coef"], out["d_inscale"], out["d_param"]] + list(out["gx"]))
    hold(case, DG.logpdf_units(out, R), DG.reference_figures(case))


@pytest.mark.parametrize("case", [c for c in DG.CASES if c[1] == "elbo"], ids=lambda c: c[0])
def test_elbo_gradient_against_truth(case):
    F, x, z, noise, y = DG.problem(case)
    g = P.elbo_and_gradient_param(P.VFE(F(z, 1e-2)), F(x, noise), y, inputs=True, scales=True)
    R = DG.truth(case)[0]
    out = _elbo_outputs(g)
    assert all(sp.has_kprod for sp in g["_specs"].values())
    flat = [out["value"], out["y"], out["mean"], out["noise"], out["z_noise"], out["var"]]
    for key in ("zz", "xz"):
        flat += [out[key]["d_coef"], out[key]["d_inscale"], out[key]["d_param"]] + list(out[key]["gx"])
    _finite(flat)
    assert np.max(np.abs(out["var"] - R["var"]) / np.abs(R["var"])) <= 2 * KT.EPS      # -1 / (2 sy): one division
    hold(case, KT.elbo_units(out, R), DG.reference_figures(case))
