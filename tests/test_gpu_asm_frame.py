"""The frame of the assembly kernels (csrc/asm_frame.h): the tile clip, the store tails and the rule that Sigma_y enters with a
pair's first launch, for every term class (tools/assembly_bits.py: classes) on blocks of 129, 1, 128 and 70 points -- pairs that
begin at rows 129, 130 and 258, share tiles and sit at odd and even offsets.  No formula is needed: the same entries reached
through different tiles, offsets and store branches carry the same bits.  N = 328 throughout."""
import functools
import os
import sys

import numpy as np
import pytest

import deriv_np as dn
import kprod_np as kn
import stheno_jl_amd as P
from stheno_jl_amd import lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import assembly_bits as ab  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUT = (129, 1, 128, 70)
N, TILE = sum(LAYOUT), 128
OFF = np.concatenate([[0], np.cumsum(LAYOUT)])
EPS = 2.0 ** -53
NAMES = ["plain D=1", "plain D=3", "plain D=17 three terms", "plain D=70 two terms", "plain then chain", "chain first", "stencil",
         "patch", "derivative", "derivative after plain", "no terms"]
# a diagonal pair of more than one launch: the evaluator of the class and the bound of the class's own test
# (tests/test_gpu_kprod.py: rel <= 1e-13; tests/test_gpu_deriv.py: 64 eps of the largest entry)
EVALUATOR = {"plain D=17 three terms": (kn.np_spec_matrix, 1e-13), "plain D=70 two terms": (kn.np_spec_matrix, 1e-13),
             "plain then chain": (kn.np_spec_matrix, 1e-13), "derivative after plain": (dn.dense_from_spec, 64 * EPS)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, its four inputs, prior_cov(F, x), the same matrix assembled as a cross-covariance -- every pair computed, none
    mirrored --, launches of a diagonal pair); the two matrices computed once and read-only"""
    F, procs, D, launches = ab.classes(P)[name]
    ins = ab.blocks(P, procs, D, LAYOUT, seed=7)
    K = P.prior_cov(F, P.BlockData(ins))
    Kd = P.prior_cov(F, P.BlockData(ins), P.BlockData(ins))
    K.setflags(write=False)
    Kd.setflags(write=False)
    return F, ins, K, Kd, launches


def test_the_class_table_is_the_one_listed_here():
    assert sorted(ab.classes(P)) == sorted(NAMES)
    assert all((ab.classes(P)[n][3] > 1) == (n in EVALUATOR) for n in NAMES)


# classes whose entry is a sum that is not symmetric under swapping its two sides bit for bit (the stencil's and the patches'
# double sums run over the row side's points outermost; derivative terms after a plain term are added in another order in the
# transposed pair).  The full matrix of a symmetric spec is assembled in its lower tiles and mirrored, so above the diagonal
# it holds the transposed pair's bits, and a standalone block computes its own: there only the entries the full matrix
# computed itself (row >= column) can be compared.  The parent commit answers alike (profiles/r25_asm_frame_bits.txt: 30
# blocks with I <= J of these three classes differ from the mirror, none with I > J, the same on both builds).  Every class,
# these three included, is held in full on the matrix assembled as a cross-covariance, where all sixteen pairs are launched.
MIRROR_DIFFERS = {"stencil", "patch", "derivative after plain"}


@pytest.mark.parametrize("name", NAMES)
def test_slices_of_the_full_matrix_equal_the_standalone_pairs(name):
    F, ins, K, Kd, _ = case(name)
    assert K.shape == Kd.shape == (N, N) and np.array_equal(K, K.T)
    computed = np.arange(N)[:, None] >= np.arange(N)[None, :]
    assert np.array_equal(K[computed], Kd[computed])
    for I in range(4):
        for J in range(4):
            Kc = P.prior_cov(F, ins[I], ins[J])
            rows, cols = slice(OFF[I], OFF[I + 1]), slice(OFF[J], OFF[J + 1])
            m = computed[rows, cols] if name in MIRROR_DIFFERS else np.ones(Kc.shape, dtype=bool)
            assert np.array_equal(Kc[m], K[rows, cols][m]), (name, I, J)
            assert np.array_equal(Kc, Kd[rows, cols]), (name, I, J, "cross-covariance")


def _assemble_lower(F, ins, noise):
    """sgp_dev_assemble_cols as stheno.jl_amd/dist.py calls it (lower tiles only, Sigma_y, padding) into a matrix of NaN:
    every column at once (c0 = 0, nc = n_pad)"""
    import torch
    from stheno_jl_amd import dist
    spec, _, _ = P.build_spec(F, P.BlockData(ins))
    ops = dist.HipOps()
    n_pad, m_tot = dist.geometry(N, 0)
    assert n_pad == m_tot == 384
    with ops.stream_context():
        ds = ops.make_dspec(spec)
        try:
            A = torch.full((n_pad * n_pad,), float("nan"), dtype=torch.float64, device=ops.device)
            host = np.array([noise], dtype=np.float64) if np.ndim(noise) == 0 else None
            dev = None if host is not None else ops.from_host(noise)
            rc = ops.lib.sgp_dev_assemble_cols(ops.ctx.handle, ds, N, 0, n_pad, A.data_ptr(), n_pad, m_tot, None,
                                               L.NOISE_SCALAR if dev is None else L.NOISE_DIAG,
                                               L.dptr(host) if host is not None else None,
                                               dev.data_ptr() if dev is not None else None, None, N, 0, ops.stream())
            L.check(rc, "sgp_dev_assemble_cols")
            out = ops.to_host(A).reshape(n_pad, n_pad).T       # element (r, c) sits at r + c * ld
        finally:
            ops.free_dspec(ds)
    return out, spec


@pytest.mark.parametrize("noise", ["scalar", "diag"])
@pytest.mark.parametrize("name", NAMES)
def test_lower_only_assembly_with_noise_through_every_class_as_first_launch(name, noise):
    F, ins, K, Kd, launches = case(name)
    nz = np.full(N, 0.3) if noise == "scalar" else 0.1 + np.random.default_rng(5).random(N)
    A, spec = _assemble_lower(F, ins, 0.3 if noise == "scalar" else nz)
    tr, tc = np.divmod(np.arange(384), TILE)[0][:, None], np.divmod(np.arange(384), TILE)[0][None, :]
    # tiles above the diagonal: the assembly never touches them.  (The padding does: with c0 = 0 the identity columns
    # N .. n_pad are filled from row c0 = 0 on, launch_fill_pad; they belong to no block pair and are checked as what they are.)
    assert np.all(np.isnan(A[:, :N][np.broadcast_to(tr < tc, A.shape)[:, :N]]))
    assert np.array_equal(A[:, N:], np.eye(384)[:, N:]) and np.array_equal(A[N:, :N], np.zeros((384 - N, N)))
    A = A[:N, :N]
    low = np.tril(np.ones((N, N), dtype=bool), -1)
    assert np.array_equal(A[low], K[low])
    # above the diagonal inside a diagonal tile only the pairs with I >= J write (the factorisation never reads there): an
    # entry is untouched or the value computed at its own place, which the cross-covariance assembly holds
    up = np.triu(np.ones((N, N), dtype=bool), 1) & (tr == tc)[:N, :N]
    assert np.all(np.isnan(A[up]) | (A[up] == Kd[up]))
    blk = np.searchsorted(OFF, np.arange(N), "right")                       # the block of every point
    assert np.array_equal(np.isnan(A[up]), (blk[:, None] < blk[None, :])[up])
    if launches == 1:     # Sigma_y is added to the finished sum: the same float64 addition
        assert np.array_equal(np.diag(A), np.diag(K) + nz)
    else:                 # the first launch carries Sigma_y, the later ones add onto it: another order of the same sum
        evaluator, bound = EVALUATOR[name]
        ref = np.diag(evaluator(spec)) + nz
        err = np.max(np.abs(np.diag(A) - ref)) / np.max(np.abs(ref))
        print(f"\n{name} {noise}: diagonal against the evaluator, rel = {err:.3g} (bound {bound:.3g})")
        assert err <= bound
