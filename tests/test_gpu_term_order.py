"""The order in which a caller lists the terms of a block pair does not reach the device: dspec_create sorts every pair's terms
by class with a stable pass (plain | patch | stencil | chains; stheno.jl_amd/csrc/spec_segments.h), and every per-term result
goes back through term_src.  So two specs whose pairs list the SAME terms, one interleaving the classes (stencil, plain, patch,
plain, stencil), the other already sorted, must return the same bits, entry by entry, once the per-term outputs are matched by
term.  No tolerance anywhere: np.array_equal.  A term whose result is routed to the wrong entry, or whose launch takes another
class's place in the stream, shows here.

What each call covers (the stencil family, include/sthenomi_stencil_grad.h, carries plain, patch and stencil terms; it takes no
row / column scale tables, so there are no scale vectors to compare here):
  * sgp_logpdf_grad_stencil: a symmetric spec of two blocks of 70 and 75 points (N = 145: the second block starts off the 64-row
    alignment, the matrix crosses a 128 tile); both off-diagonal pairs hold all five terms, the diagonal pairs a plain and a
    stencil term; grad_inputs for every input that holds points.  Value, y, mean, noise, grad_coef, grad_inscale, every input.
  * sgp_elbo_grad_stencil: zz of M = 37 inducing points (plain and stencil terms interleaved), xz of 145 x 37 with all five
    terms in both pairs, the one-sided patch term once with the images on the row side and once on the column side; grad_inputs
    of both specs.  Value, y, mean, noise, var_x, z_noise, the four per-term vectors, every input of zz and of xz.
  * sgp_kernelmatrix_diag_grad_stencil: a cross spec whose two diagonal pairs hold all five terms, every stencil and plain term
    reading two different inputs (so that its point gradient does not cancel); the entries of both sides of the one-sided patch
    terms are NULL, as that entry point asks.  grad_coef, grad_inscale, every input.
D = 2 for the plain and stencil terms, 4 x 4 images with 2 x 2 patches, a 2-point and a 3-point stencil on the two sides.
The chain class and the scale vectors come through include/sthenomi_kprod_grad.h, on chain + plain specs of the same two
blocks (a chain of two with function scales, a scaled plain term, a lone RQ term, a plain term, interleaved):
  * sgp_logpdf_grad_param_xs: value, y, mean, noise, grad_coef, grad_inscale, grad_param, both inputs, every row-scale vector.
  * sgp_kernelmatrix_diag_grad_param on a cross spec of two views: the three per-term vectors, the four inputs, every row- and
    every column-scale vector."""
import ctypes as C

import numpy as np
import pytest

import stheno_jl_amd as P

pytestmark = pytest.mark.gpu

L = P.lib
d = L.dptr
N0, N1, M, D = 70, 75, 37, 2
GEOM = (4, 4, 2, 2)
S2 = (np.array([[0.3, -0.2], [0.1, 0.25]]), np.array([0.6, -0.4]))                      # offsets D x Q, weights Q
S3 = (np.array([[0.15, -0.3, 0.05], [-0.1, 0.2, 0.35]]), np.array([0.5, 0.3, -0.2]))


def _points(rng, dim, n):
    return np.asfortranarray(0.7 * rng.standard_normal((dim, n)))


def _term(kind, ri, ci, coef, geoms=(None, None), stencils=(None, None), param=0.0, scales=(None, None), chain=False):
    """(the tuple lib.Spec takes, the two sides' patch geometries, their stencils, whether the term belongs to a product chain)"""
    return (kind, ri, ci, coef, param, *scales), geoms, stencils, chain


def _mixed(a, b, pa, pb, c, images_on_rows):
    """stencil, plain, patch, plain, stencil between the point inputs a (rows) and b (columns); pa / pb: the inputs of the
    one-sided patch term's two sides.  c scales every coefficient"""
    geoms = (GEOM, None) if images_on_rows else (None, GEOM)
    return [_term(L.SE, a, b, 1.0 * c, stencils=(S2, S3)), _term(L.MATERN52, a, b, 0.9 * c),
            _term(L.SE, pa, pb, 0.15 * c, geoms=geoms), _term(L.SE, a, b, 0.7 * c), _term(L.MATERN32, a, b, 0.8 * c, stencils=(None, S2))]


def _mirrored(terms):
    return [((k, ci, ri, coef, p, None, None), g[::-1], st[::-1], ch) for (k, ri, ci, coef, p, _, _), g, st, ch in terms]


def _two_orders(row_len, col_len, inputs, pairs, symmetric):
    """the spec as listed, the spec with every pair's terms sorted by class, and perm: the sorted spec's term j is the listed
    spec's term perm[j]"""
    cls = lambda t: 3 if t[3] else 1 if t[1] != (None, None) else 2 if t[2] != (None, None) else 0     # noqa: E731
    specs, perm, base = [], [], 0
    for I in range(len(row_len)):
        for J in range(len(col_len)):
            n = len(pairs.get((I, J), []))
            perm += [base + k for k in sorted(range(n), key=lambda k: cls(pairs[(I, J)][k]))]     # (sorted is stable)
            base += n
    for order in (False, True):
        ps = {key: sorted(v, key=cls) if order else v for key, v in pairs.items()}
        specs.append(L.Spec(row_len, col_len, inputs, {k: [t[0] for t in v] for k, v in ps.items()}, symmetric,
                            geoms={k: [t[1] for t in v] for k, v in ps.items()}, stencils={k: [t[2] for t in v] for k, v in ps.items()}))
    perm = np.asarray(perm)
    assert not np.array_equal(perm, np.arange(len(perm)))
    assert sorted(perm) == list(range(specs[0].n_terms))
    return specs[0], specs[1], perm


def _input_table(spec, skip):
    arrs = [np.zeros(a.shape, order="F") for a in spec.inputs]
    tab = (C.POINTER(C.c_double) * len(arrs))(*[None if k in skip else d(a) for k, a in enumerate(arrs)])
    return arrs, tab


def _same(a, b, what):
    assert np.all(np.isfinite(a)) and np.array_equal(a, b), what


def _own_results(spec, v):
    """every term of a pair has a non-zero result that no other term of its pair has: a mis-routed one would show (the mirror
    pair of a symmetric spec repeats its pair's sums)"""
    for p in range(len(spec._term_ptr) - 1):
        part = v[spec._term_ptr[p]:spec._term_ptr[p + 1]]
        assert np.all(part != 0) and len(set(part)) == len(part), (p, part)


def test_logpdf_gradient_is_the_same_bits_in_either_order():
    rng = np.random.default_rng(2301)
    inputs = [_points(rng, D, N0), _points(rng, D, N1), _points(rng, 16, N0), _points(rng, 4, N1)]     # 2: images, 3: patch-sized points
    low = _mixed(1, 0, 3, 2, 0.002, images_on_rows=False)      # pair (1, 0); entries <= 0.011, so K + I stays positive definite
    pairs = {(0, 0): [_term(L.MATERN52, 0, 0, 0.5, stencils=(S2, S2)), _term(L.SE, 0, 0, 1.0)],
             (1, 1): [_term(L.SE, 1, 1, 0.3, stencils=(S3, S3)), _term(L.MATERN32, 1, 1, 0.8)],
             (1, 0): low, (0, 1): _mirrored(low)}
    A, B, perm = _two_orders([N0, N1], [N0, N1], inputs, pairs, True)
    assert A.has_patch and A.has_stencil
    n = N0 + N1
    y, mean, noise = rng.standard_normal(n), 0.1 * rng.standard_normal(n), np.array([1.0])
    ctx = L.default_context()
    outs = []
    for spec in (A, B):
        o = dict(lp=np.zeros(1), gy=np.zeros(n), gm=np.zeros(n), gn=np.zeros(1), gc=np.zeros(spec.n_terms), gs=np.zeros(spec.n_terms))
        gx, tab = _input_table(spec, skip={2})
        rc = ctx.stencil_grad.sgp_logpdf_grad_stencil(ctx.handle, spec.ref(), d(mean), L.NOISE_SCALAR, d(noise), d(y), d(o["lp"]),
                                                      d(o["gy"]), d(o["gm"]), d(o["gn"]), d(o["gc"]), d(o["gs"]), tab)
        assert rc == 0, L.last_error()
        outs.append((o, gx))
    (a, ax), (b, bx) = outs
    for k in ("lp", "gy", "gm", "gn"):
        _same(a[k], b[k], k)
    _same(a["gc"][perm], b["gc"], "grad_coef")
    _same(a["gs"][perm], b["gs"], "grad_inscale")
    _own_results(A, a["gc"])
    for k in (0, 1, 3):
        _same(ax[k], bx[k], f"input {k}")
        assert np.abs(ax[k]).max() > 0


def test_elbo_gradient_is_the_same_bits_in_either_order():
    rng = np.random.default_rng(2302)
    z2, z4, zimg = _points(rng, D, M), _points(rng, 4, M), _points(rng, 16, M)
    zz_pairs = {(0, 0): [_term(L.SE, 0, 0, 0.4, stencils=(S2, S2)), _term(L.MATERN52, 0, 0, 1.0), _term(L.SE, 1, 1, 0.6),
                         _term(L.MATERN32, 0, 0, 0.3, stencils=(S3, S3))]}
    Az, Bz, pz = _two_orders([M], [M], [z2, z4], zz_pairs, True)
    x_inputs = [_points(rng, D, N0), _points(rng, D, N1), _points(rng, 16, N0), _points(rng, 4, N1), z2, z4, zimg]
    xz_pairs = {(0, 0): _mixed(0, 4, 2, 5, 1.0, images_on_rows=True), (1, 0): _mixed(1, 4, 3, 6, 0.8, images_on_rows=False)}
    Ax, Bx, px = _two_orders([N0, N1], [M], x_inputs, xz_pairs, False)
    assert Ax.has_patch and Ax.has_stencil and Az.has_stencil and not Az.has_patch
    n = N0 + N1
    y, mean_x, var_x = rng.standard_normal(n), 0.1 * rng.standard_normal(n), 2.0 + rng.random(n)
    noise_x, z_noise = 0.3 + 0.2 * rng.random(n), np.array([0.05])
    ctx = L.default_context()
    outs = []
    for zz, xz in ((Az, Ax), (Bz, Bx)):
        o = dict(elbo=np.zeros(1), gy=np.zeros(n), gm=np.zeros(n), gn=np.zeros(n), gv=np.zeros(n), gzn=np.zeros(1),
                 gcz=np.zeros(zz.n_terms), gsz=np.zeros(zz.n_terms), gcx=np.zeros(xz.n_terms), gsx=np.zeros(xz.n_terms))
        gz, tz = _input_table(zz, skip=())
        gx, tx = _input_table(xz, skip={2, 6})
        rc = ctx.stencil_grad.sgp_elbo_grad_stencil(ctx.handle, zz.ref(), xz.ref(), d(var_x), d(mean_x), L.NOISE_DIAG, d(noise_x),
                                                    L.NOISE_SCALAR, d(z_noise), d(y), d(o["elbo"]), d(o["gy"]), d(o["gm"]), d(o["gn"]),
                                                    d(o["gv"]), d(o["gzn"]), d(o["gcz"]), d(o["gsz"]), d(o["gcx"]), d(o["gsx"]), tz, tx)
        assert rc == 0, L.last_error()
        outs.append((o, gz, gx))
    (a, az, ax), (b, bz, bx) = outs
    for k in ("elbo", "gy", "gm", "gn", "gv", "gzn"):
        _same(a[k], b[k], k)
    for k, perm in (("gcz", pz), ("gsz", pz), ("gcx", px), ("gsx", px)):
        _same(a[k][perm], b[k], k)
        _own_results(Az if k.endswith("z") else Ax, a[k])
    for k in range(2):
        _same(az[k], bz[k], f"zz input {k}")
        assert np.abs(az[k]).max() > 0
    for k in (0, 1, 3, 4, 5):
        _same(ax[k], bx[k], f"xz input {k}")
        assert np.abs(ax[k]).max() > 0


def test_diagonal_gradient_is_the_same_bits_in_either_order():
    rng = np.random.default_rng(2303)
    inputs = [_points(rng, D, N0), _points(rng, D, N0), _points(rng, D, N1), _points(rng, D, N1),
              _points(rng, 16, N0), _points(rng, 4, N0), _points(rng, 16, N1), _points(rng, 4, N1)]
    pairs = {(0, 0): _mixed(0, 1, 4, 5, 1.0, images_on_rows=True), (1, 1): _mixed(2, 3, 7, 6, 0.8, images_on_rows=False)}
    A, B, perm = _two_orders([N0, N1], [N0, N1], inputs, pairs, False)
    assert A.has_patch and A.has_stencil
    w = rng.standard_normal(N0 + N1)
    ctx = L.default_context()
    outs = []
    for spec in (A, B):
        gc, gs = np.zeros(spec.n_terms), np.zeros(spec.n_terms)
        gx, tab = _input_table(spec, skip={4, 5, 6, 7})
        rc = ctx.stencil_grad.sgp_kernelmatrix_diag_grad_stencil(ctx.handle, spec.ref(), d(w), d(gc), d(gs), tab)
        assert rc == 0, L.last_error()
        outs.append((gc, gs, gx))
    (ac, as_, ax), (bc, bs, bx) = outs
    _same(ac[perm], bc, "grad_coef")
    _same(as_[perm], bs, "grad_inscale")
    _own_results(A, ac)
    for k in range(4):
        _same(ax[k], bx[k], f"input {k}")
        assert np.abs(ax[k]).max() > 0


# ---- the chain class and the scale vectors: sthenomi_kprod_grad.h -------------------------------------------------------------
def _chain_spec(rng, symmetric):
    """two blocks of 70 and 75 points, terms on the diagonal pairs alone: a chain of two factors with function scales, a plain
    term with function scales, a lone RQ term (a chain of one) and a plain term, interleaved.  symmetric: both sides of a term
    read one input and carry one scale vector; else a cross spec of two views, each side with a vector of its own"""
    ns = (N0, N1)
    inputs = [_points(rng, D, n) for n in ns] + ([] if symmetric else [_points(rng, D, n) for n in ns])
    pairs = {}
    for I, n in enumerate(ns):
        a, b = I, I if symmetric else I + 2
        s = [1.0 + 0.3 * rng.random(n) for _ in range(4)]
        sc = (lambda k: (s[k], s[k])) if symmetric else (lambda k: (s[k], s[k + 2]))
        head, cont = _term(L.SE, a, b, 0.9, scales=sc(0), chain=True), _term(L.MATERN32 | L.KIND_TIMES_PREV, a, b, 1.0, chain=True)
        scaled, rq, plain = _term(L.MATERN52, a, b, 0.6, scales=sc(1)), _term(L.RQ, a, b, 0.4, param=1.3, chain=True), _term(L.SE, a, b, 0.5)
        pairs[(I, I)] = [head, cont, scaled, rq, plain] if I == 0 else [plain, rq, scaled, head, cont]
    A, B, perm = _two_orders(ns, ns, inputs, pairs, symmetric)
    assert A.has_kprod and not A.has_stencil and not A.has_patch
    return A, B, perm


def _scale_table(spec, which):
    vecs = spec.term_row_scale if which == "row" else spec.term_col_scale
    arrs = [None if v is None else np.zeros(len(v)) for v in vecs]
    tab = (C.POINTER(C.c_double) * len(arrs))(*[d(a) for a in arrs])
    return arrs, tab


def _same_scales(a, b, perm, what):
    assert any(v is not None for v in a)
    for j, v in enumerate(b):
        assert (v is None) == (a[perm[j]] is None)
        if v is not None:
            _same(a[perm[j]], v, f"{what} of term {j}")
            assert np.abs(v).max() > 0


def test_chains_and_scale_vectors_through_the_logpdf_gradient():
    rng = np.random.default_rng(2304)
    A, B, perm = _chain_spec(rng, True)
    n = N0 + N1
    y, mean, noise = rng.standard_normal(n), 0.1 * rng.standard_normal(n), np.array([0.5])
    ctx = L.default_context()
    outs = []
    for spec in (A, B):
        o = dict(lp=np.zeros(1), gy=np.zeros(n), gm=np.zeros(n), gn=np.zeros(1), gc=np.zeros(spec.n_terms), gs=np.zeros(spec.n_terms),
                 gp=np.zeros(spec.n_terms))
        gx, tx = _input_table(spec, skip=())
        gr, tr = _scale_table(spec, "row")
        rc = ctx.kprod_grad.sgp_logpdf_grad_param_xs(ctx.handle, spec.ref(), d(mean), L.NOISE_SCALAR, d(noise), d(y), d(o["lp"]),
                                                     d(o["gy"]), d(o["gm"]), d(o["gn"]), d(o["gc"]), d(o["gs"]), d(o["gp"]), tx, tr)
        assert rc == 0, L.last_error()
        outs.append((o, gx, gr))
    (a, ax, ar), (b, bx, br) = outs
    for k in ("lp", "gy", "gm", "gn"):
        _same(a[k], b[k], k)
    for k in ("gc", "gs", "gp"):
        _same(a[k][perm], b[k], k)
    _own_results(A, a["gs"])          # (grad_coef of a continuation is 0: the head carries the chain's coefficient)
    for k in range(2):
        _same(ax[k], bx[k], f"input {k}")
        assert np.abs(ax[k]).max() > 0
    _same_scales(ar, br, perm, "row scale")


def test_chains_and_scale_vectors_through_the_diagonal_gradient():
    rng = np.random.default_rng(2305)
    A, B, perm = _chain_spec(rng, False)
    w = rng.standard_normal(N0 + N1)
    ctx = L.default_context()
    outs = []
    for spec in (A, B):
        o = dict(gc=np.zeros(spec.n_terms), gs=np.zeros(spec.n_terms), gp=np.zeros(spec.n_terms))
        gx, tx = _input_table(spec, skip=())
        (gr, tr), (gcs, tc) = _scale_table(spec, "row"), _scale_table(spec, "col")
        rc = ctx.kprod_grad.sgp_kernelmatrix_diag_grad_param(ctx.handle, spec.ref(), d(w), d(o["gc"]), d(o["gs"]), d(o["gp"]), tx, tr, tc)
        assert rc == 0, L.last_error()
        outs.append((o, gx, gr, gcs))
    (a, ax, ar, ac), (b, bx, br, bc) = outs
    for k in ("gc", "gs", "gp"):
        _same(a[k][perm], b[k], k)
    _own_results(A, a["gs"])          # (grad_coef of a continuation is 0: the head carries the chain's coefficient)
    for k in range(4):
        _same(ax[k], bx[k], f"input {k}")
        assert np.abs(ax[k]).max() > 0
    _same_scales(ar, br, perm, "row scale")
    _same_scales(ac, bc, perm, "column scale")
