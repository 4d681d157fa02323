"""Model flattener: a Stheno GP tree evaluated at (BlockData) inputs -> kernel terms per block
pair, i.e. the `sgp_cov_spec` the HIP library consumes (include/sthenomi.h).

The reference evaluates cov(f_i, f_j, x_I, x_J) by recursive dispatch on creation order
(/root/reference/src/gp/derived_gp.jl:31-44) through dense N x N' temporaries.  Covariance is
bilinear and distinct AtomicGPs are independent (src/gp/atomic_gp.jl:36-38), so the same
matrix is the *path expansion* of SURVEY.md Appendix B:

  paths(f, x) = [(atom, c, r, X)]   : f(x) = sum_p c_p * diag(r_p) * atom_p(X_p) (+ mean)
  K[I, J] = sum_{p in paths(I), q in paths(J), atom_p is atom_q}
                c_p c_q diag(r_p) k_atom(X_p, X_q) diag(r_q)

with  +            -> union of paths                 (addition.jl:20-47; known-function add :67-86)
      * real       -> c <- c * sigma                  (product.jl:54-70; -f = (-1) * f, :73)
      * function   -> r <- r .* sigma.(x)             (product.jl:25-48; x as seen at that node)
      o g          -> X <- g.(X)                      (compose.jl:16-28, fast warps :36-127)
      cross / GPPP -> one process per block           (cross.jl:54-93, gppp.jl:25-43)
      stencil      -> the path carries (offsets, weights): ONE term per pair of paths, the library sums the
                      shifted evaluations (include/sthenomi_stencil.h)
      derivative   -> the path carries a direction; a pair of paths gives one term of a derivative kind per pair of
                      non-zero direction components (include/sthenomi.h: SGP_DERIV_*)
and the leaf kernel expanded into SimpleKernel terms (ScaledKernel -> coefficient, KernelSum ->
several terms, ScaleTransform -> input scale, KernelProduct -> a chain of terms the library multiplies entry by
entry: include/sthenomi_kprod.h).  Block pairs without a common atom get no
terms, which the library writes as exact zeros (test/gp/atomic_gp.jl:33).
"""
from __future__ import annotations

import numpy as np

from . import gp as _gp
from . import kernels as _kernels
from . import lib as _lib
from .gppp import GPPP, extract_components
from .inputs import BlockData, ColVecs, GPPPInput, as_matrix, blocks, is_pair_vector, regroup_pairs


class _Path:
    __slots__ = ("key", "atom", "c", "r", "X", "chain", "geom", "st", "prov", "dv")

    def __init__(self, key, atom, c, r, X, chain=(), geom=None, st=None, prov=None, dv=None):
        # chain: the input warps applied on the way down, outermost first, as (warp, inputs before it)
        # geom: (H, W, ph, pw) when the path passed a patch_convolve node -- X then holds the flattened images
        # st: (offsets D x Q, weights Q) when the path passed a stencil node -- the offsets in the coordinates of X
        # prov: where st came from, for the chain rule of stencil_node_gradients: [(c_i, layers_i)], one entry per walk that
        #       was merged into this path (sum c_i == c); layers = ((stencil node, M), ...) outermost first, M (dim of X x dim
        #       of the node's offsets) the product of the Stretch / Select maps below the node.  Point (p_1, ..., p_K) of st
        #       sits at the C-order index of its tuple: offsets sum_k M_k A_k[:, p_k], weight prod_k w_k[p_k]
        # dv: the direction (length dim of X) along which the process is differentiated when the path passed a derivative node
        self.key, self.atom, self.c, self.r, self.X, self.chain, self.geom, self.st = key, atom, c, r, X, chain, geom, st
        self.prov, self.dv = prov, dv


class _ScaleVector(np.ndarray):
    """The row-scale vector r of a path (a product of sigma.(x) factors) that remembers its factors:
    `factors` = [(node, x, values)] with node the `sigma * f` process, x the inputs sigma was mapped over and
    values = sigma.(x) -- what the chain rule of the scale gradients needs (finite_gp.logpdf_and_gradient)."""

    def __new__(cls, values, factors):
        obj = np.asarray(values, dtype=np.float64).view(cls)
        obj.factors = list(factors)
        return obj

    def __array_finalize__(self, obj):
        self.factors = getattr(obj, "factors", [])


class _MatCache:
    """as_matrix with identity caching so equal inputs are uploaded once -- and the memo of the walk down the tree:
    a shared sub-tree is reached along several paths (f5 = f3 + f4 with f4 = f1 + f3: the reference's recursion
    re-evaluates it once per path, test/affine_transformations/addition.jl:7-9); the warped inputs of a compose node
    and the scale vector of a `sigma * f` node are computed ONCE per (node, inputs[, incoming scale]) and the same
    object is handed to every path, so that paths which read the same points with the same scales merge into one
    kernel term (identity keys) instead of one term per path."""

    def __init__(self):
        self.m = {}
        self.keep = []
        self.warped = {}
        self.scaled = {}

    def warp(self, f, g, x):
        k = (id(f), id(x))
        if k not in self.warped:
            self.warped[k] = _gp.warp(g, x)
            self.keep.append((f, x))
        return self.warped[k]

    def scale(self, f, s, x, r):
        k = (id(f), id(x), id(r) if r is not None else None)
        if k not in self.scaled:
            sx = np.asarray(_gp._map_points(s, x), dtype=np.float64)
            fac = ([] if r is None else list(r.factors)) + [(f, x, sx)]
            self.scaled[k] = _ScaleVector(sx if r is None else np.asarray(r) * sx, fac)
            self.keep.append((f, x, r))
        return self.scaled[k]

    def __call__(self, x):
        k = id(x)
        if k not in self.m:
            self.m[k] = np.asfortranarray(as_matrix(x))
            self.keep.append(x)
        return self.m[k]


def block_list(f, x):
    """[(process node, inputs)] per block of x, in order (cross.jl / gppp.jl semantics)."""
    if isinstance(f, GPPP):
        node, v = extract_components(f, x)
        return block_list(node, v)
    if isinstance(f, _gp.DerivedGP) and f.args[0] == "cross":
        if not isinstance(x, BlockData) or len(blocks(x)) != len(f.args[1]):
            raise ValueError("a cross(...) process must be indexed with a BlockData of matching length")
        out = []
        for g, b in zip(f.args[1], blocks(x)):
            out.extend(block_list(g, b))
        return out
    if is_pair_vector(x):
        # (key, value) pairs on their way to a NESTED programme below f (gppp.jl:32-43 regroups them by key when they reach
        # it, changing the element order): regrouped here, so that every block reads ONE inner process
        x = regroup_pairs(x)
    if isinstance(x, BlockData):
        # BlockData is an ordinary AbstractVector for any GP (input_collection_types.jl:61-95): the
        # same process evaluated on each block
        out = []
        for b in blocks(x):
            out.extend(block_list(f, b))
        return out
    return [(f, x)]


def _warp_name(g):
    return getattr(g, "__name__", type(g).__name__)


def _paths(f, x, c, r, key, mat, chain=(), geom=None):
    if geom is not None:
        return _conv_paths(f, x, c, r, key, mat, chain, geom)
    if isinstance(f, GPPP):  # a GPPP wrapped in atomic(...) (nested programmes, test gppp.jl:107-120)
        node, v = extract_components(f, x)
        if isinstance(node, _gp.DerivedGP) and node.args[0] == "cross":
            # (block_list splits BlockData and regroups pair vectors before any path is walked)
            raise ValueError("internal: a nested GPPP reached with inputs of several of its processes")
        return _paths(node, v, c, r, key, mat, chain)
    if isinstance(f, _gp.AtomicGP):
        k2 = key + (id(f),)
        if isinstance(f.gp, _gp.GP):
            return [_Path(k2, f, c, r, mat(x), chain)]
        return _paths(f.gp, x, c, r, k2, mat, chain)
    op = f.args[0]
    if op == "+":
        return _paths(f.args[1], x, c, r, key, mat, chain) + _paths(f.args[2], x, c, r, key, mat, chain)
    if op == "+known":
        return _paths(f.args[2], x, c, r, key, mat, chain)
    if op == "*":
        s = f.args[1]
        if _gp._is_real(s):
            return _paths(f.args[2], x, c * float(s), r, key, mat, chain)
        return _paths(f.args[2], x, c, mat.scale(f, s, x, r), key, mat, chain)
    if op == "o":
        return _paths(f.args[1], mat.warp(f, f.args[2], x), c, r, key, mat, chain + ((f.args[2], x),))
    if op == "conv":
        # patch_convolve: the paths of g read the patches of these images (flattened, one per column); the library sums
        # over the patches (include/sthenomi_conv.h)
        return _paths(f.args[1], x, c, r, key, mat, chain, _gp.conv_geometry(f, x))
    if op == "stencil":
        # sum_q w_q f(x - a_q): the paths of f read these points, shifted by the stencil in the library
        # (include/sthenomi_stencil.h)
        return _stencil_paths(f.args[1], x, c, r, key, mat, chain, (f.args[2], f.args[3]),
                              ((f, np.eye(f.args[2].shape[0])),))
    if op == "deriv":
        # d f / d x[dim]: the paths of f read these points and carry the direction e_dim (include/sthenomi.h: SGP_DERIV_*)
        D = as_matrix(x).shape[0] if isinstance(x, ColVecs) else 1
        if f.args[2] >= D:
            raise ValueError(f"derivative: dim = {f.args[2]} for inputs of dimension {D}")
        v = np.zeros(D)
        v[f.args[2]] = 1.0
        return _deriv_paths(f.args[1], x, c, r, key, mat, chain, v)
    if op == "cross":
        raise ValueError("cross(...) can only appear at block level")
    raise ValueError(op)


def _deriv_paths(f, x, c, r, key, mat, chain, v):
    """the paths below a derivative node: what commutes with differentiation along the direction v (in the coordinates of
    x) -- sums, scalar scales, `+ known`, Shift, and Stretch / Select, which map the direction as _map_offsets maps offsets
    (the chain rule: f(g(x)) differentiated along v is f differentiated along Dg v) -- and nothing else"""
    if isinstance(f, _gp.AtomicGP):
        if not isinstance(f.gp, _gp.GP):
            raise NotImplementedError("derivative of a nested GPPP is not supported")
        m = f.gp.mean_spec
        if m is not None and not _gp._is_real(m):
            raise NotImplementedError("derivative: a callable prior mean below the node cannot be differentiated (a constant "
                                      "mean differentiates to 0)")
        X = mat(x)
        if X.shape[0] != v.shape[0]:
            raise ValueError(f"derivative: a direction of dimension {v.shape[0]} for inputs of dimension {X.shape[0]}")
        return [_Path(key + (id(f),), f, c, r, X, chain, dv=v)]
    if isinstance(f, GPPP) or not isinstance(f, _gp.DerivedGP):
        raise NotImplementedError("derivative of a nested GPPP is not supported" if isinstance(f, GPPP) else
                                  f"derivative over {type(f).__name__} is not supported")
    op = f.args[0]
    if op == "+":
        return _deriv_paths(f.args[1], x, c, r, key, mat, chain, v) + _deriv_paths(f.args[2], x, c, r, key, mat, chain, v)
    if op == "+known":
        return _deriv_paths(f.args[2], x, c, r, key, mat, chain, v)
    if op == "*":
        s = f.args[1]
        if not _gp._is_real(s):
            raise NotImplementedError("derivative: a function-valued scale below the node is not supported (the product rule "
                                      "needs the scale's own derivative; only scalar scales commute)")
        return _deriv_paths(f.args[2], x, c * float(s), r, key, mat, chain, v)
    if op == "o":
        g = f.args[2]
        if isinstance(g, _gp.Shift):
            return _deriv_paths(f.args[1], mat.warp(f, g, x), c, r, key, mat, chain + ((g, x),), v)
        if isinstance(g, (_gp.Stretch, _gp.Select)):
            return _deriv_paths(f.args[1], mat.warp(f, g, x), c, r, key, mat, chain + ((g, x),),
                                _map_offsets(g, v[:, None])[:, 0])
        raise NotImplementedError(f"derivative: the warp {_warp_name(g)} below the node is not supported (only Shift, Stretch "
                                  "and Select are)")
    if op == "deriv":
        raise NotImplementedError("derivative of a derivative on one side (a second derivative) is not supported")
    if op == "conv":
        raise NotImplementedError("derivative of a patch_convolve is not supported")
    if op == "stencil":
        raise NotImplementedError("derivative of a stencil is not supported")
    raise NotImplementedError(f"derivative over `{op}` is not supported")


def _conv_paths(f, x, c, r, key, mat, chain, geom):
    """the paths below a patch_convolve node: what commutes with patch extraction -- sums, scalar scales, `+ known`,
    scalar Stretch warps -- and nothing else"""
    if isinstance(f, _gp.AtomicGP):
        if isinstance(f.gp, _gp.GP):
            return [_Path(key + (id(f),), f, c, r, mat(x), chain, geom)]
        raise NotImplementedError("patch_convolve of a nested GPPP is not supported")
    if isinstance(f, GPPP) or not isinstance(f, _gp.DerivedGP):
        raise NotImplementedError(f"patch_convolve over {type(f).__name__} is not supported")
    op = f.args[0]
    if op == "+":
        return (_conv_paths(f.args[1], x, c, r, key, mat, chain, geom) +
                _conv_paths(f.args[2], x, c, r, key, mat, chain, geom))
    if op == "+known":
        return _conv_paths(f.args[2], x, c, r, key, mat, chain, geom)
    if op == "*":
        s = f.args[1]
        if not _gp._is_real(s):
            raise NotImplementedError("patch_convolve: a function scale below patch_convolve does not commute with patch "
                                      "extraction (only scalar scales do)")
        return _conv_paths(f.args[2], x, c * float(s), r, key, mat, chain, geom)
    if op == "o":
        g = f.args[2]
        if isinstance(g, _gp.Stretch) and np.ndim(g.l) == 0:
            return _conv_paths(f.args[1], mat.warp(f, g, x), c, r, key, mat, chain + ((g, x),), geom)
        raise NotImplementedError(f"patch_convolve: the warp {_warp_name(g)} below patch_convolve does not commute with "
                                  "patch extraction (only a scalar Stretch does)")
    if op == "conv":
        raise NotImplementedError("patch_convolve of a patch_convolve is not supported")
    if op == "stencil":
        raise NotImplementedError("patch_convolve of a stencil is not supported")
    if op == "deriv":
        raise NotImplementedError("patch_convolve of a derivative is not supported")
    raise NotImplementedError(f"patch_convolve over `{op}` is not supported")


def _map_offsets(g, A):
    """the offsets A (D x Q) seen through the linear warp g (Stretch / Select): g(x - a) = g(x) - g(a)"""
    if isinstance(g, _gp.Stretch):
        return float(g.l) * A if np.ndim(g.l) == 0 else np.asarray(g.l, dtype=np.float64) @ A
    if isinstance(g.idx, (int, np.integer)):
        return A[[int(g.idx)], :]
    return A[np.asarray(g.idx), :]


def _stencil_paths(f, x, c, r, key, mat, chain, st, layers):
    """the paths below a stencil node: what commutes with shifting the points -- sums, scalar scales, `+ known`, Shift
    (moves the points), Stretch and Select (map the points and the offsets alike), and stencils (which fold into one) --
    and nothing else.  layers: the provenance of st (_Path.prov)"""
    A, w = st
    if isinstance(f, _gp.AtomicGP):
        if isinstance(f.gp, _gp.GP):
            X = mat(x)
            if X.shape[0] != A.shape[0]:
                raise ValueError(f"stencil: offsets of dimension {A.shape[0]} for inputs of dimension {X.shape[0]}")
            if A.shape[0] > _lib.STENCIL_MAX_DIM or len(w) > _lib.STENCIL_MAX_POINTS:
                raise NotImplementedError(f"stencil: {len(w)} points of dimension {A.shape[0]} are beyond the library's "
                                          f"limits ({_lib.STENCIL_MAX_POINTS} points, dimension "
                                          f"{_lib.STENCIL_MAX_DIM})")
            return [_Path(key + (id(f),), f, c, r, X, chain, None, st, [(c, layers)])]
        raise NotImplementedError("stencil of a nested GPPP is not supported")
    if isinstance(f, GPPP) or not isinstance(f, _gp.DerivedGP):
        raise NotImplementedError(f"stencil over {type(f).__name__} is not supported")
    op = f.args[0]
    if op == "+":
        return (_stencil_paths(f.args[1], x, c, r, key, mat, chain, st, layers) +
                _stencil_paths(f.args[2], x, c, r, key, mat, chain, st, layers))
    if op == "+known":
        return _stencil_paths(f.args[2], x, c, r, key, mat, chain, st, layers)
    if op == "*":
        s = f.args[1]
        if not _gp._is_real(s):
            raise NotImplementedError("stencil: a function scale below a stencil does not commute with its shifts (only "
                                      "scalar scales do)")
        return _stencil_paths(f.args[2], x, c * float(s), r, key, mat, chain, st, layers)
    if op == "o":
        g = f.args[2]
        if isinstance(g, _gp.Shift):
            return _stencil_paths(f.args[1], mat.warp(f, g, x), c, r, key, mat, chain + ((g, x),), st, layers)
        if isinstance(g, (_gp.Stretch, _gp.Select)):
            # (the maps are linear: the provenance matrices go through the same function as the offsets)
            return _stencil_paths(f.args[1], mat.warp(f, g, x), c, r, key, mat, chain + ((g, x),), (_map_offsets(g, A), w),
                                  tuple((n, _map_offsets(g, M)) for n, M in layers))
        raise NotImplementedError(f"stencil: the warp {_warp_name(g)} below a stencil does not commute with its shifts "
                                  "(only Shift, Stretch and Select do)")
    if op == "stencil":
        # a stencil of a stencil: sum_p w_p sum_q v_q f(x - a_p - b_q), point (p, q) at p * Q_b + q
        B, v = f.args[2], f.args[3]
        if B.shape[0] != A.shape[0]:
            raise ValueError(f"stencil: offsets of dimension {B.shape[0]} below offsets of dimension {A.shape[0]}")
        A2 = (A[:, :, None] + B[:, None, :]).reshape(A.shape[0], -1)
        return _stencil_paths(f.args[1], x, c, r, key, mat, chain, (A2, np.outer(w, v).reshape(-1)),
                              layers + ((f, np.eye(B.shape[0])),))
    if op == "conv":
        raise NotImplementedError("stencil of a patch_convolve is not supported")
    if op == "deriv":
        raise NotImplementedError("stencil of a derivative is not supported")
    raise NotImplementedError(f"stencil over `{op}` is not supported")


def _st_key(st):
    return None if st is None else (st[0].shape, st[0].tobytes(), st[1].tobytes())


def _merge_paths(ps, cancelled=None):
    """cancelled (a list): gains the stencil paths that cancel exactly -- their term is gone, and with it the gradient with
    respect to their stencils, which does not vanish (stencil_node_gradients refuses such a spec)"""
    out, index = [], {}
    for p in ps:
        k = (p.key, id(p.X), id(p.r) if p.r is not None else None, p.geom, _st_key(p.st),
             None if p.dv is None else p.dv.tobytes())
        if k in index:
            index[k].c += p.c
            if p.prov is not None:
                index[k].prov = index[k].prov + p.prov
        else:
            q = _Path(p.key, p.atom, p.c, p.r, p.X, p.chain, p.geom, p.st, None if p.prov is None else list(p.prov), p.dv)
            index[k] = q
            out.append(q)
    # paths that cancel exactly (f - f, 2 f - f - f, ...) leave no term: the block is an exact zero, as in the
    # reference's recursion, which adds and subtracts identical matrices
    if cancelled is not None:
        cancelled.extend(q for q in out if q.c == 0.0 and q.st is not None)
    return [q for q in out if q.c != 0.0]


class _InputTable:
    def __init__(self):
        self.arrays, self.index, self.origin = [], {}, []

    def get(self, X, chain, origin=None):
        """chain: the kernel-level input transformation (kernels.apply_chain); origin = (side, block
        index, warp chain): where the points came from (for the chain rule of input gradients); the
        first path that registers an array names it."""
        k = (id(X), chain)
        if k not in self.index:
            self.index[k] = len(self.arrays)
            self.arrays.append(X if not chain else _kernels.apply_chain(chain, X))
            self.origin.append(origin + (chain, X) if origin is not None else None)
        return self.index[k]


def build_spec(f, x, f2=None, x2=None):
    """lib.Spec for cov(f, x) (symmetric) or cov(f, f2, x, x2) (cross; no noise).

    f / f2: GPPP or Stheno GP nodes of one model (same GPC).  Returns (spec, row_blocks,
    col_blocks) where the block lists are [(node, inputs)]."""
    symmetric = x2 is None
    mat = _MatCache()
    rows = block_list(f, x)
    cols = rows if symmetric else block_list(f if f2 is None else f2, x2)
    gpcs = {id(n.gpc) for n, _ in rows} | {id(n.gpc) for n, _ in cols}
    if len(gpcs) > 1:
        raise AssertionError("f.gpc === f'.gpc violated: processes come from different GPCs")
    cancelled = []
    rpaths = [_merge_paths(_paths(n, v, 1.0, None, (), mat), cancelled) for n, v in rows]
    cpaths = rpaths if symmetric else [_merge_paths(_paths(n, v, 1.0, None, (), mat), cancelled) for n, v in cols]
    table = _InputTable()
    pairs, geoms, stencils, provs = {}, {}, {}, {}
    for I, pi in enumerate(rpaths):
        for J, pj in enumerate(cpaths):
            merged, order, prov = {}, [], {}
            for p in pi:
                for q in pj:
                    if p.key != q.key:
                        continue
                    if _point_dim(p) != _point_dim(q):
                        raise ValueError("input dimension mismatch between two views of one process")
                    if p.geom is not None and q.geom is not None and p.geom[2:] != q.geom[2:]:
                        raise ValueError("patch_convolve: two views of one process with different patch sizes")
                    has_st = p.st is not None or q.st is not None
                    if has_st and (p.geom is not None or q.geom is not None):
                        raise NotImplementedError("a covariance between a patch_convolve view and a stencil view of one "
                                                  "process is not supported")
                    has_dv = p.dv is not None or q.dv is not None
                    if has_dv and (has_st or p.geom is not None or q.geom is not None):
                        raise NotImplementedError("a covariance between a derivative view and a patch_convolve or stencil "
                                                  "view of one process is not supported")
                    for (kc, factors) in p.atom.gp.kernel.leaf_products():
                        if has_dv:
                            _deriv_terms(p, q, kc, factors, table, symmetric, I, J, merged, order)
                            continue
                        if len(factors) > 1 or factors[0][0] > _lib.CONST:
                            # a product of kernels, or a kind that exists on the product path only: a chain of terms
                            # (include/sthenomi_kprod.h), each factor reading its own view of the points
                            if has_st or p.geom is not None or q.geom is not None:
                                raise NotImplementedError("a product of kernels (or a RationalQuadratic / Linear / Polynomial / "
                                                          "Cosine / GammaExponential kernel, which runs on the product path) below patch_convolve or a "
                                                          "stencil is not supported")
                            if len(factors) > _lib.KPROD_MAX_FACTORS:
                                raise NotImplementedError(f"a product of {len(factors)} kernels is beyond the library's limit "
                                                          f"of {_lib.KPROD_MAX_FACTORS} factors")
                            chain = []
                            for (kind, param, s) in factors:
                                ri = table.get(p.X, s, ("row", I, p.chain))
                                ci = table.get(q.X, s, ("row" if symmetric else "col", J, q.chain))
                                chain.append((kind, param, ri, ci))
                            # the library's limits (include/sthenomi_kprod.h), named here as it names them
                            dims = [int(np.asarray(table.arrays[c[2]]).shape[0]) for c in chain]
                            for (kind, param, _, _), dm in zip(chain, dims):
                                if _lib.PIECEWISE0 <= kind <= _lib.PIECEWISE3 and dm > _kernels.piecewise_max_dim(kind, param):
                                    raise ValueError(f"PiecewisePolynomialKernel (degree {kind - _lib.PIECEWISE0}, j = {int(param)}) is "
                                                     f"positive definite up to dimension {_kernels.piecewise_max_dim(kind, param)} "
                                                     f"and reads points of dimension {dm} after its transforms: pass dim >= {dm}")
                            dmax = 1 << max(0, max(dims) - 1).bit_length()
                            if max(dims) > _lib.KPROD_MAX_DIM or len(chain) * dmax > 64:
                                raise NotImplementedError(f"a product of {len(chain)} kernels (or a kernel of the product path) on "
                                                          f"inputs of dimension {max(dims)} is beyond the library's limits: factor "
                                                          f"dimension <= {_lib.KPROD_MAX_DIM}, factors x dimension (rounded up to a "
                                                          "power of two) <= 64")
                            k = ("product", tuple(chain), id(p.r) if p.r is not None else None,
                                 id(q.r) if q.r is not None else None)
                            if k in merged:
                                merged[k][0][0][3] += p.c * q.c * kc
                            else:
                                terms = [[chain[0][0], chain[0][2], chain[0][3], p.c * q.c * kc, chain[0][1], p.r, q.r]]
                                terms += [[kind | _lib.KIND_TIMES_PREV, ri, ci, 1.0, param, None, None]
                                          for (kind, param, ri, ci) in chain[1:]]
                                merged[k] = (terms, (None, None), (None, None))
                                order.append(k)
                            continue
                        (kind, param, s), = factors
                        if (p.geom is not None or q.geom is not None) and _kernels.chain_scale(s) is None:
                            raise NotImplementedError("patch_convolve: the kernel's input transform does not commute with "
                                                      "patch extraction (only a scalar ScaleTransform / with_lengthscale "
                                                      "does)")
                        sts = (None, None)
                        if has_st:
                            sc = _kernels.chain_scale(s)
                            if sc is None:
                                raise NotImplementedError("stencil: the kernel's input transform (PeriodicTransform) does "
                                                          "not commute with its shifts (only a scalar ScaleTransform / "
                                                          "with_lengthscale does)")
                            sts = tuple(None if st is None else (st[0] if sc == 1.0 else sc * st[0], st[1])
                                        for st in (p.st, q.st))
                        ri = table.get(p.X, s, ("row", I, p.chain))
                        ci = table.get(q.X, s, ("row" if symmetric else "col", J, q.chain))
                        k = (kind, param, ri, ci, id(p.r) if p.r is not None else None,
                             id(q.r) if q.r is not None else None, p.geom, q.geom, _st_key(sts[0]), _st_key(sts[1]))
                        if k in merged:
                            merged[k][0][0][3] += p.c * q.c * kc
                        else:
                            merged[k] = ([[kind, ri, ci, p.c * q.c * kc, param, p.r, q.r]], (p.geom, q.geom), sts)
                            order.append(k)
                        if has_st:
                            # the provenance of the term's two stencils: every walk's part of the coefficient, per side
                            acc = prov.setdefault(k, (sc, [], []))
                            if p.st is not None:
                                acc[1].extend((ci_ * q.c * kc, layers) for ci_, layers in p.prov)
                            if q.st is not None:
                                acc[2].extend((p.c * cj_ * kc, layers) for cj_, layers in q.prov)
            if order:
                # (a key holds one term, or the terms of one chain: a head and its continuations, which have plain sides)
                pairs[(I, J)] = [tuple(t) for k in order for t in merged[k][0]]
                plain = (None, None)
                if any(merged[k][1] != plain for k in order):
                    geoms[(I, J)] = [merged[k][1] if n == 0 else plain for k in order for n in range(len(merged[k][0]))]
                if any(merged[k][2] != plain for k in order):
                    stencils[(I, J)] = [merged[k][2] if n == 0 else plain for k in order for n in range(len(merged[k][0]))]
                    provs[(I, J)] = [prov.get(k) if n == 0 else None for k in order for n in range(len(merged[k][0]))]
    spec = _lib.Spec([len(v) for _, v in rows], [len(v) for _, v in cols], table.arrays, pairs, symmetric,
                     geoms=geoms or None, stencils=stencils or None)
    spec._mat_keep = mat  # keep the source arrays alive (ids are identity keys)
    # per term (the order of spec.term_stencils): None, or (kernel input scale, row side, column side), a side being the
    # list of (part of the term's coefficient, layers) of _Path.prov -- what stencil_node_gradients chains back through
    spec.term_stencil_prov = [e for I in range(len(rows)) for J in range(len(cols))
                              for e in provs.get((I, J), [None] * len(pairs.get((I, J), [])))]
    spec.stencil_cancelled = bool(cancelled)
    spec.input_origin = table.origin   # per spec input: (side, block, warp chain, kernel input chain, raw points)
    spec.block_shapes = ([_leaf_shape(v) for _, v in rows], [_leaf_shape(v) for _, v in cols])
    return spec, rows, cols


def _deriv_terms(p, q, kc, factors, table, symmetric, I, J, merged, order):
    """the terms of one leaf of the kernel between the paths p and q, at least one of which carries a direction: one term of
    the leaf's derivative kind per pair of non-zero components of the two directions, seen through the kernel's own input
    transform (kernels.chain_direction), the components -- the Jacobian factors -- in its coefficient"""
    if len(factors) > 1 or factors[0][0] not in _lib.DERIV_OF:
        raise NotImplementedError("derivative: the kernel below the node must be SE, Matern-3/2 or Matern-5/2, or a sum or "
                                  "scaling of these (no products of kernels, no Matern-1/2, no kernel of the product path)")
    (kind, _, s), = factors
    sides = []
    for path in (p, q):
        if path.dv is None:
            sides.append([(0, 1.0)])
            continue
        v = _kernels.chain_direction(s, path.dv)
        if v is None:
            raise NotImplementedError("derivative: the kernel's input transform (PeriodicTransform) is not linear: only "
                                      "ScaleTransform / ARDTransform / LinearTransform / SelectTransform / with_lengthscale are "
                                      "supported below the node")
        sides.append([(d + 1, float(v[d])) for d in range(v.shape[0]) if v[d] != 0.0])
    ri = table.get(p.X, s, ("row", I, p.chain))
    ci = table.get(q.X, s, ("row" if symmetric else "col", J, q.chain))
    if np.asarray(table.arrays[ri]).shape[0] > _lib.DERIV_MAX_DIM:
        raise NotImplementedError(f"derivative: inputs of dimension {np.asarray(table.arrays[ri]).shape[0]} are beyond the "
                                  f"library's limit of {_lib.DERIV_MAX_DIM}")
    for a, va in sides[0]:
        for b, vb in sides[1]:
            param = float(_lib.DERIV_PARAM_BASE * a + b)
            k = (_lib.DERIV_OF[kind], param, ri, ci, id(p.r) if p.r is not None else None,
                 id(q.r) if q.r is not None else None, None, None, None, None)
            if k in merged:
                merged[k][0][0][3] += p.c * q.c * kc * va * vb
            else:
                merged[k] = ([[_lib.DERIV_OF[kind], ri, ci, p.c * q.c * kc * va * vb, param, p.r, q.r]], (None, None), (None, None))
                order.append(k)


def _point_dim(p):
    """the dimension of the points the kernel of path p compares: the patch for a patch_convolve path"""
    return p.geom[2] * p.geom[3] if p.geom is not None else p.X.shape[0]


def _leaf_shape(v):
    while isinstance(v, GPPPInput):   # nested programmes index a process of the inner GPPP
        v = v.x
    return as_matrix(v).shape


def stencil_node_gradients(spec, gw, go, into=None):
    """The chain from the library's stencils back to the `stencil(...)` nodes of the model.  gw[t][side] / go[t][side]: the
    gradient with respect to the weights (Q) and offsets (D x Q) of the stencil that term t of `spec` reads on its row (0) or
    column (1) side, None on a plain side (include/sthenomi_stencil_wo.h: every term's own copy, mirror pairs included).
    The library's offsets are sc M_k A_k summed over the nested nodes k (sc: the kernel's scalar input scale, M_k: the
    Stretch / Select maps below node k) and its weights their outer product, so
        dA_k[:, p_k] = sc M_k' sum_others dA_lib,      dw_k[p_k] = sum_others dw_lib prod_{j != k} w_j[p_j];
    a term merged from several walks gives each its part of the coefficient, c_walk / coef.  Returns (and adds onto) `into`:
    id(node) -> {"node", "d_offsets" (D x Q, the node's own shape), "d_weights" (Q)}, in the order the nodes are met."""
    into = {} if into is None else into
    if getattr(spec, "stencil_cancelled", False):
        raise NotImplementedError("gradients with respect to stencils: two stencil views of one process cancel exactly in this "
                                  "model (their term is gone, their stencils' gradient is not)")
    for t, prov in enumerate(getattr(spec, "term_stencil_prov", None) or []):
        if prov is None:
            continue
        sc, coef = prov[0], float(spec._terms[t].coef)
        for side in (0, 1):
            walks = prov[1 + side]
            if not walks:
                continue
            if coef == 0.0 and len(walks) > 1:
                raise NotImplementedError("gradients with respect to stencils: a term merged from several stencil views whose "
                                          "coefficients cancel exactly has no shares to hand out")
            dA, dw = np.asarray(go[t][side], dtype=np.float64), np.asarray(gw[t][side], dtype=np.float64)
            for part, layers in walks:
                share = part / coef if coef != 0.0 else 1.0
                ws = [np.asarray(n.args[3], dtype=np.float64) for n, _ in layers]
                qs = tuple(len(w) for w in ws)
                dAr, dwr = dA.reshape((dA.shape[0],) + qs), dw.reshape(qs)
                for k, (node, M) in enumerate(layers):
                    others = tuple(j for j in range(len(qs)) if j != k)
                    wo = dwr
                    for j in others:      # times the other nodes' weights, along their own axes
                        wo = wo * ws[j].reshape([-1 if a == j else 1 for a in range(len(qs))])
                    e = into.setdefault(id(node), {"node": node, "d_offsets": np.zeros(np.shape(node.args[2])),
                                                   "d_weights": np.zeros(qs[k])})
                    e["d_offsets"] += share * sc * (M.T @ dAr.sum(axis=tuple(1 + j for j in others)))
                    e["d_weights"] += share * wo.sum(axis=others)
    return into


def zero_spec(n):
    """A spec with no terms: K == 0 exactly (used to feed an explicit covariance as dense noise)."""
    return _lib.Spec([n], [n], [], {}, True)


# ---- chain rule of input gradients through the host-side transformations ------------------------
def _warp_vjp(g, x_in, gout):
    """Cotangent of the warp's input given the cotangent `gout` (dim_out x n) of its output."""
    if isinstance(g, _gp.Stretch):
        if np.ndim(g.l) == 0:
            return float(g.l) * gout
        return np.asarray(g.l, dtype=np.float64).T @ gout
    if isinstance(g, _gp.Shift):
        return gout
    if isinstance(g, _gp.Select):
        X = as_matrix(x_in)
        gin = np.zeros(X.shape)
        if isinstance(g.idx, (int, np.integer)):
            gin[g.idx, :] += gout.reshape(-1)
        else:
            np.add.at(gin, np.asarray(g.idx), gout)
        return gin
    if isinstance(g, _gp.Periodic):
        t = (2.0 * np.pi * g.f) * as_matrix(x_in)          # 1 x n; output rows are [cos t; sin t]
        return (2.0 * np.pi * g.f) * (-np.sin(t) * gout[0:1, :] + np.cos(t) * gout[1:2, :])
    raise NotImplementedError("input gradients through an arbitrary point-wise warp: supply its Jacobian yourself")


def chain_input_gradients(spec, grads):
    """Map gradients w.r.t. the spec inputs (the transformed points the terms read, as returned by
    sgp_*_grad_x) back onto the blocks the spec was built from: the kernel's input scale
    (ScaleTransform / with_lengthscale) and the Stretch / Select / Periodic / Shift warps of the
    model are undone in reverse.  Returns (row_block_grads, col_block_grads): lists of (D, n) arrays
    aligned with the blocks of x (and of x2 for a cross spec; for a symmetric spec the second list
    is the first)."""
    rshapes, cshapes = spec.block_shapes
    rows = [np.zeros(sh) for sh in rshapes]
    cols = rows if spec.symmetric else [np.zeros(sh) for sh in cshapes]
    for k, g in enumerate(grads):
        org = spec.input_origin[k]
        if org is None or g is None:
            continue
        side, I, chain, kchain, X_raw = org
        gg = _kernels.chain_vjp(kchain, X_raw, g) if kchain else np.asarray(g, dtype=np.float64)
        for (w, x_in) in reversed(chain):
            gg = _warp_vjp(w, x_in, gg)
        (rows if side == "row" else cols)[I] += gg.reshape((rows if side == "row" else cols)[I].shape)
    return rows, cols
