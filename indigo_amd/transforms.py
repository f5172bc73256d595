"""Setup-time tree rewrites.

`Transform` / `Visitor` / `Optimize` / `RealizeMatrices` follow
indigo/transforms.py:19-175; the SENSE recipe passes (`MakeRightLeaning`,
`AssocSpMatrices`, `DistKroniOverFFT`, `MriRealize`, `MriGoodAdjoints`) restate
the classes the reference keeps inside its driver script
(examples/pics.py:104-177) so that `sense_recipe(level)` reproduces `pics.py -O<level>`.

All of this runs on the host with scipy; it decides WHICH leaves run, the HIP
library decides how fast.  `Optimize` also reserves the scratch arena, sized by
`ScratchUsage` (the reference's own sizing under-counts KronI trees and trips
its arena assertion, backend.py:272).
"""
import logging

import numpy as np
import scipy.sparse as spp

from indigo_amd.operators import (Adjoint, BlockDiag, CompositeOperator, Eye, HeadRows, HStack, Kron, One,  # noqa: F401
                                  Product, Scale, SpMatrix, UnscaledFFT, VStack)

log = logging.getLogger(__name__)


class Transform(object):
    """Rewrites a tree bottom-up or top-down via `visit_<ClassName>` methods (cf. ast.NodeTransformer)."""

    def visit(self, node):
        method = getattr(self, "visit_%s" % type(node).__name__, None)
        return method(node) if method else self.generic_visit(node)

    def generic_visit(self, node):
        if isinstance(node, CompositeOperator):
            node._adopt([self.visit(c) for c in node._children])
        return node


class Visitor(object):
    """Read-only traversal, children first (cf. ast.NodeVisitor)."""

    def visit(self, node):
        self.generic_visit(node)
        method = getattr(self, "visit_%s" % type(node).__name__, None)
        if method:
            method(node)

    def generic_visit(self, node):
        if isinstance(node, CompositeOperator):
            for child in node._children:
                self.visit(child)


class Optimize(Transform):
    """Run a recipe (list of Transform classes), then reserve the backend's scratch arena."""

    def __init__(self, recipe=None, ncols=1):
        self._recipe = recipe or []
        self._ncols = ncols

    def visit(self, node):
        for Step in self._recipe:
            log.info("running optimization step: %s", Step.__name__)
            node = Step().visit(node)
        from indigo_amd.analyses import ScratchUsage
        # A and A^H need the same temporaries; AHA = A^H A stacks one more Product on top, so
        # callers that wrap the optimised tree should call `reserve_for` again on the final tree.
        reserve_for(node, self._ncols)
        return node


def reserve_for(node, ncols=1, slack_products=2, extra=0):
    """Size and allocate `backend._scratch` for evaluating `node` (and `node.H * node`) on `ncols` columns, with `extra` elements
    for the temporaries of products that wrap `node`."""
    from indigo_amd.analyses import ScratchUsage
    elems = ScratchUsage().measure(node, ncols)
    # room for the extra Product levels of A^H*A (+ lamda*I): each adds one panel of A's rows or cols
    extra = int(extra) + slack_products * ((max(node.shape) * ncols + 31) // 32 * 32)
    node._backend.reserve_scratch(elems + extra)
    return elems + extra


def _struct(node):
    return getattr(node, '_struct', None) if isinstance(node, SpMatrix) else None


class RealizeMatrices(Transform):
    """Fold subtrees made only of sparse matrices into a single SpMatrix (indigo/transforms.py:81-175).  Factors that carry a
    description of what they are (indigo_amd.structured: diagonals, selections, gridding matrices -- everything the SENSE
    factories make) are composed as index arithmetic; anything else is multiplied by scipy on the host, as in the reference."""

    def visit_Product(self, node):
        node = self.generic_visit(node)
        L, R = node._children
        if isinstance(L, SpMatrix) and isinstance(R, SpMatrix):
            from indigo_amd.structured import compose_product
            name = "{}*{}".format(L._name, R._name)
            s = compose_product(_struct(L), _struct(R))
            if s is not None:
                out = SpMatrix(node._backend, None, struct=s, name=name)
                for attr in ('_grid_dims',):
                    if getattr(L, attr, None) is not None:
                        setattr(out, attr, getattr(L, attr))
                return out
            return SpMatrix(node._backend, L._matrix @ R._matrix, name=name)
        return node

    def _stack(self, node, stacker):
        node = self.generic_visit(node)
        kids = node._children
        if all(isinstance(c, SpMatrix) for c in kids):
            m = stacker([c._matrix for c in kids], dtype=kids[0].dtype)
            return SpMatrix(node._backend, m, name="{}+".format(kids[0]._name))
        return node

    def visit_VStack(self, node):
        from indigo_amd.structured import DiagS, vstack_diags
        node = self.generic_visit(node)
        kids = node._children
        if kids and all(isinstance(_struct(c), DiagS) for c in kids):
            return SpMatrix(node._backend, None, struct=vstack_diags([c._struct for c in kids]), name="{}+".format(kids[0]._name))
        return self._stack(node, spp.vstack)

    def visit_HStack(self, node):
        return self._stack(node, spp.hstack)

    def visit_BlockDiag(self, node):
        return self._stack(node, spp.block_diag)

    def visit_Kron(self, node):
        from indigo_amd.structured import DiagS, SelectS
        L, R = node._children
        if isinstance(L, Eye):
            R = self.visit(R)
            if isinstance(_struct(R), (DiagS, SelectS)):          # I_c (x) a selection: kept as the pair (c, selection)
                from indigo_amd.structured import KronS
                s = R._struct if isinstance(R._struct, SelectS) else SelectS.from_diag(R._struct)
                return SpMatrix(node._backend, None, struct=KronS(L.shape[0], s), name="({}(x){})".format(L._name, R._name))
            node._adopt([L, R])
        node = self.generic_visit(node)
        L, R = node._children
        if isinstance(L, Eye):
            L = self.visit_Eye(L)
        if isinstance(L, SpMatrix) and isinstance(R, SpMatrix):
            return SpMatrix(node._backend, spp.kron(L._matrix, R._matrix), name="({}(x){})".format(L._name, R._name))
        return node

    def visit_Adjoint(self, node):
        node = self.generic_visit(node)
        child = node.child
        if isinstance(child, SpMatrix):
            s = _struct(child)
            sa = s.adjoint() if hasattr(s, 'adjoint') else None          # (a diagonal or a selection: its triples swapped and conjugated)
            if sa is not None:
                return SpMatrix(node._backend, None, struct=sa, name="{}.H".format(child._name))
            return SpMatrix(node._backend, child._matrix.conjugate().transpose(), name="{}.H".format(child._name))
        return node

    def visit_Eye(self, node):
        return SpMatrix(node._backend, spp.eye(node.shape[0], dtype=node.dtype), name=node._name)

    def visit_Scale(self, node):
        node = self.generic_visit(node)
        if isinstance(node.child, SpMatrix):
            s = _struct(node.child)
            if hasattr(s, 'scaled'):
                return SpMatrix(node._backend, None, struct=s.scaled(node._val), name=node._name)
            return SpMatrix(node._backend, node.child._matrix * node._val, name=node._name)
        return node

    def visit_One(self, node):
        return SpMatrix(node._backend, spp.csr_matrix(np.ones(node.shape, dtype=node.dtype)), name=node._name)


class DistributeKroniOverProd(Transform):
    """Kron(I, A*B) => Kron(I, A) * Kron(I, B)"""

    def visit_Kron(self, node):
        node = self.generic_visit(node)
        L, R = node._children
        if isinstance(L, Eye) and isinstance(R, Product):
            b = node._backend
            return self.visit(b.Kron(L, R.left) * b.Kron(L, R.right))
        return node


class DistributeAdjointOverProd(Transform):
    """Adjoint(A*B) => Adjoint(B) * Adjoint(A)"""

    def visit_Adjoint(self, node):
        node = self.generic_visit(node)
        if isinstance(node.child, Product):
            l, r = node.child._children
            return r.H * l.H
        return node


# -------------------------------------------------------------------------------
# SENSE recipe (examples/pics.py:104-193)
# -------------------------------------------------------------------------------

class MakeRightLeaning(Transform):
    """(A*B)*C => A*(B*C), recursively"""

    def visit_Product(self, node):
        l = self.visit(node.left)
        r = self.visit(node.right)
        if isinstance(l, Product):
            return self.visit(l.left * (l.right * r))
        return l * r


class MakeLeftLeaning(Transform):
    """A*(B*C) => (A*B)*C, recursively"""

    def visit_Product(self, node):
        l = self.visit(node.left)
        r = self.visit(node.right)
        if isinstance(r, Product):
            return self.visit((l * r.left) * r.right)
        return l * r


class AssocSpMatrices(Transform):
    """S*(X*Y) => (S*X)*Y when S is sparse and X is not an FFT: brings sparse factors together"""

    def visit_Product(self, node):
        l = self.visit(node.left)
        r = self.visit(node.right)
        if isinstance(l, SpMatrix) and isinstance(r, Product) and not isinstance(r.left, UnscaledFFT):
            return (l * r.left) * r.right
        return l * r


class DistKroniOverFFT(Transform):
    """Kron(I, A*B) => Kron(I,A)*Kron(I,B) for subtrees containing an FFT"""

    def visit_Kron(self, node):
        L, R = node._children
        if isinstance(L, Eye) and isinstance(R, Product) and node.has(UnscaledFFT):
            b = node._backend
            return self.visit(b.Kron(L, R.left) * b.Kron(L, R.right))
        return node


class MriRealize(Transform):
    """Fold the all-sparse parts of a SENSE tree into single CSR matrices"""

    def visit_VStack(self, node):
        return node.realize()

    def visit_Product(self, node):
        l, r = node._children
        if isinstance(r, VStack) and isinstance(l, Kron):
            return node.realize()
        node = self.generic_visit(node)
        l, r = node._children
        if isinstance(r, SpMatrix) and isinstance(l, SpMatrix):
            return node.realize()
        return node


class MriGoodAdjoints(Transform):
    """Store zero-pad-like matrices transposed (wrapped in Adjoint) so their forward is an exwrite scatter"""

    def visit_SpMatrix(self, node):
        if 'zpad' in node._name:
            return node.H.realize().H
        return node


class UseExwriteProperty(Transform):
    def visit_SpMatrix(self, node):
        node._allow_exwrite = True
        return node


class FuseZpadFFT(Transform):
    """KronI(C, G') * (KronI(C, UnscaledFFT) * S')  =>  KronI(C, G'_perm) * ZpadFFT.

    Runs after `sense_recipe(3)` (the reference's `pics.py -O3`, examples/pics.py:179-193).  That recipe leaves the
    forward operator as two sparse factors around a batched FFT; S' (stored transposed inside an Adjoint by
    MriGoodAdjoints) is zero-pad * modulation * roll-off * maps -- a box position and one weight per voxel and coil.
    Where the backend has zero-pad-aware transforms for the grid (`supports_padded_fft`), S' and the FFT collapse into the
    `ZpadFFT` leaf and G' is renumbered for the leaf's grid order; the result evaluates to the same numbers
    (tests: golden `-O3` vectors).  Trees that do not match are returned unchanged."""
    chunk = 8

    def visit_Product(self, node):
        node = self.generic_visit(node)
        from indigo_amd import fused
        from indigo_amd.operators import ZpadFFT    # noqa: F401  (the leaf this pass introduces)
        L, R = node._children
        b = node._backend
        if not (isinstance(L, Kron) and isinstance(L.left, Eye) and isinstance(L.right, SpMatrix) and isinstance(R, Product)):
            return node
        F, X = R._children
        if not (isinstance(F, Kron) and isinstance(F.left, Eye) and isinstance(F.right, UnscaledFFT)):
            return node
        C = F.left.shape[0]
        grid = F.right._ft_shape
        if L.left.shape[0] != C or len(grid) != 3:
            return node
        # a grid the leaf refuses may still run with the image axes relabelled (fused.image_permutation): the leaf is then assembled
        # on the permuted grid and follows an AxisPermute of the image
        perm = None
        if not b.supports_padded_fft(grid, C):
            perm = fused.image_permutation(b, grid, C)
            if perm is None:
                return node
        from indigo_amd.structured import InterpS, SelectS
        P = int(np.prod(grid))
        if isinstance(X, Adjoint) and isinstance(X.child, SpMatrix):
            Sx, St = X.child, None
        elif isinstance(X, SpMatrix):
            Sx, St = None, X
        else:
            return node
        from indigo_amd.structured import AdjointS, StackS
        sel = _struct(Sx if Sx is not None else St)
        stack = sel.inner if (Sx is not None and isinstance(sel, AdjointS)) else sel if (St is not None and isinstance(sel, StackS)) else None
        if isinstance(stack, StackS) and len(stack.blocks) == C and stack.blocks[0].shape[0] == P and stack.shared_pattern() \
                and stack.blocks[0].rows_unique and stack.blocks[0].cols_unique:
            # S' as the realisation passes composed it: C blocks (mod * zpad * apod) * diag(map_c) over ONE pattern (grid position
            # of every voxel) -- no (C P)-row CSR was ever made
            b0 = stack.blocks[0]
            Nn = b0.shape[1]
            dec = fused.decode_zpad_entries(b0.cols, b0.rows, np.ones(b0.nnz, dtype=np.complex64), Nn, 1, P, grid)
            if dec is not None:
                w = np.zeros((Nn, C), dtype=np.complex64)
                for c, blk in enumerate(stack.blocks):
                    w[blk.cols, c] = blk.vals
                dec = (dec[0], dec[1], np.asfortranarray(w).reshape(tuple(dec[1]) + (C,), order='F'))
        elif isinstance(sel, SelectS):
            sel = sel if Sx is not None else sel.adjoint()
            dec = fused.decode_zpad_entries(sel.rows, sel.cols, sel.vals, sel.shape[0], C, P, grid)
        else:
            Sm = Sx._matrix if Sx is not None else St._matrix.conjugate().transpose()
            dec = fused.decode_zpad_maps(Sm.astype(np.complex64), C, P, grid)
        if dec is None:
            log.warning("FuseZpadFFT: %s is not a zero-pad * diagonal factor; the tree keeps the unfused -O3 leaves (S' csrmm + dense FFT)", X._name)
            return node
        lo, box, w = dec
        gs = _struct(L.right)
        grid0 = tuple(grid)          # (the grid the recipe's G' numbers its columns on)
        if perm is not None:
            image = tuple(box)
            lo, box = tuple(lo[a] for a in perm), tuple(box[a] for a in perm)
            w = w.transpose(tuple(perm) + (3,))
            gs = _permuted_interp(b, gs, grid0, perm)
            grid = tuple(grid0[a] for a in perm)
        tuning = getattr(b, 'tuning', {})
        layout, chunks = fused.choose_layout(C, self.chunk, None, getattr(b, 'supports_single_coil_layout', lambda g: True)(grid),
                                             tuning.get('chunk_cost'), tuning.get('chunk_pad', True))
        # G' = interp * mod * scale: where the factories' description survived the recipe and the backend has a native builder, the
        # matrix is built directly in the leaf's grid order (ig_interp3_fill_modulated); else from the scipy product, renumbered
        # (round 6) the modulation of an odd chirp-z axis moves from G' into the transform that the leaf to its right runs: G' keeps real weights
        kshift, folded, gconst = None, None, 1.0
        if layout == 2 and isinstance(gs, InterpS) and gs.colscale is not None and hasattr(b, 'fold_axis_shifts'):
            sp = gs.colscale.separable()
            if sp is not None and tuple(sp[0].shape) == tuple(gs.N) == tuple(grid):
                kshift, folded = b.fold_axis_shifts(grid, sp[0].phases)
                # ... and what is left as (a constant) x (a sign per axis): the constant goes to the transform's weights, G' is real
                gconst, split = b.split_gridding_constant(folded if folded is not None else sp[0].phases)
                folded = split if split is not None else folded
        Gm = b.gridding_from_struct(gs, 1 if layout >= 1 else 0, **({'phases': folded} if folded is not None else {})) if (isinstance(gs, InterpS) and hasattr(b, 'gridding_from_struct')) else None
        if Gm is None:
            kshift, folded, gconst = None, None, 1.0
        if Gm is None:
            if perm is None:
                Gm = L.right._matrix.astype(np.complex64).tocsr()
                if layout >= 1:
                    Gm = fused.permute_grid_columns(Gm, grid)
            else:
                # the columns of the recipe's matrix renumbered for the permuted grid (and, layout >= 1, its (x, z, y) order)
                order = (perm[0], perm[2], perm[1]) if layout >= 1 else tuple(perm)
                Gm = fused.permute_grid_columns(L.right._matrix.astype(np.complex64).tocsr(), grid0, order)
        zw = fused.support_words(b, grid)
        table = fused.grid_support(Gm, grid, 16, zw) if (layout >= 1 and zw is not None and (layout == 2 or zw == (16, 16))) else None
        # ... and the same matrix as one record per sample, where its modulation is a sign per axis (even grids): the interleaved
        # products then compute their taps (indigo_amd.interp.interp_sep_records)
        sep = b.gridding_sep_from_struct(gs, 1, **({'phases': folded} if folded is not None else {})) if (layout == 2 and isinstance(gs, InterpS) and hasattr(b, 'gridding_sep_from_struct')) else None
        wsel = (lambda c0, c1: w[..., c0:c1]) if complex(gconst) == 1.0 else (lambda c0, c1: (w[..., c0:c1] * np.complex64(gconst)).astype(np.complex64))
        A = fused.assemble(b, Gm, grid, box, wsel, C, layout, chunks, table=table, box_lo=lo,
                           name=node._name, zw=zw or (16, 16), sep=sep, kshift=kshift)
        if perm is not None:
            A = A * b.AxisPermute(image, perm)
            A._name = node._name
            A._image_permutation = tuple(perm)
        A._fused_layout = layout
        return A

    @staticmethod
    def layout_of(node):
        return getattr(node, '_fused_layout', 0)


class AttachCoilMaps(Transform):
    """ZpadFFT => ZpadFFTMaps on a fused SENSE tree that was built from UNIT maps: soft-SENSE, M sets of coil maps.

    `maps` is the host array dims + (C, M).  The tree is what `sense_recipe(3) + [FuseZpadFFT]` makes of
    KronI(C, NUFFT) * VStack(Diag(ones)): every `ZpadFFT` leaf then holds the per-voxel weights of the transform alone (modulation x
    roll-off x gridding constant) and knows its chunk's coils (`_coil_range`, set by `fused.assemble`).  Each leaf becomes a
    `ZpadFFTMaps` over its coils of every set, with the same grid, box, layout, support table, support tile and kshift; the parents
    (`Product`, `HeadRows`, `VStack` over coil chunks) take their widths from their children and so widen to N M columns."""

    def __init__(self, maps):
        self._maps = np.asarray(maps, dtype=np.complex64)
        assert self._maps.ndim == 5, "maps must be dims + (coils, sets)"

    def visit_ZpadFFT(self, node):
        from indigo_amd.operators import ZpadFFTMaps
        lo, hi = node._coil_range
        assert node._w_h is not None and node._box == self._maps.shape[:3], "AttachCoilMaps runs on a fresh tree over the maps' own volume"
        return ZpadFFTMaps(node._backend, node._grid, node._box, node._w_h, self._maps[..., lo:hi, :], hi - lo, box_lo=node._lo,
                           layout=node._layout, support=node._support_h, support_tile=node._tile_kw.get('support_tile', 16),
                           kshift=node._tile_kw.get('kshift'), name=node._name)


def soft_sense_tree(b, nufft, maps, recipe):
    """A = KronI(C, F1) * (the map stack of M sets) for the host `maps` = dims + (C, M), F1 = nufft() a fresh single-coil NUFFT, rewritten by
    `recipe` (`sense_recipe(level)`, with `FuseZpadFFT` at its end for the fused route); shape (C * samples, N M).  Where the recipe
    fuses the unit-map tree into `ZpadFFT` leaves on the image's own axes, those become `ZpadFFTMaps` (`AttachCoilMaps`).  Else -- no
    `FuseZpadFFT` in the recipe, a grid the leaf refuses, or one it takes only behind an `AxisPermute` -- the result is the unfused
    composition Optimize(recipe)(KronI(C, F1)) * CoilMaps(maps)."""
    from indigo_amd.operators import AxisPermute, ZpadFFT
    maps = np.asarray(maps, dtype=np.complex64)
    dims, C = maps.shape[:3], int(maps.shape[3])
    if FuseZpadFFT in recipe:
        ones = np.ones(dims + (1,), dtype=np.complex64)
        S1 = b.VStack([b.Diag(ones) for _ in range(C)], name='maps')
        A = b.KronI(C, nufft()) * S1
        A._name = 'SENSE1'
        A = Optimize(recipe).visit(A)
        if A.has(ZpadFFT) and not A.has(AxisPermute):
            A = AttachCoilMaps(maps).visit(A)
            reserve_for(A, 1)
            return A
        log.info("soft-SENSE: the fused leaf does not take this grid on the image's own axes; the maps run as a CoilMaps leaf")
    A = Optimize([step for step in recipe if step is not FuseZpadFFT]).visit(b.KronI(C, nufft())) * b.CoilMaps(maps, name='maps')
    A._name = 'SENSE1'
    reserve_for(A, 1)
    return A


def _permuted_interp(b, gs, grid, perm):
    """the InterpS description of G' on the grid with its axes relabelled by `perm` (trajectory rows, grid and the per-axis phases
    of a separable column scaling permuted) -- or None where there is no description or its column scaling is not separable
    (the caller then renumbers the columns of the scipy matrix)"""
    from indigo_amd.structured import DiagS, InterpS, SepPhase
    if not isinstance(gs, InterpS) or tuple(gs.N) != tuple(grid):
        return None
    N = tuple(int(gs.N[a]) for a in perm)
    coord = np.asarray(gs.coord)[list(perm)]
    colscale = None
    if gs.colscale is not None:
        sp = gs.colscale.separable()
        if sp is None or tuple(sp[0].shape) != tuple(grid):
            return None
        colscale = DiagS(int(np.prod(N)), [('sep', SepPhase(N, [sp[0].phases[a] for a in perm]))] + ([('const', sp[1])] if sp[1] != 1.0 else []))
    npts, width, table = gs.npts, gs.width, gs.table
    dtype = np.float32
    return InterpS(N, coord, width, table, npts, colscale=colscale,
                   make_plain=lambda: b._interp_matrix(npts, N, width, table, coord, dtype))


def sense_recipe(level=3):
    """The pass list of `pics.py -O<level>` (examples/pics.py:179-193)."""
    recipe = []
    if level >= 1:
        recipe += [MakeRightLeaning, AssocSpMatrices, DistKroniOverFFT, MakeRightLeaning]
    if level >= 2:
        recipe += [MriRealize]
    if level >= 3:
        recipe += [MriGoodAdjoints]
    if level >= 4:
        recipe += [UseExwriteProperty]
    return recipe
