"""Structured linear-operator tree evaluated on a `Backend`.

Re-statement (own code) of the operator algebra of the reference,
indigo/operators.py: the class names, constructor arguments, the
`eval(y, x, alpha, beta, forward, left)` contract and the order in which a
composite hands (alpha, beta) to its children are the reference's, so a tree
built for the reference evaluates identically here:

  * `Product`   puts alpha on the factor applied first and beta on the one
                applied last, with a scratch panel in between (operators.py:520-530)
  * `Sum`       evaluates the right child with beta, then the left with beta=1 (:562-567)
  * `Scale`     conjugates its factor on the adjoint (:587-591)
  * `Kron(I,B)` is B applied to the (N, c) reshaped panel (:374-375)
  * `VStack`    adjoint = scale(y, beta) then accumulate children with beta=1 (:440-447)
  * `UnscaledFFT` requires alpha == 1 and beta == 0 (:314-315)

Only left-multiplication is provided (the reference's right-multiplication
exists solely for dense real-symmetric factors, which are outside the hot path).

Leaves report the reference's own algorithmic-bytes model to `backend.trace`
when one is attached (operators.py:246-259, :319-334, :351-353); nothing here
synchronises the device.
"""
import contextlib
import io
import numpy as np
import scipy.sparse as spp

_C64 = np.dtype('complex64')


def _is_number(v):
    return isinstance(v, (int, float, complex, np.number)) and not isinstance(v, bool)


class Operator(object):
    """Base class: shape (M, N), dtype, eval, algebra."""

    def __init__(self, backend, name='', alpha=1, batch=None):
        self._backend = backend
        self._name = name
        self._batch = batch

    # -- evaluation -----------------------------------------------------------
    def eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        """y = alpha * op(A) * x + beta * y, with op = identity (forward) or ^H."""
        if not left:
            raise NotImplementedError("Right-multiplication is not implemented for %s." % type(self).__name__)
        rows, cols = self.shape if forward else self.shape[::-1]
        x2 = x.reshape((cols, -1))
        y2 = y.reshape((rows, -1))
        if x2.shape[1] != y2.shape[1]:
            raise AssertionError("Dimension mismatch: x has %d columns, y has %d" % (x2.shape[1], y2.shape[1]))
        self._eval(y2, x2, alpha=alpha, beta=beta, forward=forward, left=left)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        raise NotImplementedError()

    @property
    def shape(self):
        raise NotImplementedError()

    @property
    def dtype(self):
        raise NotImplementedError()

    # -- algebra ----------------------------------------------------------------
    def __mul__(self, other):
        if isinstance(other, Operator):
            return Product(self._backend, self, other)
        if isinstance(other, np.ndarray):
            # convenience: host array in, host array out
            x = np.asfortranarray(other.reshape((self.shape[1], -1), order='F'))
            x_d = self._backend.copy_array(x)
            y_d = self._backend.zero_array((self.shape[0], x.shape[1]), dtype=other.dtype)
            self.eval(y_d, x_d)
            return y_d.to_host()
        if _is_number(other):
            return Scale(self._backend, other, self)
        raise ValueError("Cannot multiply Operator by %s" % type(other))

    def __rmul__(self, other):
        if _is_number(other):
            return self * other
        raise ValueError("Cannot right-multiply Operator by %s" % type(other))

    def __add__(self, other):
        if _is_number(other):
            other = other * self._backend.Eye(self.shape[1])
        if isinstance(other, Operator):
            return Sum(self._backend, self, other)
        raise ValueError("Cannot add %s to an Operator" % type(other))

    __radd__ = __add__

    def __sub__(self, other):
        return self + Scale(self._backend, -1, other)

    @property
    def H(self):
        return Adjoint(self._backend, self, name=self._name + ".H")

    # -- introspection ------------------------------------------------------------
    def dump(self):
        """Indented text rendering of the tree (one node per line)."""
        buf = io.StringIO()
        self._dump(buf, 0)
        return buf.getvalue()

    def _dump(self, file, indent=0):
        print('%s%s, %s, %s, %s MB, %s' % ('|   ' * indent, self._name or 'noname', type(self).__name__,
                                           self.shape, self._mem_usage(ncols=1) / 1e6, self.dtype), file=file)

    def optimize(self, recipe=None):
        from indigo_amd.transforms import Optimize
        return Optimize(recipe).visit(self)

    def memusage(self, ncols=1):
        from indigo_amd.analyses import Memusage
        return Memusage().measure(self, ncols)

    def _mem_usage(self, ncols):
        return 0

    def has(self, *op_classes):
        from indigo_amd.analyses import TreeHasOp
        return TreeHasOp(op_classes).search(self)


class CompositeOperator(Operator):
    def __init__(self, backend, *children, **kwargs):
        super().__init__(backend, **kwargs)
        self._adopt(children)

    def _adopt(self, children):
        self._children = list(children)

    @property
    def children(self):
        return self._children

    @property
    def child(self):
        assert len(self._children) == 1
        return self._children[0]

    @property
    def dtype(self):
        return self._children[0].dtype

    def _dump(self, file, indent=0):
        super()._dump(file, indent)
        for c in self._children:
            c._dump(file, indent + 1)

    def realize(self):
        from indigo_amd.transforms import RealizeMatrices
        return RealizeMatrices().visit(self)


class BinaryOperator(CompositeOperator):
    @property
    def left(self):
        return self._children[0]

    @property
    def right(self):
        return self._children[1]


class MatrixFreeOperator(CompositeOperator):
    def __init__(self, backend, shape, *args, dtype=_C64, **kwargs):
        super().__init__(backend, *args, **kwargs)
        self._shape = tuple(int(s) for s in shape)
        self._dtype = np.dtype(dtype)

    @property
    def shape(self):
        return self._shape

    @property
    def dtype(self):
        return self._dtype


# ------------------------------------------------------------------------------
# leaves
# ------------------------------------------------------------------------------

class SpMatrix(Operator):
    """Leaf holding a scipy sparse matrix; device CSR is built lazily on first use.

    `struct` (optional): what the matrix IS -- a diagonal, a selection with weights, a gridding matrix (indigo_amd.structured) --
    as the factories of the backend know it.  With a description the scipy matrix itself is only made when somebody reads
    `_matrix`; the recipe's realisation passes compose descriptions instead of multiplying 1e8-row matrices."""

    def __init__(self, backend, M=None, struct=None, **kwargs):
        super().__init__(backend, **kwargs)
        assert (M is not None and spp.issparse(M)) or struct is not None
        self._m = M
        self._struct = struct
        self._matrix_d = None
        self._allow_exwrite = True
        self._use_dia = False

    @property
    def _matrix(self):
        if self._m is None:
            self._m = self._struct.to_scipy()
        return self._m

    @_matrix.setter
    def _matrix(self, M):
        self._m = M

    @property
    def shape(self):
        return tuple(int(s) for s in (self._m.shape if self._m is not None else self._struct.shape))

    @property
    def dtype(self):
        return self._m.dtype if self._m is not None else _C64

    @property
    def nnz(self):
        return self._m.nnz if self._m is not None else self._struct.nnz

    def _mem_usage(self, ncols=1):
        return self._m.data.nbytes if self._m is not None else self._struct.nnz * 8

    def _get_or_create_device_matrix(self):
        if self._matrix_d is None:
            self._matrix = self._matrix.astype(_C64)
            if self._use_dia:
                self._matrix_d = self._backend.dia_matrix(self._backend, self._matrix.todia(), self._name)
                return self._matrix_d
            csr = self._matrix.tocsr()
            csr.sort_indices()
            self._matrix_d = self._backend.csr_matrix(self._backend, csr, self._name)
            if not self._allow_exwrite:
                self._matrix_d._exwrite = False
            if getattr(self, '_grid_support', None) is not None:
                self._matrix_d.set_grid_support(*self._grid_support)
            # (the binned adjoint formats and the fine support tables come per panel width: a dict {columns: arguments} when the
            # matrix serves coil chunks of several widths, indigo_amd.fused.assemble)
            fine = getattr(self, '_grid_support_fine', None)
            if fine is not None and hasattr(self._matrix_d, 'set_grid_support_fine'):
                if isinstance(fine, dict):
                    for w in sorted(fine):
                        self._matrix_d.set_grid_support_fine(fine[w][0], fine[w][1], ncols=w)
                else:
                    self._matrix_d.set_grid_support_fine(*fine)
            if getattr(self, '_row_order', None) is not None:
                self._matrix_d.set_row_order(self._row_order)
            if getattr(self, '_grid_interleaved', False):
                self._matrix_d.set_grid_interleaved(True)
            for attr, setter in (('_grid_bricks', 'set_grid_bricks'), ('_grid_slots', 'set_grid_slots')):
                args = getattr(self, attr, None)
                if args is not None and hasattr(self._matrix_d, setter):
                    for a in ([args[w] for w in sorted(args)] if isinstance(args, dict) else [args]):
                        getattr(self._matrix_d, setter)(*a)
            sep = getattr(self, '_grid_separable', None)
            if sep is not None and hasattr(self._matrix_d, 'set_grid_separable'):
                self._matrix_d.set_grid_separable(sep)
            shares = getattr(self, '_grid_shares', None)
            if shares is not None and hasattr(self._matrix_d, 'set_grid_shares'):
                for w in sorted(shares):
                    self._matrix_d.set_grid_shares(w, *shares[w])
            dims = getattr(self, '_grid_dims', None) or getattr(self._matrix, '_grid_dims', None)
            if dims is not None and hasattr(self._matrix_d, 'set_grid_dims'):
                self._matrix_d.set_grid_dims(*dims)          # (n0, nm, ns), n0 fastest: the grid the columns form
        return self._matrix_d

    def csrmm_bytes(self, x, y, beta, forward):
        """The reference's traffic model for one csrmm (operators.py:246-256)."""
        M = self._get_or_create_device_matrix()
        read_frac, write_frac = (M._col_frac, M._row_frac) if forward else (M._row_frac, M._col_frac)
        if beta == 0:
            y_part = 1
        elif beta == 1:
            y_part = write_frac * (1 if M._exwrite else 2)
        else:
            y_part = 2
        return M.nbytes + x.nbytes * read_frac + y.nbytes * y_part

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        M = self._get_or_create_device_matrix()
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            trace.add('csrmm' if 'csr' in type(M).__name__ else 'diamm', nbytes=self.csrmm_bytes(x, y, beta, forward),
                      nflops=5 * self._matrix.nnz * x.shape[1], shape=x.shape, forward=forward,
                      name=self._name)
        if forward:
            M.forward(y, x, alpha=alpha, beta=beta)
        else:
            M.adjoint(y, x, alpha=alpha, beta=beta)


class UnscaledFFT(MatrixFreeOperator):
    """Unnormalised n-dimensional DFT of every column (a column is an F-ordered volume)."""

    def __init__(self, backend, ft_shape, forward=True, **kwargs):
        self._ft_shape = tuple(int(s) for s in ft_shape)
        n = int(np.prod(self._ft_shape))
        super().__init__(backend, shape=(n, n), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        assert alpha == 1, "FFT expected alpha == 1, got %s" % alpha
        assert beta == 0, "FFT expected beta == 0, got %s" % beta
        batch = x.shape[1]
        X = x.reshape(self._ft_shape + (batch,))
        Y = y.reshape(self._ft_shape + (batch,))
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            n = self.shape[0]
            trace.add('fft', nbytes=4 * x.nbytes, nflops=batch * 5 * n * np.log2(n), shape=X.shape,
                      forward=forward, name=self._name)
        if forward:
            self._backend.fftn(Y, X)
        else:
            self._backend.ifftn(Y, X)

    def _mem_usage(self, ncols):
        ncols = min(ncols, self._batch or ncols)
        return self._backend._fft_workspace_size(self._ft_shape + (ncols,))


class ZpadFFT(MatrixFreeOperator):
    """Fused leaf  KronI(C, UnscaledFFT) * (I_C (x) Zpad) * VStack(Diag(w_c)):  image -> C oversampled k-space grids.

        forward :  y[:, c] = FFT( zeropad( w[:, c] * x ) )                    shape (C*P, N)
        adjoint :  x = sum_c conj(w[:, c]) * crop( IFFT( y[:, c] ) )

    Mathematically this is the `KronI(C, fft) * S'` part of the reference's `-O3` SENSE tree
    (examples/pics.py:104-193; Zpad backend.py:371-387, FFTc modulation :355-369, roll-off :439-440)
    with the (C*P) x N CSR matrix S' replaced by its generator: a box position and one complex weight
    per voxel and coil.  A backend that implements `fft_padded / ifft_cropped / sum_columns` can skip
    the zero parts of the grid inside the transform; the numpy oracle implements the same three calls
    with dense arrays, and tests pin both to the reference's S' + FFT composition.
    """

    def __init__(self, backend, grid_shape, box_shape, weights, box_lo=None, layout=0, support=None, support_tile=16, kshift=None, **kwargs):
        # memory order of the output grids: 0 = (x, y, z) per coil, 1 = (x, z, y) per coil, 2 = (c, x, z, y) coils interleaved
        self._layout = int(layout)
        # optional k-space support table (layout 1): int16 [z_lo, z_hi) per (kx tile of 16, ky); outside it the
        # forward grid is left unwritten and the adjoint's input is taken as zero (see ig_fft_exec_padded)
        self._support_h = None if support is None else np.ascontiguousarray(support, dtype=np.int16)
        self._support_d = None
        # kx points per entry of the support table (layout 2 on backends that take a finer table: ig_fft_set_support_tile)
        self._tile_kw = {} if int(support_tile) == 16 else {'support_tile': int(support_tile)}
        # circular shifts on the image side of the y / z axes that the transform itself carries (layout 2, chirp-z axes: ig_fft_set_axis_shift)
        # = the centred transform's modulation on an odd axis, which the gridding matrix to the left then does not hold
        if kshift is not None and any(int(v) for v in kshift):
            assert int(layout) == 2 and int(kshift[0]) == 0
            self._tile_kw['kshift'] = tuple(int(v) for v in kshift)
        self._grid = tuple(int(s) for s in grid_shape)
        self._box = tuple(int(s) for s in box_shape)
        assert len(self._grid) == 3 and len(self._box) == 3
        if box_lo is None:      # centred, as Backend.Zpad(mode='center')
            box_lo = tuple(m // 2 + int(np.ceil(-n / 2)) for m, n in zip(self._grid, self._box))
        self._lo = tuple(int(s) for s in box_lo)
        w = np.asarray(weights, dtype=_C64)
        # layout 2 wants the coils of a voxel side by side: an array that already is (voxels in F order) x (coils, contiguous)
        # -- SenseProblem.fused_weights(interleaved=True) -- is kept as it is instead of being turned coil-major and back
        if not (self._layout == 2 and w.ndim == 4 and w.reshape((-1, w.shape[3]), order='F').flags['C_CONTIGUOUS']):
            w = np.asfortranarray(w)
        assert w.shape[:3] == self._box, "weights must be box_shape + (ncoils,)"
        self._C = int(w.shape[3])
        self._w_h = w
        self._w_d = None
        P, N = int(np.prod(self._grid)), int(np.prod(self._box))
        super().__init__(backend, shape=(self._C * P, N), **kwargs)

    def _support(self):
        if self._support_h is None:
            return None
        if self._support_d is None:
            self._support_d = self._backend.copy_array(self._support_h.reshape(-1), name=self._name + '.support')
        return self._support_d

    def _weights(self):
        if self._w_d is None:
            w2 = self._w_h.reshape((-1, self._C), order='F')
            if self._layout == 2:       # interleaved: w[i*C + c]
                w2 = np.ascontiguousarray(w2).reshape(-1)
            self._w_d = self._backend.copy_array(w2, name=self._name + '.weights')
            self._w_h = None
        return self._w_d

    def _trace(self, forward):
        trace = getattr(self._backend, 'trace', None)
        if trace is None:
            return
        # book what the reference's S' csrmm + batched FFT would move for the same result
        P, N, C = int(np.prod(self._grid)), int(np.prod(self._box)), self._C
        nnz = C * N
        mat = nnz * 12 + (N + 1) * 4                  # S'^H stored as N x (C*P) CSR
        if forward:
            spmm = mat + N * 8 * 1.0 + C * P * 8 * 1
        else:
            spmm = mat + C * P * 8 * (nnz / (C * P)) + N * 8 * 1
        trace.add('csrmm', nbytes=spmm, nflops=5 * nnz, name=self._name + '.S', forward=forward, fused=True)
        trace.add('fft', nbytes=4 * C * P * 8, nflops=C * 5 * P * np.log2(P), name=self._name + '.F', forward=forward, fused=True)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        B = self._backend
        P, N, C = int(np.prod(self._grid)), int(np.prod(self._box)), self._C
        ncols = x.shape[1]
        w = self._weights()
        for j in range(ncols):
            xj = x if ncols == 1 else x[:, j:j + 1]
            yj = y if ncols == 1 else y[:, j:j + 1]
            self._trace(forward)
            if forward:
                assert beta == 0, "ZpadFFT forward expects beta == 0, got %s" % beta
                if self._layout:
                    with B.scratch(nbytes=self._ws_bytes()) as ws:
                        B.fft_padded(yj.reshape((P, C)), xj, w, self._grid, self._lo, self._box, ws, self._layout,
                                     self._support(), **self._tile_kw)
                else:
                    B.fft_padded(yj.reshape((P, C)), xj, w, self._grid, self._lo, self._box)
                if alpha != 1:
                    B.scale(yj, alpha)
            elif self._layout == 2 and hasattr(B, 'ifft_cropped_sum'):
                # coil combination inside the transform's last pass: no per-coil image arrays at all
                hook = getattr(self, '_slab_hook', None)
                if alpha == 1 and hook is not None and ncols == 1:
                    # multi-GPU: the image leaves slab by slab -- hook(y, lo, hi) all-reduces voxels [lo, hi) of y on the
                    # communicator's stream while the next slab is still being transformed (indigo_amd/dist.py).  beta != 0
                    # (the last coil chunk of a VStack: y already holds the earlier chunks' images): the slab goes through
                    # an accumulator and is added to y before it leaves.
                    nslabs, fn = hook
                    b2, plane = self._box[2], self._box[0] * self._box[1]
                    with (B.scratch(shape=(N, 1)) if beta != 0 else contextlib.nullcontext()) as acc:
                        with B.scratch(nbytes=self._ws_bytes()) as ws:
                            xg = xj.reshape((P, C))
                            dst = acc if beta != 0 else yj
                            B.ifft_cropped_sum(dst, xg, w, self._grid, self._lo, self._box, ws, self._support(), slab='z', **self._tile_kw)
                            edges = [b2 * i // nslabs for i in range(nslabs + 1)]
                            for z0, z1 in zip(edges[:-1], edges[1:]):
                                if z1 > z0:
                                    B.ifft_cropped_sum(dst, xg, w, self._grid, self._lo, self._box, ws, self._support(), slab=(z0, z1), **self._tile_kw)
                                    if beta != 0:
                                        B.axpby(beta, yj[z0 * plane:z1 * plane], 1, acc[z0 * plane:z1 * plane])
                                    fn(yj, z0 * plane, z1 * plane)
                elif alpha == 1 and beta == 0:
                    with B.scratch(nbytes=self._ws_bytes()) as ws:
                        B.ifft_cropped_sum(yj, xj.reshape((P, C)), w, self._grid, self._lo, self._box, ws, self._support(), **self._tile_kw)
                else:
                    # (a read-modify-write of y inside the pass was measured slower than this extra axpby over one image)
                    with B.scratch(shape=(N, 1)) as acc:
                        with B.scratch(nbytes=self._ws_bytes()) as ws:
                            B.ifft_cropped_sum(acc, xj.reshape((P, C)), w, self._grid, self._lo, self._box, ws, self._support(), **self._tile_kw)
                        B.axpby(beta, yj, alpha, acc)
            elif (self._layout == 1 and C == 1 and alpha == 1 and beta == 0 and ncols == 1 and getattr(self, '_slab_hook', None) is not None
                  and hasattr(B, 'ifft_cropped_sum')):
                # one coil on a rank of a coil-sharded run (per-coil grid layout): the image IS the cropped transform of the one
                # column -- written straight into y, slab by slab, every finished slab handed to the all-reduce hook
                nslabs, fn = self._slab_hook
                b2, plane = self._box[2], self._box[0] * self._box[1]
                with B.scratch(nbytes=self._ws_bytes()) as ws:
                    xg = xj.reshape((P, C))
                    B.ifft_cropped(yj, xg, w, self._grid, self._lo, self._box, ws, 1, self._support(), slab='z')
                    edges = [b2 * i // nslabs for i in range(nslabs + 1)]
                    for z0, z1 in zip(edges[:-1], edges[1:]):
                        if z1 > z0:
                            B.ifft_cropped(yj, xg, w, self._grid, self._lo, self._box, ws, 1, self._support(), slab=(z0, z1))
                            fn(yj, z0 * plane, z1 * plane)
            else:
                with B.scratch(shape=(N, C)) as tmp:
                    with B.scratch(nbytes=self._ws_bytes()) as ws:
                        B.ifft_cropped(tmp, xj.reshape((P, C)), w, self._grid, self._lo, self._box, ws, self._layout,
                                       self._support(), **self._tile_kw)
                    if self._layout == 2:
                        B.sum_columns(yj, tmp, alpha=alpha, beta=beta, interleaved=True)
                    else:
                        B.sum_columns(yj, tmp, alpha=alpha, beta=beta)

    def _ws_bytes(self):
        return self._backend._fft_padded_workspace(self._grid, self._lo, self._box, self._C, self._layout)

    def _mem_usage(self, ncols):
        N, C = int(np.prod(self._box)), self._C
        return (N * C * 8 + 255) // 256 * 256 + self._ws_bytes()


class ZpadFFTMaps(ZpadFFT):
    """The fused leaf `ZpadFFT` with M images on its image side: soft-SENSE, M sets of coil maps, shape (C*P, N*M).

        forward :  y[:, c] = FFT( zeropad( sum_m S'[:, c, m] * x_m ) )
        adjoint :  x_m = sum_c conj(S'[:, c, m]) * crop( IFFT( y[:, c] ) )

    The input is M images stacked map-major, image m in rows [mN, (m+1)N).  `weights` (box + (C,)) are the per-voxel weights of the
    `ZpadFFT` this leaf replaces in a tree built from unit maps (modulation x roll-off x gridding constant, zero for the padding
    coils of a chunk), `maps` (box + (ncoils, M)) the chunk's `ncoils` <= C real coils of every set: S' = weights x maps, padded
    with zero coils to the chunk's width C.  Grid, box, layout, support table, support tile and kshift are `ZpadFFT`'s, and so are
    the transform kernels: forward, `Backend.coil_maps` writes W = sum_m S'_m x_m into a scratch panel in the leaf's weight layout
    and `fft_padded` transforms an image of ones with the weights W; adjoint, `ifft_cropped` with unit weights leaves the C cropped
    coil images in a scratch panel (coil-interleaved for layout 2) and `coil_maps(adjoint=True)` combines them into the M images
    with alpha and beta.  Forward expects beta == 0, as `ZpadFFT` does.  Scratch: one N x C panel and the transform's workspace."""

    def __init__(self, backend, grid_shape, box_shape, weights, maps, ncoils, **kwargs):
        super().__init__(backend, grid_shape, box_shape, weights, **kwargs)
        real = int(ncoils)
        maps = np.asarray(maps, dtype=_C64)
        if maps.ndim != 5 or maps.shape[:3] != self._box or maps.shape[3] != real or not 1 <= real <= self._C:
            raise ValueError("ZpadFFTMaps: maps must be box + (ncoils, sets) with ncoils <= %d, got shape %s for box %s and %d coils"
                             % (self._C, maps.shape, self._box, real))
        M = int(maps.shape[4])
        if not 1 <= M <= 4:
            raise ValueError("ZpadFFTMaps: %d sets of maps, between 1 and 4 are supported" % M)
        self._real, self._M = real, M
        N = int(np.prod(self._box))
        w2 = self._w_h.reshape((N, self._C), order='F')
        m2 = maps.reshape((N, real, M), order='F')
        # M planes in the form of the leaf's weights: layout 2 a voxel's C slots side by side, else one coil image after the other
        planes = np.zeros((M, N, self._C) if self._layout == 2 else (M, self._C, N), dtype=_C64)
        for m in range(M):
            prod = w2[:, :real] * m2[:, :, m]
            if self._layout == 2:
                planes[m, :, :real] = prod
            else:
                planes[m, :real, :] = prod.T
        self._w_h = None
        self._s_h, self._s_d, self._ones_d = planes.reshape(-1), None, None
        self._shape = (self._shape[0], N * M)

    def _maps(self):
        if self._s_d is None:
            self._s_d = self._backend.copy_array(self._s_h, name=self._name + '.maps')
            self._s_h = None
            N = int(np.prod(self._box))
            self._ones_d = self._backend.copy_array(np.ones((N * self._C, 1), dtype=_C64), name=self._name + '.ones')
        return self._s_d

    def maps_bytes(self):
        """device bytes of S' and of the unit weights"""
        return int(np.prod(self._box)) * self._C * (self._M + 1) * 8

    def _trace_maps(self, forward, beta):
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            N, C, M = int(np.prod(self._box)), self._real, self._M
            trace.add('coil_maps', nbytes=8 * N * (C * M + C + M) + (0 if beta == 0 else 8 * N * M), nflops=8 * N * C * M,
                      shape=(N, C, M), forward=forward, name=self._name + '.maps')

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        B = self._backend
        P, N, C, M = int(np.prod(self._grid)), int(np.prod(self._box)), self._C, self._M
        il = self._layout == 2
        S = self._maps()
        ncols = x.shape[1]
        for j in range(ncols):
            xj = x if ncols == 1 else x[:, j:j + 1]
            yj = y if ncols == 1 else y[:, j:j + 1]
            self._trace(forward)
            self._trace_maps(forward, 0 if forward else beta)
            if forward:
                assert beta == 0, "ZpadFFTMaps forward expects beta == 0, got %s" % beta
                with B.scratch(shape=(N * C, 1)) as W:
                    B.coil_maps(W, xj, S, N, self._real, M, alpha=alpha, interleaved=il, width=C if il else None)
                    ones = self._ones_d.dense_rows(0, N)
                    if self._layout:
                        with B.scratch(nbytes=self._ws_bytes()) as ws:
                            B.fft_padded(yj.reshape((P, C)), ones, W, self._grid, self._lo, self._box, ws, self._layout,
                                         self._support(), **self._tile_kw)
                    else:
                        B.fft_padded(yj.reshape((P, C)), ones, W, self._grid, self._lo, self._box)
            else:
                with B.scratch(shape=(N, C)) as tmp:
                    with B.scratch(nbytes=self._ws_bytes()) as ws:
                        B.ifft_cropped(tmp, xj.reshape((P, C)), self._ones_d, self._grid, self._lo, self._box, ws, self._layout,
                                       self._support(), **self._tile_kw)
                    B.coil_maps(yj, tmp, S, N, self._real, M, adjoint=True, alpha=alpha, beta=beta, interleaved=il, width=C if il else None)


class CoilMaps(MatrixFreeOperator):
    """The map stack of soft-SENSE: `maps` is a host array dims + (C, M), M sets of C coil maps on a volume of N voxels; shape
    (N C, N M).  The input is M images stacked map-major, image m in rows [mN, (m+1)N); the output is C coil images stacked
    coil-major, coil image c = sum_m maps[..., c, m] * image m in rows [cN, (c+1)N), as `KronI(C, NUFFT)` consumes them.  .H is the
    adjoint, image m = sum_c conj(maps[..., c, m]) * coil image c.  M <= 4.  The maps go to the device once, on first evaluation.
    With M = 1 it equals VStack(Diag(map_c)); it is the leaf of every soft-SENSE tree that does not run through `ZpadFFTMaps`
    (DESIGN.md §3.12)."""

    def __init__(self, backend, maps, **kwargs):
        try:
            maps = np.asarray(maps, dtype=_C64)
        except (TypeError, ValueError):
            raise ValueError("CoilMaps: the maps do not convert to complex64")
        if maps.ndim < 3 or min(maps.shape) < 1:
            raise ValueError("CoilMaps: maps must be dims + (coils, sets), got shape %s" % (maps.shape,))
        C, M = int(maps.shape[-2]), int(maps.shape[-1])
        if not 1 <= M <= 4:
            raise ValueError("CoilMaps: %d sets of maps, between 1 and 4 are supported" % M)
        self._n = int(np.prod(maps.shape[:-2]))
        self._C, self._M = C, M
        self._matrix = np.asfortranarray(maps.reshape((self._n * C * M, 1), order='F'))          # element (i, c, m) at i + n c + n C m
        self._matrix_d = None
        kwargs.setdefault('name', 'maps')
        super().__init__(backend, shape=(self._n * C, self._n * M), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        if self._matrix_d is None:
            self._matrix_d = self._backend.copy_array(self._matrix, name=self._name)
        n, C, M = self._n, self._C, self._M
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # a single pass: every map, every coil image and every image moves once (8 B per voxel each); beta != 0 reads the output
            trace.add('coil_maps', nbytes=8 * n * (C * M + C + M) * x.shape[1] + (0 if beta == 0 else y.nbytes), nflops=8 * n * C * M * x.shape[1],
                      shape=x.shape, forward=forward, name=self._name)
        if x.shape[1] == 1:
            return self._backend.coil_maps(y, x, self._matrix_d, n, C, M, adjoint=not forward, alpha=alpha, beta=beta)
        for j in range(x.shape[1]):             # the images become the columns of a panel inside: one product per column
            self._backend.coil_maps(y[:, j:j + 1], x[:, j:j + 1], self._matrix_d, n, C, M, adjoint=not forward, alpha=alpha, beta=beta)

    def _mem_usage(self, ncols):
        return 0            # (no scratch: the maps themselves are counted with the matrices, analyses.Memusage)


class NlinvProduct(MatrixFreeOperator):
    """The derivative of NLINV's bilinear coil product rho * c_c at the point (rho, c), shape (n C, n (1 + C)).
    The input is (d rho | d c_1 ... d c_C), block b in rows [bn, (b+1)n); the output is C coil images stacked coil-major,
    coil image c = d rho * c_c + rho * d c_c, as `KronI(C, NUFFT)` consumes them.  .H is the adjoint:
    d rho = sum_c conj(c_c) * z_c, d c_c = conj(rho) * z_c.  The point is two device arrays, rho (n) and c (n x C), handed over with
    `set_point`: the Newton iteration swaps them between steps without rebuilding the tree, and the leaf keeps no copy."""

    def __init__(self, backend, n, ncoils, **kwargs):
        self._n, self._C = int(n), int(ncoils)
        if self._n < 1 or self._C < 1:
            raise ValueError("NlinvProduct: %d voxels and %d coils, at least 1 each is supported" % (self._n, self._C))
        self._rho_d = self._coils_d = None
        kwargs.setdefault('name', 'nlinv product')
        super().__init__(backend, shape=(self._n * self._C, self._n * (1 + self._C)), **kwargs)

    def set_point(self, rho_d, coils_d):
        """the linearisation point: device arrays of n and n C elements, read at every evaluation until the next call"""
        if rho_d.size != self._n or coils_d.size != self._n * self._C:
            raise ValueError("NlinvProduct.set_point: rho %s and coils %s for %d voxels and %d coils" % (rho_d.shape, coils_d.shape, self._n, self._C))
        self._rho_d, self._coils_d = rho_d, coils_d

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        if self._rho_d is None:
            raise RuntimeError("NlinvProduct: no linearisation point, call set_point(rho, coils) first")
        n, C = self._n, self._C
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # a single pass: rho, the coils, x and y move once (8 B per voxel each); beta != 0 reads the output
            trace.add('nlinv_product', nbytes=8 * n * (3 * C + 2) * x.shape[1] + (0 if beta == 0 else y.nbytes), nflops=16 * n * C * x.shape[1],
                      shape=x.shape, forward=forward, name=self._name)
        if x.shape[1] == 1:
            return self._backend.nlinv_product(y, x, self._rho_d, self._coils_d, n, C, adjoint=not forward, alpha=alpha, beta=beta)
        for j in range(x.shape[1]):             # the blocks become the columns of a panel inside: one product per column
            self._backend.nlinv_product(y[:, j:j + 1], x[:, j:j + 1], self._rho_d, self._coils_d, n, C, adjoint=not forward, alpha=alpha, beta=beta)

    def _mem_usage(self, ncols):
        return 0            # (no scratch; the point belongs to the caller)


class SobolevCoils(MatrixFreeOperator):
    """The coil weighting of NLINV on the unknown u = (rho, c^_1 ... c^_C) of an F-ordered `dims` volume of N voxels, shape
    (N (1 + C), N (1 + C)): rows [0, N) (rho) are copied through; every c^_c becomes the coil sensitivity

        c_c = W c^_c = (1 / sqrt N) ifftn( w * c^_c ),      W^H z = w * fftn(z) / sqrt N,      w(k) = (1 + a |kappa|^2)^(-b/2)

    with the backend's plain, uncentred, unnormalised transforms (Backend.sobolev_weights).  w is real and even, so
    W commutes with shifts and no centring modulation is needed.  Forward is `sobolev_weight` (scale 1 / sqrt N) and `ifftn` in
    place on the dims + (C,) view; the adjoint is `fftn`, then `sobolev_weight`.  With a real alpha and beta == 0 both run in the
    output; otherwise the coil part goes through a scratch panel of N C elements and one axpby."""

    def __init__(self, backend, dims, ncoils, a, b, **kwargs):
        self._dims = tuple(int(n) for n in dims)
        self._C = int(ncoils)
        if len(self._dims) != 3 or min(self._dims) < 1 or self._C < 1:
            raise ValueError("SobolevCoils: dims must be three positive lengths and coils at least 1, got %s and %s" % (dims, ncoils))
        if not float(a) >= 0:
            raise ValueError("SobolevCoils: a = %s, a non-negative value is supported" % (a,))
        self._a, self._b = float(a), float(b)
        self._N = int(np.prod(self._dims))
        kwargs.setdefault('name', 'sobolev coils')
        super().__init__(backend, shape=(self._N * (1 + self._C),) * 2, **kwargs)

    def _coil_part(self, yc, xc, alpha, beta, forward):
        """yc = beta*yc + alpha * (W or W^H) xc on contiguous vectors of N C elements"""
        B, N, C = self._backend, self._N, self._C
        vol = self._dims + (C,)
        s = 1.0 / np.sqrt(float(N))

        def run(dst, scale):
            if forward:
                B.sobolev_weight(dst, xc, self._dims, C, self._a, self._b, scale=scale)
                B.ifftn(dst.reshape(vol), dst.reshape(vol))
            else:
                B.fftn(dst.reshape(vol), xc.reshape(vol))
                B.sobolev_weight(dst, dst, self._dims, C, self._a, self._b, scale=scale)

        if beta == 0 and np.imag(alpha) == 0:
            run(yc, s * float(np.real(alpha)))
        else:
            with B.scratch(shape=(N * C, 1)) as tmp:
                run(tmp, s)
                B.axpby(beta, yc, alpha, tmp)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        B, N, C = self._backend, self._N, self._C
        trace = getattr(B, 'trace', None)
        for j in range(x.shape[1]):
            xj = x if x.shape[1] == 1 else x[:, j:j + 1]
            yj = y if x.shape[1] == 1 else y[:, j:j + 1]
            if trace is not None:
                # the weight pass moves 16 B per element and the transform is booked as UnscaledFFT books it; rho is one axpby
                trace.add('sobolev_weight', nbytes=16 * N * C, nflops=2 * N * C, shape=(N, C), forward=forward, name=self._name)
                trace.add('fft', nbytes=4 * 8 * N * C, nflops=C * 5 * N * np.log2(max(N, 2)), shape=self._dims + (C,), forward=forward, name=self._name + '.F')
                trace.add('axpby', nbytes=8 * N * (2 if beta == 0 else 3), name=self._name + '.rho')
            B.axpby(beta, yj.dense_rows(0, N), alpha, xj.dense_rows(0, N))
            self._coil_part(yj.dense_rows(N, N * (1 + C)), xj.dense_rows(N, N * (1 + C)), alpha, beta, forward)

    def _mem_usage(self, ncols):
        # the scratch panel of a complex alpha or a beta != 0, and what the in-place transform takes
        return (self._N * self._C * 8 + 255) // 256 * 256 + self._backend._fft_workspace_size(self._dims + (self._C,))


class AxisPermute(MatrixFreeOperator):
    """Relabelling of the axes of an F-ordered image volume of shape `dims`: output axis a is input axis perm[a], i.e.
    y = x.reshape(dims, order='F').transpose(perm).ravel(order='F');  the adjoint is the inverse permutation.  Pure data
    movement (backend.permute3), shape (N, N).

    What lets the fused SENSE leaf run a grid it refuses: the NUFFT is separable, so relabelling the image axes relabels
    the grid axes, the trajectory rows, the roll-off, the maps and the modulation phases and nothing else --
    A = A_perm * AxisPermute(N, perm), with A_perm the leaf on the permuted problem (indigo_amd.fused.image_permutation)."""

    def __init__(self, backend, dims, perm, **kwargs):
        self._dims = tuple(int(n) for n in dims)
        self._perm = tuple(int(p) for p in perm)
        assert len(self._dims) == 3 and sorted(self._perm) == [0, 1, 2], (dims, perm)
        self._inv = tuple(int(a) for a in np.argsort(self._perm))
        n = int(np.prod(self._dims))
        kwargs.setdefault('name', 'permute%s' % (self._perm,))
        super().__init__(backend, shape=(n, n), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        dims, perm = (self._dims, self._perm) if forward else (tuple(self._dims[p] for p in self._perm), self._inv)
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            trace.add('permute', nbytes=x.nbytes + y.nbytes * (1 if beta == 0 else 2), nflops=0, shape=x.shape,
                      forward=forward, name=self._name)
        self._backend.permute3(y, x, dims, perm, alpha=alpha, beta=beta)


class Wavelet(MatrixFreeOperator):
    """The orthonormal periodic multi-level wavelet transform of an F-ordered complex64 volume of shape `dims` (2-D: dims[2] == 1),
    shape (N, N): Daubechies filters 'haar', 'db2' or 'db4' (backend.WAVELETS), at most `levels` levels (backend.dwt_plan),
    coefficients in place of the samples, the coarse approximation band in the corner box `coarse`.  Unitary: .H is the inverse.
    Every axis is at most 1024 long (the HIP kernel stages whole lines in LDS).  The sparsifying transform of pics --l1."""

    def __init__(self, backend, dims, wavelet='db2', levels=3, **kwargs):
        from indigo_amd.backends.backend import DWT_MAX_AXIS, WAVELETS, dwt_plan
        self._dims = tuple(int(n) for n in dims)
        if len(self._dims) != 3 or min(self._dims) < 1:
            raise ValueError("Wavelet: dims must be three positive lengths, got %s" % (dims,))
        if max(self._dims) > DWT_MAX_AXIS:
            raise ValueError("Wavelet: axes are at most %d long, got %s" % (DWT_MAX_AXIS, self._dims))
        if wavelet not in WAVELETS:
            raise ValueError("Wavelet: unknown wavelet %r (one of %s)" % (wavelet, ", ".join(sorted(WAVELETS))))
        self._wavelet, self._levels = wavelet, int(levels)
        passes, self.coarse = dwt_plan(self._dims, wavelet, self._levels)
        self._pass_elems = sum(int(np.prod(box)) for box, _ in passes)
        n = int(np.prod(self._dims))
        kwargs.setdefault('name', 'wavelet(%s, %d)' % (wavelet, self._levels))
        super().__init__(backend, shape=(n, n), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # every split pass reads and writes its box once (16 B per element); beta != 0 runs the transform twice
            # (y = beta y + alpha W x = W (beta W^H y + alpha x)) around a combining pass
            ncols = x.shape[1]
            nbytes = 16 * self._pass_elems * ncols * (1 if beta == 0 else 2) + (0 if beta == 0 else 24 * self.shape[0] * ncols)
            trace.add('wavelet', nbytes=nbytes, nflops=0, shape=x.shape, forward=forward, name=self._name)
        self._backend.dwt3(y, x, self._dims, self._wavelet, self._levels, inverse=not forward, alpha=alpha, beta=beta)


class Gradient(MatrixFreeOperator):
    """The forward-difference gradient D of an F-ordered complex64 volume of shape `dims` with N voxels (2-D: dims[2] == 1), shape
    (3N, N): (D_a x)[i] = x[i + e_a] - x[i] where i_a < n_a - 1 and 0 on the far face, component a in rows [aN, (a+1)N); an
    axis of length 1 contributes nothing.  .H is the adjoint (minus the divergence); ||D||^2 <= 4 per axis longer than 1.
    The analysis operator of pics --tv."""

    def __init__(self, backend, dims, **kwargs):
        self._dims = tuple(int(n) for n in dims)
        if len(self._dims) != 3 or min(self._dims) < 1:
            raise ValueError("Gradient: dims must be three positive lengths, got %s" % (dims,))
        n = int(np.prod(self._dims))
        kwargs.setdefault('name', 'gradient')
        super().__init__(backend, shape=(3 * n, n), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # either way one volume and three components move (32 B per voxel); beta != 0 reads the output as well
            trace.add('gradient', nbytes=32 * self.shape[1] * x.shape[1] + (0 if beta == 0 else y.nbytes), nflops=0,
                      shape=x.shape, forward=forward, name=self._name)
        self._backend.grad3(y, x, self._dims, adjoint=not forward, alpha=alpha, beta=beta)


class SymGradient(MatrixFreeOperator):
    """The symmetrised backward difference E of a 3-component complex64 field on an F-ordered volume of shape `dims` with N voxels,
    shape (6N, 3N): component a of the input in rows [aN, (a+1)N), the components xx, yy, zz, xy, xz, yz of the output in rows
    [cN, (c+1)N).  With B_a = -D_a^H the backward difference that matches `Gradient`: (E v)_aa = B_a v_a and (E v)_ab = (B_b v_a +
    B_a v_b) / sqrt(2), stored once, so that the 2-norm of the six is the Frobenius norm of the symmetric tensor.  .H is the adjoint;
    ||E||^2 <= 12.  The second analysis operator of pics --tgv."""

    def __init__(self, backend, dims, **kwargs):
        self._dims = tuple(int(n) for n in dims)
        if len(self._dims) != 3 or min(self._dims) < 1:
            raise ValueError("SymGradient: dims must be three positive lengths, got %s" % (dims,))
        n = int(np.prod(self._dims))
        kwargs.setdefault('name', 'symgradient')
        super().__init__(backend, shape=(6 * n, 3 * n), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # either way three components and six move (72 B per voxel); beta != 0 reads the output as well
            trace.add('symgradient', nbytes=72 * (self.shape[1] // 3) * x.shape[1] + (0 if beta == 0 else y.nbytes), nflops=0,
                      shape=x.shape, forward=forward, name=self._name)
        self._backend.symgrad3(y, x, self._dims, adjoint=not forward, alpha=alpha, beta=beta)


class GradientT(MatrixFreeOperator):
    """The gradient D4 of T = `frames` time frames of an F-ordered complex64 volume of shape `dims` with N voxels, shape (4NT, NT).
    The input is frame-major, frame t in rows [tN, (t+1)N); the output holds 4N rows per frame: components 0..2 are `Gradient`'s
    D x_t, component 3 is the forward difference in time x_{t+1} - x_t, 0 in the last frame.  .H is the adjoint, which does not
    read the temporal component of the last frame.  ||D4||^2 <= 4 * (axes longer than 1, time included) <= 16.  frames == 1 is
    `Gradient` with a zero fourth component.  The analysis operator of pics --tv / --tv-time on several frames."""

    def __init__(self, backend, dims, frames, **kwargs):
        self._dims = tuple(int(n) for n in dims)
        self._frames = int(frames)
        if len(self._dims) != 3 or min(self._dims) < 1:
            raise ValueError("GradientT: dims must be three positive lengths, got %s" % (dims,))
        if self._frames < 1:
            raise ValueError("GradientT: frames must be positive, got %s" % (frames,))
        n = int(np.prod(self._dims)) * self._frames
        kwargs.setdefault('name', 'gradient_t')
        super().__init__(backend, shape=(4 * n, n), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # one volume and four components per frame (40 B per voxel, adjoint 32: the last frame's temporal component is
            # not read) and the neighbouring frame again, T - 1 times (8 B, adjoint 16); beta != 0 reads the output as well
            n, T = self.shape[1] // self._frames, self._frames
            per_col = n * (T * 40 + (T - 1) * 8) if forward else n * (T * 32 + (T - 1) * 16)
            trace.add('gradient_t', nbytes=per_col * x.shape[1] + (0 if beta == 0 else y.nbytes), nflops=0,
                      shape=x.shape, forward=forward, name=self._name)
        if x.shape[1] == 1:
            return self._backend.grad4(y, x, self._dims, self._frames, adjoint=not forward, alpha=alpha, beta=beta)
        for j in range(x.shape[1]):             # the frames become the columns of a panel inside: one product per column
            self._backend.grad4(y[:, j:j + 1], x[:, j:j + 1], self._dims, self._frames, adjoint=not forward, alpha=alpha, beta=beta)


class FrameBasis(MatrixFreeOperator):
    """Phi (x) I_n: the temporal-subspace operator of a T x K complex64 basis `phi` on images of `n` voxels, shape (nT, nK).  The
    input is K coefficient images stacked coefficient-major, image k in rows [kn, (k+1)n); the output is T frames stacked
    frame-major, frame t = sum_k phi[t, k] * image k in rows [tn, (t+1)n), as `BlockDiag` and `GradientT` expect them.  .H is
    the adjoint, image k = sum_t conj(phi[t, k]) * frame t.  Phi need not be orthonormal; K <= 32.  The basis goes to the
    device once, on first evaluation.  The synthesis operator of pics --basis."""

    def __init__(self, backend, phi, n, **kwargs):
        try:
            phi = np.require(np.asarray(phi), dtype=_C64, requirements='F')
        except (TypeError, ValueError):
            raise ValueError("FrameBasis: the basis does not convert to complex64")
        if phi.ndim != 2:
            raise ValueError("FrameBasis: the basis must be 2-D (frames x coefficients), got shape %s" % (phi.shape,))
        T, K = phi.shape
        if not 1 <= K <= 32 or T < 1:
            raise ValueError("FrameBasis: a basis of %d frames x %d coefficients; between 1 and 32 coefficients and at least one "
                             "frame are supported" % (T, K))
        self._n = int(n)
        if self._n < 1:
            raise ValueError("FrameBasis: n must be positive, got %s" % (n,))
        self._matrix = phi
        self._matrix_d = None
        kwargs.setdefault('name', 'basis')
        super().__init__(backend, shape=(self._n * T, self._n * K), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        if self._matrix_d is None:
            self._matrix_d = self._backend.copy_array(self._matrix, name=self._name)
        T, K = self._matrix.shape
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # a single pass: every coefficient image and every frame moves once (8 B per voxel each); beta != 0 reads the output
            trace.add('frame_basis', nbytes=8 * self._n * (K + T) * x.shape[1] + (0 if beta == 0 else y.nbytes), nflops=0,
                      shape=x.shape, forward=forward, name=self._name)
        if x.shape[1] == 1:
            return self._backend.frame_basis(y, x, self._matrix_d, self._n, adjoint=not forward, alpha=alpha, beta=beta)
        for j in range(x.shape[1]):             # the images become the columns of a panel inside: one product per column
            self._backend.frame_basis(y[:, j:j + 1], x[:, j:j + 1], self._matrix_d, self._n, adjoint=not forward, alpha=alpha, beta=beta)


class SegmentPhase(MatrixFreeOperator):
    """The voxel side of the time-segmented off-resonance model, shape (nL, n): the image of `n` voxels times exp(-2 pi i f tau_l)
    for every one of the L <= 16 segment times `taus` (seconds, equispaced), the segments stacked segment-major, segment l in rows
    [ln, (l+1)n), as `BlockDiag` expects them.  `f` is the field map in Hz, n real values; it is rounded to float32 once and is
    from then on what those values say.  .H is the adjoint, image = sum_l exp(+2 pi i f tau_l) * segment l.  The field map goes
    to the device once, on first evaluation.  With `SegmentCombine` the forward model of pics --fmap."""

    def __init__(self, backend, f, taus, n, **kwargs):
        try:
            f = np.asarray(f)
            if np.iscomplexobj(f):
                raise TypeError
            f = np.ascontiguousarray(f.reshape(-1, order='F'), dtype=np.float32)
            taus = np.asarray(taus, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("SegmentPhase: the field map and the segment times must be real arrays")
        self._n = int(n)
        if self._n < 1:
            raise ValueError("SegmentPhase: n must be positive, got %s" % (n,))
        if f.size != self._n:
            raise ValueError("SegmentPhase: a field map of %d values for n = %d voxels" % (f.size, self._n))
        L = taus.size
        if not 1 <= L <= 16:
            raise ValueError("SegmentPhase: %d segments, between 1 and 16 are supported" % L)
        if not (np.isfinite(f).all() and np.isfinite(taus).all()):
            raise ValueError("SegmentPhase: the field map and the segment times must be finite")
        self._tau0, self._dtau = float(taus[0]), float(taus[1] - taus[0]) if L > 1 else 0.0
        if L > 2 and np.abs(taus - (self._tau0 + np.arange(L) * self._dtau)).max() > 1e-9 * np.abs(taus).max():
            raise ValueError("SegmentPhase: the segment times must be equispaced, got %s" % (taus,))
        self._L = L
        self._matrix = f
        self._matrix_d = None
        kwargs.setdefault('name', 'segment phase')
        super().__init__(backend, shape=(self._n * L, self._n), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        if self._matrix_d is None:
            self._matrix_d = self._backend.copy_array(self._matrix, name=self._name)
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # a single pass: the image and every segment move once (8 B per voxel each), the field map 4 B; beta != 0 reads the output
            trace.add('segment_phase', nbytes=(8 * self._n * (self._L + 1) + 4 * self._n) * x.shape[1] + (0 if beta == 0 else y.nbytes),
                      nflops=0, shape=x.shape, forward=forward, name=self._name)
        args = (self._matrix_d, self._tau0, self._dtau, self._L, self._n)
        if x.shape[1] == 1:
            return self._backend.segment_phase(y, x, *args, adjoint=not forward, alpha=alpha, beta=beta)
        for j in range(x.shape[1]):             # the segments become the columns of a panel inside: one product per column
            self._backend.segment_phase(y[:, j:j + 1], x[:, j:j + 1], *args, adjoint=not forward, alpha=alpha, beta=beta)


class SegmentCombine(MatrixFreeOperator):
    """The sample side of the time-segmented off-resonance model, shape (n, nL): sample r = sum_l b[r mod P, l] * (sample r of
    segment l) for the P x L complex64 interpolator table `b`, P = `period`, L <= 16, `n` a multiple of P.  The input is the L
    segments' samples stacked segment-major, segment l in rows [ln, (l+1)n), as `BlockDiag` leaves them.  P is the readout length
    when the sample times depend on the readout index alone, or the samples of one coil; the coils repeat the table.  .H is the
    adjoint, segment l = conj(b[r mod P, l]) * sample r.  The table goes to the device once, on first evaluation.  With
    `SegmentPhase` the forward model of pics --fmap."""

    def __init__(self, backend, b, period, n, **kwargs):
        try:
            b = np.require(np.asarray(b), dtype=_C64, requirements='F')
        except (TypeError, ValueError):
            raise ValueError("SegmentCombine: the table does not convert to complex64")
        if b.ndim != 2:
            raise ValueError("SegmentCombine: the table must be 2-D (period x segments), got shape %s" % (b.shape,))
        P, L = b.shape
        if not 1 <= L <= 16:
            raise ValueError("SegmentCombine: %d segments, between 1 and 16 are supported" % L)
        if int(period) != P or P < 1:
            raise ValueError("SegmentCombine: a table of %d rows for the period %s" % (P, period))
        self._n = int(n)
        if self._n < 1 or self._n % P:
            raise ValueError("SegmentCombine: n = %s rows are no positive multiple of the period %d" % (n, P))
        self._matrix = b
        self._matrix_d = None
        kwargs.setdefault('name', 'segment combine')
        super().__init__(backend, shape=(self._n, self._n * L), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        if self._matrix_d is None:
            self._matrix_d = self._backend.copy_array(self._matrix, name=self._name)
        P, L = self._matrix.shape
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            # a single pass: the samples and every segment move once (8 B per row each), the table once; beta != 0 reads the output
            trace.add('segment_combine', nbytes=(8 * self._n * (L + 1) + 8 * P * L) * x.shape[1] + (0 if beta == 0 else y.nbytes),
                      nflops=0, shape=x.shape, forward=forward, name=self._name)
        if x.shape[1] == 1:
            return self._backend.segment_combine(y, x, self._matrix_d, P, self._n, adjoint=not forward, alpha=alpha, beta=beta)
        for j in range(x.shape[1]):             # the segments become the columns of a panel inside: one product per column
            self._backend.segment_combine(y[:, j:j + 1], x[:, j:j + 1], self._matrix_d, P, self._n, adjoint=not forward, alpha=alpha, beta=beta)


class SampleWeights(MatrixFreeOperator):
    """diag(w) (x) I_ncols, shape (n ncols, n ncols): row i of every one of the `ncols` columns of `n` samples (the coils of a
    k-space vector stacked coil-major) times the real weight w[i].  Real, diagonal and self-adjoint: .H evaluates the same product.
    `w` is n real values, rounded to float32 once; n floats on the device where a `Diag` of the same operator would hold
    n ncols complex values and a CSR index.  With w the square roots of density-compensation weights, SampleWeights * A is the
    forward model of the weighted data term of pics --dcf.  The weights go to the device once, on first
    evaluation."""

    def __init__(self, backend, w, n, ncols, **kwargs):
        try:
            w = np.asarray(w)
            if np.iscomplexobj(w):
                raise TypeError
            w = np.ascontiguousarray(w.reshape(-1, order='F'), dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("SampleWeights: the weights must be a real array")
        self._n, self._ncols = int(n), int(ncols)
        if self._n < 1 or self._ncols < 1:
            raise ValueError("SampleWeights: n and ncols must be positive, got %s and %s" % (n, ncols))
        if w.size != self._n:
            raise ValueError("SampleWeights: %d weights for n = %d samples" % (w.size, self._n))
        if not np.isfinite(w).all():
            raise ValueError("SampleWeights: the weights must be finite")
        self._matrix = w
        self._matrix_d = None
        kwargs.setdefault('name', 'sample weights')
        super().__init__(backend, shape=(self._n * self._ncols,) * 2, **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        B = self._backend
        if self._matrix_d is None:
            self._matrix_d = B.copy_array(self._matrix, name=self._name)
        trace = getattr(B, 'trace', None)
        if trace is not None:
            # a single pass: every element moves once each way (8 B), the weights once per column of x
            trace.add('row_scale', nbytes=(16 * self._n * self._ncols + 4 * self._n) * x.shape[1] + (0 if beta == 0 else y.nbytes),
                      nflops=2 * self._n * self._ncols * x.shape[1], shape=x.shape, forward=forward, name=self._name)
        plain = alpha == 1 and beta == 0
        for j in range(x.shape[1]):
            xj, yj = (x, y) if x.shape[1] == 1 else (x[:, j:j + 1], y[:, j:j + 1])
            if plain:
                B.row_scale(yj, xj, self._matrix_d, self._n, self._ncols)
            else:
                with B.scratch(shape=(self.shape[0], 1)) as tmp:
                    B.row_scale(tmp, xj, self._matrix_d, self._n, self._ncols)
                    B.axpby(beta, yj, alpha, tmp)


class ToeplitzNormal(MatrixFreeOperator):
    """A^H A of a non-Cartesian SENSE problem -- in a temporal subspace of K coefficient images, or K = 1 for one frame -- as ONE
    Toeplitz operator, shape (N K, N K):

        (A^H A alpha)_k = sum_c S_c^H crop F^-1 ( sum_k' P_kk' . (F zpad S_c alpha_k') )

    S_c the coil maps `maps` (dims + (C,)), F the plain FFT on the grid of twice the image size `dims`, P the K x K Hermitian
    matrix of transformed point-spread functions at every grid point (indigo_amd.toeplitz.psf_kernel, all constants folded
    in).  No gridding, no per-frame trees, no frame panels: per evaluation C K padded transforms each way and one streaming
    pass (Backend.psf_mix).  The input and the output are K images stacked coefficient-major, as `FrameBasis` takes them.

    `kern` is a host float32 array (K^2, 8N): the planes of `Backend.psf_unpack`, each flattened in the memory order `order` of
    the grid: 'xyz' (F order) or 'xzy' (the order of ZpadFFT's layouts 1 and 2).  `memory_order(backend, dims)` tells which of
    the two the operator runs in; a kernel in the other order is transposed on the host before it is uploaded, once, on the
    first evaluation.  Where the backend has zero-pad-aware transforms for the grid (`supports_padded_fft`) the coils go through
    `ZpadFFT` leaves in the chunks of `fused.plan_chunks`; else through the unfused composition Crop * UnscaledFFT * Zpad, `chunk`
    coils at a time.  Scratch: K grid panels of one chunk, and what the chunk's transform takes.  Hermitian: .H is the
    operator itself.  DESIGN.md §3.11."""

    MAXK = 8          # the kernel array is 4 K^2 bytes per grid point: 8.6 GB at K = 4 on a 512^3 grid, 34 GB at K = 8, 137 GB at K = 16

    @staticmethod
    def memory_order(backend, dims):
        return 'xzy' if backend.supports_padded_fft(tuple(2 * int(n) for n in dims)) else 'xyz'

    def __init__(self, backend, dims, maps, kern, K, order='xyz', chunk=8, **kwargs):
        from indigo_amd import fused
        self._dims = tuple(int(n) for n in dims)
        if len(self._dims) != 3 or min(self._dims) < 1:
            raise ValueError("ToeplitzNormal: dims must be three positive lengths, got %s" % (dims,))
        self._K = int(K)
        if not 1 <= self._K <= self.MAXK:
            raise ValueError("ToeplitzNormal: %d coefficient images, between 1 and %d are supported: the kernel array holds 4 K^2 bytes "
                             "per grid point (34 GB at K = 8 on a 512^3 grid, 137 GB at K = 16)" % (self._K, self.MAXK))
        self._grid = tuple(2 * n for n in self._dims)
        N, P = int(np.prod(self._dims)), int(np.prod(self._grid))
        maps = np.asarray(maps, dtype=_C64)
        if maps.ndim == 3:
            maps = maps.reshape(maps.shape + (1,))
        if maps.ndim != 4 or maps.shape[:3] != self._dims:
            raise ValueError("ToeplitzNormal: maps must be dims + (coils,), got shape %s for dims %s" % (maps.shape, self._dims))
        C = self._C = int(maps.shape[3])
        kern = np.asarray(kern, dtype=np.float32)
        if kern.size != self._K ** 2 * P or order not in ('xyz', 'xzy'):
            raise ValueError("ToeplitzNormal: a kernel of %d floats in order %r; K^2 = %d planes of the %s grid in 'xyz' or 'xzy' order "
                             "are expected" % (kern.size, order, self._K ** 2, self._grid))
        self._kern_h, self._kern_order, self._kern_d = kern.reshape((self._K ** 2, P)), order, None
        self._order = self.memory_order(backend, self._dims)
        self._parts = []                                 # (transform operator, real coils, coil slots, interleaved)
        if self._order == 'xzy':
            single_ok = getattr(backend, 'supports_single_coil_layout', lambda g: True)(self._grid)
            tuning = getattr(backend, 'tuning', {})
            for lo, hi, w in fused.plan_chunks(C, chunk, single_ok, tuning.get('chunk_cost'), tuning.get('chunk_pad', True)):
                wts = fused.pad_coils(maps[..., lo:hi], w) if w > 1 else np.asfortranarray(maps[..., lo:hi])
                Z = backend.ZpadFFT(self._grid, self._dims, wts, layout=2 if w > 1 else 1, name='fft*zpad*maps')
                self._parts.append((Z, hi - lo, w, w > 1))
        else:
            for lo in range(0, C, int(chunk)):
                hi = min(lo + int(chunk), C)
                c = hi - lo
                S = backend.VStack([backend.Diag(maps[:, :, :, i].reshape(self._dims + (1,))) for i in range(lo, hi)], name='maps')
                F = backend.KronI(c, backend.UnscaledFFT(self._grid, name='fft')) * backend.KronI(c, backend.Zpad(self._grid, self._dims, name='zpad')) * S
                self._parts.append((F, c, c, False))
        kwargs.setdefault('name', 'toeplitz')
        super().__init__(backend, shape=(N * self._K, N * self._K), **kwargs)

    @property
    def H(self):
        return self

    def kernel_bytes(self):
        return self._K ** 2 * int(np.prod(self._grid)) * 4

    def _kernel(self):
        if self._kern_d is None:
            k = self._kern_h
            if self._kern_order != self._order:
                g = self._grid
                shape = (g[0], g[1], g[2]) if self._kern_order == 'xyz' else (g[0], g[2], g[1])
                k = np.stack([p.reshape(shape, order='F').transpose(0, 2, 1).reshape(-1, order='F') for p in k])
            self._kern_d = self._backend.copy_array(np.ascontiguousarray(k).reshape(-1), name=self._name + '.psf')
            self._kern_h = None
        return self._kern_d

    def _mem_usage(self, ncols):
        from indigo_amd.analyses import ScratchUsage
        P, worst = int(np.prod(self._grid)), 0
        for T, real, w, il in self._parts:
            panel = (P * w * self._K + 31) // 32 * 32
            worst = max(worst, (panel + ScratchUsage().measure(T, 1)) * 8)
        return worst

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        B, K = self._backend, self._K
        N, P = int(np.prod(self._dims)), int(np.prod(self._grid))
        kern = self._kernel()
        fused_path = self._order == 'xzy'
        trace = getattr(B, 'trace', None)
        for j in range(x.shape[1]):
            xj = x if x.shape[1] == 1 else x[:, j:j + 1]
            yj = y if y.shape[1] == 1 else y[:, j:j + 1]
            for i, (T, real, w, il) in enumerate(self._parts):
                with B.scratch(shape=(P * w, K)) as panel:
                    cols = [panel[:, k:k + 1] for k in range(K)]
                    for k in range(K):
                        # (the unfused transforms take alpha == 1 only: there alpha rides on the maps of the way in)
                        T.eval(cols[k], xj.dense_rows(k * N, (k + 1) * N), alpha=1 if fused_path else alpha, beta=0, forward=True)
                    if trace is not None:
                        trace.add('psf_mix', nbytes=16 * P * real * K + 4 * K * K * P, nflops=8 * P * real * K * K, shape=(P, real, K), name=self._name)
                    B.psf_mix(panel, panel, kern, P, real, interleaved=il, width=w)
                    for k in range(K):
                        T.eval(yj.dense_rows(k * N, (k + 1) * N), cols[k], alpha=alpha if fused_path else 1,
                               beta=beta if i == 0 else 1, forward=False)


class Eye(MatrixFreeOperator):
    def __init__(self, backend, n, **kwargs):
        super().__init__(backend, shape=(n, n), **kwargs)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        trace = getattr(self._backend, 'trace', None)
        if trace is not None:
            trace.add('axpby', nbytes=(0 if alpha == 0 else x.nbytes) + (0 if beta == 0 else y.nbytes) + y.nbytes,
                      name=self._name)
        self._backend.axpby(beta, y, alpha, x)


class One(MatrixFreeOperator):
    """Matrix of ones (reference operators.py:283-302; evaluates through backend.onemm)."""

    def _eval(self, y, x, alpha=1, beta=0, forward=None, left=True):
        self._backend.onemm(y, x, alpha, beta)


class DenseMatrix(Operator):
    """Dense complex64 matrix (reference operators.py:266-281; evaluates through backend.cgemm)."""

    def __init__(self, backend, M, **kwargs):
        super().__init__(backend, **kwargs)
        M = np.require(M, requirements='F')
        assert M.dtype == _C64 and M.ndim == 2
        self._matrix = M
        self._matrix_d = None

    @property
    def shape(self):
        return self._matrix.shape

    @property
    def dtype(self):
        return self._matrix.dtype

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        if self._matrix_d is None:
            self._matrix_d = self._backend.copy_array(self._matrix)
        self._backend.cgemm(y, self._matrix_d, x, alpha=alpha, beta=beta, forward=forward)


# ------------------------------------------------------------------------------
# composites
# ------------------------------------------------------------------------------

class Adjoint(CompositeOperator):
    def __init__(self, backend, child, *args, **kwargs):
        super().__init__(backend, child, *args, **kwargs)

    @property
    def shape(self):
        return self.child.shape[::-1]

    @property
    def dtype(self):
        return self.child.dtype

    @property
    def H(self):
        return self.child

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        self.child.eval(y, x, alpha, beta, forward=not forward, left=left)


class Scale(CompositeOperator):
    def __init__(self, backend, v, child, **kwargs):
        super().__init__(backend, child, **kwargs)
        self._name = "%s*{}".format(child._name)
        self._val = v

    @property
    def shape(self):
        return self.child.shape

    @property
    def dtype(self):
        return self.child.dtype

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        factor = self._val if forward else np.conj(self._val)
        self.child.eval(y, x, alpha=alpha * factor, beta=beta, forward=forward, left=left)


class Product(BinaryOperator):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._name = "{}*{}".format(self.left._name, self.right._name)

    def _adopt(self, children):
        L, R = children
        if L.shape[1] != R.shape[0]:
            raise ValueError("Mismatched shapes in Product: attempting {} x {} ({} x {})".format(
                L.shape, R.shape, L._name, R._name))
        super()._adopt(children)

    @property
    def shape(self):
        return self.left.shape[0], self.right.shape[1]

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        L, R = self._children
        first, last = (R, L) if forward else (L, R)
        with self._backend.scratch(shape=(R.shape[0], x.shape[1])) as tmp:
            first.eval(tmp, x, alpha=alpha, beta=0, forward=forward, left=left)
            last.eval(y, tmp, alpha=1, beta=beta, forward=forward, left=left)

    def _mem_usage(self, ncols):
        ncols = min(ncols, self._batch or ncols)
        return self._children[1].shape[0] * ncols * self.dtype.itemsize


class Sum(BinaryOperator):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._name = "{}+{}".format(self.left._name, self.right._name)

    def _adopt(self, children):
        L, R = children
        if L.shape != R.shape:
            raise ValueError("Mismatched shapes in Sum: attempting {} + {} ({} + {})".format(
                L.shape, R.shape, L._name, R._name))
        super()._adopt(children)

    @property
    def shape(self):
        return self.left.shape

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        L, R = self._children
        R.eval(y, x, alpha=alpha, beta=beta, forward=forward, left=left)
        L.eval(y, x, alpha=alpha, beta=1.0, forward=forward, left=left)


class Kron(BinaryOperator):
    """A (x) B.  Only the KronI form (A = identity) is on the hot path."""

    @property
    def shape(self):
        h = int(np.prod([c.shape[0] for c in self._children]))
        w = int(np.prod([c.shape[1] for c in self._children]))
        return h, w

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        L, R = self._children
        if isinstance(L, Eye):
            if x.shape[1] > 1 and getattr(R, '_grid_interleaved', False):
                # a coil-interleaved grid (ZpadFFT layout 2) per column: the c blocks of ONE column are the c columns of its own
                # row-major panel, so the columns cannot be stacked side by side as one wider panel -- one product per column
                for j in range(x.shape[1]):
                    R.eval(y[:, j:j + 1], x[:, j:j + 1], alpha=alpha, beta=beta, forward=forward, left=left)
                return
            # I_c (x) B: the c blocks become c panel columns; R.eval does the reshape
            R.eval(y, x, alpha=alpha, beta=beta, forward=forward, left=left)
        else:
            raise NotImplementedError(
                "Kron with a non-identity left factor needs right-multiplication, which only the "
                "reference's dense real-symmetric path provides; outside the SENSE hot path.  For a temporal basis "
                "Phi (x) I_n use FrameBasis(phi, n).")


def _slice_rows(arr, start, stop):
    return arr[slice(start, stop), :]


class BlockDiag(CompositeOperator):
    @property
    def shape(self):
        return (sum(c.shape[0] for c in self._children), sum(c.shape[1] for c in self._children))

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        yo = xo = 0
        for C in self._children:
            h, w = C.shape if forward else C.shape[::-1]
            # (dense_rows: a child may be a leaf that takes contiguous vectors only -- the fused SENSE leaf)
            C.eval(y.dense_rows(yo, yo + h), x.dense_rows(xo, xo + w),
                   alpha=alpha, beta=beta, forward=forward, left=left)
            yo += h
            xo += w


class VStack(CompositeOperator):
    def _adopt(self, children):
        widths = [c.shape[1] for c in children]
        if len(set(widths)) > 1:
            raise ValueError("Mismatched widths in VStack: attempting to stack {}".format(
                list(zip(widths, [c._name for c in children]))))
        super()._adopt(children)

    @property
    def shape(self):
        return sum(c.shape[0] for c in self._children), self._children[-1].shape[1]

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        off = 0
        if forward:
            for C in self._children:
                h = C.shape[0]
                C.eval(_slice_rows(y, off, off + h), x, alpha=alpha, beta=beta, forward=True, left=left)
                off += h
        else:
            # y = beta*y + sum_i C_i^H x_i.  The reference scales y by beta and then accumulates every child with
            # beta = 1 (operators.py:440-447); handing beta to the first child is the same sum without the extra
            # read-modify-write of y (and lets a leaf take its beta == 0 fast path).
            for i, C in enumerate(self._children):
                h = C.shape[0]
                C.eval(y, _slice_rows(x, off, off + h), alpha=alpha, beta=beta if i == 0 else 1, forward=False, left=left)
                off += h


class HeadRows(CompositeOperator):
    """The first `keep` rows of a child operator:  y = alpha * A[:keep, :] x + beta * y;  adjoint  y = alpha * A[:keep, :]^H x + beta * y.

    What a chunk of coils padded with zero-weight coils evaluates through (indigo_amd.fused.assemble): the coil-interleaved
    kernels take 2, 4 or 8 coils, a 3-coil chunk is a 4-coil one whose last map is zero -- its k-space rows come last
    (KronI stacks the coils, reference operators.py:374-375), are exactly zero in the forward product and must read as zero
    in the adjoint one.  One panel of the child's height from the scratch arena, one copy in each direction."""

    def __init__(self, backend, child, keep, **kwargs):
        super().__init__(backend, child, **kwargs)
        self._keep = int(keep)
        assert 0 < self._keep <= child.shape[0]

    @property
    def shape(self):
        return self._keep, self.child.shape[1]

    def _mem_usage(self, ncols):
        return self.child.shape[0] * ncols * 8

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        B, A = self._backend, self.child
        ncols = x.shape[1]
        with B.scratch(shape=(A.shape[0], ncols)) as tmp:
            if forward:
                A.eval(tmp, x, alpha=alpha, beta=0, forward=True, left=left)
                for j in range(ncols):
                    B.axpby(beta, y[:, j:j + 1] if ncols > 1 else y, 1, tmp[:self._keep, j:j + 1] if ncols > 1 else tmp[:self._keep])
            else:
                for j in range(ncols):
                    tj = tmp[:, j:j + 1] if ncols > 1 else tmp
                    tj[self._keep:]._zero()
                    B.axpby(0, tj[:self._keep], 1, x[:, j:j + 1] if ncols > 1 else x)
                A.eval(y, tmp, alpha=alpha, beta=beta, forward=False, left=left)


class HStack(CompositeOperator):
    def _adopt(self, children):
        heights = [c.shape[0] for c in children]
        if len(set(heights)) > 1:
            raise ValueError("Mismatched heights in HStack: attempting to stack {}".format(
                list(zip(heights, [c._name for c in children]))))
        super()._adopt(children)

    @property
    def shape(self):
        return self._children[-1].shape[0], sum(c.shape[1] for c in self._children)

    def _eval(self, y, x, alpha=1, beta=0, forward=True, left=True):
        off = 0
        if forward:
            self._backend.scale(y, beta)
            for C in self._children:
                w = C.shape[1]
                C.eval(y, _slice_rows(x, off, off + w), alpha=alpha, beta=1, forward=True, left=left)
                off += w
        else:
            for C in self._children:
                w = C.shape[1]
                C.eval(_slice_rows(y, off, off + w), x, alpha=alpha, beta=beta, forward=False, left=left)
                off += w
