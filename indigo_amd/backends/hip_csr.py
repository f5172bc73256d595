"""`HipBackend.csr_matrix`: the device CSR matrix of the MI355X backend, with the device formats of a gridding matrix
(indigo_amd/grid_formats.py builds them on the host; this class uploads them, chooses the kernel of a product and launches it).

The state of a matrix is declared in `__init__`.  A format is registered per panel width where panels of several widths share one
matrix (`_bricks_by`, `_slots_by`, `_shares_by`, `_support_fine_by`): a dict of scalars and device arrays, or None when the matrix
declined the format.  Of the formats built on first use (`_wide`, `_runs_fmt`, `_values_re`), `_tried` names those that were asked
for: such a one is a dict (an array), or None after a decline.  Until then `_runs_fmt` and `_values_re` are None and `_wide` is
False, which is how its readers outside the class tell "never asked for" from "declined".
"""
import logging

import numpy as np

from indigo_amd import _lib, grid_formats
from indigo_amd._lib import cplx as _cplx
from indigo_amd.backends.backend import Backend

log = logging.getLogger(__name__)
_C64 = np.dtype('complex64')

# key of a builder's dict -> name of its device array, in upload order
_BRICK_ARRAYS = dict(tasks=".brickTasks", table=".brickTable", entries=".brickEntries", rounds=".brickRoundRows", shared=".sharedBricks")
_SLOT_ARRAYS = dict(tasks=".slotTasks", table=".slotTable", entries=".slotEntries", slot_ptr=".slotPtr", shared=".slotSharedBricks")
_SHARE_ARRAYS = dict(tasks=".shareTasks", table=".shareTable", shares=".shares", shared=".shareSharedBricks")
_WIDE_ARRAYS = dict(owned=".wideOwnedTiles", tasks=".wideTasks", table=".wideTable", entries=".wideEntries", rows=".wideEntryRows")
_RUN_ARRAYS = dict(order=".runOrder", dptr=".runPtr", dcols=".runCols", entries=".runEntries")


def _ptr(a):
    return None if a is None else a._arr


class csr_matrix(Backend.csr_matrix):
    """Device CSR with an optional cached CSR of the transpose for gather-form adjoints."""

    def __init__(self, backend, A, name='mat'):
        super().__init__(backend, A, name)
        self._host_csr = A if A.dtype == _C64 else A.astype(_C64)   # kept until the transpose is built
        self._perm = self._sep = self._grid_dims = None     # set_row_order (device array), set_grid_separable, set_grid_dims
        # set_grid_support: (device table, n0, nm), the host table, words per bitmap; _fine: the last (device table, tile), and per width
        self._support, self._support_host, self._support_zw = None, None, 16
        self._support_fine, self._support_fine_by, self._support_fine_host_by = None, {}, {}
        # set_grid_bricks / _slots / _shares: the last format built (None after a decline), and per panel width
        self._bricks, self._bricks_by, self._slots, self._slots_by, self._shares_by = None, {}, None, {}, {}
        self._invalidate()

    def _invalidate(self):
        """Forget everything derived on first use from the order of the rows or from the values (the formats of the set_grid_*
        calls are the caller's to rebuild: no route takes them while a row order is set)."""
        self._t = None                      # device CSR of the transpose
        self._weights_real = None           # weights_are_real(values), once known
        self._xrows = None                  # (touched columns, compact column indices) of the xrows routes
        self._values_re = self._runs_fmt = None                     # _real_values, _runs: built on first use ...
        self._wide = False                  # ... as is _wide_bricks (False: not asked for yet)
        self._tried = set()                 # those of the three that were asked for (None then says: declined)

    def _upload(self, fmt, names):
        """a builder's dict with every array in `names` replaced by its device copy (None stays None)"""
        if fmt is None:
            return None
        b = self._backend
        return dict(fmt, **{key: b.copy_array(fmt[key], name=self._name + suffix) for key, suffix in names.items() if fmt[key] is not None})

    def _host(self, part):
        """'indptr', 'indices' or 'data' of the matrix as stored: of the host copy while there is one, else read back"""
        if self._host_csr is not None:
            return getattr(self._host_csr, part)
        return dict(indptr=self.rowPtrs, indices=self.colInds, data=self.values)[part].to_host()

    def _transposed(self):
        if self._t is None:
            b = self._backend
            pt, it, dt = b.csr_transpose(self._host_csr)
            self._t = (b.copy_array(pt, name=self._name + ".T.rowPtrs"),
                       b.copy_array(it, name=self._name + ".T.colInds"),
                       b.copy_array(dt, name=self._name + ".T.data"))
            self._host_csr = None
        return self._t

    def set_grid_support(self, table, n0, nm, zw=16):
        """zw: words per entry of the table's bitmaps (the input-side form, ig_grid_support); 16 for 256- / 512-point nm"""
        self._support = (self._backend.copy_array(np.ascontiguousarray(table, dtype=np.int16).reshape(-1),
                                                  name=self._name + ".support"), int(n0), int(nm))
        self._support_zw = int(zw)
        self._support_host = table

    def set_grid_support_fine(self, table, tile, ncols=None):
        """a support table with `tile` (8 or 4) kx points per entry: what the brick scatter writes by (the gather routes keep
        the 16-point table of set_grid_support; a reader with the finer table reads a subset of what they write).
        ncols: the panel width whose adjoint writes by this table (a matrix shared by coil chunks of several widths carries
        one table per width); None = every width without a table of its own."""
        built, key = self._bricks_by, None if ncols is None else int(ncols)
        assert not (any(v is not None for v in built.values()) if key is None else built.get(key) is not None), \
            "set_grid_support_fine must come before set_grid_bricks: the runs of bricks are sized for the table's segments"
        assert int(tile) in (4, 8, 16)
        self._support_fine = (self._backend.copy_array(np.ascontiguousarray(table, dtype=np.int16).reshape(-1),
                                                       name=self._name + ".supportFine"), int(tile))
        self._support_fine_by[key] = self._support_fine
        self._support_fine_host_by[key] = (table, int(tile))

    def _format(self, which, ncols, exact=False):
        """the format ('_bricks' / '_slots' / '_shares') or fine table ('_support_fine' / '_support_fine_host') registered for
        panels of `ncols` columns; exact=False: else the one registered for every width"""
        by = getattr(self, which + '_by')
        key = None if ncols is None else int(ncols)
        if key in by or exact:
            return by.get(key)
        return by.get(None)

    def _fine_tile(self, ncols):
        fine = self._format('_support_fine', ncols)
        return fine[1] if fine is not None else 16

    def set_grid_bricks(self, n0, nm, ns, ncols=8, bm=2, bs=2, chunk=4096, run=4096):
        """The brick format (grid_formats.bricks) of the n0 x nm x ns grid the columns form, on the device: the adjoint of an
        `ncols`-column interleaved panel then scatters brick by brick through LDS (ig_ccsrmm_t_bricks) and needs neither the
        transposed matrix nor its 4-bytes-per-grid-point row pointers."""
        A = self._host_csr
        assert A is not None and A.shape[1] == n0 * nm * ns
        fmt = grid_formats.bricks(A.indptr, A.indices, A.data, n0, nm, ns, ncols, bm, bs, chunk, run,
                                  tile=self._fine_tile(ncols), real_entries=self._real_weights(A.data))
        if fmt is None:
            log.info("%s: no brick-binned format (%s); the adjoint keeps the gather route", self._name, _lib.last_error(None))
        self._bricks = self._bricks_by[int(ncols)] = self._upload(fmt, _BRICK_ARRAYS)

    def set_grid_slots(self, n0, nm, ns, ncols=1, bm=2, bs=2, chunk=256, run=128):
        """The slot format (grid_formats.slots) for an `ncols`-column panel (1, 2 or 4), on the device: the scatter of
        ig_ccsrmm_t_slots"""
        A = self._host_csr
        assert A is not None and A.shape[1] == n0 * nm * ns
        fmt = grid_formats.slots(A.indptr, A.indices, A.data, n0, nm, ns, ncols, bm, bs, chunk, run,
                                 tile=self._fine_tile(ncols), real_entries=self._real_weights(A.data))
        if fmt is None:
            log.info("%s: no slot format; the adjoint keeps the gather route", self._name)
        self._slots = self._slots_by[int(ncols)] = self._upload(fmt, _SLOT_ARRAYS)

    def set_grid_separable(self, sep):
        """The matrix in SEPARABLE form (indigo_amd.interp.interp_sep_records: one record per sample, columns numbered in the
        memory order of the coil-interleaved grid panel): the products with interleaved panels of 2, 4 or 8 columns compute their
        taps from the records (ig_grid_gather_sep / ig_grid_scatter_sep) instead of streaming the stored ones."""
        n0, nm, ns = (int(v) for v in sep['dims'])
        assert sep['records'].shape[0] == self.shape[0] and n0 * nm * ns == self.shape[1]
        rec = np.ascontiguousarray(sep['records'])
        # the forward reads the records as they are (16 or 32 words apart: one 64- or 128-byte line each); the share scatter wants every
        # record followed by room for the sample's panel row -- a second, wider copy (recx) that set_grid_shares uploads when it is needed.
        # order: the gather order per panel width (_gather_order)
        self._sep = dict(tw=int(sep['tw']), dims=(n0, nm, ns), gconst=complex(sep['gconst']), host=rec, stride=rec.shape[1],
                         records=self._backend.copy_array(rec.reshape(-1), name=self._name + ".sepRecords"), recx=None, stride_x=0, order={})

    def _gather_order(self, ncols):
        """grid_formats.gather_order for an `ncols`-column panel on the device, built once per panel width from the host copy of the
        records (None: too few groups to order)"""
        by = self._sep['order']
        if ncols not in by:
            order = grid_formats.gather_order(self._sep['host'], self._sep['tw'], ncols)
            by[ncols] = None if order is None else self._backend.copy_array(order, name=self._name + ".gatherOrder%d" % ncols)
        return by[ncols]

    def set_grid_shares(self, ncols=8, bm=8, bs=2, chunk=1024, run=1024):
        """The share format (grid_formats.shares) on the device: the adjoint of an `ncols`-column interleaved panel as a scatter of
        (sample, brick) shares with computed taps (ig_grid_scatter_sep).  set_grid_separable must come first, as must
        set_grid_support_fine: a brick's flagged segments are looked up here, once."""
        sep = self._sep
        assert sep is not None
        fine = self._format('_support_fine_host', ncols)
        tab, tile = fine if fine is not None else (self._support_host, 16)
        fmt = grid_formats.shares(sep['host'], sep['tw'], sep['dims'], ncols, bm, bs, chunk, run,
                                  table=tab, tile=tile, zw=self._support_zw)
        if fmt is None:
            log.info("%s: no share format; the adjoint keeps the stored-tap routes", self._name)
        elif sep['recx'] is None:
            recx, sep['stride_x'] = grid_formats.records_with_rows(sep['host'])
            sep['recx'] = self._backend.copy_array(recx, name=self._name + ".sepRecordsWithRows")
        self._shares_by[int(ncols)] = self._upload(fmt, _SHARE_ARRAYS)

    def set_grid_dims(self, n0, nm, ns):
        """Hint: the columns of the matrix are the points of an n0 x nm x ns grid, n0 running fastest (a gridding matrix).
        The wide adjoint then bins by bricks of 16 x 2 x 2 points instead of 16 consecutive columns."""
        assert int(n0) * int(nm) * int(ns) == self.shape[1]
        self._grid_dims = (int(n0), int(nm), int(ns))
        self._wide = False
        self._tried.discard('wide')

    def _dims(self):
        return self._grid_dims or grid_formats.guess_grid_dims(self.shape[1])

    def _wide_bricks(self):
        """The wide-brick format (grid_formats.wide_bricks; bricks of the grid of set_grid_dims, or of a cube guessed from the column
        count) on the device: built on first use; None when the matrix does not qualify."""
        if 'wide' not in self._tried:
            self._tried.add('wide')
            t, data = self._backend.tuning, self._host('data')
            self._wide = self._upload(grid_formats.wide_bricks(
                self._host('indptr'), self._host('indices'), data, self.shape[1], self._dims(),
                t.get('wide_brick_shape', (2, 2)), t.get('wide_task_shape', (8192, 2048)), real_entries=self._real_weights(data)), _WIDE_ARRAYS)
        return self._wide

    def _touched(self):
        """(touched columns, the nonzeros' column indices into them) on the device: what the xrows routes repack and read by"""
        if self._xrows is None:
            b = self._backend
            indices = self._host('indices')
            mark = np.zeros(self.shape[1], dtype=bool)
            mark[indices] = True
            touched = np.flatnonzero(mark).astype(np.int32)
            compact = np.searchsorted(touched, indices).astype(np.int32)
            self._xrows = (b.copy_array(touched, name=self._name + ".touchedCols"), b.copy_array(compact, name=self._name + ".compactColInds"))
        return self._xrows

    def _runs(self, sub):
        """The run format (grid_formats.runs) over the touched columns `sub` = _touched(), on the device: built on first use, None
        when the matrix does not qualify."""
        if 'runs' not in self._tried:
            self._tried.add('runs')
            fmt = grid_formats.runs(self._host('indptr'), sub[1].to_host(), self._host('data'), sub[0].to_host(), self._dims(),
                                    self._backend.tuning.get('runs_order', True))
            if fmt is None:
                log.info("%s: no run format (%s); the forward product keeps the per-nonzero gather", self._name, _lib.last_error(None))
            self._runs_fmt = self._upload(fmt, _RUN_ARRAYS)
        return self._runs_fmt

    def set_row_order(self, perm):
        """Store the matrix with its rows in the order `perm` (stored row r = row perm[r] of A), e.g. gridding
        samples sorted by the grid cell they touch: neighbouring rows then gather neighbouring panel rows.
        The products are unchanged -- the forward result is written through the permutation and the
        adjoint reads its panel through it."""
        b = self._backend
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        assert self._host_csr is not None and perm.shape == (self.shape[0],)
        Ap = self._host_csr[perm]
        Ap.sort_indices()
        self.rowPtrs = b.copy_array(Ap.indptr.astype(np.int32), name=self._name + ".rowPtrs")
        self.colInds = b.copy_array(Ap.indices.astype(np.int32), name=self._name + ".colInds")
        self.values = b.copy_array(Ap.data.astype(_C64), name=self._name + ".data")
        self._host_csr = Ap
        self._invalidate()
        self._perm = b.copy_array(perm, name=self._name + ".rowOrder")

    def _real_weights(self, data):
        """are the matrix's weights real up to rounding residue (weights_are_real; one pass over the values, remembered) -- and
        does the backend's tuning allow the 4-byte forms?"""
        if not self._backend.tuning.get('real_entries', True):
            return False
        if self._weights_real is None:
            self._weights_real = grid_formats.weights_are_real(data)
        return self._weights_real

    def _real_values(self):
        """the weights' real parts as a float32 device array when the matrix is real up to rounding residue (built on first
        use; None otherwise, or when the backend's tuning asks for complex entries)"""
        if 'values_re' not in self._tried:
            self._tried.add('values_re')
            data = self._host('data')
            if self._real_weights(data):
                self._values_re = self._backend.copy_array(np.ascontiguousarray(data.real, dtype=np.float32), name=self._name + ".dataRe")
        return self._values_re

    # -- which kernel a product runs ---------------------------------------------------------------------------------------------
    def forward_route(self, ncols):
        """The route of y = alpha A x + beta y for an x of `ncols` columns: 'sep' (taps computed from the records), 'il_rw' / 'il'
        (interleaved grid panel, 4-byte / 8-byte weights), 'xrows_runs' / 'xrows' (wide panels of which few rows are touched), 'rowperm'
        (set_row_order) or 'csr'.  Builds what it has to look at (the real weights, the run format) on first use."""
        t = self._backend.tuning
        if self._grid_il:
            if self._sep is not None and ncols in (2, 4, 8) and t.get('sep_gather', True):
                return 'sep'
            return 'il_rw' if ncols in (2, 4, 8) and self._real_values() is not None else 'il'
        if self._perm is None and 16 <= ncols <= 64 and self._col_frac <= 0.6 and self.values.size >= self.shape[1] and t['xrows']:
            # a wide panel of which the matrix touches a fraction of the rows (a gridding matrix: 30 % of its grid):
            # the panel is repacked row-major anyway -- repack only the touched rows
            sub = self._touched()
            return 'xrows_runs' if ncols == 64 and t.get('runs', True) and sub[0].size * 512 < 2 ** 32 and self._runs(sub) is not None else 'xrows'
        return 'csr' if self._perm is None else 'rowperm'

    def adjoint_route(self, ncols, beta, y):
        """The route of y = alpha A^H x + beta y for an x of `ncols` columns: the scatters 'shares', 'bricks', 'slots' (interleaved
        grid panel y) and 'wide' (64 columns), the gathers over the transposed matrix 'gather_il' (interleaved), 'gather_t_grid' (by the
        support table, or through a row order) and 'gather_t', or 'scatter' (float atomics from A's CSR).  Builds the wide-brick format
        on first use."""
        b, perm = self._backend, self._perm
        scatter = perm is None and beta == 0 and y.contiguous
        shf = self._format('_shares', ncols, exact=True)
        if shf is not None and scatter and self._grid_il and shf['ntasks'] > 0 and b.tuning.get('sep_scatter', True):
            return 'shares'
        br = self._format('_bricks', ncols, exact=True)
        if br is not None and scatter and self._grid_il and ncols == br['ncols']:
            return 'bricks'
        sl = self._format('_slots', ncols, exact=True)
        if sl is not None and scatter and ncols == sl['ncols'] and sl['ntasks'] > 0:
            return 'slots'
        if (ncols == 64 and beta == 0 and perm is None and not self._grid_il and self.shape[1] % 16 == 0
                and self.shape[1] > 0 and self.shape[0] * 512 < 2 ** 31 and self.values.size >= self.shape[1] // 4
                and b.tuning['wide_bricks'] and self._wide_bricks() is not None):
            return 'wide'           # 64 columns at the reference boundary (BASELINE config 3): scatter through LDS brick images
        if self._grid_il:
            assert scatter, "interleaved panels: no row order, beta = 0"
            return 'gather_il'
        if perm is not None:
            assert not self._exwrite and b.adjoint_policy == 'transpose' and ncols <= 8, \
                "row-ordered matrices use the packed transposed gather"
        if (self._gather_support() is not None or perm is not None) and not self._exwrite and b.adjoint_policy == 'transpose':
            return 'gather_t_grid'
        return 'scatter' if self._exwrite or b.adjoint_policy != 'transpose' else 'gather_t'

    def _gather_support(self):
        """the support table of the gather routes over the transposed matrix: they read 16-word bitmaps only -- with another table
        they compute every row, a superset of what any reader of the grid looks at"""
        return self._support if self._support_zw == 16 else None

    def _scatter_support(self, ncols, y):
        """(table, tile) the scatter into y writes by: the fine table of the panel width, else the 16-point table, else none -- and then
        every row is defined: y is zeroed, bricks no sample touches stay zero"""
        fine = self._format('_support_fine', ncols)
        tab, tile = fine if fine is not None else (self._support[0] if self._support is not None else None, 16)
        if tab is None:
            y._zero()
        return tab, tile

    # -- one launch per route ----------------------------------------------------------------------------------------------------
    def _call(self, kernel, *args):
        b = self._backend
        b._check(getattr(b._L, kernel)(b._ctx, *args), kernel)

    def _fwd_sep(self, y, x, alpha, beta):
        # the taps computed from one 64-byte record per sample: no index or value stream
        sep = self._sep
        order = self._gather_order(x.shape[1]) if self._backend.tuning.get('gather_order', True) else None
        self._call("ig_grid_gather_sep", self.shape[0], x.shape[1], sep['tw'], sep['records']._arr, sep['stride'], x._arr, *sep['dims'],
                   *_cplx(complex(alpha) * sep['gconst']), *_cplx(beta), y._arr, y._leading_dim, _ptr(order))

    def _fwd_il_rw(self, y, x, alpha, beta):
        # every weight real (see weights_are_real): the gather reads 4-byte values
        self._call("ig_ccsrmm_il_rw", *self.shape, x.shape[1], self.values.size, *_cplx(alpha), self.values._arr, self._real_values()._arr,
                   self.colInds._arr, self.rowPtrs._arr, x._arr, *_cplx(beta), y._arr, y._leading_dim)

    def _fwd_il(self, y, x, alpha, beta):
        self._call("ig_ccsrmm_il", *self.shape, x.shape[1], self.values.size, *_cplx(alpha), self.values._arr, self.colInds._arr,
                   self.rowPtrs._arr, x._arr, *_cplx(beta), y._arr, y._leading_dim)

    def _fwd_xrows_runs(self, y, x, alpha, beta):
        # 64 columns: the run format -- every panel row a run of 16 matrix rows touches is loaded once
        sub, runs = self._xrows, self._runs_fmt
        self._call("ig_ccsrmm_xrows_runs", *self.shape, self.values.size, *_cplx(alpha), self.rowPtrs._arr, runs['dptr']._arr, runs['dcols']._arr,
                   runs['entries']._arr, runs['all_real'], _ptr(runs['order']), x._arr, x._leading_dim, *_cplx(beta), y._arr, y._leading_dim,
                   sub[0]._arr, sub[0].size)

    def _fwd_xrows(self, y, x, alpha, beta):
        sub = self._xrows
        self._call("ig_ccsrmm_xrows", *self.shape, x.shape[1], self.values.size, *_cplx(alpha), self.values._arr, sub[1]._arr, self.rowPtrs._arr,
                   x._arr, x._leading_dim, *_cplx(beta), y._arr, y._leading_dim, sub[0]._arr, sub[0].size)

    def _fwd_rowperm(self, y, x, alpha, beta):
        self._call("ig_ccsrmm_rowperm", *self.shape, x.shape[1], self.values.size, *_cplx(alpha), self.values._arr, self.colInds._arr,
                   self.rowPtrs._arr, x._arr, x._leading_dim, *_cplx(beta), y._arr, y._leading_dim, self._perm._arr)

    _FORWARD = dict(sep=_fwd_sep, il_rw=_fwd_il_rw, il=_fwd_il, xrows_runs=_fwd_xrows_runs, xrows=_fwd_xrows, rowperm=_fwd_rowperm,
                    csr=Backend.csr_matrix.forward)

    def forward(self, y, x, alpha=1, beta=0):
        if self._grid_il:
            assert self._perm is None and x.contiguous, "interleaved panels: no row order, contiguous grid panel"
        self._check_panels(y, x, self.values)
        self._FORWARD[self.forward_route(x.shape[1])](self, y, x, alpha, beta)

    def _adj_shares(self, y, x, alpha, beta):
        sep, shf = self._sep, self._format('_shares', x.shape[1], exact=True)
        self._scatter_support(x.shape[1], y)
        self._call("ig_grid_scatter_sep", self.shape[0], x.shape[1], sep['tw'], sep['recx']._arr, sep['stride_x'], shf['shares']._arr, x._arr,
                   x._leading_dim, y._arr, *sep['dims'], shf['bm'], shf['bs'], shf['tasks']._arr, shf['ntasks'], shf['table']._arr,
                   shf['shared']._arr, shf['nshared'], shf['tile'], *_cplx(complex(alpha) * np.conj(sep['gconst'])))

    def _adj_bricks(self, y, x, alpha, beta, kernel="ig_ccsrmm_t_bricks", which='_bricks', rows='rounds'):
        f = self._format(which, x.shape[1], exact=True)
        tab, tile = self._scatter_support(x.shape[1], y)
        self._call(kernel, *self.shape, x.shape[1], *_cplx(alpha), f['entries']._arr, f[rows]._arr, x._arr, x._leading_dim, y._arr, _ptr(tab),
                   f['n0'], f['nm'], f['bm'], f['bs'], f['tasks']._arr, f['ntasks'], f['table']._arr, f['shared']._arr, f['nshared'], tile,
                   self._support_zw, f['words'])

    def _adj_slots(self, y, x, alpha, beta):
        # the same argument list: where the slots start in place of the rows of the rounds
        self._adj_bricks(y, x, alpha, beta, "ig_ccsrmm_t_slots", '_slots', 'slot_ptr')

    def _adj_wide(self, y, x, alpha, beta):
        wb = self._wide
        self._call("ig_ccsrmm_t_bricks_wide_grid", *self.shape, *_cplx(alpha), wb['entries']._arr, wb['rows']._arr, x._arr, x._leading_dim, y._arr,
                   y._leading_dim, wb['tasks']._arr, wb['ntasks'], wb['table']._arr, wb['owned']._arr, *wb['geom'], wb['words'])

    def _adj_gather_il(self, y, x, alpha, beta):
        pt, it, dt = self._transposed()
        tab, n0, nm = self._gather_support() or (None, 0, 0)
        self._call("ig_ccsrmm_t_grid_il", *self.shape, x.shape[1], dt.size, *_cplx(alpha), dt._arr, it._arr, pt._arr, x._arr, x._leading_dim,
                   y._arr, _ptr(tab), n0, nm)

    def _adj_gather_t(self, y, x, alpha, beta):
        # ('gather_t': no 16-word support table and no row order)
        pt, it, dt = self._transposed()
        self._backend.ccsrmm_t(y, self.shape, it, pt, dt, x, alpha=alpha, beta=beta, support=self._gather_support(), xperm=self._perm)

    def _adj_scatter(self, y, x, alpha, beta):
        self._backend.ccsrmm(y, self.shape, self.colInds, self.rowPtrs, self.values, x, alpha=alpha, beta=beta, adjoint=True, exwrite=self._exwrite)

    _ADJOINT = dict(shares=_adj_shares, bricks=_adj_bricks, slots=_adj_slots, wide=_adj_wide, gather_il=_adj_gather_il,
                    gather_t_grid=_adj_gather_t, scatter=_adj_scatter, gather_t=_adj_gather_t)

    def adjoint(self, y, x, alpha=1, beta=0):
        self._check_panels(y, x, self.values)
        self._ADJOINT[self.adjoint_route(x.shape[1], beta, y)](self, y, x, alpha, beta)
