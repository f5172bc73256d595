"""A float64 restatement of the slot scatter of the adjoint gridding path -- k_grid_slots<NC, REALW> for NC = 1, 2, 4 with its zero-fill
k_grid_bricks_zero<NC> (indigo_amd/csrc/ig_spmm.hip, entry ig_ccsrmm_t_slots) --, hand-built matrices whose slot formats
(grid_formats.slots over ig_grid_slots_build) sit on the seams of that kernel, a table that says what every case is for, and a float32
emulation that walks the DEVICE FORMAT in the kernel's own order.  Plain numpy / scipy: nothing here needs a GPU.

THE CONTRACT (what the kernel does today: flush() of k_grid_slots and k_grid_bricks_zero):
  Y_il = alpha conj(G)^T X, Y_il the n0 x nm x ns grid (kx fastest) with its NC columns interleaved, cell (kx, km, ks) column c at
  [(kx + n0 (km + nm ks)) NC + c].  The format is tasks [lo, hi, first table row, rows | shared << 16] over SLOTS, a brick table
  [brick, end of its slots] of the NON-EMPTY bricks, slot_ptr and entries {cell in the brick, re, (im,) sample}.
  * A task that OWNS its run of bricks stores, at every brick boundary (the first slot at or past the brick's end) and at its end,
    every FLAGGED segment of the brick in full: alpha times what its entries added, zero where none did.  Plain stores in a fixed order
    of plain float32 operations: owned bricks are deterministic bit for bit.
  * A SHARED brick (more than `chunk` slots: several tasks hold a piece each) has its flagged segments zeroed first
    (k_grid_bricks_zero), then every piece adds alpha times its image into every cell of the flagged segments with float atomics.
  * The WRITE MASK is therefore: the flagged segments of the bricks of the table, every cell of them.  Everything else keeps the
    caller's bytes: the unflagged segments, and the bricks that hold no entry (with a support table they are unflagged anyway; with
    `support` NULL every segment of a brick in the table is written and the caller zeroes the grid first, as
    csr_matrix._scatter_support does).
  * Precondition (a segment is flagged iff it holds a nonzero of the matrix): no NONZERO weight falls into an unflagged
    segment.  The kernel clears only what it stores, so such a weight would stay in the wave's image and reach the next brick of the
    run.  The cases put entries of weight ZERO there (explicit zeros of the CSR): they add nothing wherever they land.

Exact inputs (spmm64.exact_values): weights and panel entries have nonzero integer parts in [-4, 4], alpha = 0.5 - 0.25j.  A part of a
product is an integer of magnitude <= 32, every partial sum over the n hits of a cell -- in any order and grouping, fused or not -- an
integer of magnitude <= 32 n < 2^24 (test_slots64_cpu.py asserts n <= 1024 for every case), alpha times it a multiple of 1/4 with at
most 17 significant bits, and the float atomics of shared pieces add such multiples: nothing rounds, shared bricks compare by value
too.  The device must give the reference by value in every cell of the write mask and the emulation bit for bit on owned bricks."""
import numpy as np
import scipy.sparse as spp

from spmm64 import ALPHA, C64, C128, EXACT_LIMIT, WAVES_PER_BLOCK, cf32, exact_values, is_f32, rounding_values  # noqa: F401

# ---- the constants of the kernel the cases and the emulation are built on (test_slots64_cpu.py reads them out of the sources) -----------
WINDOW = 63                 # usable slots of a window of 64 slot offsets (base += 63)
WAVE = 64                   # lanes: bricks per task, entries per slot
MASK_PASSES = 8             # passes of 64 (brick, segment) pairs of the mask lookup: 512 pairs per task
MAX_SEGMENTS = 32           # segments per brick (bits of my_mask)
ENTRY_BYTES = {4: 16, 3: 12}
DIMS = (32, 8, 8)           # the default grid (n0 fastest, nm, ns)
CAP_DIMS = (64, 16, 16)     # the grid of the runs at the brick cap
F32 = np.float32


class SlotCase:
    """bricks: [(brick id, [(cell, multiplicity), ...])] -- the k-th hit of cell c of brick b comes from sample (7 b + 3 c + k) mod M;
    dims / shape (bm, bs) / chunk / run / tile: what grid_formats.slots is given; zw: words per bitmap of the support table;
    table False: `support` NULL; unflag: (brick, segment) pairs left unflagged although entries fall there (their weights are zero);
    flag: (brick, segment) pairs flagged although nothing falls there; claims: what the case is for, name -> set of values (or True)
    that slot_seams must find"""

    def __init__(self, name, purpose, bricks, dims=DIMS, shape=(2, 2), chunk=256, run=1 << 20, tile=16, zw=16, table=True, M=97,
                 unflag=(), flag=(), **claims):
        self.name, self.purpose, self.bricks, self.dims, self.shape = name, purpose, tuple(bricks), dims, shape
        self.chunk, self.run, self.tile, self.zw, self.table, self.M = chunk, run, tile, zw, table, M
        self.unflag, self.flag, self.claims = frozenset(unflag), frozenset(flag), claims
        self.ncell = 16 * shape[0] * shape[1]
        self.nseg = (16 // tile) * shape[0] * shape[1]
        self.K = int(np.prod(dims))

    def __repr__(self):
        return self.name


def max_bricks(tile, bm, bs):
    from indigo_amd import grid_formats
    return grid_formats._max_bricks(tile, bm, bs)


def _tower(S, b, ncell, width=6, c0=None):
    """a brick of S slots: one cell hit S times, `width` more cells (the next ones, wrapped) hit once, every third of them twice"""
    c0 = (5 * b + 3) % ncell if c0 is None else c0
    return [(c0, S)] + [((c0 + 1 + i) % ncell, min(S, 2 if i % 3 == 0 else 1)) for i in range(width)]


def _seq(groups, seps, ncell, heavy_width=20):
    """bricks 0, 1, 2 ...: the light bricks of groups[0] (slots each), a heavy brick of seps[0] slots, the bricks of groups[1], ...:
    with a run length beyond the matrix every group between two heavy bricks is ONE task.  Heavy bricks start at cell 3 and stay
    inside the first 24 cells"""
    out, b = [], 0
    for i, g in enumerate(groups):
        for S in g:
            out.append((b, _tower(S, b, ncell))); b += 1
        if i < len(seps):
            out.append((b, _tower(seps[i], b, ncell, width=heavy_width, c0=3))); b += 1
    return out


TASK_SLOTS = (1, 2, 62, 63, 64, 65, 126, 127)
_WINDOW_GROUPS = ([1], [1, 1], [62], [63], [63, 1], [40, 25], [62, 64], [30, 97])
assert tuple(sum(g) for g in _WINDOW_GROUPS) == TASK_SLOTS
_WINDOW_SEPS = (128, 255, 129, 130, 128, 131, 254, 300)


def _cap_case(tag, shape, tile, purpose):
    """two stretches of 2 C - 1 light bricks (C = the brick cap: tasks of C and of C - 1 bricks each) around a heavy brick.  Every light
    brick holds a cell of its first segment (twice), one of its last and one in between; in the second stretch the first segment of
    each task's first brick and the last segment of each task's last brick are unflagged (zero weights), in the first they are flagged"""
    bm, bs = shape
    ncell, nseg = 16 * bm * bs, (16 // tile) * bm * bs
    C = max_bricks(tile, bm, bs)
    bricks, unflag, flag = [], [], []
    for b in list(range(2 * C - 1)) + list(range(2 * C, 4 * C - 1)):
        bricks.append((b, [(b % 4, 2), (ncell // 2 + b % 4, 1), (ncell - 1 - b % 3, 1)]))
        if nseg >= 4 and b % 3 == 0:
            flag.append((b, 1))                                    # (a segment nothing falls into: zeros)
    bricks.append((2 * C - 1, _tower(9, 0, ncell, width=3, c0=1)))
    for first, last in ((2 * C, 3 * C - 1), (3 * C, 4 * C - 2)):
        unflag += [(first, 0), (last, nseg - 1)]
    return SlotCase('cap-' + tag, purpose, sorted(bricks), dims=CAP_DIMS, shape=shape, chunk=4, tile=tile, unflag=unflag, flag=flag,
                    bricks_per_task={C, C - 1}, nseg={nseg}, cap_flags={(n, e, f) for n in (C, C - 1) for e in ('first', 'last') for f in (False, True)},
                    shared=True, owned=True, tile_pts={tile})


def _cells(n, ncell, start=0, step=1):
    return [((start + step * i) % ncell, 1) for i in range(n)]


SLOT_CASES = (
    SlotCase('window', "tasks of 1, 2, 62, 63, 64, 65, 126 and 127 slots as owned runs of one or two bricks between heavy bricks cut into shared "
             "pieces of 127 slots (and pieces of 1, 2, 3, 4 and 46): a brick boundary at the first slot of the second window (63 | 1), at the "
             "last slot of a window (62 | 64) and inside one (40 | 25, 30 | 97); windows of 1 and 2 slots; cells hit 1, 2 and up to 300 times; "
             "heavy bricks whose last two segments are unflagged, one with a flagged segment nothing falls into; 26 tasks",
             _seq(_WINDOW_GROUPS, _WINDOW_SEPS, 64), chunk=127, M=307, flag=((1, 3),),
             task_slots=set(TASK_SLOTS), boundary={'first', 'last', 'middle'}, window_cnt={1, 2, 63}, mult={1, 2, 300}, shared=True, owned=True,
             pieces={2, 3}, piece_of_one=True, shared_unflagged=True, shared_partial=True, ntasks_mod4=True, partial_segment=True,
             unflagged_beside_flagged=True, tile_pts={16}, nseg={4}),
    SlotCase('entries', "bricks of 128 cells: groups of 128, 100 and 65 distinct cells cut into 64 + 64, 64 + 36 and 64 + 1; slots of 1, 63 and 64 "
             "entries, a slot of 1 beside a slot of 64; every cell of a brick hit twice; cells 0 and 127, samples 0 and M - 1; runs of 4 slots",
             [(0, _cells(128, 128)), (1, _cells(100, 128, 3, 5)), (2, [(c, 2 if c == 1 else 1) for c, _ in _cells(64, 128, 1, 3)]), (5, _cells(63, 128, 64)),
              (6, _cells(65, 128, 60)), (7, [(127, 1)]), (8, [(c, 2) for c, _ in _cells(64, 128, 0, 2)]), (12, [(0, 1), (77, 3)]),
              (15, _cells(7, 128, 120, 1))],
             shape=(2, 4), run=4, slot_entries={1, 36, 63, 64}, one_by_64=True, cut_64=True, sample_ends=True, cell_ends=True, mult={1, 2, 3},
             single_second_group=True, nseg={8}, tile_pts={16}, owned=True),
    _cap_case('seg1', (1, 1), 16, "runs of 64 and 63 bricks of one segment each (the cap of 64 lanes), the first and the last brick of a run "
              "flagged and unflagged"),
    _cap_case('seg4', (1, 1), 4, "runs of 64 and 63 bricks of four 4-point segments (256 and 252 pairs of the mask lookup)"),
    _cap_case('seg16', (2, 2), 4, "runs of 32 and 31 bricks of sixteen 4-point segments (512 and 496 pairs: every pass of the lookup)"),
    _cap_case('seg32', (4, 4), 8, "runs of 16 and 15 bricks of thirty-two 8-point segments (512 and 480 pairs; a whole word of my_mask)"),
    SlotCase('zw4', "bitmaps of 4 words on nm = 8: km = 4 .. 7 are bit 1 of words 0 .. 3; 8-point segments; pieces of two slots",
             [(b, _tower(1 + b % 4, b, 64, width=9)) for b in range(0, 32, 3)], tile=8, zw=4, chunk=2, nseg={8}, tile_pts={8},
             zw_bit={0, 1}, nm_gt_zw=True, shared=True, owned=True, partial_segment=True, unflagged_beside_flagged=True),
    SlotCase('zw16-nm64', "bitmaps of 16 words on nm = 64: km / 16 = 0 .. 3 is the bit, km mod 16 the word", [(b, _tower(1 + b % 3, b, 32, width=5)) for b in range(1, 64, 2)],
             dims=(32, 64, 1), shape=(2, 1), chunk=2, run=6, zw_bit={0, 1, 2, 3}, nm_gt_zw=True, nseg={2}, shared=True, owned=True),
    SlotCase('no-table', "support NULL: every segment of a brick of the table is written, bricks that hold no entry keep the caller's zeros",
             [(b, _tower(1 + b % 5, b, 64, width=4)) for b in (0, 1, 2, 7, 8, 20, 21, 31)], table=False, chunk=3, run=5,
             no_table=True, shared=True, owned=True, partial_segment=True),
    SlotCase('one-task', "one task of one brick of three slots; bricks of 16 x 1 x 2 cells, 8-point segments", [(9, _tower(3, 9, 32, width=8))],
             shape=(1, 2), tile=8, one_task=True, ntasks_mod4=True, nseg={4}, task_slots={3}),
)
SLOT_BY_NAME = {c.name: c for c in SLOT_CASES}
SLOT_ROUNDING = 'window'
ROUTE_CASES = (('window', False), ('cap-seg16', True))       # the csr_matrix route: (case, through set_grid_support_fine)


class Data:
    pass


# =========================================================================================================================================
# geometry
# =========================================================================================================================================
def brick_origin(dims, shape, b):
    n0, nm, ns = dims
    nbx, nbm = n0 // 16, nm // shape[0]
    return 16 * (b % nbx), shape[0] * ((b // nbx) % nbm), shape[1] * (b // (nbx * nbm))


def cell_index(dims, shape, b, c):
    """row of the grid of cell c of brick b (arrays allowed)"""
    n0, nm, ns = dims
    bm, bs = shape
    nbx, nbm = n0 // 16, nm // bm
    b, c = np.asarray(b, dtype=np.int64), np.asarray(c, dtype=np.int64)
    return 16 * (b % nbx) + c % 16 + n0 * ((bm * ((b // nbx) % nbm) + (c // 16) % bm) + nm * (bs * (b // (nbx * nbm)) + c // (16 * bm)))


def segment_of(case_or_fmt, c):
    """segment of cell c inside its brick: xs + XS (im + bm is)"""
    tile = case_or_fmt.tile if isinstance(case_or_fmt, SlotCase) else case_or_fmt['tile']
    return (c % 16) // tile + (16 // tile) * (c // 16)


def support_table(seg, zw):
    """the flat int16 support table of ig_grid_support from seg[ks, km, kx tile]: the z ranges per (ks, tile) and the ks range per tile
    (the gather routes' part), then the bitmaps the scatters read: bit km / zw of word km mod zw of entry (ks, tile)"""
    ns, nm, nt = seg.shape
    km = np.arange(nm)[None, :, None]
    lo, hi = np.where(seg, km, nm).min(axis=1), np.where(seg, km + 1, 0).max(axis=1)
    ranges = np.zeros((ns * nt + nt, 2), dtype=np.int16)
    ranges[:ns * nt, 0], ranges[:ns * nt, 1] = np.where(hi > lo, lo, 0).reshape(-1), np.where(hi > lo, hi, 0).reshape(-1)
    for t in range(nt):
        ys = np.flatnonzero(hi[:, t] > lo[:, t])
        if ys.size:
            ranges[ns * nt + t] = (ys[0], ys[-1] + 1)
    bits = np.zeros((ns, nt, zw), dtype=np.uint32)
    s, m, t = np.nonzero(seg)
    np.bitwise_or.at(bits, (s, t, m % zw), np.uint32(1) << (m // zw).astype(np.uint32))
    return np.concatenate([ranges.reshape(-1), bits.reshape(-1).view(np.int16)])


# =========================================================================================================================================
# the cases' arrays
# =========================================================================================================================================
_data = {}


def slot_data(case, real=False, exact=True):
    """The arrays of a case.  A: scipy CSR (M x K), explicit zeros where a (brick, segment) is in case.unflag; X4 (M, 4): the panel, of
    which a product of NC columns takes the first NC; fmt: grid_formats.slots' dict with ns, tile, zw, seg (bool [ks, km, kx tile] or
    None) and support (the flat int16 table or None) added."""
    key = (case.name, real, exact)
    if key in _data:
        return _data[key]
    from indigo_amd import grid_formats
    rng = np.random.default_rng(6300 + SLOT_CASES.index(case))
    draw = exact_values if exact else rounding_values
    n0, nm, ns = case.dims
    bm, bs = case.shape
    rows, cols, zero = [], [], []
    for b, mults in case.bricks:
        assert len(set(c for c, m in mults)) == len(mults), (case, b)
        for c, m in mults:
            assert 0 <= c < case.ncell and 1 <= m <= case.M
            rows.append((7 * b + 3 * c + np.arange(m)) % case.M)
            cols.append(np.full(m, cell_index(case.dims, case.shape, b, c)))
            zero.append(np.full(m, (b, int(segment_of(case, c))) in case.unflag))
    rows, cols, zero = np.concatenate(rows).astype(np.int64), np.concatenate(cols), np.concatenate(zero)
    assert np.unique(rows * case.K + cols).size == rows.size
    vals = draw(rng, rows.size, real=real)
    vals[zero] = 0
    A = spp.csr_matrix((vals, (rows, cols)), shape=(case.M, case.K))
    assert A.nnz == rows.size
    A.sort_indices()
    D = Data()
    D.case, D.M, D.K, D.real, D.A = case, case.M, case.K, real, A
    D.X4 = draw(rng, case.M * 4).reshape(case.M, 4)
    fmt = grid_formats.slots(A.indptr, A.indices, A.data, n0, nm, ns, 1, bm, bs, case.chunk, case.run, tile=case.tile, real_entries=real)
    assert fmt is not None and fmt['nentries'] == A.nnz
    XS = 16 // case.tile
    seg = None
    if case.table:
        seg = np.zeros((ns, nm, n0 // case.tile), dtype=bool)
        c = A.indices.astype(np.int64)
        seg[c // (n0 * nm), (c // n0) % nm, (c % n0) // case.tile] = True
        for pairs, value in ((case.unflag, False), (case.flag, True)):
            for b, s in pairs:
                x0, m0, s0 = brick_origin(case.dims, case.shape, b)
                seg[s0 + s // (XS * bm), m0 + (s // XS) % bm, x0 // case.tile + s % XS] = value
    fmt.update(ns=ns, tile=case.tile, zw=case.zw, seg=seg, support=None if seg is None else support_table(seg, case.zw))
    D.fmt = fmt
    _data[key] = D
    return D


def panel(D, ncols):
    return np.ascontiguousarray(D.X4[:, :ncols])


# =========================================================================================================================================
# the format, read
# =========================================================================================================================================
def slot_tasks(fmt):
    """(tasks (n, 4) [lo, hi, first table row, rows | shared << 16], table (nb, 2) [brick, end of its slots])"""
    n = fmt['ntasks']
    return fmt['tasks'].reshape(-1, 4)[:n].astype(np.int64), (fmt['table'].reshape(-1, 2).astype(np.int64) if n else np.zeros((0, 2), np.int64))


def fmt_dims(fmt):
    return (fmt['n0'], fmt['nm'], fmt['ns']), (fmt['bm'], fmt['bs'])


def slot_walk(fmt):
    """every entry of the format with where it sits: arrays task, brick (ordinal inside the task), row (of the table), slot (of the
    task), lane, sample, cell (inside the brick), grid (row of the grid), w (complex128); cached in the format"""
    if '_walk' in fmt:
        return fmt['_walk']
    tasks, table = slot_tasks(fmt)
    dims, shape = fmt_dims(fmt)
    words = fmt['words']
    ent = fmt['entries'].reshape(-1, words)
    eflt = ent.view(np.float32)
    sp = fmt['slot_ptr'].astype(np.int64)
    rec = []
    for ti, (lo, hi, bt, nbf) in enumerate(tasks):
        nb, shared = int(nbf) & 0xffff, (int(nbf) >> 16) & 1
        for s in range(lo, hi):
            tr = bt if shared else bt + int(np.searchsorted(table[bt:bt + nb, 1], s, side='right'))
            assert tr < bt + nb, "a slot past the last brick of its task"
            for lane, e in enumerate(range(sp[s], sp[s + 1])):
                rec.append((ti, tr - bt, tr, s - lo, lane, int(ent[e, words - 1]), int(ent[e, 0]), e))
    rec = np.asarray(rec, dtype=np.int64).reshape(-1, 8)
    W = Data()
    W.task, W.brick, W.row, W.slot, W.lane, W.sample, W.cell, W.entry = rec.T
    W.grid = cell_index(dims, shape, table[W.row, 0] if rec.size else W.row, W.cell)
    W.w = eflt[W.entry, 1].astype(np.float64) + 1j * (eflt[W.entry, 2].astype(np.float64) if words == 4 else 0.0)
    fmt['_walk'] = W
    return W


def slot_csr(fmt, M):
    """the CSR the format expands to (entries of weight zero left out)"""
    W = slot_walk(fmt)
    K = fmt['n0'] * fmt['nm'] * fmt['ns']
    keep = W.w != 0
    B = spp.csr_matrix((W.w[keep].astype(C64), (W.sample[keep], W.grid[keep])), shape=(M, K))
    B.sort_indices()
    return B


def cell_flags(fmt):
    """per row of the grid: its segment is flagged (all True without a table)"""
    n0, nm, ns = fmt_dims(fmt)[0]
    if fmt['seg'] is None:
        return np.ones(n0 * nm * ns, dtype=bool)
    return np.repeat(fmt['seg'], fmt['tile'], axis=2).reshape(-1)


def brick_of_cells(fmt):
    (n0, nm, ns), (bm, bs) = fmt_dims(fmt)
    r = np.arange(n0 * nm * ns, dtype=np.int64)
    return (r % n0) // 16 + (n0 // 16) * (((r // n0) % nm) // bm + (nm // bm) * ((r // (n0 * nm)) // bs))


def write_mask(fmt):
    """rows of the grid the call must write: the flagged segments of the bricks of the table (every one of them is in some task)"""
    tasks, table = slot_tasks(fmt)
    covered = np.zeros(table.shape[0], dtype=int)
    for lo, hi, bt, nbf in tasks:
        covered[bt:bt + (nbf & 0xffff)] += 1 if not nbf >> 16 else 0
        if nbf >> 16:
            covered[bt] = -1
    assert np.all(covered != 0) and np.all(covered <= 1), "a brick of the table in no task, or owned twice"
    return np.isin(brick_of_cells(fmt), table[:, 0]) & cell_flags(fmt)


def pieces(fmt):
    """per row of the grid: the shared pieces that add into its brick (0 on owned bricks)"""
    tasks, table = slot_tasks(fmt)
    per_brick = np.zeros(int(brick_of_cells(fmt).max()) + 1, dtype=np.int64)
    for lo, hi, bt, nbf in tasks:
        if nbf >> 16:
            per_brick[table[bt, 0]] += 1
    return per_brick[brick_of_cells(fmt)]


def slot_reference(fmt, X, alpha):
    """(Y (K, NC) complex128, write mask (K,)): alpha conj(G)^T X summed entry by entry of the format; rows outside the mask are 0 here
    and mean 'the caller's bytes'"""
    W = slot_walk(fmt)
    X = np.asarray(X).reshape(X.shape[0], -1)
    K = fmt['n0'] * fmt['nm'] * fmt['ns']
    Y = np.zeros((K, X.shape[1]), dtype=C128)
    np.add.at(Y, W.grid, np.conj(W.w)[:, None] * X[W.sample].astype(C128))
    mask = write_mask(fmt)
    Y *= cf32(alpha)
    Y[~mask] = 0
    return Y, mask


def slot_feeders(fmt):
    """row of the grid -> [(task, brick, slot, lane, sample)] of the entries that add into it"""
    W = slot_walk(fmt)
    out = {}
    for g, rec in zip(W.grid, zip(W.task, W.brick, W.slot, W.lane, W.sample)):
        out.setdefault(int(g), []).append(tuple(int(v) for v in rec))
    return out


def hits(fmt):
    W = slot_walk(fmt)
    return np.bincount(W.grid, minlength=fmt['n0'] * fmt['nm'] * fmt['ns'])


def adjoint_bound(fmt, X, alpha):
    """Per cell and column, a bound on |device - reference| (complex modulus).  With u = 2^-24 and S = sum |w| |x| over the n hits of the
    cell, one part of the image is a sum of n terms t = re x.re + im x.im (|t| <= |w| |x|):
      * a term is fmaf(re, x.re, im * x.im): two roundings, each of a quantity <= |w| |x|                       -> 2 u S in all
      * the n additions into the image (the REALW branch fuses them with its single product: fewer)             -> n u S
      * cmul(alpha, .) is fmaf(a.re, s.re, -a.im * s.im): two roundings of quantities <= |alpha| S              -> 2 u |alpha| S
      * a shared brick: one float atomic add per piece p, each of a partial sum <= |alpha| S                    -> p u |alpha| S
    to first order (n + p + 4) u |alpha| S per part (an error of the image's two parts reaches one part of alpha times it with at
    most |alpha| times its modulus), sqrt 2 of it for the modulus of both parts; the factor 1 + 2^-10 covers the second-order terms
    ((n + p + 4) u < 2^-13 for n <= 1024).  Derived, not measured."""
    W = slot_walk(fmt)
    X = np.asarray(X).reshape(X.shape[0], -1)
    K = fmt['n0'] * fmt['nm'] * fmt['ns']
    S = np.zeros((K, X.shape[1]))
    np.add.at(S, W.grid, np.abs(W.w)[:, None] * np.abs(X[W.sample].astype(C128)))
    ops = hits(fmt) + pieces(fmt) + 4
    return np.sqrt(2.0) * (1 + 2.0 ** -10) * ops[:, None] * 2.0 ** -24 * abs(cf32(alpha)) * S


# =========================================================================================================================================
# the kernels in float32, in their own order
# =========================================================================================================================================
def fma(a, b, c):
    """fmaf: the product is exact in float64; the sum is rounded to float64 and then to float32 (a double rounding differs from the one
    rounding of the instruction only where float64 itself rounds: never on the exact inputs)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def lookup_masks(fmt, bricks, events=None):
    """my_mask of the bricks of one task: 8 passes of 64 (brick, segment) pairs, read from the packed bitmaps with the kernel's own
    word / bit split; a brick whose pairs lie beyond pass 7 keeps 0"""
    (n0, nm, ns), (bm, bs) = fmt_dims(fmt)
    tile, zw = fmt['tile'], fmt['zw']
    XS = 16 // tile
    nseg = XS * bm * bs
    seg_log2 = nseg.bit_length() - 1
    if fmt['support'] is None:
        return [(1 << nseg) - 1] * len(bricks)
    nt = n0 // tile
    bits = fmt['support'][2 * (ns * nt + nt):].view(np.uint32)
    masks = [0] * len(bricks)
    for pair in range(MASK_PASSES * WAVE):
        j, seg = pair >> seg_log2, pair & (nseg - 1)
        if j >= len(bricks) or j >= WAVE:
            continue
        x0, m0, s0 = brick_origin((n0, nm, ns), (bm, bs), int(bricks[j]))
        xs, im, is_ = seg % XS, (seg // XS) % bm, seg // (XS * bm)
        km, ks = m0 + im, s0 + is_
        kmq, kmr = km // zw, km % zw
        if (int(bits[(ks * nt + (x0 // 16) * XS + xs) * zw + kmr]) >> kmq) & 1:
            masks[j] |= 1 << seg
        if events is not None:
            events['pairs'] = max(events.get('pairs', 0), pair + 1)
    return masks


def emulate_slots(fmt, X, alpha, Y0, events=None):
    """ig_ccsrmm_t_slots in float32 on the caller's grid Y0 (K, NC) complex64 -> Y: k_grid_bricks_zero clears the flagged segments of the
    shared bricks, then every task walks its slots in windows of 63 (cnt = min(63, left)), flushes ONCE when base + i >= cur_end,
    adds fmaf(re, x.re, im * x.im) / fmaf(re, x.im, -im * x.re) (complex) or fuses the addition into fmaf(re, x, t) (REALW) per entry
    and column, and flushes at its end: flagged segments only, cmul(alpha, .) stored (owned) or added (shared), then cleared."""
    tasks, table = slot_tasks(fmt)
    dims, shape = fmt_dims(fmt)
    bm, bs = shape
    tile, words = fmt['tile'], fmt['words']
    XS = 16 // tile
    ncell, nseg = 16 * bm * bs, XS * bm * bs
    X = np.asarray(X, dtype=C64).reshape(X.shape[0], -1)
    NC = X.shape[1]
    xre, xim = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    ent = fmt['entries'].reshape(-1, words)
    eflt = ent.view(F32)
    sp = fmt['slot_ptr'].astype(np.int64)
    a = cf32(alpha)
    ar, ai = F32(a.real), F32(a.imag)
    Y = np.array(Y0, dtype=C64, copy=True)
    yre, yim = np.ascontiguousarray(Y.real), np.ascontiguousarray(Y.imag)
    ev = events if events is not None else {}
    ev.update(window_cnt=set(), flush_at=[], stored=0)
    seg_cells = [np.flatnonzero(segment_of(fmt, np.arange(ncell)) == s) for s in range(nseg)]
    for b in fmt['shared'][:fmt['nshared']]:
        mask = lookup_masks(fmt, [int(b)])[0]
        for s in range(nseg):
            if (mask >> s) & 1:
                g = cell_index(dims, shape, int(b), seg_cells[s])
                yre[g] = 0; yim[g] = 0
    for ti, (lo, hi, bt, nbf) in enumerate(tasks):
        nb, shared = int(nbf) & 0xffff, bool((int(nbf) >> 16) & 1)
        nslot = int(hi - lo)
        assert 1 <= nb <= WAVE and nslot >= 1
        my_end = [int(table[bt + l, 1] - lo) if (l < nb and not shared) else 0x7fffffff for l in range(WAVE)]
        my_mask = lookup_masks(fmt, table[bt:bt + nb, 0], ev) + [0] * (WAVE - nb)
        are, aim = np.zeros((ncell, NC), dtype=F32), np.zeros((ncell, NC), dtype=F32)
        st = dict(cur=0, cur_end=my_end[0])

        def flush():
            assert st['cur'] < nb, "a flush past the last brick of the task"
            b, mask = int(table[bt + st['cur'], 0]), my_mask[st['cur']]
            for s in range(nseg):
                if not (mask >> s) & 1:
                    continue
                c = seg_cells[s]
                g = cell_index(dims, shape, b, c)
                o_re = fma(ar, are[c], -ai * aim[c])
                o_im = fma(ar, aim[c], ai * are[c])
                if shared:
                    yre[g] = yre[g] + o_re; yim[g] = yim[g] + o_im
                else:
                    yre[g] = o_re; yim[g] = o_im
                are[c] = 0; aim[c] = 0
                ev['stored'] += 1
            st['cur'] += 1
            st['cur_end'] = my_end[st['cur'] & 63]

        for base in range(0, nslot, WINDOW):
            cnt = min(WINDOW, nslot - base)
            ev['window_cnt'].add(cnt)
            for i in range(cnt):
                if base + i >= st['cur_end']:
                    ev['flush_at'].append((ti, base, i))
                    flush()
                e0, e1 = int(sp[lo + base + i]), int(sp[lo + base + i + 1])
                assert 1 <= e1 - e0 <= WAVE
                c = ent[e0:e1, 0].astype(np.int64)
                assert np.unique(c).size == c.size and c.max() < ncell
                wr = eflt[e0:e1, 1][:, None]
                row = ent[e0:e1, words - 1].astype(np.int64)
                xr, xi = xre[row], xim[row]
                if words == 3:
                    are[c] = fma(wr, xr, are[c])
                    aim[c] = fma(wr, xi, aim[c])
                else:
                    wi = eflt[e0:e1, 2][:, None]
                    are[c] = are[c] + fma(wr, xr, wi * xi)
                    aim[c] = aim[c] + fma(wr, xi, -wi * xr)
        flush()
        assert are.dtype == F32 and yre.dtype == F32
    return (yre + 1j * yim).astype(C64)


def owned_rows(fmt):
    """rows of the grid in the write mask whose brick no shared piece adds into"""
    return write_mask(fmt) & (pieces(fmt) == 0)


# =========================================================================================================================================
# what a case holds, read from the format
# =========================================================================================================================================
def slot_seams(D):
    fmt, case = D.fmt, D.case
    tasks, table = slot_tasks(fmt)
    dims, shape = fmt_dims(fmt)
    (n0, nm, ns), (bm, bs) = dims, shape
    tile, zw = fmt['tile'], fmt['zw']
    XS = 16 // tile
    ncell, nseg = 16 * bm * bs, XS * bm * bs
    W = slot_walk(fmt)
    sp = fmt['slot_ptr'].astype(np.int64)
    shared = (tasks[:, 3] >> 16) & 1
    ev = {}
    sentinel = np.zeros((case.K, 1), dtype=C64)
    emulate_slots(fmt, D.X4[:, :1], ALPHA, sentinel, events=ev)
    s = dict(task_slots=set(int(v) for v in tasks[:, 1] - tasks[:, 0]), window_cnt=ev['window_cnt'], boundary=set(), slot_entries=set(int(v) for v in np.diff(sp)),
             bricks_per_task=set(int(v) & 0xffff for v in tasks[shared == 0, 3]), nseg={nseg}, tile_pts={tile}, shared=bool(shared.any()), owned=bool((shared == 0).any()),
             ntasks_mod4=tasks.shape[0] % WAVES_PER_BLOCK != 0, one_task=tasks.shape[0] == 1, no_table=fmt['support'] is None, cap_flags=set(),
             sample_ends={0, D.M - 1} <= set(int(v) for v in W.sample), cell_ends={0, ncell - 1} <= set(int(v) for v in W.cell))
    for ti, base, i in ev['flush_at']:
        s['boundary'].add('first' if i == 0 and base > 0 else 'last' if i == WINDOW - 1 else 'middle')
    # slots side by side inside a task
    s['one_by_64'] = s['cut_64'] = False
    for lo, hi, bt, nbf in tasks:
        for q in range(lo, hi - 1):
            n1, n2 = int(sp[q + 1] - sp[q]), int(sp[q + 2] - sp[q + 1])
            s['one_by_64'] |= {n1, n2} == {1, WAVE}
            same_brick = np.searchsorted(table[:, 1], q, side='right') == np.searchsorted(table[:, 1], q + 1, side='right')
            ent = fmt['entries'].reshape(-1, fmt['words'])
            if same_brick and n1 == WAVE and not set(ent[sp[q]:sp[q + 1], 0]) & set(ent[sp[q + 1]:sp[q + 2], 0]):
                s['cut_64'] = True                                  # one group of more than 64 distinct cells: 64 + rest
    # how often a cell is hit; a brick whose second group is one entry
    key = table[W.row, 0] * ncell + W.cell
    mult = np.bincount(key)
    s['mult'] = set(int(v) for v in mult[mult > 0])
    per_brick = {}
    for k in np.flatnonzero(mult):
        per_brick.setdefault(k // ncell, []).append(int(mult[k]))
    s['single_second_group'] = any(sum(m >= 2 for m in ms) == 1 and len(ms) > 1 for ms in per_brick.values())
    # the support table
    flags = cell_flags(fmt)
    mask = write_mask(fmt)
    h = hits(fmt)
    s['partial_segment'] = bool(np.any(mask & (h == 0)))
    rows_of = lambda b, seg: cell_index(dims, shape, b, np.flatnonzero(segment_of(fmt, np.arange(ncell)) == seg))
    s['unflagged_beside_flagged'] = s['shared_unflagged'] = s['shared_partial'] = False
    for lo, hi, bt, nbf in tasks:
        nb = int(nbf) & 0xffff
        segflag = [[bool(flags[rows_of(int(table[bt + j, 0]), q)[0]]) for q in range(nseg)] for j in range(nb)]
        s['unflagged_beside_flagged'] |= any(any(f) and not all(f) for f in segflag)
        if nbf >> 16:
            s['shared_unflagged'] |= not all(segflag[0])
            s['shared_partial'] |= any(f and not h[rows_of(int(table[bt, 0]), q)].any() for q, f in enumerate(segflag[0]))
        else:
            s['cap_flags'] |= {(nb, 'first', segflag[0][0]), (nb, 'last', segflag[-1][-1])}
    if fmt['seg'] is not None:
        ks, km, t = np.nonzero(fmt['seg'])
        s['zw_bit'] = set(int(v) for v in km // zw)
        s['nm_gt_zw'] = nm > zw
    per = np.bincount(tasks[shared == 1, 2], minlength=1) if shared.any() else np.zeros(1, int)
    s['pieces'] = set(int(v) for v in per[per > 0])
    s['piece_of_one'] = bool(np.any((tasks[:, 1] - tasks[:, 0] == 1) & (shared == 1)))
    s['pairs'] = ev.get('pairs', 0)
    return s
