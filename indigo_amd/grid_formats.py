"""Host side of the device formats of a gridding matrix: the brick, slot, share, wide-brick and run formats and the Morton gather
order that `HipBackend.csr_matrix` (backends/hip_csr.py) uploads and its kernels read (include/indigo_hip.h).

Every builder takes host arrays and scalars and returns a plain dict of numpy arrays and Python scalars, or None when the matrix
does not qualify for the format.  Nothing here touches a device or a backend: the only library calls are the native HOST routines
(ig_grid_bricks_count / _fill, ig_grid_slots_build, ig_grid_shares_count / _fill, ig_csr_runs_build), so all of it runs and is
tested without a GPU (tests/test_grid_formats_cpu.py).
"""
import ctypes

import numpy as np

from indigo_amd import _lib

_C64 = np.dtype('complex64')


def weights_are_real(data):
    """True when the imaginary parts of a complex64 array are nothing but rounding residue: at most 2^-34 of the largest magnitude
    (the residue of exp(2 pi i phase) for a phase of some hundred half turns is ~1e-13 relative; 2^-34 = 5.8e-11 is still a thousand
    times below the float32 rounding of the products it would enter)"""
    if data.size == 0:
        return False
    im = float(np.abs(data.imag).max())
    return im == 0.0 or im <= float(np.abs(data.real).max()) * 2.0 ** -34


def brick_tasks(counts, ptr, chunk, run, max_bricks=64, longest_first=True):
    """Task list and brick table of ig_ccsrmm_t_bricks (include/indigo_hip.h) from the entries per brick `counts` and their
    prefix sums `ptr`: table = (brick, end of its entries) per non-empty brick; a brick with more than `chunk` entries is
    cut into shared tasks of at most `chunk`; the others are grouped into runs of consecutive table rows -- a new run
    starts when the entry offset crosses a multiple of `run`, after a heavy brick, and after `max_bricks` bricks.  Returns
    tasks (n, 4) int32 [lo, hi, first table row, rows | shared << 16] sorted longest first (or, longest_first=False, in
    brick order), table (nb, 2) int32, and the ids of the shared bricks."""
    bricks = np.flatnonzero(counts)
    if bricks.size == 0:
        return np.zeros((0, 4), np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    cnt = counts[bricks].astype(np.int64)
    lo_b, hi_b = ptr[bricks], ptr[bricks + 1]
    table = np.stack([bricks, hi_b], axis=1).astype(np.int32)
    heavy = cnt > chunk
    # runs of light bricks
    light = np.flatnonzero(~heavy)
    key = np.cumsum(heavy)[light] * (int(ptr[-1]) // max(run, 1) + 2) + lo_b[light] // max(run, 1)
    new_run = np.ones(light.size, dtype=bool)
    new_run[1:] = key[1:] != key[:-1]
    run_id = np.cumsum(new_run) - 1
    first_of_run = np.flatnonzero(new_run)
    rank = np.arange(light.size) - first_of_run[run_id]
    new_run |= (rank % max_bricks) == 0
    starts = np.flatnonzero(new_run)
    ends = np.append(starts[1:], light.size) - 1
    t_run = np.stack([lo_b[light[starts]], hi_b[light[ends]], light[starts], ends - starts + 1], axis=1) if light.size else np.zeros((0, 4), np.int64)
    # pieces of heavy bricks
    hv = np.flatnonzero(heavy)
    npiece = (cnt[hv] + chunk - 1) // chunk
    rep = np.repeat(np.arange(hv.size), npiece)
    firstp = np.concatenate(([0], np.cumsum(npiece)[:-1])) if hv.size else np.zeros(0, np.int64)
    part = np.arange(rep.size) - firstp[rep]
    plo = lo_b[hv][rep] + part * chunk
    phi = np.minimum(plo + chunk, hi_b[hv][rep])
    t_hv = np.stack([plo, phi, hv[rep], np.full(rep.size, 1 | (1 << 16))], axis=1) if rep.size else np.zeros((0, 4), np.int64)
    tasks = np.concatenate([t_hv, t_run]).astype(np.int32)
    order = np.argsort(-(tasks[:, 1] - tasks[:, 0]), kind='stable') if longest_first else np.argsort(tasks[:, 0], kind='stable')
    tasks = np.ascontiguousarray(tasks[order])
    return tasks, np.ascontiguousarray(table), bricks[hv].astype(np.int32)


def _csr(indptr, indices, data):
    return np.ascontiguousarray(indptr, dtype=np.int32), np.ascontiguousarray(indices, dtype=np.int32), np.ascontiguousarray(data, dtype=_C64)


def bin_by_bricks(indptr, indices, data, n0, nm, ns, bm, bs, unit, accept=None):
    """The nonzeros of a CSR matrix sorted by the 16 x bm x bs brick of the n0 x nm x ns grid their column falls into (native host
    routines), a row's share of a brick padded to a multiple of `unit` entries: (counts per brick, their prefix sums, entries
    (n, 3) uint32 {cell inside the brick, re, im}, row of every `unit` entries).  None when ig_grid_bricks_count declines (e.g. a row
    that touches more than 64 bricks: very wide gridding kernels) or `accept(counts)` is false."""
    L = _lib.lib()
    indptr, indices, data = _csr(indptr, indices, data)
    m = indptr.size - 1
    counts = np.zeros((n0 // 16) * (nm // bm) * (ns // bs), dtype=np.int32)
    if L.ig_grid_bricks_count(m, indptr.ctypes.data, indices.ctypes.data, n0, nm, ns, bm, bs, unit, counts.ctypes.data) != 0 \
            or (accept is not None and not accept(counts)):
        return None
    ptr = np.zeros(counts.size + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    entries = np.empty((max(int(ptr[-1]), 1), 3), dtype=np.uint32)
    rows = np.empty(max(int(ptr[-1]) // unit, 1), dtype=np.uint32)
    _lib.check(L.ig_grid_bricks_fill(m, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, n0, nm, ns, bm, bs, unit,
                                     ptr.ctypes.data, entries.ctypes.data, rows.ctypes.data), None, "ig_grid_bricks_fill")
    return counts, ptr, entries, rows


def _max_bricks(tile, bm, bs):
    """bricks per run: the kernels look up 512 support segments per run, (16 / tile) * bm * bs per brick"""
    return min(64, 512 // ((16 // tile) * bm * bs))


def _task_arrays(tasks, table, shared):
    """what is uploaded of brick_tasks' result (an empty list is a placeholder: the kernels are handed valid pointers)"""
    return dict(ntasks=int(tasks.shape[0]), nshared=int(shared.size), tasks=tasks.reshape(-1) if tasks.size else np.zeros(4, np.int32),
                table=table.reshape(-1) if table.size else np.zeros(2, np.int32), shared=shared if shared.size else np.zeros(1, np.int32))


def bricks(indptr, indices, data, n0, nm, ns, ncols=8, bm=2, bs=2, chunk=4096, run=4096, tile=16, real_entries=False):
    """The brick format of ig_ccsrmm_t_bricks: the nonzeros sorted by brick, padded so that a wave instruction (64/ncols entries x
    ncols panel columns) holds entries of one row only.  A task (one wave) is a run of consecutive non-empty bricks of about `run`
    entries, or a piece of at most `chunk` entries of a heavy brick (more than `chunk` entries: shared).  `tile`: kx points per entry
    of the support table the scatter writes by (the runs of bricks are sized for its segments)."""
    assert ncols in (4, 8) and bm * bs <= 32
    unit = 64 // ncols
    chunk = max(unit, chunk // unit * unit)
    binned = bin_by_bricks(indptr, indices, data, n0, nm, ns, bm, bs, unit)
    if binned is None:
        return None
    counts, ptr, entries, round_rows = binned
    assert ptr[-1] < 2**31, "brick entries are addressed with 32 bits"
    # Real weights (a gridding matrix times the +-1 modulation of a centred transform on an even grid, whose imaginary parts
    # are the 1e-16 rounding residue of exp(i pi k)): 8-byte entries {cell, re}
    if real_entries:
        entries = np.ascontiguousarray(entries[:, :2])
    return dict(_task_arrays(*brick_tasks(counts, ptr, chunk, run, max_bricks=_max_bricks(tile, bm, bs))),
                n0=int(n0), nm=int(nm), bm=int(bm), bs=int(bs), ncols=int(ncols), words=entries.shape[1], nentries=int(ptr[-1]),
                entries=entries.reshape(-1), rounds=round_rows)


def slots(indptr, indices, data, n0, nm, ns, ncols=1, bm=2, bs=2, chunk=256, run=128, tile=16, real_entries=False):
    """The slot format of ig_ccsrmm_t_slots for an `ncols`-column panel (1, 2 or 4): the nonzeros binned by 16 x bm x bs bricks
    WITHOUT padding (unit 1), reordered inside every brick so that a slot of at most 64 entries never holds a cell twice
    (ig_grid_slots_build), tasks = runs of about `run` slots of consecutive bricks, heavy bricks (more than `chunk` slots) cut into
    shared pieces."""
    assert ncols in (1, 2, 4)
    binned = bin_by_bricks(indptr, indices, data, n0, nm, ns, bm, bs, 1, accept=lambda counts: int(counts.sum(dtype=np.int64)) * 16 < 2 ** 31)
    if binned is None:
        return None
    counts, ptr, e12, rows = binned
    nb, nent = counts.size, int(ptr[-1])
    e16 = np.empty((max(nent, 1), 4), dtype=np.uint32)
    brick_slots = np.zeros(nb, dtype=np.int32)
    slot_ptr = np.empty(nent + 1, dtype=np.int32)
    nslots = ctypes.c_int64()
    _lib.check(_lib.lib().ig_grid_slots_build(nb, ptr.ctypes.data, e12.ctypes.data, rows.ctypes.data, 16 * bm * bs, e16.ctypes.data,
                                              brick_slots.ctypes.data, slot_ptr.ctypes.data, ctypes.byref(nslots)), None, "ig_grid_slots_build")
    del e12, rows
    sptr = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(brick_slots, out=sptr[1:])
    if real_entries:
        e16 = np.ascontiguousarray(e16[:, [0, 1, 3]])     # {cell, re, row}: 12 bytes per nonzero
    return dict(_task_arrays(*brick_tasks(brick_slots, sptr, chunk, run, max_bricks=_max_bricks(tile, bm, bs))),
                n0=int(n0), nm=int(nm), bm=int(bm), bs=int(bs), ncols=int(ncols), words=e16.shape[1], nslots=int(nslots.value), nentries=nent,
                entries=e16.reshape(-1), slot_ptr=slot_ptr[:int(nslots.value) + 1].copy())


def records_with_rows(rec):
    """The separable records widened for the share scatter, and their stride in words: the MFMA scatter reads a share's record and
    panel row as ONE line -- the record, then room for the row k_sep_pack_recx writes there"""
    rw = rec.shape[1]
    rs = 32 if rw == 16 else 64
    recx = np.zeros((rec.shape[0], rs), dtype=np.uint32)
    recx[:, :rw] = rec
    return recx.reshape(-1), rs


def shares(rec, tw, dims, ncols=8, bm=8, bs=2, chunk=1024, run=1024, table=None, tile=16, zw=16):
    """The share format of ig_grid_scatter_sep: every (sample, brick of 16 x bm x bs cells) pair a sample's footprint meets is one
    8-byte share, binned by brick (ig_grid_shares_count / _fill: brick order, sample order inside a brick); the taps come from the
    separable records `rec`.  A task (one wave) is a run of consecutive non-empty bricks of about `run` shares, or a piece of at most
    `chunk` shares of a heavy brick (shared).  `table`: the support table (`tile` kx points per entry, `zw` words per bitmap) whose
    flagged segments are looked up here, once per brick; None flags every segment inside the grid."""
    L = _lib.lib()
    assert ncols in (4, 8)
    bm, bs = min(int(bm), 4), min(int(bs), 4)          # (the brick image is four MFMA blocks x four accumulator groups)
    n0, nm, ns = dims
    xs = 16 // tile
    while xs * bm * bs > 64 and bs > 1:
        bs //= 2
    while xs * bm * bs > 64 and bm > 1:
        bm //= 2
    # (bricks need not divide the middle and slow axes: the part of a last brick outside the grid is never flagged below)
    nbx, nbm, nbs = n0 // 16, -(-nm // bm), -(-ns // bs)
    nb = nbx * nbm * nbs
    counts = np.zeros(nb, dtype=np.int32)
    if n0 % 16 or L.ig_grid_shares_count(rec.shape[0], rec.ctypes.data, tw, n0, nm, ns, bm, bs, counts.ctypes.data) != 0:
        return None
    ptr = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    assert ptr[-1] < 2**31, "shares are addressed with 32 bits"
    sh = np.empty((max(int(ptr[-1]), 1), 2), dtype=np.uint32)
    _lib.check(L.ig_grid_shares_fill(rec.shape[0], rec.ctypes.data, tw, n0, nm, ns, bm, bs, ptr.ctypes.data, sh.ctypes.data), None, "ig_grid_shares_fill")
    tasks, btable, shared = brick_tasks(counts, ptr, int(chunk), int(run), max_bricks=64)
    # the flagged segments of every non-empty brick: bit xs + XS * (im + bm * is), from the support table's input-side bitmaps
    bricks_ = btable[:, 0].astype(np.int64) if btable.size else np.zeros(0, np.int64)
    mask = np.zeros(bricks_.size, dtype=np.uint64)
    if bricks_.size:
        bits = None
        if table is not None:
            nt = n0 // tile
            tabh = np.ascontiguousarray(table, dtype=np.int16).reshape(-1)
            off = 2 * (ns * nt + nt)
            bits = tabh[off:off + 2 * ns * nt * zw].view(np.uint32).reshape(ns * nt, zw)
        bx, bmi, bsi = bricks_ % nbx, (bricks_ // nbx) % nbm, bricks_ // (nbx * nbm)
        for is_ in range(bs):
            for im in range(bm):
                km, ks = bmi * bm + im, bsi * bs + is_
                inside = (km < nm) & (ks < ns)                 # (a last brick may reach beyond the grid)
                kmc, ksc = np.minimum(km, nm - 1), np.minimum(ks, ns - 1)
                for x in range(xs):
                    bit = inside.astype(np.uint64) if bits is None else \
                        (((bits[ksc * nt + bx * xs + x, kmc % zw] >> (kmc // zw).astype(np.uint32)) & np.uint32(1)).astype(np.uint64) * inside)
                    mask |= bit << np.uint64(x + xs * (im + bm * is_))
    tab16 = np.empty((max(bricks_.size, 1), 4), dtype=np.uint32)
    if bricks_.size:
        tab16[:, 0:2] = btable.astype(np.uint32)
        tab16[:, 2] = (mask & np.uint64(0xffffffff)).astype(np.uint32)
        tab16[:, 3] = (mask >> np.uint64(32)).astype(np.uint32)
    sh_rows = tab16[np.searchsorted(bricks_, shared.astype(np.int64))] if shared.size else np.zeros((1, 4), np.uint32)
    return dict(bm=int(bm), bs=int(bs), tile=int(tile), ncols=int(ncols), ntasks=int(tasks.shape[0]), nshared=int(shared.size),
                nshares=int(ptr[-1]), nbricks=int(bricks_.size), tasks=tasks.reshape(-1) if tasks.size else np.zeros(4, np.int32),
                table=tab16.reshape(-1), shares=sh.reshape(-1), shared=np.ascontiguousarray(sh_rows).reshape(-1))


def guess_grid_dims(k):
    """(n, n, n) when the column count `k` is a cube with n a multiple of 32, else None.  Only a grouping of the columns:
    a wrong guess costs speed, never correctness (rows that touch more than 64 bricks decline the format)."""
    n = int(round(k ** (1.0 / 3.0)))
    return (n, n, n) if n > 0 and n ** 3 == k and n % 32 == 0 else None


def wide_bricks(indptr, indices, data, k, dims=None, wide_brick_shape=(2, 2), wide_task_shape=(8192, 2048), real_entries=False):
    """The matrix (k columns) binned by bricks, 12-byte entries {column inside the brick, re, im} + their rows: the format of
    ig_ccsrmm_t_bricks_wide[_grid] (adjoint of a 64-column column-major panel as a scatter).  Bricks are 16 x bm x bs
    (`wide_brick_shape`) points of the grid `dims` the columns form, else 16 consecutive columns.  None when the matrix does not
    qualify (a row touching more than 64 bricks)."""
    indptr, indices, data = _csr(indptr, indices, data)
    bm, bs = wide_brick_shape
    geoms = []
    if dims is not None and bm * bs > 1 and dims[0] % 16 == 0 and dims[1] % bm == 0 and dims[2] % bs == 0:
        geoms.append((dims[0], dims[1], dims[2], bm, bs))
    geoms.append((k, 1, 1, 1, 1))
    nnz = max(int(indptr[-1] - indptr[0]), 1)
    for n0, nm, ns, bm, bs in geoms:
        # grid bricks: a row's share of a brick padded to QUADS (one panel row is loaded per four entries).  A matrix whose rows do
        # not cluster on the (guessed) grid would be mostly padding in quads: keep 16-row bricks
        unit = 4 if bm * bs > 1 else 1
        binned = bin_by_bricks(indptr, indices, data, n0, nm, ns, bm, bs, unit,
                               accept=lambda counts: unit == 1 or int(counts.sum(dtype=np.int64)) <= 1.6 * nnz)
        if binned is not None:
            break
    else:
        return None
    counts, ptr, e12, rows = binned
    nbx, nbm = n0 // 16, nm // bm
    if unit > 1 and ptr[-1] > 0:
        # padding entries (weight zero) take the cell of the real entry before them: whatever the panel row holds
        # (an infinity times zero) lands on a cell the sample touches anyway
        cell = e12[:int(ptr[-1]), 0]
        last_real = np.maximum.accumulate(np.where(cell != 0xffffffff, np.arange(cell.size), 0))
        cell[:] = cell[last_real]
    # tasks: pieces of at most 4096 entries of a heavy brick, runs of about 1024 entries of consecutive bricks, longest first.
    # Measured on BASELINE config 3 and rejected (round 3, profiles/r03_cfg3_sweep_*.txt): bricks in index order or in a
    # (y, z)-blocked order of the grid, with chunks of 4..64 consecutive workgroups dealt to one XCD so that the bricks that
    # need the same rows of X meet behind one L2 -- 3.7..4.2 ms against 3.35 ms, and the same 9.7 GB of re-fetched rows by
    # the PMC counters: a brick takes a wave ~25 us, a line lives ~7 us in a 4 MB L2 that 0.5 TB/s stream through.
    chunk, run = (max(4, int(v) // 4 * 4) for v in wide_task_shape)
    tasks, table, shared = brick_tasks(counts, ptr, chunk, run, max_bricks=64, longest_first=True)
    # tiles (16 rows of the result) some task stores in full: those of the non-empty bricks that are not cut into shared pieces
    owned_b = np.zeros(counts.size, dtype=bool)
    owned_b[table[:, 0]] = True
    owned_b[shared] = False
    ob = np.flatnonzero(owned_b).astype(np.int64)
    bx, bmi, bsi = ob % nbx, (ob // nbx) % nbm, ob // (nbx * nbm)
    owned = np.zeros(k // 16, dtype=bool)
    for im in range(bm):
        for is_ in range(bs):
            owned[bx + nbx * ((bmi * bm + im) + nm * (bsi * bs + is_))] = True
    bits = np.packbits(np.concatenate([owned, np.zeros((-owned.size) % 32, dtype=bool)]), bitorder='little').view(np.uint32)
    if bm * bs > 1 and real_entries:
        e12 = np.ascontiguousarray(e12[:, :2])            # {cell, re}: the register-image kernel's real-weight form
    return dict(ntasks=int(tasks.shape[0]), geom=(n0, nm, bm, bs), words=e12.shape[1], owned=bits,
                tasks=tasks.reshape(-1) if tasks.size else np.zeros(4, np.int32), table=table.reshape(-1) if table.size else np.zeros(2, np.int32),
                entries=e12.reshape(-1), rows=rows)


def runs(indptr, compact, data, touched, dims=None, runs_order=True):
    """The run format of a matrix over its touched columns (ig_csr_runs_build; `touched` = the columns some nonzero names, `compact`
    = the nonzeros' column indices into them).  None when the matrix does not qualify."""
    L = _lib.lib()
    indptr, compact, data = _csr(indptr, compact, data)
    m, K = indptr.size - 1, int(touched.size)
    nruns = (m + 15) // 16
    dptr = np.zeros(nruns + 1, dtype=np.int32)
    if indptr[0] != 0 or L.ig_csr_runs_build(m, K, indptr.ctypes.data, compact.ctypes.data, data.ctypes.data, dptr.ctypes.data, None, None, None) != 0:
        return None
    dcols = np.empty(max(int(dptr[-1]), 1), dtype=np.uint32)
    entries = np.empty((max(int(indptr[-1]), 1), 3), dtype=np.uint32)
    real = ctypes.c_int(0)
    _lib.check(L.ig_csr_runs_build(m, K, indptr.ctypes.data, compact.ctypes.data, data.ctypes.data, dptr.ctypes.data,
                                   dcols.ctypes.data, entries.ctypes.data, ctypes.byref(real)), None, "ig_csr_runs_build")
    # order of the runs: by the 16 x 16 x 16 brick of the grid `dims` their first nonzero falls into -- runs that are neighbours in
    # space share panel rows and then meet behind one L2.  Only a grouping: any order gives the same product.
    order = None
    if dims is not None and runs_order and nruns > 1:
        first = np.minimum(indptr[np.minimum(np.arange(nruns, dtype=np.int64) * 16, m - 1)], max(int(indptr[-1]) - 1, 0))
        col = touched.astype(np.int64)[compact[first]] if indptr[-1] > 0 else np.zeros(nruns, np.int64)
        n0, nm, ns = dims
        bx, bm_, bs_ = (col % n0) // 16, ((col // n0) % nm) // 16, (col // (n0 * nm)) // 16
        key = bx + ((n0 + 15) // 16) * (bm_ + ((nm + 15) // 16) * bs_)
        order = np.argsort(key, kind='stable').astype(np.int32)
    return dict(order=order, dptr=dptr, dcols=dcols, entries=entries.reshape(-1), all_real=int(real.value), ndistinct=int(dptr[-1]))


def gather_order(rec, tw, ncols):
    """The order in which the workgroups of the record gather take their groups of consecutive samples (ig_grid_gather_sep's
    group_order) for an `ncols`-column panel: the groups sorted by the 32^3-cell block of the grid their first sample's first tap
    lies in, blocks in Morton order; None for too few groups to matter.  Measured (profiles/r06_gather_order.txt): 8 x the spokes
    3.28 -> 2.79 ms, half-width 3 1.46 -> 1.36 ms, the headline 0.430 -> 0.416 ms."""
    group = int(_lib.lib().ig_grid_gather_sep_group(int(ncols), int(tw)))
    if group <= 0 or rec.shape[0] <= 4 * group:
        return None
    h0, h1 = rec[::group, 3 * tw], rec[::group, 3 * tw + 1]
    j = [(h0 & 0xffff).astype(np.int64) >> 5, (h0 >> 16).astype(np.int64) >> 5, (h1 & 0xffff).astype(np.int64) >> 5]
    key = np.zeros_like(j[0])
    for bit in range(11):                       # axes of up to 65535 points: 11 bits of 32-cell blocks each
        for a in range(3):
            key |= ((j[a] >> bit) & 1) << (3 * bit + a)
    return np.argsort(key, kind='stable').astype(np.uint32)


DCF_TILE = (16, 8, 8)


def dcf_tiles(rec, tw, dims, piece=None):
    """The samples of the separable records `rec` binned for the Pipe-Menon spread (ig_dcf_spread_r32) by the
    16 x 8 x 8 tile of the grid `dims` (memory order; need not be multiples of the tile) in which their wrapped first tap lies, tile
    t0 + ceil(n0 / 16) * (t1 + ceil(nm / 8) * t2): dict(order = the samples sorted by tile (stable: trajectory order inside a tile),
    uint32; ids = the non-empty tiles, ascending, int32; ptr = int64, len(ids) + 1: the samples of tile ids[k] are
    order[ptr[k]:ptr[k + 1]]).  A workgroup of the spread sums one tile; the gather and divide visits the samples in the same order.
    piece: a tile of more samples (the k-space centre of a radial scan puts 3e5 of 2^24 samples on one tile) is listed several times,
    each entry with at most `piece` consecutive samples of it, so that no workgroup is left with a hundredth of the whole scan; integer
    sums do not care.  None: every tile once."""
    n0, nm, ns = (int(n) for n in dims)
    h0, h1 = rec[:, 3 * tw], rec[:, 3 * tw + 1]
    t0, t1, t2 = (h0 & 0xffff).astype(np.int64) // DCF_TILE[0], (h0 >> 16).astype(np.int64) // DCF_TILE[1], (h1 & 0xffff).astype(np.int64) // DCF_TILE[2]
    nt0, nt1 = -(-n0 // DCF_TILE[0]), -(-nm // DCF_TILE[1])
    tile = t0 + nt0 * (t1 + nt1 * t2)
    order = np.argsort(tile, kind='stable')
    ids, counts = np.unique(tile, return_counts=True)
    ptr = np.zeros(ids.size + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    if piece is not None and counts.size and int(counts.max()) > int(piece):
        pieces = -(-counts // int(piece))
        within = np.arange(int(pieces.sum()), dtype=np.int64) - np.repeat(np.cumsum(pieces) - pieces, pieces)
        ptr = np.append(np.repeat(ptr[:-1], pieces) + within * int(piece), ptr[-1])
        ids = np.repeat(ids, pieces)
    return dict(order=order.astype(np.uint32), ptr=ptr, ids=ids.astype(np.int32))
