"""The host builders of the device formats of a gridding matrix (indigo_amd/grid_formats.py), no GPU: invariants that do not depend
on how a format is built.  Expanded, the entries of the brick, slot and wide-brick formats reproduce every nonzero of the matrix exactly
once, inside the brick they are filed under; tasks tile the entries; the shares' table flags what the support table flags and nothing
outside the grid; the owned-tile bitmap names the tiles of the whole bricks; orders are permutations; the real-weight forms drop the
imaginary word and nothing else.  Every format has a case with shared pieces and, where it can decline, a declining case -- and the test
checks that its inputs really take those paths."""
import numpy as np
import pytest
import scipy.sparse as spp

from indigo_amd import fused, grid_formats as gf
from indigo_amd.sense import SenseProblem

C64 = np.dtype('complex64')
PAD = 0xffffffff


def _gridding(N=(16, 16, 16), width=2, cplx=False, seed=4):
    """(G' in the interleaved panel's column order, its separable records, the problem) with samples on faces, corners and grid points"""
    p = SenseProblem.synthetic(N, 2, nspokes=53, nreadout=2 * N[0], width=width, oversamp=2.0, seed=seed)
    c = p.coord.reshape(3, -1, order='F').copy()
    k = c.shape[1] // 3
    c[:, :k] = np.random.default_rng(seed).choice([-0.5, -0.5 + 1.0 / p.oN[0], 0.5 - 1.0 / p.oN[0], 0.0, 0.25], size=(3, k))
    p.coord = c.reshape(p.coord.shape, order='F')
    p.drop_cache()
    G = p.fused_interp(1).astype(C64)
    if cplx:
        G = (G * np.exp(0.3j)).astype(C64)
    G.sort_indices()
    return G, p.fused_interp_sep(1), p


def _random_csr(T, dims, per_row, seed=1, cplx=True):
    rng = np.random.default_rng(seed)
    K = int(np.prod(dims))
    rows = np.repeat(np.arange(T), per_row)
    vals = rng.standard_normal(rows.size) + (1j * rng.standard_normal(rows.size) if cplx else 0)
    A = spp.csr_matrix((vals.astype(C64), (rows, rng.integers(0, K, size=rows.size))), shape=(T, K))
    A.sum_duplicates(); A.sort_indices()
    return A


def _bricks_of_rows(A, n0, nm, bm, bs):
    """the largest number of 16 x bm x bs bricks one row touches"""
    col = A.indices.astype(np.int64)
    brick = (col % n0) // 16 + (n0 // 16) * (((col // n0) % nm) // bm + (nm // bm) * ((col // (n0 * nm)) // bs))
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return np.bincount(np.unique(rows * (brick.max() + 1) + brick) // (brick.max() + 1)).max()


def _brick_of_entry(table, n):
    table = table.reshape(-1, 2).astype(np.int64)
    return np.repeat(table[:, 0], np.diff(np.concatenate(([0], table[:, 1]))))[:n]


def _check_expansion(A, cell, w, rows, brick, n0, nm, bm, bs):
    """entries (cell inside the brick, complex weight, row, brick) against the matrix: every nonzero exactly once, the rest weight zero"""
    real = w != 0
    assert (cell[real] < 16 * bm * bs).all() and (w[(cell == PAD)] == 0).all()
    nbx, nbm = n0 // 16, nm // bm
    c, b = cell[real].astype(np.int64), brick[real]
    col = (b % nbx) * 16 + c % 16 + n0 * ((((b // nbx) % nbm) * bm + (c // 16) % bm) + nm * ((b // (nbx * nbm)) * bs + c // (16 * bm)))
    key = rows[real].astype(np.int64) * A.shape[1] + col
    assert np.unique(key).size == key.size == np.count_nonzero(A.data)          # every nonzero once, no cell twice
    B = spp.csr_matrix((w[real], (rows[real], col)), shape=A.shape)
    assert abs(A - B).max() == 0


def _check_tasks(tasks, n, unit, chunk):
    """tasks [lo, hi, first table row, rows | shared << 16] tile [0, n) without gap or overlap; shared pieces are at most `chunk` long"""
    t = tasks.reshape(-1, 4).astype(np.int64)
    t = t[np.argsort(t[:, 0], kind='stable')]
    assert t[0, 0] == 0 and t[-1, 1] == n and np.array_equal(t[1:, 0], t[:-1, 1]) and (t[:, 1] > t[:, 0]).all()
    assert (t[:, :2] % unit == 0).all()
    shared = (t[:, 3] >> 16) != 0
    assert ((t[shared, 1] - t[shared, 0]) <= chunk).all()
    return int(np.count_nonzero(shared))


def _cplx(e):
    e = np.ascontiguousarray(e)
    return e[:, 1].view(np.float32) + 1j * (e[:, 2].view(np.float32) if e.shape[1] > 2 else 0)


MATRICES = {'gridding': lambda: (_gridding()[0], (32, 32, 32)), 'gridding-cplx': lambda: (_gridding((16, 12, 20), 2.5, True)[0], (32, 40, 24)),
            'random': lambda: (_random_csr(700, (32, 8, 4), 3), (32, 8, 4))}


@pytest.mark.parametrize("name", sorted(MATRICES))
@pytest.mark.parametrize("ncols,bm,bs,chunk", [(8, 2, 2, 4096), (4, 2, 4, 64), (8, 2, 2, 16)])
def test_bricks_hold_every_nonzero_exactly_once(name, ncols, bm, bs, chunk):
    A, (n0, nm, ns) = MATRICES[name]()
    unit = 64 // ncols
    f = gf.bricks(A.indptr, A.indices, A.data, n0, nm, ns, ncols, bm, bs, chunk, 256)
    assert f is not None and f['words'] == 3 and f['nentries'] % unit == 0 and f['ntasks'] > 0
    e = f['entries'].reshape(-1, 3)[:f['nentries']]
    _check_expansion(A, e[:, 0], _cplx(e), np.repeat(f['rounds'][:f['nentries'] // unit], unit), _brick_of_entry(f['table'], f['nentries']), n0, nm, bm, bs)
    assert _check_tasks(f['tasks'], f['nentries'], unit, max(unit, chunk // unit * unit)) > 0 or chunk == 4096
    if chunk < 4096:
        assert f['nshared'] > 0 and np.isin(f['shared'], f['table'].reshape(-1, 2)[:, 0]).all()


@pytest.mark.parametrize("name", sorted(MATRICES))
@pytest.mark.parametrize("ncols,bm,bs,chunk", [(1, 4, 4, 256), (2, 2, 2, 4), (4, 2, 2, 2)])
def test_slots_hold_every_nonzero_once_and_no_cell_twice(name, ncols, bm, bs, chunk):
    A, (n0, nm, ns) = MATRICES[name]()
    f = gf.slots(A.indptr, A.indices, A.data, n0, nm, ns, ncols, bm, bs, chunk, 16)
    assert f is not None and f['words'] == 4 and f['nentries'] == A.nnz and f['slot_ptr'].size == f['nslots'] + 1
    e = f['entries'].reshape(-1, 4)
    per_slot = np.diff(f['slot_ptr'])
    assert f['slot_ptr'][0] == 0 and f['slot_ptr'][-1] == A.nnz and (per_slot > 0).all() and (per_slot <= 64).all()
    slot = np.repeat(np.arange(f['nslots']), per_slot)
    assert np.unique(slot.astype(np.int64) << 32 | e[:, 0]).size == A.nnz                        # no slot holds a cell twice
    brick = _brick_of_entry(f['table'], f['nslots'])[slot]                                       # (the table counts slots)
    _check_expansion(A, e[:, 0], _cplx(e), e[:, 3], brick, n0, nm, bm, bs)
    assert _check_tasks(f['tasks'], f['nslots'], 1, chunk) > 0 or chunk == 256
    assert f['nshared'] > 0 or chunk == 256


@pytest.mark.parametrize("name,dims,shape,geom", [('gridding', (32, 32, 32), (2, 2), (32, 32, 2, 2)), ('gridding-cplx', (32, 40, 24), (4, 1), (32, 40, 4, 1)),
                                                  ('gridding', None, (2, 2), (32 ** 3, 1, 1, 1)), ('random', (32, 8, 4), (2, 2), (1024, 1, 1, 1))])
@pytest.mark.parametrize("task_shape", [(8192, 2048), (32, 16)])
def test_wide_bricks_hold_every_nonzero_once_and_own_their_whole_bricks(name, dims, shape, geom, task_shape):
    A = MATRICES[name]()[0]
    K = A.shape[1]
    f = gf.wide_bricks(A.indptr, A.indices, A.data, K, dims, shape, task_shape)
    assert f is not None and f['geom'] == geom and f['words'] == 3
    n0, nm, bm, bs = f['geom']
    unit = 4 if bm * bs > 1 else 1
    if dims is not None and unit == 1:
        # the fallback to 16-column bricks: the grid geometry bins, but quads of it would be mostly padding
        binned = gf.bin_by_bricks(A.indptr, A.indices, A.data, *dims, *shape, 4)
        assert binned is not None and binned[0].sum() > 1.6 * A.nnz
    table, tasks = f['table'].reshape(-1, 2), f['tasks'].reshape(-1, 4)
    n = int(table[-1, 1])
    e = f['entries'].reshape(-1, 3)[:n]
    assert (e[:, 0] != PAD).all() and n % unit == 0                          # padding names a valid cell
    _check_expansion(A, e[:, 0], _cplx(e), np.repeat(f['rows'][:n // unit], unit), _brick_of_entry(table, n), n0, nm if bm * bs > 1 else 1, bm, bs)
    nshared = _check_tasks(tasks, n, unit, max(4, task_shape[0] // 4 * 4))
    assert nshared > 0 or task_shape[0] == 8192
    # owned tiles: exactly the 16-row tiles of the non-empty bricks no shared task works on
    whole = np.setdiff1d(table[:, 0], table[tasks[(tasks[:, 3] >> 16) != 0, 2], 0]).astype(np.int64)
    nbx, nbm = n0 // 16, nm // bm
    tiles = {int(b % nbx + nbx * ((((b // nbx) % nbm) * bm + im) + nm * ((b // (nbx * nbm)) * bs + is_))) for b in whole for im in range(bm) for is_ in range(bs)}
    owned = np.flatnonzero(np.unpackbits(f['owned'].view(np.uint8), bitorder='little'))
    assert set(owned.tolist()) == tiles and f['owned'].size == -(-(K // 16) // 32)


def test_rows_all_over_the_grid_decline():
    """a row that touches more than 64 bricks: no brick, slot or wide-brick format (the gather routes serve it)"""
    A = _random_csr(40, (32, 32, 32), 200)
    assert _bricks_of_rows(A, 32, 32, 2, 2) > 64 and _bricks_of_rows(A, 32 ** 3, 1, 1, 1) > 64
    assert gf.bricks(A.indptr, A.indices, A.data, 32, 32, 32, 8) is None
    assert gf.slots(A.indptr, A.indices, A.data, 32, 32, 32, 2) is None
    assert gf.bin_by_bricks(A.indptr, A.indices, A.data, 32, 32, 32, 2, 2, 4) is None
    assert gf.wide_bricks(A.indptr, A.indices, A.data, 32 ** 3, (32, 32, 32)) is None


@pytest.mark.parametrize("N,width,bm,bs,tile,zw", [((16, 16, 16), 3, 4, 4, None, 16), ((16, 16, 16), 2.5, 4, 4, 16, 16), ((16, 16, 16), 3, 4, 4, 4, 16),
                                                   ((16, 16, 16), 3, 8, 2, 8, 20), ((8, 13, 9), 3, 4, 4, None, 16), ((8, 13, 9), 2.5, 4, 4, 8, 16)])
def test_share_table_flags_what_the_support_table_flags(N, width, bm, bs, tile, zw):
    G, sep, p = _gridding(N, width)
    n0, nm, ns = sep['dims']
    table = None if tile is None else fused.grid_support(G, p.oN, tile, (zw, 16))
    f = gf.shares(sep['records'], sep['tw'], sep['dims'], 8, bm, bs, 16, 64, table=table, tile=tile or 16, zw=zw)
    assert f is not None and f['tile'] == (tile or 16) and f['bm'] <= 4 and f['nshared'] > 0
    bm, bs, xs = f['bm'], f['bs'], 16 // f['tile']
    assert xs * bm * bs <= 64
    tab = f['table'].reshape(-1, 4)
    assert f['nbricks'] == tab.shape[0] and tab[-1, 1] == f['nshares'] and (np.diff(tab[:, 0].astype(np.int64)) > 0).all()
    _check_tasks(f['tasks'], f['nshares'], 1, 16)
    bits = None if table is None else fused.split_support(table, p.oN, tile, zw)[2]
    nbx, nbm = n0 // 16, -(-nm // bm)
    beyond = 0
    for brick, lo, hi in tab[:, [0, 2, 3]].astype(np.int64):
        want = 0
        for is_ in range(bs):
            for im in range(bm):
                km, ks = ((brick // nbx) % nbm) * bm + im, (brick // (nbx * nbm)) * bs + is_
                beyond += not (km < nm and ks < ns)
                for x in range(xs):
                    if km < nm and ks < ns and (bits is None or (int(bits[ks * (n0 // f['tile']) + (brick % nbx) * xs + x, km % zw]) >> (km // zw)) & 1):
                        want |= 1 << (x + xs * (im + bm * is_))
        assert int(lo) | int(hi) << 32 == want, brick
    assert (beyond > 0) == (nm % bm != 0 or ns % bs != 0)          # (the non-dividing cases do reach beyond the grid)
    rows = tab[np.searchsorted(tab[:, 0], np.unique(tab[np.flatnonzero(np.diff(np.concatenate(([0], tab[:, 1].astype(np.int64)))) > 16), 0]))]
    assert np.array_equal(f['shared'].reshape(-1, 4), rows)        # the table rows of the bricks cut into pieces
    recx, stride = gf.records_with_rows(sep['records'])
    rw = sep['records'].shape[1]
    assert stride >= rw + 2 * 8 and np.array_equal(recx.reshape(-1, stride)[:, :rw], sep['records']) and not recx.reshape(-1, stride)[:, rw:].any()


def test_shares_decline_an_x_axis_that_is_no_multiple_of_16():
    G, sep, p = _gridding((12, 8, 8), 3)
    assert sep['dims'][0] == 24
    assert gf.shares(sep['records'], sep['tw'], sep['dims'], 8, 4, 4) is None


@pytest.mark.parametrize("dims,runs_order", [((32, 32, 32), True), (None, True), ((32, 32, 32), False)])
def test_runs_order_is_a_permutation(dims, runs_order):
    A = _gridding()[0]
    A.data = A.data.real.astype(C64)          # (the run format's real form wants imaginary parts that are exactly zero)
    touched = np.unique(A.indices).astype(np.int32)
    f = gf.runs(A.indptr, np.searchsorted(touched, A.indices).astype(np.int32), A.data, touched, dims, runs_order)
    nruns = (A.shape[0] + 15) // 16
    assert f is not None and f['all_real'] == 1 and f['dptr'].size == nruns + 1 and f['ndistinct'] == f['dptr'][-1] < A.nnz
    if dims is None or not runs_order:
        assert f['order'] is None
    else:
        assert np.array_equal(np.sort(f['order']), np.arange(nruns)) and not np.array_equal(f['order'], np.arange(nruns))


@pytest.mark.parametrize("ncols", [2, 4, 8])
def test_gather_order_is_a_permutation_of_the_groups(ncols):
    from indigo_amd import _lib
    _, sep, _ = _gridding()
    group = _lib.lib().ig_grid_gather_sep_group(ncols, sep['tw'])
    order = gf.gather_order(sep['records'], sep['tw'], ncols)
    assert group > 0 and np.array_equal(np.sort(order), np.arange(-(-sep['records'].shape[0] // group)))
    assert gf.gather_order(sep['records'][:4 * group], sep['tw'], ncols) is None          # too few groups to order


def test_real_weight_forms_drop_exactly_the_imaginary_word():
    A, (n0, nm, ns) = MATRICES['gridding']()
    assert gf.weights_are_real(A.data) and not gf.weights_are_real(MATRICES['gridding-cplx']()[0].data)
    args = (A.indptr, A.indices, A.data, n0, nm, ns)
    for build, kw, keep in ((gf.bricks, dict(ncols=8), [0, 1]), (gf.slots, dict(ncols=2), [0, 1, 3])):
        full, real = build(*args, real_entries=False, **kw), build(*args, real_entries=True, **kw)
        e = full['entries'].reshape(-1, full['words'])
        assert real['words'] == full['words'] - 1 and np.array_equal(real['entries'].reshape(-1, real['words']), e[:, keep])
        im = np.abs(np.ascontiguousarray(e[:, 2]).view(np.float32)).max()                     # (the word dropped held the residue weights_are_real allows)
        assert im <= 2.0 ** -34 * np.abs(A.data.real).max()
        assert all(np.array_equal(full[k], real[k]) for k in full if k not in ('entries', 'words'))
    full, real = (gf.wide_bricks(A.indptr, A.indices, A.data, A.shape[1], (n0, nm, ns), real_entries=r) for r in (False, True))
    assert (full['words'], real['words']) == (3, 2) and np.array_equal(real['entries'].reshape(-1, 2), full['entries'].reshape(-1, 3)[:, :2])
    flat = gf.wide_bricks(A.indptr, A.indices, A.data, A.shape[1], None, real_entries=True)
    assert flat['geom'] == (A.shape[1], 1, 1, 1) and flat['words'] == 3                    # (16-column bricks keep the complex entries)
