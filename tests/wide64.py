"""A float64 restatement of the two 64-column products of BASELINE config 3 -- the forward product by runs (k_csrmm_runs64r,
indigo_amd/csrc/ig_spmm_runs.hip, entry ig_ccsrmm_xrows_runs) and the adjoint by wide bricks (k_bricks_wide64r, k_bricks_wide64,
k_wide_zero_unowned, indigo_amd/csrc/ig_spmm_bricks.hip, entries ig_ccsrmm_t_bricks_wide[_grid]) --, hand-built matrices that put
run lengths, window offsets, task lengths and brick boundaries on the seams of those kernels, tables that say what every case is
for, and float32 emulations of the kernels that read the DEVICE FORMATS (grid_formats.runs, grid_formats.wide_bricks) in the
kernels' own order.  Plain numpy / scipy: nothing here needs a GPU.

References, in complex128:
  forward   beta Y0 + alpha A X[xrows]; beta == 0 does not read Y0 (BLAS rule)
  adjoint   alpha A^H X; rows of Y that no nonzero touches are exactly zero

Exact inputs (spmm64.exact_values): matrix values and panel entries have NONZERO INTEGER parts in [-4, 4], alpha = 0.5 - 0.25j,
beta = -0.5 + 1.5j.  A part of a product is an integer of magnitude <= 32, so every partial sum of the n nonzeros that feed one
result element -- in any order and grouping, with fused multiply-adds or without -- is an integer of magnitude <= 32 n.  THE BOUND:
32 x (most nonzeros in a row; for the adjoint most nonzeros in a column) < 2^24, up to which float32 holds every integer
(tests/test_wide64_cpu.py asserts it for every case, and n <= 1024 besides).  alpha acc is then a multiple of 1/4 of magnitude
<= 0.75 x 32 n and beta y a multiple of 1/2 below 8: with n <= 1024 the result has at most 17 significant bits and nothing rounds.
The float atomic adds of shared pieces add such multiples of 1/4, and their partial sums obey the same bound in whatever order the
pieces arrive: shared bricks compare deterministically too.  The zero-weight
padding entries of the quad format multiply finite panel values and add nothing.  The device must reproduce the reference by value,
element for element (np.array_equal: -0.0 equals 0.0)."""
import functools

import numpy as np
import scipy.sparse as spp

from spmm64 import ALPHA, BETA, C64, C128, EXACT_LIMIT, cf32, exact_values, finish_f32, is_f32, rounding_values  # noqa: F401

# ---- the constants of the kernels the cases and emulations are built on (test_wide64_cpu.py reads them out of the sources) --------------
RUN_ROWS = 16               # matrix rows per run
RING = 16                   # panel rows in flight (v64..v95)
WINDOW = 64                 # distinct rows / entries per prefetched window
TRIP, TQ, AHEAD = 48, 12, 11    # k_bricks_wide64r: entries / quads per trip, look-ahead of the panel rows in quads
MAX_BRICKS = 64             # bricks per task (lanes of my_end / my_row0; grid_formats.wide_bricks' max_bricks)
WIDE_LD = 65                # LDS image row stride
GROUP, ROTATION = 4, 3      # k_bricks_wide64: entries per group, groups in the rotation
ZERO_BLOCK = 4096           # rows of Y per workgroup of k_wide_zero_unowned
COL_BITS = 27               # dcols: panel row | (entries - 1) << 27
SENTINEL = 7 - 3j           # what a result holds before a product


def l1(z):
    return np.abs(z.real) + np.abs(z.imag)


# =========================================================================================================================================
# the forward product by runs
# =========================================================================================================================================
NX = 230                    # compact columns (rows of the repacked panel)
XTOTAL = 2 * NX + 3         # rows of the panel the caller holds: the touched ones are a strict subset
TOUCHED = np.concatenate([[0], 2 * np.arange(1, NX - 1) + 1, [XTOTAL - 1]]).astype(np.int32)     # panel row 0 and the last one included
RUNS_DIMS = (32, 4, 4)      # the grid handed to grid_formats.runs for its order of the runs (only a grouping)


def _cycle(pattern, n):
    return [pattern[i % len(pattern)] for i in range(n)]


def _fill(pattern, total):
    """entries per panel row from `pattern` in turn until they sum to `total` (the last one cut short)"""
    out, i = [], 0
    while sum(out) < total:
        out.append(min(pattern[i % len(pattern)], total - sum(out)))
        i += 1
    return out


class RunsCase:
    """runs: per run of 16 matrix rows the entries of its distinct panel rows in turn (a list of counts 1..16: len = nd, sum = ne);
    M: matrix rows (the last run may be partial); order: 'none' (run_order NULL), 'perm' (a given permutation), 'dims' (the one
    grid_formats.runs builds); claims: what the case is for, name -> set of values (or True) that runs_seams must find"""

    def __init__(self, name, purpose, M, runs, order='none', **claims):
        assert len(runs) == (M + RUN_ROWS - 1) // RUN_ROWS
        self.name, self.purpose, self.M, self.runs, self.order, self.claims = name, purpose, M, runs, order, claims

    def __repr__(self):
        return self.name


ND_SEAMS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 79, 80, 81, 127, 128, 129, 200)
NE_SEAMS = (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 600)
CNT_SEAMS = (1, 2, 3, 4, 5, 7, 8, 15, 16)

RUNS_CASES = (
    RunsCase('distinct', "distinct panel rows per run around the ring of 16 and the windows of 64; a partial last run of 15 rows; "
             "19 runs: the last workgroup holds three", 18 * 16 + 15,
             [_cycle((1, 2, 1, 3, 1, 1, 4, 1, 2, 1, 5, 1), nd) for nd in ND_SEAMS] + [[1, 2, 15, 1, 3]],
             nd=set(ND_SEAMS), empty_run=True, empty_rows=True, m_mod16={15}, partial_block=True),
    RunsCase('entries', "entries per run around the entry windows of 64, every count of entries per panel row, one run of 600 entries; "
             "a last run of one row; the runs in a given order", 12 * 16 + 1,
             [_fill((4, 1, 2, 3, 5, 7, 8, 15, 16, 1, 1, 2), ne) for ne in NE_SEAMS] + [[1, 1]], order='perm',
             ne=set(NE_SEAMS), cnt=set(CNT_SEAMS), m_mod16={1}, partial_block=True, quad_path=True, single_path=True),
    RunsCase('windows', "panel rows of 4+ entries that start with 1, 2 and 3 entries left in the window (single path, window switch "
             "inside the row), one that starts at a window's end, a row of 16 over a window's end; a window used up after 4 requests "
             "(rows of 16: the since < 16 wait) and after 32+ (rows of 1 and 2); the order grid_formats.runs builds", 8 * 16 + 15,
             [[1] * 61 + [5] + [1] * 3, [1] * 62 + [4] + [2] * 5, [1] * 63 + [8] + [3], [1] * 64 + [4] + [1], [1] * 58 + [16] + [7],
              [16] * 14, [1, 2] * 65, [2] * 40 + [1] * 50, [15, 1, 7]], order='dims',
             left_at_row_of_4={1, 2, 3}, row_at_window_end=True, switch_inside_row=True, since_lt_16=True, since_ge_16=True,
             m_mod16={15}, partial_block=True),
    RunsCase('m1', "one matrix row", 1, [[1] * 5], m={1}),
    RunsCase('m15', "15 matrix rows", 15, [[15, 1, 4, 2]], m={15}),
    RunsCase('m16', "16 matrix rows: one whole run", 16, [[16, 1, 4]], m={16}),
    RunsCase('m17', "17 matrix rows: a run and a row", 17, [[3, 16, 1], [1, 1]], m={17}),
    RunsCase('empty', "an empty matrix of 33 rows", 33, [[], [], []], nnz={0}, empty_run=True),
)
RUNS_BY_NAME = {c.name: c for c in RUNS_CASES}
RUNS_ROUNDING = 'windows'


class Data:
    pass


@functools.lru_cache(maxsize=None)
def runs_data(case, exact=True, real=False):
    """The arrays of a forward case.  A: scipy CSR (M x NX) over the compact columns; X (XTOTAL, 64): the caller's panel, of which the
    rows TOUCHED are the ones the columns mean; Y0 (M, 64); fmt: grid_formats.runs' dict (its order replaced by a given permutation for 'perm').
    Run r puts its distinct panel rows on consecutive columns from 0 (even r) or up to the last one (odd r); column j of a run with
    c entries holds them in the rows (3 j + 0 .. c - 1) mod (rows of the run)."""
    from indigo_amd import grid_formats
    rng = np.random.default_rng(4100 + RUNS_CASES.index(case))
    draw = exact_values if exact else rounding_values
    rows, cols = [], []
    for r, cnts in enumerate(case.runs):
        R = min(RUN_ROWS, case.M - RUN_ROWS * r)
        nd = len(cnts)
        assert nd <= NX
        o = 0 if r % 2 == 0 else NX - nd
        for j, c in enumerate(cnts):
            assert 1 <= c <= R, (case, r, j, c, R)
            rows.append(RUN_ROWS * r + (3 * j + np.arange(c)) % R)
            cols.append(np.full(c, o + j))
    rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, np.int64)
    A = spp.csr_matrix((draw(rng, rows.size, real=real), (rows, cols)), shape=(case.M, NX))
    A.sort_indices()
    D = Data()
    D.case, D.M, D.real = case, case.M, real
    D.A = A
    D.X = draw(rng, XTOTAL * 64).reshape(XTOTAL, 64)
    D.Y0 = draw(rng, case.M * 64).reshape(case.M, 64)
    D.indptr = A.indptr.astype(np.int32)
    fmt = grid_formats.runs(D.indptr, A.indices, A.data, TOUCHED, RUNS_DIMS if case.order == 'dims' else None)
    assert fmt is not None
    nruns = len(case.runs)
    if case.order == 'perm':
        fmt['order'] = ((5 * np.arange(nruns) + 3) % nruns).astype(np.int32)          # (5 and the run counts used are coprime)
        assert np.array_equal(np.sort(fmt['order']), np.arange(nruns))
    D.fmt = fmt
    return D


def forward_reference(D, alpha, beta):
    res = cf32(alpha) * (D.A.astype(C128) @ D.X[TOUCHED].astype(C128))
    b = cf32(beta)
    return res if b == 0 else res + b * D.Y0.astype(C128)


def forward_bound(D, alpha, beta):
    """(n + 4) 2^-23 (|alpha|_1 (|A|_1 |X|_1) + |beta|_1 |Y0|_1) per element, n the nonzeros of its row: the form of
    spmm64.gather_bound (n complex multiply-adds in float32 in any order, fused or not, alpha and beta on top)"""
    A1 = spp.csr_matrix((l1(D.A.data.astype(C128)), D.A.indices, D.A.indptr), shape=D.A.shape)
    w = (np.diff(D.A.indptr.astype(np.int64))[:, None] + 4) * 2.0 ** -23
    return w * (l1(cf32(alpha)) * (A1 @ l1(D.X[TOUCHED].astype(C128))) + l1(cf32(beta)) * l1(D.Y0.astype(C128)))


def runs_walk(fmt, indptr, M):
    """The run format read as k_csrmm_runs64r reads it, without the arithmetic: yields (run, j, col, cnt, e_first) per distinct panel
    row j of every run -- col its compact column, cnt its entries, e_first the ordinal of its first entry inside the run"""
    dptr, dcols = fmt['dptr'], fmt['dcols']
    for run in range((M + RUN_ROWS - 1) // RUN_ROWS):
        d0, nd = int(dptr[run]), int(dptr[run + 1] - dptr[run])
        e = 0
        for j in range(nd):
            w = int(dcols[d0 + j])
            yield run, j, w & ((1 << COL_BITS) - 1), (w >> COL_BITS) + 1, e
            e += (w >> COL_BITS) + 1


def runs_to_csr(fmt, indptr, M, K):
    """regroup dcols / entries into the CSR they came from"""
    ent = fmt['entries'].reshape(-1, 3)
    rows, cols, vals = [], [], []
    for run, j, col, cnt, e in runs_walk(fmt, indptr, M):
        e0 = int(indptr[run * RUN_ROWS])
        for q in range(cnt):
            rec = ent[e0 + e + q]
            rows.append(run * RUN_ROWS + int(rec[0])); cols.append(col)
            vals.append(complex(rec[1:2].view(np.float32)[0], rec[2:3].view(np.float32)[0]))
    B = spp.csr_matrix((np.asarray(vals, dtype=C64), (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))), shape=(M, K))
    B.sort_indices()
    return B


def runs_feeders(fmt, indptr, M):
    """matrix row -> [(run, panel-row ordinal, entry ordinal inside the run)] of the entries that add into it"""
    ent = fmt['entries'].reshape(-1, 3)
    out = {}
    for run, j, col, cnt, e in runs_walk(fmt, indptr, M):
        e0 = int(indptr[run * RUN_ROWS])
        for q in range(cnt):
            out.setdefault(run * RUN_ROWS + int(ent[e0 + e + q, 0]), []).append((run, j, e + q))
    return out


def emulate_runs(D, real=None):
    """k_csrmm_runs64r in float32, reading dptr / dcols / entries: the windows of 64 distinct rows and 64 entries with their
    prefetched successors, the ring of 16 panel rows (a request past the run's end fetches panel row 0), quads while the panel row
    and the window both hold four more entries, single entries otherwise, the result rows named by the entry's low four bits.
    -> (acc (M, 64) complex64: what alpha multiplies, seams: what the walk met, see runs_seams).  real: REALW (default: all_real)"""
    fmt, indptr, M = D.fmt, D.indptr, D.M
    realw = bool(fmt['all_real']) if real is None else real
    Xp = D.X[TOUCHED]                                              # the repacked panel
    xre, xim = np.ascontiguousarray(Xp.real, dtype=np.float32), np.ascontiguousarray(Xp.imag, dtype=np.float32)
    dptr, dcols, ent = fmt['dptr'], fmt['dcols'], fmt['entries'].reshape(-1, 3)
    eflt = ent.view(np.float32)
    nruns = (M + RUN_ROWS - 1) // RUN_ROWS
    order = fmt['order'] if fmt['order'] is not None else np.arange(nruns)
    acc = np.zeros((M, 64), dtype=C64)
    seams = dict(since_lt_16=0, since_ge_16=0, quads=0, singles=0, switch_inside_row=0, tail_requests=0)
    for slot in range(nruns):
        run = int(order[slot])
        d0, nd = int(dptr[run]), int(dptr[run + 1] - dptr[run])
        rlo, rhi = run * RUN_ROWS, min(run * RUN_ROWS + RUN_ROWS, M)
        e0, ne = int(indptr[rlo]), int(indptr[rhi] - indptr[rlo])

        def rows_window(base):
            return [int(dcols[d0 + base + l]) if base + l < nd else 0 for l in range(WINDOW)]

        def entries_window(base):
            return [e0 + base + l if base + l < ne else -1 for l in range(WINDOW)]          # -1: out of range, reads as zeros

        are, aim = np.zeros((RUN_ROWS, 64), dtype=np.float32), np.zeros((RUN_ROWS, 64), dtype=np.float32)
        st = dict(dbase=0, ebase=0, dv=rows_window(0), ev=entries_window(0), pe=entries_window(WINDOW), pd=rows_window(WINDOW), ei=0, since=0)
        ring = [None] * RING

        def request(k, j):
            w = st['dv'][(j - st['dbase']) & 63]
            ring[k] = (w & ((1 << COL_BITS) - 1)) if j < nd else 0
            seams['tail_requests'] += j >= nd
            st['since'] += 1
            return w

        def mac(k, idx):
            assert idx >= 0, "an entry past the run's end was consumed"
            row = int(ent[idx, 0]) & 15
            wr, wi = eflt[idx, 1], eflt[idx, 2]
            xr, xi = xre[ring[k]], xim[ring[k]]
            are[row] = are[row] + wr * xr
            aim[row] = aim[row] + wr * xi
            if not realw:
                are[row] = are[row] - wi * xi
                aim[row] = aim[row] + wi * xr

        def consume(k, w, j):
            if j >= nd:
                return
            cnt, first = (w >> COL_BITS) + 1, True
            while cnt > 0:
                if st['ei'] >= WINDOW:
                    seams['since_lt_16' if st['since'] < 16 else 'since_ge_16'] += 1
                    seams['switch_inside_row'] += not first
                    st['ev'] = st['pe']; st['ebase'] += WINDOW; st['ei'] = 0
                    st['pe'] = entries_window(st['ebase'] + WINDOW)
                    st['since'] = 0
                first = False
                if cnt >= 4 and WINDOW - st['ei'] >= 4:
                    for q in range(4):
                        mac(k, st['ev'][st['ei'] + q])
                    st['ei'] += 4; cnt -= 4; seams['quads'] += 1
                else:
                    mac(k, st['ev'][st['ei']])
                    st['ei'] += 1; cnt -= 1; seams['singles'] += 1

        wr_ = [request(k, k) for k in range(RING)]
        for d in range(0, nd, RING):
            dn = d + RING
            move = dn < nd and ((dn - st['dbase']) & 63) == 0
            for k in range(RING):
                consume(k, wr_[k], d + k)
                if k == 0 and move:
                    st['dv'] = st['pd']; st['dbase'] = dn
                    st['pd'] = rows_window(dn + WINDOW)
                wr_[k] = request(k, dn + k)
        assert are.dtype == np.float32
        acc[rlo:rhi] = (are + 1j * aim)[:rhi - rlo]
        assert not np.any(are[rhi - rlo:]) and not np.any(aim[rhi - rlo:]), "an entry named a row past the matrix"
    return acc, seams


def runs_seams(D):
    """what a forward case holds, read from the run format: name -> set (or count)"""
    fmt, indptr, M = D.fmt, D.indptr, D.M
    nruns = (M + RUN_ROWS - 1) // RUN_ROWS
    s = dict(nd=set(int(v) for v in np.diff(fmt['dptr'])), ne=set(int(indptr[min(M, 16 * r + 16)] - indptr[16 * r]) for r in range(nruns)),
             cnt=set(), left_at_row_of_4=set(), row_at_window_end=False, m={M}, m_mod16={M % 16}, nnz={int(indptr[-1])},
             empty_run=bool(np.any(np.diff(fmt['dptr']) == 0)), empty_rows=bool(np.any(np.diff(indptr) == 0)), partial_block=nruns % 4 != 0)
    for run, j, col, cnt, e in runs_walk(fmt, indptr, M):
        s['cnt'].add(cnt)
        if cnt >= 4:
            s['left_at_row_of_4'].add(WINDOW - e % WINDOW)
        if e > 0 and e % WINDOW == 0:
            s['row_at_window_end'] = True
    em = emulate_runs(D)[1]
    s.update(since_lt_16=em['since_lt_16'] > 0, since_ge_16=em['since_ge_16'] > 0, quad_path=em['quads'] > 0, single_path=em['singles'] > 0,
             switch_inside_row=em['switch_inside_row'] > 0)
    return s


# =========================================================================================================================================
# the adjoint by wide bricks
# =========================================================================================================================================
class WideCase:
    """dims: the grid (n0 fastest, nm, ns), None: no grid (16 consecutive rows per brick, k_bricks_wide64) with K columns;
    shape: (bm, bs); task: wide_task_shape (chunk, run);
    bricks: [(brick id, entries, flags)] the DIRECT part -- rows that each hold one share of one brick, `entries` the brick's padded
    entry count; samples: [(kx, km, ks, tx, tm, ts)] the FOOTPRINT part -- rows with tx x tm x ts taps from (kx, km, ks), wrapped;
    claims: what the case is for, name -> set of values (or True) that wide_seams must find"""

    def __init__(self, name, purpose, dims, shape, task, bricks=(), samples=(), K=None, direct_rows=160, **claims):
        self.name, self.purpose, self.dims, self.shape, self.task = name, purpose, dims, shape, task
        self.bricks, self.samples, self.direct_rows, self.claims = tuple(bricks), tuple(samples), direct_rows if bricks else 0, claims
        self.K = int(np.prod(dims)) if dims is not None else K
        self.NT = shape[0] * shape[1]

    def __repr__(self):
        return self.name


def _seq(groups, seps):
    """bricks 0, 1, 2 ... : the light bricks of groups[0], a heavy brick seps[0], the bricks of groups[1], ...: with a run length
    beyond the matrix every group between two heavy bricks is ONE task"""
    out, b = [], 0
    for i, g in enumerate(groups):
        for n in g:
            out.append((b, n, '')); b += 1
        if i < len(seps):
            n, flag = seps[i] if isinstance(seps[i], tuple) else (seps[i], '')
            out.append((b, n, flag)); b += 1
    return out


NENT_SEAMS = (4, 8, 40, 44, 48, 52, 92, 96, 100, 144, 148, 192, 196, 240, 292)
_GROUPS = ([4], [4, 4], [12, 12, 16], [44], [48], [48, 4], [44, 48], [48, 48], [20, 32, 48], [48, 48, 48], [40, 8, 48, 48, 4], [48] * 4,
           [24, 28, 48, 48, 48], [48] * 5, [44, 48, 48, 8, 48, 48, 48])
assert tuple(sum(g) for g in _GROUPS) == NENT_SEAMS
_SEPS = (52, 56, 88, 92, 100, 148, (200, 'tile0'), 60, 64, 68, 72, 76, 196, 80)
_SEAM_BRICKS = _seq(_GROUPS + ([16],), _SEPS + (84,))           # (one more heavy brick and a last light one: 55 tasks, the last workgroup holds three)
PLAIN_NENT = (1, 2, 3, 4, 5, 11, 12, 13, 24, 25)
_PLAIN_GROUPS = ([1], [2], [1, 2], [4], [2, 3], [11], [5, 7], [13], [8] * 3, [12, 13], [1] * 70)
_PLAIN_SEPS = (27, 29, 30, 31, 38, 39, 50, 51, 26, 52)


def _samples(dims, n):
    """n footprints: 3 or 4 taps per axis (27, 36, 48 and 64 per row where the axis holds four points), starting near the far edge
    of every axis so that they wrap all three"""
    n0, nm, ns = dims
    taps = ((3, 3, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4))
    return [((n0 - 4 + (3 * i) % 9) % n0, (nm - 1 + i) % nm, (ns - 2 + i // 2) % ns) + tuple(min(t, d) for t, d in zip(taps[i % 4], dims))
            for i in range(n)]


def _seam_case(shape, tag):
    dims = (32, 4, 32)
    return WideCase('seams-' + tag, "task lengths around the look-ahead of 11 quads, the trips of 48 entries, the two preloaded trips and "
                    "the t + 4 reloads, as owned runs of 1 to 7 bricks between heavy bricks cut into shared pieces of 48; brick boundaries "
                    "at quad 0, at quad 11 and inside a trip; a heavy brick whose first pieces touch tile 0 only; untouched bricks",
                    dims, shape, (48, 1 << 20), bricks=_SEAM_BRICKS,
                    nent=set(NENT_SEAMS), nquad={10, 11, 12}, boundary_quad={0, 11, 5}, bricks_per_task={1, 2, 3, 7}, shared=True, owned=True,
                    skipped_tile=True, split_over_workgroups=True, tasks_mod4=True, untouched_tiles=True, pad={0, 1, 2, 3})


WIDE_CASES = (
    _seam_case((2, 1), '2x1'), _seam_case((1, 2), '1x2'), _seam_case((2, 2), '2x2'),
    WideCase('cap-2x1', "a run of 70 light bricks: tasks of 64 (the cap) and 6 bricks; shared pieces of 240 entries; K = 4608: a partial "
             "last block of 4096 rows", (64, 2, 36), (2, 1), (240, 1 << 20),
             bricks=_seq([[4] * 70, []], [244, (488, 'tile0')]), bricks_per_task={64, 6}, nent={256, 24, 240, 4, 8}, shared=True, owned=True,
             partial_zero_block=True, skipped_tile=True),
    WideCase('cap-2x2', "the same for bricks of four tiles", (64, 2, 36), (2, 2), (240, 1 << 20),
             bricks=_seq([[4] * 70, []], [244, (488, 'tile0')]), bricks_per_task={64, 6}, nent={256, 24, 240, 4, 8}, shared=True, owned=True,
             partial_zero_block=True, skipped_tile=True),
    WideCase('taps-2x2', "footprints of 27, 36, 48 and 64 taps that wrap all three grid edges; wide_task_shape (4, 4): every brick is cut "
             "into pieces of one quad", (32, 4, 4), (2, 2), (4, 4), samples=_samples((32, 4, 4), 40),
             taps={27, 36, 48, 64}, wraps=True, nent={4}, shared=True, pad={0, 1, 2, 3}),
    WideCase('taps-2x1', "footprints on 48 x 2 x 4, bricks 2 x 1, owned runs beside shared pieces", (48, 2, 4), (2, 1), (160, 64),
             samples=_samples((48, 2, 4), 40), wraps=True, shared=True, owned=True, untouched_tiles=True),
    WideCase('taps-1x2', "footprints on 48 x 2 x 4, bricks 1 x 2", (48, 2, 4), (1, 2), (160, 48),
             samples=_samples((48, 2, 4), 40), wraps=True, shared=True, owned=True, untouched_tiles=True),
    WideCase('one-brick', "16 x 2 x 2: the whole grid is one brick of four tiles, K = 64", (16, 2, 2), (2, 2), (16, 16),
             samples=_samples((16, 2, 2), 12), shared=True),
    WideCase('plain', "k_bricks_wide64: task lengths around the group of four and the rotation of three groups, tasks of 1, 2 and 64 "
             "bricks, shared pieces of 24 and less", None, (1, 1), (24, 1 << 20), K=16 * 100, bricks=_seq(_PLAIN_GROUPS, _PLAIN_SEPS),
             nent=set(PLAIN_NENT), bricks_per_task={1, 2, 64}, shared=True, owned=True, untouched_tiles=True),
)
WIDE_BY_NAME = {c.name: c for c in WIDE_CASES}
WIDE_ROUNDING = ('seams-2x1', 'seams-2x2', 'plain')           # (real and complex each)
_SHARE_PATTERN = (4, 3, 4, 8, 4, 2, 4, 7, 1, 4, 4, 4, 6, 4)  # nonzeros per (row, brick) share: padding of 0 .. 3 entries per quad


def brick_origin(case, b):
    """(kx, km, ks) of the first point of brick b"""
    if case.dims is None:
        return 16 * b, 0, 0
    n0, nm, ns = case.dims
    bm, bs = case.shape
    nbx, nbm = n0 // 16, nm // bm
    return 16 * (b % nbx), bm * ((b // nbx) % nbm), bs * (b // (nbx * nbm))


@functools.lru_cache(maxsize=None)
def wide_data(case, exact=True, real=False):
    """The arrays of an adjoint case.  A: scipy CSR (M x K); X (M, 64); fmt: grid_formats.wide_bricks' dict."""
    from indigo_amd import grid_formats
    rng = np.random.default_rng(5200 + WIDE_CASES.index(case))
    draw = exact_values if exact else rounding_values
    n0, nm, ns = case.dims if case.dims is not None else (case.K, 1, 1)
    bm, bs = case.shape
    unit = 4 if case.NT > 1 else 1
    cells = 16 * case.NT
    rows, cols = [], []
    cursor, k = 0, 0
    for b, nent, flag in case.bricks:
        assert nent % unit == 0
        kx0, km0, ks0 = brick_origin(case, b)
        left, i = nent, 0
        assert (nent + unit - 1) // unit <= case.direct_rows
        while left > 0:
            s = _SHARE_PATTERN[k % len(_SHARE_PATTERN)] if unit == 4 else (1, 2, 1, 3, 1, 1)[k % 6]
            k += 1
            if (s + unit - 1) // unit * unit > left:
                s = min(left, 4)
            # the share's cells: distinct (an odd step through a power of two); 'tile0': all but the last two shares stay inside tile 0
            tile0 = flag == 'tile0' and left > 2 * unit + 4
            c = ((5 * k + 7 * np.arange(s)) % (16 if tile0 else cells)).astype(np.int64)
            x, im, is_ = c % 16, (c // 16) % bm, c // (16 * bm)
            rows.append(np.full(s, (cursor + i) % case.direct_rows)); cols.append(kx0 + x + n0 * ((km0 + im) + nm * (ks0 + is_)))
            left -= (s + unit - 1) // unit * unit
            i += 1
        cursor += i
    for t, (kx, km, ks, tx, tm, ts) in enumerate(case.samples):
        ax = [(kx + np.arange(tx)) % n0, (km + np.arange(tm)) % nm, (ks + np.arange(ts)) % ns]
        c = (ax[0][None, None, :] + n0 * (ax[1][None, :, None] + nm * ax[2][:, None, None])).reshape(-1)
        assert np.unique(c).size == c.size
        rows.append(np.full(c.size, case.direct_rows + t)); cols.append(c)
    rows, cols = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    M = case.direct_rows + len(case.samples)
    A = spp.csr_matrix((draw(rng, rows.size, real=real), (rows, cols)), shape=(M, case.K))
    assert A.nnz == rows.size, "a row holds a column twice"
    A.sort_indices()
    D = Data()
    D.case, D.M, D.K, D.real, D.A = case, M, case.K, real, A
    D.X = draw(rng, M * 64).reshape(M, 64)
    D.fmt = grid_formats.wide_bricks(A.indptr, A.indices, A.data, case.K, case.dims, case.shape, case.task, real_entries=real)
    return D


def adjoint_reference(D, alpha):
    return cf32(alpha) * (D.A.astype(C128).conj().T @ D.X.astype(C128))


def wide_tasks(fmt):
    """(tasks (n, 4) [lo, hi, first table row, bricks | shared << 16], table (nb, 2) [brick, end of its entries])"""
    n = fmt['ntasks']
    return fmt['tasks'].reshape(-1, 4)[:n], (fmt['table'].reshape(-1, 2) if n else np.zeros((0, 2), np.int32))


def tile_rows(geom, K, b, q):
    """first row of Y of tile q of brick b: my_row0 and tile_out's row offset"""
    n0, nm, bm, bs = geom
    if bm * bs == 1:
        return 16 * b
    nbx, nbm = n0 // 16, nm // bm
    bx, bmi, bsi = b % nbx, (b // nbx) % nbm, b // (nbx * nbm)
    bml, bsl = bm.bit_length() - 1, bs.bit_length() - 1
    row00 = bx * 16 + n0 * ((bmi << bml) + nm * (bsi << bsl))
    return row00 + n0 * ((q & ((1 << bml) - 1)) + nm * (q >> bml))


def adjoint_pieces(D):
    """per row of Y: the shared pieces that add into its brick (0 for the rows of owned and of untouched bricks)"""
    fmt = D.fmt
    tasks, table = wide_tasks(fmt)
    NT = fmt['geom'][2] * fmt['geom'][3]
    p = np.zeros(D.K, dtype=np.int64)
    for lo, hi, bt, nbf in tasks:
        if nbf >> 16:
            for q in range(NT):
                r0 = tile_rows(fmt['geom'], D.K, int(table[bt, 0]), q)
                p[r0:r0 + 16] += 1
    return p


def adjoint_bound(D, alpha):
    """(n + p + 4) 2^-23 |alpha|_1 (|A|_1^T |X|_1) per element: n the nonzeros of its column of A, p the pieces whose float atomics
    add into its brick (one rounding each)"""
    A1 = spp.csr_matrix((l1(D.A.data.astype(C128)), D.A.indices, D.A.indptr), shape=D.A.shape)
    n = np.bincount(D.A.indices, minlength=D.K)
    w = ((n + adjoint_pieces(D) + 4) * 2.0 ** -23)[:, None]
    return w * l1(cf32(alpha)) * (A1.T @ l1(D.X.astype(C128)))


def emulate_wide(D, alpha, y_aligned=True, ldy_even=True, events=None):
    """ig_ccsrmm_t_bricks_wide_grid in float32, reading owned / tasks / table / entries / rows: Y (a sentinel everywhere) is zeroed
    where the bitmap names no owner (everywhere when Y is not 16-byte aligned or ldy is odd), then every task walks its quads (its
    single entries for 16-row bricks) trip by trip, flushes the brick image when the entry offset reaches the brick's end and once
    more at the task's end -- tile by tile at my_row0 + n0 ((q & (bm - 1)) + nm (q >> log2 bm)), stored by an owner, added by a shared
    piece, which skips a tile it never touched.  events (a dict) collects the tiles skipped and stored.  -> Y (K, 64) complex64"""
    fmt, K = D.fmt, D.K
    tasks, table = wide_tasks(fmt)
    geom = fmt['geom']
    n0, nm, bm, bs = geom
    NT, words = bm * bs, fmt['words']
    unit = 4 if NT > 1 else 1
    ent = fmt['entries'].reshape(-1, words)
    eflt = ent.view(np.float32)
    qrows = fmt['rows']
    xre, xim = np.ascontiguousarray(D.X.real, dtype=np.float32), np.ascontiguousarray(D.X.imag, dtype=np.float32)
    a = cf32(alpha)
    ar, ai = np.float32(a.real), np.float32(a.imag)
    Y = np.full((K, 64), SENTINEL, dtype=C64)
    if fmt['ntasks'] > 0 and D.M > 0 and y_aligned and ldy_even:
        for r0 in range(0, K, ZERO_BLOCK):                       # k_wide_zero_unowned: a workgroup per 4096 rows, tiles past K left alone
            for t in range(r0 // 16, (r0 + ZERO_BLOCK) // 16):
                if t * 16 < K and not (int(fmt['owned'][t >> 5]) >> (t & 31)) & 1:
                    Y[16 * t:16 * t + 16] = 0
    else:
        Y[:] = 0
    ev = events if events is not None else {}
    ev.update(skipped=0, stored=[], flush_quads=[])
    for ti, (lo, hi, bt, nbf) in enumerate(tasks):
        lo, hi, bt = int(lo), int(hi), int(bt)
        nb, shared = int(nbf) & 0xffff, bool((int(nbf) >> 16) & 1)
        nent = hi - lo
        assert nent % unit == 0 and 1 <= nb <= MAX_BRICKS
        my_end = [int(table[bt + l, 1]) - lo if (l < nb and not shared) else 0x7fffffff for l in range(64)]
        img_re, img_im = np.zeros((16 * NT, 64), dtype=np.float32), np.zeros((16 * NT, 64), dtype=np.float32)
        st = dict(cur=0, cur_end=my_end[0])

        def flush():
            b = int(table[bt + st['cur'], 0])
            for q in range(NT):
                tr, tim = img_re[16 * q:16 * q + 16], img_im[16 * q:16 * q + 16]
                if NT > 1 and shared and not (np.any(tr) or np.any(tim)):
                    ev['skipped'] += 1
                    continue
                r0 = tile_rows(geom, K, b, q)
                out = (ar * tr - ai * tim) + 1j * (ar * tim + ai * tr)
                if shared:
                    Y[r0:r0 + 16] = ((Y[r0:r0 + 16].real + out.real) + 1j * (Y[r0:r0 + 16].imag + out.imag)).astype(C64)
                else:
                    Y[r0:r0 + 16] = out.astype(C64)
                ev['stored'].append((ti, st['cur'], r0))
            img_re[:] = 0; img_im[:] = 0
            st['cur'] += 1
            st['cur_end'] = my_end[st['cur'] & 63]

        step = TRIP if NT > 1 else GROUP
        for t in range(0, nent, step):                         # a trip (a group of four for 16-row bricks)
            for base in range(t, min(t + step, nent), unit):   # a quad (an entry)
                if base >= st['cur_end']:
                    ev['flush_quads'].append((base // unit) % TQ)
                    flush()
                row = int(qrows[(lo + base) // unit])
                xr, xi = xre[row], xim[row]
                for e in range(lo + base, lo + base + unit):
                    cell = int(ent[e, 0]) & (16 * NT - 1)
                    wr = eflt[e, 1]
                    img_re[cell] = img_re[cell] + wr * xr
                    img_im[cell] = img_im[cell] + wr * xi
                    if words == 3:
                        wi = eflt[e, 2]
                        img_re[cell] = img_re[cell] + wi * xi                 # conj(v) x
                        img_im[cell] = img_im[cell] - wi * xr
        flush()
    return Y


def wide_to_csr(D):
    """regroup entries / rows / table into the CSR they came from (padding entries have weight zero; the exact values have none)"""
    fmt = D.fmt
    tasks, table = wide_tasks(fmt)
    geom = fmt['geom']
    n0, nm, bm, bs = geom
    NT, words = bm * bs, fmt['words']
    unit = 4 if NT > 1 else 1
    ent = fmt['entries'].reshape(-1, words)
    eflt = ent.view(np.float32)
    rows, cols, vals = [], [], []
    start = 0
    for b, end in table:
        for e in range(start, int(end)):
            v = complex(eflt[e, 1], eflt[e, 2] if words == 3 else 0.0)
            if v != 0:
                cell = int(ent[e, 0]) & (16 * NT - 1)
                rows.append(int(fmt['rows'][e // unit])); vals.append(v)
                cols.append(tile_rows(geom, D.K, int(b), cell >> 4) + (cell & 15))
        start = int(end)
    B = spp.csr_matrix((np.asarray(vals, dtype=C64), (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))), shape=(D.M, D.K))
    B.sort_indices()
    return B


def wide_feeders(D):
    """row of Y -> [(task, brick ordinal inside the task, quad of the task)] of the quads (entries for 16-row bricks) that add into it"""
    fmt = D.fmt
    tasks, table = wide_tasks(fmt)
    geom = fmt['geom']
    NT, words = geom[2] * geom[3], fmt['words']
    unit = 4 if NT > 1 else 1
    ent = fmt['entries'].reshape(-1, words)
    ends = table[:, 1].astype(np.int64)
    out = {}
    for ti, (lo, hi, bt, nbf) in enumerate(tasks):
        for e in range(int(lo), int(hi)):
            if not np.any(ent[e, 1:]):
                continue
            tr = int(np.searchsorted(ends, e, side='right'))                 # the table row whose entries hold e
            cell = int(ent[e, 0]) & (16 * NT - 1)
            r = tile_rows(geom, D.K, int(table[tr, 0]), cell >> 4) + (cell & 15)
            rec = (ti, tr - int(bt), (e - int(lo)) // unit)
            if rec not in out.setdefault(r, []):
                out[r].append(rec)
    return out


def wide_seams(D):
    """what an adjoint case holds, read from the wide-brick format: name -> set (or bool)"""
    fmt, case = D.fmt, D.case
    tasks, table = wide_tasks(fmt)
    NT, words = fmt['geom'][2] * fmt['geom'][3], fmt['words']
    unit = 4 if NT > 1 else 1
    nent = tasks[:, 1] - tasks[:, 0]
    shared = (tasks[:, 3] >> 16) & 1
    s = dict(nent=set(int(v) for v in nent), nquad=set(int(v) // unit for v in nent), bricks_per_task=set(int(v) & 0xffff for v in tasks[:, 3]),
             shared=bool(shared.any()), owned=bool((shared == 0).any()), tasks_mod4=tasks.shape[0] % 4 != 0, boundary_quad=set(), pad=set(),
             taps=set(int(v) for v in np.diff(D.A.indptr)[case.direct_rows:]), partial_zero_block=D.K % ZERO_BLOCK != 0)
    for lo, hi, bt, nbf in tasks:
        if not nbf >> 16:
            for i in range((nbf & 0xffff) - 1):
                s['boundary_quad'].add(int(table[bt + i, 1] - lo) // unit % TQ)
    # a brick whose pieces run in different workgroups (four tasks each)
    wg = {}
    for ti, (lo, hi, bt, nbf) in enumerate(tasks):
        if nbf >> 16:
            wg.setdefault(int(bt), set()).add(ti // 4)
    s['split_over_workgroups'] = any(len(v) > 1 for v in wg.values())
    if unit == 4:
        ent = fmt['entries'].reshape(-1, words)[:int(table[-1, 1]) if table.size else 0]
        s['pad'] = set(int(v) for v in (~np.any(ent[:, 1:] != 0, axis=1)).reshape(-1, 4).sum(axis=1))
    ev = {}
    emulate_wide(D, ALPHA, events=ev)
    s['skipped_tile'] = ev['skipped'] > 0
    touched = np.zeros(D.K // 16, dtype=bool)
    touched[np.unique(D.A.indices) // 16] = True
    s['untouched_tiles'] = bool((~touched).any())
    if case.dims is not None:
        n0, nm, ns = case.dims
        c = D.A.indices
        kx, km, ks = c % n0, (c // n0) % nm, c // (n0 * nm)
        r = np.repeat(np.arange(D.M), np.diff(D.A.indptr))
        sample = np.arange(D.M) >= case.direct_rows
        wrap = lambda v, n: np.any(np.bincount(r[v == 0], minlength=D.M).astype(bool) & np.bincount(r[v == n - 1], minlength=D.M).astype(bool) & sample)
        s['wraps'] = bool(wrap(kx, n0) and wrap(km, nm) and wrap(ks, ns))
    return s


def owned_bits(D):
    return np.unpackbits(D.fmt['owned'].view(np.uint8), bitorder='little')[:D.K // 16].astype(bool)
