"""A float64 restatement of the two products of the separable gridding kernels (indigo_amd/csrc/ig_gridsep.hip: k_grid_gather_sep,
k_grid_scatter_mfma), straight from the records; hand-built records with any tap counts, first taps and weights; a Python mirror
of the launch geometry; and the tables of cases built through that mirror.  Plain numpy / scipy and the library's HOST routines
(the share format): nothing here needs a GPU.

Reference (tap_matrix): for sample t the first taps (j0, j1, j2) and counts (c0, c1, c2) come from words 3 tw and 3 tw + 1 of its
record; tap (a < c0, b < c1, c < c2) sits at cell (j0 + a) % n0 + n0 * ((j1 + b) % nm + nm * ((j2 + c) % ns)) with the weight
w0[a] * w1[b] * w2[c], formed in float64 from the float32 words.  Forward Y[t, k] = alpha sum w X[cell, k] + beta Y0[t, k] (beta == 0
does not read Y0), adjoint Yg[cell, k] = alpha sum_{t, tap -> cell} w X[t, k]; alpha and beta with float32 parts, as the ABI takes
them.  Nothing of interp.sep_expand or of the CSR builder is used (tests/test_gridsep64_cpu.py compares with both).

Exact inputs: weights inside the counts from {+-1, +-2}, panel parts NONZERO INTEGERS in [-4, 4], alpha = 0.5 - 0.25j,
beta = -0.5 + 1.5j.  A tap's weight is an integer of magnitude <= 8 and it contributes at most 8 * 4 = 32 to a part of a sum (64 is
what the checks below allow).  Forward: a sample of 8^3 taps keeps every partial sum, in any order and grouping, an integer of at most
64 * 512 = 2^15.  Adjoint: a sample meets a cell at most once (counts never exceed the axis), so a cell is hit by at most M <= 4096
samples and its partial sums are integers below 64 * 4096 = 2^18.  Times alpha every value is a multiple of 1/4 below 2^20 -- 22
significant bits -- and beta y is a multiple of 1/2 below 16: float32 (24 bits) holds every intermediate and every result.  No kernel
may round anything on these inputs, through the matrix cores and the float atomics alike, so the device must give the float64 sum
EXACTLY, element by element (test_gridsep64_cpu.py asserts the bound per case and emulates the sums in float32).

Rounding inputs: records from interp_sep_records on a SenseProblem.synthetic trajectory with samples pushed onto faces, corners and
grid points, panels of uniform random parts.  Per element the classical worst case  (n + c) 2^-23 |alpha|_1 sum |w| |x|_1  (+ the
same factor on |beta|_1 |y0|_1) with n the taps summed into the element (one rounding per addition a term passes through, in ANY
order; unit roundoff 2^-24, so 2^-23 per operation is generous by two and swallows the second-order terms) and c the roundings
outside the sum, counted from the kernels:
  gather   (w0 * w2) * w1: 2; the multiply of the fma is exact, its addition is one of the n; the shuffle adds across the x-tap
           lanes: log2(XL) <= 3; alpha: a product and an fma per part: 2; beta: two fmas per part: 2.                    c = 9
  scatter  wm * x: 1; * ws: 1; the MFMA's multiply: 1 (its addition is one of the n); the alpha fma and the product inside it: 2;
           and one more addition per piece of a shared brick (float atomics, any order).                       c = 5 + pieces
Zero-weight padding (a lane re-reading its sample's last tap) adds an exact zero."""
import collections
import functools

import numpy as np
import scipy.sparse as spp

from spmm64 import ALPHA, BETA, C64, C128, cf32          # noqa: F401  (the dyadic scalars of the CSR family)

VMAX = 4
WVALS = np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32)
NAN32 = 0x7fc0dead

# ---- the constants of ig_gridsep.hip the mirror is built on (test_gridsep64_cpu.py reads them out of the source) --------------------
BLK = 256
WPB = BLK // 64
G, R = 4, 16                # k_grid_scatter_mfma: shares per group, ring slots
HDR = 64                    # share headers per batch
MAX_BRICKS = 64             # bricks per task


def sep_words(tw):
    return 16 if tw == 4 else 32


def gather_geometry(NC, tw):
    """(QL, XL, SPW, group, CG) of k_grid_gather_sep<NC, tw>: lanes per 16-byte piece of a grid point, x-tap lanes, samples per wave,
    samples per workgroup, slow-axis rows in flight together"""
    QL, XL = NC // 2, 4 if tw <= 4 else 8
    SPW = 64 // (QL * XL)
    return QL, XL, SPW, WPB * SPW, 4 if tw <= 4 else 2


# =========================================================================================================================================
# records
# =========================================================================================================================================
def make_records(tw, dims, j, cnt, rng, exact=True):
    """(M, ig_interp3_sep_words(tw)) uint32 records with first taps j (M, 3) and tap counts cnt (M, 3) on the grid `dims`: weights
    inside the counts from {+-1, +-2} (exact) or uniform in +-[0.25, 1); weights past an axis' count are 0, every word from
    3 tw + 2 on is 0, counts are >= 1 (the format's invariants, ig_interp.hip)"""
    j, cnt = np.asarray(j, dtype=np.int64).reshape(-1, 3), np.asarray(cnt, dtype=np.int64).reshape(-1, 3)
    M = j.shape[0]
    assert cnt.shape[0] == M and (cnt >= 1).all() and (cnt <= tw).all() and (j >= 0).all() and (j < np.asarray(dims)).all()
    assert all(n >= tw for n in dims)
    w = WVALS[rng.integers(0, 4, size=(M, 3, tw))] if exact else \
        (rng.uniform(0.25, 1.0, size=(M, 3, tw)) * rng.choice([-1.0, 1.0], size=(M, 3, tw))).astype(np.float32)
    w = np.where(np.arange(tw)[None, None, :] < cnt[:, :, None], w, np.float32(0)).astype(np.float32)
    rec = np.zeros((M, sep_words(tw)), dtype=np.uint32)
    rec[:, :3 * tw] = w.reshape(M, 3 * tw).view(np.uint32)
    rec[:, 3 * tw] = (j[:, 0] | (j[:, 1] << 16)).astype(np.uint32)
    rec[:, 3 * tw + 1] = (j[:, 2] | (cnt[:, 0] << 16) | (cnt[:, 1] << 20) | (cnt[:, 2] << 24)).astype(np.uint32)
    return rec


def unpack(rec, tw):
    """-> first taps (M, 3), counts (M, 3), weights (M, 3, tw) float32"""
    h0, h1 = rec[:, 3 * tw].astype(np.int64), rec[:, 3 * tw + 1].astype(np.int64)
    j = np.stack([h0 & 0xffff, h0 >> 16, h1 & 0xffff], axis=1)
    cnt = np.stack([(h1 >> 16) & 15, (h1 >> 20) & 15, (h1 >> 24) & 15], axis=1)
    return j, cnt, np.ascontiguousarray(rec[:, :3 * tw]).view(np.float32).reshape(-1, 3, tw)


def taps(rec, tw, dims):
    """(sample, cell, weight in float64) of every tap of every record, sample by sample"""
    n0, nm, ns = dims
    j, cnt, w = unpack(rec, tw)
    ts, cells, ws = [], [], []
    for c in range(tw):
        for b in range(tw):
            for a in range(tw):
                t = np.flatnonzero((a < cnt[:, 0]) & (b < cnt[:, 1]) & (c < cnt[:, 2]))
                if t.size == 0:
                    continue
                ts.append(t)
                cells.append((j[t, 0] + a) % n0 + n0 * ((j[t, 1] + b) % nm + nm * ((j[t, 2] + c) % ns)))
                ws.append(w[t, 0, a].astype(np.float64) * w[t, 1, b].astype(np.float64) * w[t, 2, c].astype(np.float64))
    if not ts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(ts), np.concatenate(cells), np.concatenate(ws)


def tap_matrix(rec, tw, dims):
    """the (M, n0 nm ns) float64 matrix the records describe (scipy only sums: a sample never meets a cell twice)"""
    t, cell, w = taps(rec, tw, dims)
    return spp.csr_matrix((w, (t, cell)), shape=(rec.shape[0], int(np.prod(dims))))


def forward_reference(A, X, Y0, alpha, beta):
    a, b = cf32(alpha), cf32(beta)
    res = a * (A @ np.where(np.isnan(X), 0, X).astype(C128))
    return res if b == 0 else res + b * Y0.astype(C128)


def adjoint_reference(A, X, alpha):
    return cf32(alpha) * (A.T.tocsr() @ X.astype(C128))


def l1(z):
    return np.abs(z.real) + np.abs(z.imag)


def forward_bound(A, X, Y0, alpha, beta):
    """(n_t + 9) 2^-23 (|alpha|_1 sum |w| |x|_1 + |beta|_1 |y0|_1), n_t the taps of sample t (module docstring)"""
    a, b = cf32(alpha), cf32(beta)
    n = np.diff(A.indptr)[:, None]
    return (n + 9) * 2.0 ** -23 * (l1(a) * (abs(A) @ l1(np.where(np.isnan(X), 0, X).astype(C128))) + l1(b) * l1(Y0.astype(C128)))


def adjoint_bound(A, X, alpha, pieces):
    """(n_cell + 5 + pieces_cell) 2^-23 |alpha|_1 sum |w| |x|_1, n_cell the taps that land on the cell"""
    At = A.T.tocsr()
    n = np.diff(At.indptr)[:, None]
    return (n + 5 + np.asarray(pieces)[:, None]) * 2.0 ** -23 * l1(cf32(alpha)) * (abs(At) @ l1(X.astype(C128)))


def exact_panel(rng, shape):
    mag = rng.integers(1, VMAX + 1, size=shape + (2,)) * rng.choice([-1, 1], size=shape + (2,))
    return (mag[..., 0] + 1j * mag[..., 1]).astype(C64)


def random_panel(rng, shape):
    v = rng.uniform(0.25, 1.0, size=shape + (2,)) * rng.choice([-1.0, 1.0], size=shape + (2,))
    return (v[..., 0] + 1j * v[..., 1]).astype(C64)


def first_taps(n, c, rng):
    """first taps on an axis of n points for samples of c taps: 0, n - 1, n - c + 1 (the last tap wraps) or anywhere"""
    kind = rng.integers(0, 4, size=c.size)
    return np.select([kind == 0, kind == 1, kind == 2], [np.zeros_like(c), np.full_like(c, n - 1), (n - c + 1) % n], rng.integers(0, n, size=c.size))


def builder_records(tw, seed=4):
    """records of interp_sep_records on a synthetic radial trajectory over the 32 x 16 x 16 grid, a third of the samples pushed onto
    faces, corners and exact grid points (as tests/test_gridsep_cpu.py does) -> (problem, sep dict)"""
    from indigo_amd.sense import SenseProblem
    width = {4: 2, 6: 3, 8: 4}[tw]
    p = SenseProblem.synthetic((16, 8, 8), 2, nspokes=29, nreadout=32, width=width, oversamp=2.0, seed=seed)
    c = p.coord.reshape(3, -1, order='F').copy()
    rng = np.random.default_rng(seed)
    k = c.shape[1] // 3
    c[:, :k] = rng.choice([-0.5, -0.5 + 1.0 / p.oN[0], 0.5 - 1.0 / p.oN[0], 0.0, 0.25], size=(3, k))
    p.coord = c.reshape(p.coord.shape, order='F')
    p.drop_cache()
    return p, p.fused_interp_sep(1)


# =========================================================================================================================================
# gather cases
# =========================================================================================================================================
GCase = collections.namedtuple('GCase', 'NC tw dims M seed exact')
GatherData = collections.namedtuple('GatherData', 'case rec X Y0 A M P touched')
GCase.__repr__ = lambda c: "NC%d-tw%d-%s-M%d%s" % (c.NC, c.tw, 'x'.join(map(str, c.dims)), c.M, '' if c.exact else '-rnd')


def gather_grids(tw):
    return [(tw, tw, tw), (16, tw, tw), (20, 13, 11)]


def gather_sample_counts(NC, tw):
    """M at the seams of the launch: one sample, a wave short of one, a workgroup short of one / full / one over, 7, 8 and 9 workgroups
    (the remainders of xcd_block), about 40 workgroups for an ordered run"""
    _, _, spw, group, _ = gather_geometry(NC, tw)
    return [1, max(spw - 1, 1), group - 1, group, group + 1, 6 * group + 1, 7 * group + spw + 1, 9 * group - 1, 40 * group + 3]


def gather_counts(M, spw, tw, rng):
    """tap counts (M, 3) composed wave by wave: wave v's widest sample has 1 + v % tw taps on the slow axis (the nc2u exit); on the
    middle axis the waves cycle through 'nobody has all tw taps' (NBT = tw - 1), 'exactly one sample has' and 'any'"""
    t = np.arange(M)
    wv, slot = t // spw, t % spw
    in_wave = np.minimum(spw, M - wv * spw)
    holder = slot == (wv // tw) % in_wave
    top2 = 1 + wv % tw
    c2 = np.where(holder, top2, rng.integers(1, top2 + 1))
    kind = (wv // tw) % 3
    c1 = rng.integers(1, tw, size=M)
    c1 = np.where((kind == 1) & holder, tw, c1)
    c1 = np.where(kind == 2, rng.integers(1, tw + 1, size=M), c1)
    return np.stack([rng.integers(1, tw + 1, size=M), c1, c2], axis=1)


def _gather_table():
    out = []
    for k, (NC, tw) in enumerate((NC, tw) for NC in (2, 4, 8) for tw in (4, 6, 8)):
        grids = gather_grids(tw)
        Ms = gather_sample_counts(NC, tw)
        seen = set()
        for i, M in enumerate(Ms):
            for dims in (grids if i == len(Ms) - 1 else [grids[(i + k) % 3]]):
                if (M, dims) not in seen:
                    seen.add((M, dims))
                    out.append(GCase(NC, tw, dims, M, 100 * k + i, True))
    return out


GATHER_CASES = _gather_table()
GATHER_ROUNDING = [GCase(NC, tw, (32, 16, 16), 0, 7, False) for NC in (2, 4, 8) for tw in (4, 6, 8)]


@functools.lru_cache(maxsize=4)
def build_gather(case):
    """-> namespace(rec, X (cells, NC) with NaN in every cell no sample touches, Y0, A, M)"""
    rng = np.random.default_rng(1000 + case.seed)
    NC, tw, dims = case.NC, case.tw, case.dims
    if case.exact:
        spw = gather_geometry(NC, tw)[2]
        cnt = gather_counts(case.M, spw, tw, rng)
        j = np.stack([first_taps(dims[d], cnt[:, d], rng) for d in range(3)], axis=1)
        rec = make_records(tw, dims, j, cnt, rng, True)
        panel = exact_panel
    else:
        p, sep = builder_records(tw)
        assert tuple(sep['dims']) == dims and sep['tw'] == tw
        rec = np.ascontiguousarray(sep['records'])
        panel = random_panel
    M, P = rec.shape[0], int(np.prod(dims))
    A = tap_matrix(rec, tw, dims)
    X = panel(rng, (P, NC))
    touched = np.zeros(P, dtype=bool)
    touched[A.indices] = True
    X[~touched] = np.nan
    return GatherData(case, rec, X, panel(rng, (M, NC)), A, M, P, touched)


# =========================================================================================================================================
# scatter cases
# =========================================================================================================================================
SCase = collections.namedtuple('SCase', 'NC tw kind dims shape tile chunk run masks seed exact')
ScatterData = collections.namedtuple('ScatterData', 'case rec recx rs fmt tab tasks shared X A M P flag pieces brick_of')
SCase.__repr__ = lambda c: "NC%d-tw%d-%s-b%dx%d-t%d-c%d-r%d-%s%s" % (c.NC, c.tw, c.kind, c.shape[0], c.shape[1], c.tile, c.chunk, c.run, c.masks,
                                                                    '' if c.exact else '-rnd')

SHAPES = [(1, 1), (2, 4), (4, 2), (4, 4)]
TILES = [16, 8, 4]
LIGHT = 40                  # the designed layouts: bricks of up to LIGHT shares, cut by heavy bricks of LIGHT + 1 (chunk = LIGHT)
# groups of consecutive bricks (shares per brick) that become ONE unshared task each: the task lengths at the seams of the pipeline
# (4 shares per group, 16 ring slots, header batches of 64, two deep with a third in flight), brick boundaries at every position of a group
LAYOUT_A = [[1], [1, 1], [2, 1], [3, 1], [1, 1, 1, 1, 1], [6], [2, 2, 3], [7, 1], [3, 3, 3], [21, 21, 21], [1] * 64, [40, 25],
            [40, 40, 40, 7], [32] * 4, [40, 40, 40, 9], [38] * 5 + [1], [40] * 4 + [32], [39] * 4 + [37], [37] * 6 + [35]]
LAYOUT_B = [[1], [1, 1], [2, 1], [3, 1], [5], [6], [2, 2, 3], [7, 1], [3, 3, 3], [40, 40, 40, 9], [39] * 4 + [37], [37] * 6 + [35]]
SEAM_LENGTHS = list(range(1, 10)) + [63, 64, 65, 127, 128, 129, 191, 192, 193]
BLOB_CHUNKS = [63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 1024, 8]


def layout_counts(layout):
    out = []
    for g, grp in enumerate(layout):
        out += ([LIGHT + 1] if g else []) + list(grp)
    return out


def _scatter_table():
    out = []
    for k, (NC, tw) in enumerate((NC, tw) for NC in (4, 8) for tw in (4, 6, 8)):
        cr = [(16, 16), (64, 128), (1024, 1024), (7, 5)]
        for si, shape in enumerate(SHAPES):
            out.append(SCase(NC, tw, 'wrap', (16, tw, tw), shape, TILES[(si + k) % 3], *cr[(si + k) % 4], 'rand' if (si + k) % 2 else 'all', 10 * k + si, True))
        out.append(SCase(NC, tw, 'odd', (32, 13, 11), SHAPES[k % 4], TILES[k % 3], 32, 48, 'rand', 10 * k + 4, True))
        out.append(SCase(NC, tw, 'odd', (32, 13, 11), SHAPES[(k + 2) % 4], TILES[(k + 1) % 3], 9, 200, 'all', 10 * k + 5, True))
        out.append(SCase(NC, tw, 'blob', (32, 16, 16), (4, 4), 4, BLOB_CHUNKS[k], 100, 'rand', 10 * k + 6, True))
        out.append(SCase(NC, tw, 'blob', (32, 16, 16), SHAPES[(k + 1) % 4], TILES[(k + 2) % 3], BLOB_CHUNKS[k + 6], 37, 'all', 10 * k + 7, True))
        out.append(SCase(NC, tw, 'layoutA', (32, 16, 16), (1, 1), TILES[k % 3], LIGHT, 1 << 20, 'rand' if k % 2 else 'all', 10 * k + 8, True))
        out.append(SCase(NC, tw, 'layoutB', (32, 16, 16), [(2, 4), (4, 2)][k % 2], TILES[(k + 1) % 3], LIGHT, 1 << 20, 'all' if k % 2 else 'rand', 10 * k + 9, True))
    return out


SCATTER_CASES = _scatter_table()
SCATTER_ROUNDING = [SCase(NC, tw, 'builder', (32, 16, 16), (4, 4), 16, 64, 128, 'all', 3, False) for NC in (4, 8) for tw in (4, 6, 8)]


def _scatter_records(case, rng):
    tw, dims = case.tw, case.dims
    n = np.asarray(dims)
    if case.kind in ('wrap', 'odd'):
        M = 300 if case.kind == 'wrap' else 500
        cnt = rng.integers(1, tw + 1, size=(M, 3))
        j = np.stack([first_taps(dims[d], cnt[:, d], rng) for d in range(3)], axis=1)
    elif case.kind == 'blob':
        # about 3000 samples whose footprints meet the brick at (16.., 8.., 8..), the rest anywhere
        M = 3500
        cnt = rng.integers(1, tw + 1, size=(M, 3))
        j = np.stack([rng.integers(0, dims[d], size=M) for d in range(3)], axis=1)
        for d, (lo, ext) in enumerate(((16, 16), (8, case.shape[0]), (8, case.shape[1]))):
            j[:3000, d] = lo - cnt[:3000, d] + 1 + rng.integers(0, ext + cnt[:3000, d] - 1)       # any first tap whose footprint meets the brick
    else:
        # one share per sample: the footprint inside one brick, brick b getting counts[b] samples
        bm, bs = case.shape
        counts = layout_counts(LAYOUT_A if case.kind == 'layoutA' else LAYOUT_B)
        nbx, nbm, nbs = dims[0] // 16, dims[1] // bm, dims[2] // bs
        assert len(counts) <= nbx * nbm * nbs
        brick = np.repeat(np.arange(len(counts)), counts)
        M = brick.size
        ext = np.array([16, bm, bs])
        cnt = np.stack([rng.integers(1, min(tw, ext[d]) + 1, size=M) for d in range(3)], axis=1)
        org = np.stack([(brick % nbx) * 16, ((brick // nbx) % nbm) * bm, (brick // (nbx * nbm)) * bs], axis=1)
        j = org + np.stack([rng.integers(0, ext[d] - cnt[:, d] + 1) for d in range(3)], axis=1)
        perm = rng.permutation(M)                      # (sample order is not brick order)
        cnt, j = cnt[perm], j[perm]
    assert M <= 4096 and (j < n).all()
    return make_records(tw, dims, j, cnt, rng, True)


def brick_geometry(dims, bm, bs):
    return dims[0] // 16, -(-dims[1] // bm), -(-dims[2] // bs)


def flagged_cells(tab, dims, bm, bs, tile):
    """the cells of the flagged segments of the table rows {brick, end, mask lo, mask hi}: bit xs + (16 / tile) (im + bm is)"""
    n0, nm, ns = dims
    nbx, nbm, _ = brick_geometry(dims, bm, bs)
    xs = 16 // tile
    flag = np.zeros(n0 * nm * ns, dtype=bool)
    brick = tab[:, 0].astype(np.int64)
    mask = tab[:, 2].astype(np.uint64) | (tab[:, 3].astype(np.uint64) << np.uint64(32))
    bx, bmi, bsi = brick % nbx, (brick // nbx) % nbm, brick // (nbx * nbm)
    for bit in range(xs * bm * bs):
        on = ((mask >> np.uint64(bit)) & np.uint64(1)).astype(bool)
        x, im, is_ = bit % xs, (bit // xs) % bm, bit // (xs * bm)
        km, ks = bmi[on] * bm + im, bsi[on] * bs + is_
        assert (km < nm).all() and (ks < ns).all(), "a flagged segment outside the grid"
        for dx in range(tile):
            flag[bx[on] * 16 + x * tile + dx + n0 * (km + nm * ks)] = True
    return flag


@functools.lru_cache(maxsize=4)
def build_scatter(case):
    """-> namespace(rec, recx (M, rs) with poisoned words behind the panel row, rs, fmt (grid_formats.shares, masks possibly
    redrawn), tab / tasks / shared as 2-D views, X, A, flag (cells the scatter must write), pieces (per cell: tasks of its brick))"""
    from indigo_amd import grid_formats
    rng = np.random.default_rng(5000 + case.seed + 1000 * case.NC)
    NC, tw, dims = case.NC, case.tw, case.dims
    if case.exact:
        rec = _scatter_records(case, rng)
        panel = exact_panel
    else:
        rec = np.ascontiguousarray(builder_records(tw)[1]['records'])
        panel = random_panel
    M, P = rec.shape[0], int(np.prod(dims))
    recx, rs = grid_formats.records_with_rows(rec)
    recx = recx.reshape(M, rs).copy()
    recx[:, sep_words(tw) + 2 * NC:] = NAN32
    fmt = grid_formats.shares(rec, tw, dims, NC, case.shape[0], case.shape[1], case.chunk, case.run, table=None, tile=case.tile)
    assert fmt is not None and (fmt['bm'], fmt['bs']) == case.shape
    fmt = dict(fmt)
    tab = fmt['table'].reshape(-1, 4).copy()
    shared = fmt['shared'].reshape(-1, 4).copy()
    if case.masks == 'rand':
        draw = rng.integers(0, 1 << 32, size=(tab.shape[0], 2), dtype=np.uint64).astype(np.uint32)
        draw[rng.integers(0, 8, size=tab.shape[0]) == 0] = 0xffffffff          # (some bricks keep everything inside the grid)
        tab[:, 2:4] &= draw
        for i in range(fmt['nshared']):
            shared[i, 2:4] = tab[np.searchsorted(tab[:, 0], shared[i, 0]), 2:4]
    fmt['table'], fmt['shared'] = tab.reshape(-1), shared.reshape(-1)
    tasks = fmt['tasks'].reshape(-1, 4)[:fmt['ntasks']]
    A = tap_matrix(rec, tw, dims)
    flag = flagged_cells(tab, dims, case.shape[0], case.shape[1], case.tile)
    # tasks per brick -> per cell
    nbx, nbm, nbs = brick_geometry(dims, *case.shape)
    per_brick = np.zeros(nbx * nbm * nbs, dtype=np.int64)
    is_shared = ((tasks[:, 3] >> 16) & 1).astype(bool)
    np.add.at(per_brick, tab[tasks[is_shared, 2], 0].astype(np.int64), 1)
    cell = np.arange(P)
    brick_of = (cell % dims[0]) // 16 + nbx * (((cell // dims[0]) % dims[1]) // case.shape[0] + nbm * ((cell // (dims[0] * dims[1])) // case.shape[1]))
    return ScatterData(
        case, rec, recx, rs, fmt, tab, tasks, shared, panel(rng, (M, NC)), A, M, P, flag, per_brick[brick_of], brick_of)


def expand_shares(D):
    """the taps of every share through its geometry word: (share, sample, a, b, c, cell) -- tap (a, b, c) of the sample sits at brick
    cell (ox + a, om + b, os + c); the taps b in [blo, bhi), c in [clo, chi) and those a < c0 with 0 <= ox + a < 16 are the share's"""
    tw, (n0, nm, ns) = D.case.tw, D.case.dims
    bm, bs = D.case.shape
    nbx, nbm, _ = brick_geometry(D.case.dims, bm, bs)
    nsh = D.fmt['nshares']
    sh = D.fmt['shares'].reshape(-1, 2)[:nsh]
    ends = D.tab[:, 1].astype(np.int64)
    brick = D.tab[np.searchsorted(ends, np.arange(nsh), side='right'), 0].astype(np.int64)
    bx, bmi, bsi = brick % nbx, (brick // nbx) % nbm, brick // (nbx * nbm)
    t, gmask, geo = (sh[:, 0] & 0x0fffffff).astype(np.int64), sh[:, 0] >> 28, sh[:, 1]
    ox, om, os_ = (geo & 31).astype(np.int64) - 8, ((geo >> 5) & 31).astype(np.int64) - 8, ((geo >> 10) & 31).astype(np.int64) - 8
    blo, bhi, clo, chi = (geo >> 15) & 7, (geo >> 18) & 15, (geo >> 22) & 7, (geo >> 25) & 15
    cnt0 = unpack(D.rec, tw)[1][:, 0]
    out = []
    for c in range(tw):
        for b in range(tw):
            for a in range(tw):
                cx = ox + a
                ok = np.flatnonzero((cx >= 0) & (cx < 16) & (a < cnt0[t]) & (b >= blo) & (b < bhi) & (c >= clo) & (c < chi))
                if ok.size == 0:
                    continue
                im, is_ = (om + b)[ok], (os_ + c)[ok]
                assert (im >= 0).all() and (im < bm).all() and (is_ >= 0).all() and (is_ < bs).all()
                assert (((gmask[ok] >> is_.astype(np.uint32)) & 1) == 1).all(), "the share's slow-cell mask misses a tap"
                cell = bx[ok] * 16 + cx[ok] + n0 * (bmi[ok] * bm + im + nm * (bsi[ok] * bs + is_))
                out.append(np.stack([ok, t[ok], np.full(ok.size, a), np.full(ok.size, b), np.full(ok.size, c), cell], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 6), np.int64)
