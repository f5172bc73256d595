"""A float64 restatement of the CSR x panel product of the gather/scatter family (indigo_amd/csrc/ig_spmm.hip), a Python mirror of
the decision tree that picks its kernel (pick_shape, launch_gather), and a table of cases built through that mirror so that every
reachable kernel meets row lengths at its own seams.  Plain numpy / scipy: nothing here needs a GPU.

Reference: beta Y + alpha op(B) Xs in complex128, alpha and beta with float32 parts (the ABI takes floats); beta == 0 does not read Y
(BLAS rule).  B is the CSR the entry point is handed (rows x nx): the matrix itself for the forward entry points, the transpose for
ig_ccsrmm_t* whose kernels conjugate the values (CONJ); Xs are the panel rows the column indices mean (a list for ig_ccsrmm_xrows
and ig_ccsrmm_t_grid's xrow_perm); a result-row permutation stores result r at Y[yperm[r]].

Exact inputs (exact_values): matrix values and panel entries have NONZERO INTEGER parts in [-4, 4], alpha = 0.5 - 0.25j,
beta = -0.5 + 1.5j.  A product's parts are then integers of magnitude <= 2 * 16 = 32, so every partial sum of a row of n nonzeros, in
any order and grouping, is an integer of magnitude <= 32 n; the longest row of the table has 19 * 1024 + 1 = 19457 nonzeros (the
tail seam of k_csrmm_rows_block at one column), 32 n < 2^20: every partial sum is a float32 number (24 bits).  alpha acc is then a
multiple of 1/4 below 2^20 and beta y a multiple of 1/2 below 8: the result has at most 23 significant bits.  No kernel rounds
anything on these inputs, whatever its lane mapping (tests/test_spmm64_cpu.py emulates several), so the device must reproduce the
reference BIT FOR BIT, every element of every row."""
import functools

import numpy as np
import scipy.sparse as spp

C64 = np.dtype('complex64')
C128 = np.dtype('complex128')

ALPHA, BETA = 0.5 - 0.25j, -0.5 + 1.5j      # dyadic
VMAX = 4                                    # |parts| of the exact inputs
EXACT_LIMIT = 2.0 ** 24

# ---- the constants of ig_spmm.hip / ig_spmm_common.h the mirror is built on (test_spmm64_cpu.py reads them out of the sources) --------
BLK = 256
WAVES_PER_BLOCK = 4
WL_SUB = 32                 # deferred-row sub-lists per list
WL_CAP = 1 << 20            # entries per list
SUB_CAP = WL_CAP // WL_SUB  # entries per sub-list
NL_CAP = 8                  # pick_shape: nonzero lanes for rows of up to 4 * NL_CAP nonzeros
VW = 4                      # panel columns per lane of the wide k_csrmm_gather_v instantiations
DENSE_THR = 32              # k_csrmm_dense64 defers rows beyond this
THR_LONG_PER_LANE = 256     # thr_long = 256 * (64 / CL)
THR_MID_PER_LANE = 16       # thr_mid = 16 * NL
TM_SPARSE, TM_WIDE = 16, 512    # k_csrmm_rowlane's inline limit: nnz <= 2 rows / wide packed panels (k_csrmm_rowtile64: TM_WIDE too)
TILE64_U = 7                # k_csrmm_gather_tile64: 4 nonzero lanes x 7 = 28 nonzeros per pass
ROWTILE_UT = 16             # k_csrmm_rowtile64's inner unroll

# entry point -> what it passes to launch_gather
ENTRIES = {
    'ccsrmm':    dict(conj=False),                                  # ig_ccsrmm(adjoint = 0)
    'ccsrmm_t':  dict(conj=True),                                   # ig_ccsrmm_t
    'rowperm':   dict(conj=False, yperm=True),                      # ig_ccsrmm_rowperm
    'xrows':     dict(conj=False, xperm=True),                      # ig_ccsrmm_xrows (2..64 columns)
    't_grid':    dict(conj=True),                                   # ig_ccsrmm_t_grid without a panel-row list
    't_grid_xp': dict(conj=True, xperm=True),                       # ig_ccsrmm_t_grid with xrow_perm
    'il':        dict(conj=False, x_il=True),                       # ig_ccsrmm_il (power-of-two columns)
    'il_rw':     dict(conj=False, x_il=True, rvals=True),           # ig_ccsrmm_il_rw
    't_grid_il': dict(conj=True, y_il=True),                        # ig_ccsrmm_t_grid_il (2, 4, 8 columns, beta = 0)
}


def f32(v):
    return float(np.float32(v))


def cf32(v):
    v = complex(v)
    return complex(f32(v.real), f32(v.imag))


# =========================================================================================================================================
# the dispatch mirror
# =========================================================================================================================================
def pow2_ceil(v, cap):
    p = 1
    while p < v and p < cap:
        p <<= 1
    return p


def pick_shape(rows, N, nnz):
    """(CL, NL) of pick_shape: column lanes = the power of two >= N (<= 64), nonzero lanes = the power of two >= the mean row length
    that still fits the wave, at most NL_CAP while the mean is <= 4 NL_CAP"""
    CL = pow2_ceil(N, 64)
    mean = (nnz + rows - 1) // rows if rows > 0 else 1
    cap = 64 // CL
    if mean <= 4 * NL_CAP and cap > NL_CAP:
        cap = NL_CAP
    return CL, pow2_ceil(mean if mean > 0 else 1, cap)


def dispatch(entry, rows, xrows, N, nnz, beta0, x_aligned=True, masked=False):
    """launch_gather's decision for a call of `entry` with a (rows x xrows) CSR of nnz nonzeros and N panel columns.  x_aligned: the
    panel the CALLER passes is 16-byte aligned (a repacked panel always is).  ->
      main     (kernel, template arguments ...) in the order of the template's parameter list, or None with `error`
      scope    the profiling scope of the main launch
      packs    the panel is repacked first (scope pack_panel)
      t_inline rows longer than this go to the wave-per-row list (None: the kernel has no such list), thr_long: beyond that the
               workgroup-per-row list
      unit     how the main kernel hashes a row to a sub-list (see sub_list)
      deferred the deferred-row kernels launched after it, trips: the main kernel's trip sizes in nonzeros of a row"""
    e = ENTRIES[entry]
    conj, x_il, y_il = e['conj'], e.get('x_il', False), e.get('y_il', False)
    xperm, yperm, rvals = e.get('xperm', False), e.get('yperm', False), e.get('rvals', False)
    CL, NL = pick_shape(rows, N, nnz)
    sxc1, sxr, packed, packs = False, 1, False, False          # sxc1: sxc == 1 (the panel is row-major)
    if x_il:
        sxc1, sxr, packed = True, N, (N & (N - 1)) == 0 and N >= 1
    if not x_il and N == 1 and not xperm:
        packed = True
    if not x_il and ((2 <= N <= 64 and nnz >= xrows) or (xperm and N <= 64)):
        if xrows * CL * 8 > 0:                                   # (ig_pack_panel declines an empty panel; room is assumed)
            sxc1, sxr, packed, packs, x_aligned = True, CL, True, True, True
    out = dict(entry=entry, conj=conj, CL=CL, NL=NL, packed=packed, packs=packs, sxr=sxr, main=None, error=None, deferred=(), trips=())
    if xperm and not packed:
        out['error'] = 'a panel-row list needs the packed path'
        return out
    b0, bm = bool(beta0), 0 if beta0 else 1
    nlw = 64 // CL
    thr_long = THR_LONG_PER_LANE * nlw
    thr_mid = THR_MID_PER_LANE * NL if nlw > NL else thr_long
    vec = packed and sxc1 and N == sxr and nnz >= 8 * rows and x_aligned
    wide_v = VW > 0 and vec and N in (16, 32, 64) and not y_il
    rowlane = not wide_v and (nnz <= 2 * rows or (packed and N >= 16 and nnz <= 8 * rows))
    out.update(thr_long=thr_long, rowlane=rowlane)
    if rowlane:
        out['scope'] = 'csrmm_rowlane_conj' if conj else 'csrmm_rowlane'
        tm = min(thr_long, TM_SPARSE if nnz <= 2 * rows else TM_WIDE)
        bufok = packed and nnz * 8 < 0x7fffffff and xrows * sxr * 8 < 0x7fffffff
        if packed and sxc1 and N == 64 and sxr == 64 and not y_il and not masked:
            out.update(main=('rowtile64', conj, bm), t_inline=min(thr_long, TM_WIDE), unit=16, trips=(ROWTILE_UT, 64))
        elif DENSE_THR > 0 and packed and b0 and bufok and nnz <= 2 * rows and N == sxr and sxr in (8, 4, 2, 1):
            out.update(main=('dense64', sxr, conj, y_il and sxr > 1), t_inline=min(thr_long, DENSE_THR), unit=64, trips=(64,))
        elif y_il:
            out['error'] = 'an interleaved result panel needs the dense-lane kernel'
            return out
        else:
            NC = 8 if CL >= 8 else CL
            if packed and b0 and NC >= 2 and bufok:
                var = (0, True, 2, True)
            elif packed and b0:
                var = (0, True, 1, False)
            elif packed:
                var = (1, True, 1, False)
            elif b0:
                var = (0, False, 1, False)
            else:
                var = (1, False, 1, False)
            out.update(main=('rowlane', NC, conj) + var, t_inline=tm, unit=64, trips=(var[2],))
        wave = True
    else:
        if y_il:
            out['error'] = 'an interleaved result panel is only supported for matrices with mostly empty rows'
            return out
        out['scope'] = 'csrmm_gather_conj' if conj else 'csrmm_gather'
        out['t_inline'] = thr_mid
        if wide_v or (VW > 0 and vec and N in (8, 4, 2)):
            def gv(vw, clv, nl, realw=False):
                out.update(main=('gather_v', vw, clv, nl, conj, bm, realw), unit=64 // (clv * nl), trips=(4 * nl,))
            if rvals and N == 8 and 4 <= VW < 8:
                gv(4, 2, 8, True)
            elif rvals and N == 4:
                gv(2, 2, 8, True)
            elif rvals and N == 2:
                gv(2, 1, 8, True)
            elif N == 8:
                gv(8, 1, 8) if VW >= 8 else gv(4, 2, 8) if VW >= 4 else gv(2, 4, 8)
            elif N == 4:
                gv(2, 2, 8)
            elif N == 2:
                gv(2, 1, 8)
            elif nnz >= 8 * rows:
                if N == 16:
                    gv(4, 4, 8)
                elif N == 32:
                    gv(4, 8, 8)
                elif not yperm and nnz <= 0x7fffffff:
                    out.update(main=('gather_tile64', conj, bm, 4), t_inline=None, unit='tile64', trips=(4 * TILE64_U, 8 * TILE64_U))
                else:
                    gv(4, 16, 4)
            else:                       # the "short rows" arm
                gv(4, {16: 4, 32: 8, 64: 16}[N], 1)
        else:
            out.update(main=('gather', CL, NL, conj, bm), unit=64 // (CL * NL), trips=(4 * NL,))
        wave = thr_mid < thr_long
    out['deferred'] = ((('rows_wave', CL, conj, bm),) if wave else ()) + (('rows_block', CL, conj, bm),)
    return out


def sub_list(d, row):
    """the sub-list (0 .. WL_SUB - 1) the main kernel of dispatch `d` appends row `row` to"""
    row = np.asarray(row, dtype=np.int64)
    if d['unit'] == 'tile64':           # wave w of the 64-row tile takes its rows w, w + 4, ...
        return ((row // 64) * 4 + (row % 64) % 4) % WL_SUB
    return (row // d['unit']) % WL_SUB


def deferral(d, indptr, live=None):
    """rows on the wave-per-row and on the workgroup-per-row list for this row-pointer array, and the rows that found their sub-list
    full and are computed inline: dict(wave, block, wave_inline, block_inline).  live: flags of the rows a support mask keeps"""
    lens = np.diff(np.asarray(indptr, dtype=np.int64))
    rows = np.arange(lens.size)
    live = np.ones(lens.size, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    blockl = live & (lens > d['thr_long'])
    wavel = (live & (lens > d['t_inline']) & (lens <= d['thr_long'])) if d['t_inline'] is not None else np.zeros(lens.size, dtype=bool)
    out = {}
    for name, sel in (('wave', wavel), ('block', blockl)):
        cnt = np.bincount(sub_list(d, rows[sel]), minlength=WL_SUB)
        out[name] = int(np.minimum(cnt, SUB_CAP).sum())
        out[name + '_inline'] = int(np.maximum(cnt - SUB_CAP, 0).sum())
    return out


def scatter_dispatch(M, N, nnz, beta, exwrite, ldy, K):
    """ig_ccsrmm(adjoint = 1): -> (panel_scale or None: 'kernel<ZERO>' / 'memset', ('scatter', CL, NL, ATOMIC) or None)"""
    b = cf32(beta)
    if b == 1 or K == 0 or N == 0:
        pre = None
    elif b == 0 and ldy == K:
        pre = 'memset'
    else:
        pre = ('panel_scale', b == 0)
    if nnz == 0 or M == 0:
        return pre, None
    CL, NL = pick_shape(M, N, nnz)
    return pre, ('scatter', CL, NL, not exwrite)


# =========================================================================================================================================
# the cases
# =========================================================================================================================================
REGIMES = {          # name -> (filler row lengths drawn from, target mean row length)
    'sparse': ((0, 0, 0, 0, 1, 1, 2), 1.6),           # nnz <= 2 rows
    'mid3':   ((1, 2, 2, 3), 3.6),                     # 2 rows < nnz < 8 rows, mean in (3, 4]: NL = 4
    'mid':    ((3, 4, 5, 6), 6.5),                     # 2 rows < nnz < 8 rows
    'dense':  ((6, 8, 9, 11, 12), 14.0),               # nnz >= 8 rows, mean <= 32
    'vdense': ((34, 37, 41, 46), 48.0),                # mean > 32: NL up to the whole wave
}


class Case:
    """entry: key of ENTRIES; N columns; regime: key of REGIMES; big_x: more panel rows than nonzeros (a column-major panel then
    stays unpacked); want: the main kernel's name the case was designed for (asserted through the mirror)"""

    def __init__(self, entry, N, regime, want, big_x=False, rows=None, lens=None, seed=0, beta0_only=False, tag=''):
        self.entry, self.N, self.regime, self.want, self.big_x, self.rows_fixed, self.lens_fixed = entry, N, regime, want, big_x, rows, lens
        self.beta0_only = beta0_only or entry == 't_grid_il'
        self.seed = seed
        self.name = '%s-N%d-%s%s%s' % (entry, N, regime, '-bigx' if big_x else '', tag)

    def __repr__(self):
        return self.name


def seam_lengths(d):
    """the row lengths a case of dispatch `d` must hold: 0, 1, one below / at / one above every trip size of the main kernel, the two
    deferral thresholds and the length behind each, and for each deferred kernel lengths that leave a tail of 1..3 strides behind
    its 4-way unrolled loop: (4 + t) NLW -+ 1 on the wave list where that exceeds the inline limit (one pass of the unrolled loop),
    (16 + t) NLB -+ 1 on the workgroup list (thr_long is 16 NLB, so four passes is the fewest a listed row can take)"""
    s = {0, 1}
    for t in d['trips']:
        s |= {t - 1, t, t + 1}
    tl = d['thr_long']
    s |= {tl, tl + 1}
    nlw, nlb = 64 // d['CL'], 1024 // d['CL']
    if d['t_inline'] is not None:
        s |= {d['t_inline'], d['t_inline'] + 1}
        for t in (1, 2, 3):
            for L in ((4 + t) * nlw - 1, (4 + t) * nlw + 1):
                if d['t_inline'] < L <= tl and any(k[0] == 'rows_wave' for k in d['deferred']):
                    s.add(L)
    for t in (1, 2, 3):
        s |= {(16 + t) * nlb - 1, (16 + t) * nlb + 1}
    return sorted(v for v in s if v >= 0)


@functools.lru_cache(maxsize=None)
def case_lens(case):
    """the row lengths of a case: its seams (longest first: one long row first, one last, two adjacent inside one 64-row tile, the
    rest scattered) among filler rows that hold the mean row length of the regime; the row count is odd and = 37 mod 64, so the
    last wave, the last 64-row tile and the last workgroup are partial"""
    if case.lens_fixed is not None:
        return np.asarray(case.lens_fixed, dtype=np.int64)
    fill, target = REGIMES[case.regime]
    fm = float(np.mean(fill))
    rng = np.random.default_rng(1000 + case.seed)
    xr = lambda nnz: nnz + 13 if case.big_x else 97
    both = lambda rows, nnz: [dispatch(case.entry, rows, xr(nnz), case.N, nnz, b0) for b0 in ((True,) if case.beta0_only else (True, False))]
    key = lambda ds: [(d['main'], d.get('t_inline'), d['thr_long']) for d in ds]
    ds = both(1000, int(1000 * target))
    for _ in range(3):                  # the seams follow from the dispatch, the dispatch from the counts: iterate to the fixed point
        seams = sorted(set().union(*(seam_lengths(d) for d in ds)))          # beta == 0 and beta != 0 may take different kernels
        S, ns = sum(seams), len(seams)
        rows = case.rows_fixed or max(int(np.ceil((S - fm * ns) / (target - fm))), 3 * ns, 293)
        rows += (37 - rows) % 64
        lens = rng.choice(np.asarray(fill), size=rows).astype(np.int64)
        order = sorted(seams, reverse=True)
        mid = (rows // 2) // 64 * 64 + 5
        fixed = [0, rows - 1, mid, mid + 1]
        free = np.setdiff1d(np.arange(rows), fixed)
        pos = fixed + list(rng.choice(free, size=len(order) - 4, replace=False))
        lens[pos] = order
        nnz = int(lens.sum())
        ds2 = both(rows, nnz)
        if key(ds2) == key(ds):
            break
        ds = ds2
    return lens


def exact_values(rng, n, real=False):
    """n complex64 numbers whose parts are nonzero integers in [-VMAX, VMAX] (real: the imaginary parts are zero).
    The bound: a part of a product of two of them is an integer of magnitude <= 2 VMAX^2 = 32, a partial sum over any subset of a row
    of n_r nonzeros one of magnitude <= 32 n_r <= 32 * 19457 < 2^20 for the longest row of the table, far inside the 2^24 up to which
    float32 holds every integer (test_spmm64_cpu.py asserts both figures for every case)"""
    v = rng.integers(1, VMAX + 1, size=2 * n).astype(np.float32)
    v *= (1 - 2 * rng.integers(0, 2, size=2 * n)).astype(np.float32)
    v = v.view(C64).copy()
    if real:
        v.imag = 0
    return v


def rounding_values(rng, n, real=False):
    """parts uniform in [0, 1) like those of indigo_amd.util.rand64c, with random signs on top so that the sums cancel"""
    v = (rng.random(2 * n) * (1 - 2 * rng.integers(0, 2, size=2 * n))).astype(np.float32).view(C64).copy()
    if real:
        v.imag = 0
    return v


class Data:
    """the arrays of a case.  indptr / colind / vals: the CSR handed to the entry point (rows x nx); X: the panel, (xtotal, N),
    of which the rows xlist (None: all, in order) are the ones the column indices mean; yperm or None; Y0: the result's start"""


@functools.lru_cache(maxsize=4)
def build(case, exact=True):
    e = ENTRIES[case.entry]
    rng = np.random.default_rng(77 + case.seed)
    lens = case_lens(case)
    rows, nnz = lens.size, int(lens.sum())
    nx = nnz + 13 if case.big_x else 97
    draw = exact_values if exact else rounding_values
    D = Data()
    D.case, D.rows, D.nx, D.nnz, D.N = case, rows, nx, nnz, case.N
    D.indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    D.colind = rng.integers(0, nx, size=nnz).astype(np.int32)
    D.vals = draw(rng, nnz, real=e.get('rvals', False))
    D.xtotal, D.xlist, D.yperm = nx, None, None
    if case.entry == 'xrows':
        D.xtotal = 2 * nx + 3
        D.xlist = np.sort(rng.choice(D.xtotal, size=nx, replace=False)).astype(np.int32)
    elif e.get('xperm'):
        D.xlist = rng.permutation(nx).astype(np.int32)
    if e.get('yperm'):
        D.yperm = rng.permutation(rows).astype(np.int32)
    D.X = draw(rng, D.xtotal * case.N).reshape(D.xtotal, case.N)
    D.Y0 = draw(rng, rows * case.N).reshape(rows, case.N)
    return D


def csr_of(D, dtype=C128, conj=None):
    conj = ENTRIES[D.case.entry]['conj'] if conj is None else conj
    v = D.vals.astype(dtype)
    return spp.csr_matrix((v.conj() if conj else v, D.colind, D.indptr), shape=(D.rows, D.nx))


def gather_reference(D, alpha, beta):
    """beta Y0 + alpha op(B) X[xlist] in complex128, stored through yperm; beta == 0 does not read Y0"""
    Xs = D.X if D.xlist is None else D.X[D.xlist]
    res = cf32(alpha) * (csr_of(D) @ Xs.astype(C128))
    b = cf32(beta)
    if D.yperm is None:
        return res if b == 0 else res + b * D.Y0.astype(C128)
    out = np.zeros((D.rows, D.N), dtype=C128) if b == 0 else b * D.Y0.astype(C128)
    tgt = D.yperm.astype(np.int64)
    if b == 0:
        out[tgt] = res
    else:
        out[tgt] += res
    return out


def gather_bound(D, alpha, beta):
    """(n_r + 4) 2^-23 (|alpha|_1 (|B|_1 |X|_1)_rj + |beta|_1 |y_rj|_1): the classical worst case of n_r complex multiply-adds in
    float32 in ANY order (two real products and two additions per part and nonzero, unit roundoff 2^-24), alpha and beta on top"""
    l1 = lambda z: np.abs(z.real) + np.abs(z.imag)
    Xs = D.X if D.xlist is None else D.X[D.xlist]
    B1 = spp.csr_matrix((l1(D.vals.astype(C128)), D.colind, D.indptr), shape=(D.rows, D.nx))
    a, b = cf32(alpha), cf32(beta)
    w = (np.diff(D.indptr.astype(np.int64))[:, None] + 4) * 2.0 ** -23
    prod, y1 = w * l1(a) * (B1 @ l1(Xs.astype(C128))), l1(b) * l1(D.Y0.astype(C128))
    if D.yperm is None:
        return prod + w * y1
    tgt = D.yperm.astype(np.int64)
    out = np.zeros_like(prod)
    out[tgt] = prod + w * y1[tgt]
    return out


def scatter_reference(A, X, Y0, alpha, beta):
    """ig_ccsrmm(adjoint = 1): beta Y0 + alpha A^H X in complex128 (A: scipy CSR, M x K; X: (M, N); Y0: (K, N))"""
    res = cf32(alpha) * (A.astype(C128).conj().T @ X.astype(C128))
    b = cf32(beta)
    return res if b == 0 else res + b * Y0.astype(C128)


def is_f32(a):
    a = np.asarray(a)
    return bool(np.array_equal(a.astype(C64).astype(C128), a))


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def _table():
    T = []
    add = lambda *a, **k: T.append(Case(*a, seed=len(T), **k))
    # -- mostly empty rows (nnz <= 2 rows): dense64 with beta = 0, rowlane otherwise, rowtile64 at 64 packed columns
    for entry in ('ccsrmm', 'ccsrmm_t'):
        for N in (1, 2, 4, 8):
            add(entry, N, 'sparse', 'dense64|rowlane')
        add(entry, 3, 'sparse', 'rowlane')                               # packed to 4: N != sxr
        add(entry, 3, 'sparse', 'rowlane', big_x=True)                   # unpacked, column-major
        add(entry, 2, 'sparse', 'rowlane', big_x=True)
        for N in (16, 32):
            add(entry, N, 'sparse', 'rowlane')
        add(entry, 64, 'sparse', 'rowtile64')
        add(entry, 64, 'sparse', 'rowlane', big_x=True)
        add(entry, 65, 'sparse', 'rowlane')                              # the jb loop over column chunks, in the deferred kernels too
        add(entry, 130, 'sparse', 'rowlane')
    add('rowperm', 1, 'sparse', 'dense64|rowlane')
    add('rowperm', 8, 'sparse', 'dense64|rowlane')
    add('rowperm', 64, 'sparse', 'rowtile64')
    add('xrows', 4, 'sparse', 'dense64|rowlane')
    add('xrows', 6, 'sparse', 'rowlane')
    add('t_grid', 2, 'sparse', 'dense64|rowlane')
    add('t_grid_xp', 1, 'sparse', 'dense64|rowlane')
    add('t_grid_xp', 8, 'sparse', 'dense64|rowlane')
    add('t_grid_xp', 64, 'sparse', 'rowtile64')
    for N in (2, 4, 8):
        add('il', N, 'sparse', 'dense64|rowlane')
        add('t_grid_il', N, 'sparse', 'dense64')
    add('il', 16, 'sparse', 'rowlane')
    add('il', 64, 'sparse', 'rowtile64')
    add('il_rw', 4, 'sparse', 'dense64|rowlane')
    # -- wide packed panels, rows of 2..8 nonzeros on average: rowlane with the 512-nonzero inline limit, rowtile64
    for entry in ('ccsrmm', 'ccsrmm_t'):
        for N in (16, 32):
            add(entry, N, 'mid', 'rowlane')
        add(entry, 64, 'mid', 'rowtile64')
    # -- the generic row-slot gather: narrow panels between 2 and 8 nonzeros per row, unpacked panels, odd column counts
    for entry in ('ccsrmm', 'ccsrmm_t'):
        add(entry, 1, 'mid3', 'gather')
        add(entry, 1, 'mid', 'gather')
        add(entry, 1, 'vdense', 'gather')
        add(entry, 2, 'mid3', 'gather')
        add(entry, 2, 'mid', 'gather')
        add(entry, 2, 'vdense', 'gather', big_x=True)
        add(entry, 3, 'mid', 'gather')
        add(entry, 4, 'mid3', 'gather')
        add(entry, 8, 'mid', 'gather')
        add(entry, 3, 'dense', 'gather')
        add(entry, 3, 'dense', 'gather', big_x=True)
        add(entry, 4, 'vdense', 'gather', big_x=True)
        add(entry, 8, 'mid3', 'gather')
        add(entry, 16, 'dense', 'gather', big_x=True)
        add(entry, 32, 'dense', 'gather', big_x=True)
        add(entry, 64, 'dense', 'gather', big_x=True)
        add(entry, 65, 'mid', 'gather')
        add(entry, 130, 'dense', 'gather')
    add('rowperm', 3, 'mid', 'gather')
    add('xrows', 5, 'dense', 'gather')
    add('t_grid_xp', 2, 'vdense', 'gather|gather_v')
    add('il', 2, 'mid', 'gather')
    add('il_rw', 8, 'mid', 'gather')                                     # real weights handed over but not used: fewer than 8 per row
    # -- the vector row-slot gather over row-major panels, rows of 8+ nonzeros: gather_v, gather_tile64
    for entry in ('ccsrmm', 'ccsrmm_t'):
        for N in (2, 4, 8, 16, 32):
            add(entry, N, 'dense', 'gather_v')
        add(entry, 64, 'dense', 'gather_tile64')
        add(entry, 2, 'vdense', 'gather_v')
    add('rowperm', 64, 'dense', 'gather_v')                              # a row permutation keeps 64 columns off the tile kernel
    add('rowperm', 16, 'dense', 'gather_v')
    add('xrows', 32, 'dense', 'gather_v')
    add('xrows', 64, 'dense', 'gather_tile64')
    add('t_grid_xp', 4, 'dense', 'gather_v')
    for N in (2, 4, 8):
        add('il', N, 'dense', 'gather_v')
        add('il_rw', N, 'dense', 'gather_v')                             # REALW; the rows past thr_mid read the complex values again
    add('il', 16, 'dense', 'gather_v')
    add('il_rw', 16, 'dense', 'gather_v')                                # 16 columns: the real weights are ignored
    # -- row counts of 1, empty and single-nonzero matrices
    for entry, N in (('ccsrmm', 1), ('ccsrmm_t', 4), ('ccsrmm', 64), ('il', 8), ('ccsrmm', 65)):
        add(entry, N, 'sparse', '', lens=[0], tag='-onerow0')
        add(entry, N, 'sparse', '', lens=[1], tag='-onerow1')
        add(entry, N, 'dense', '', lens=[29], tag='-onerow29')
        add(entry, N, 'sparse', '', lens=[0] * 301, tag='-empty')
        add(entry, N, 'sparse', '', lens=[0] * 170 + [1] + [0] * 130, tag='-single')
    return tuple(T)


CASES = _table()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# one rand64c-like case per kernel family (rounding cases)
ROUNDING_CASES = tuple(CASE_BY_NAME[n] for n in (
    'ccsrmm-N3-mid', 'ccsrmm_t-N130-dense', 'ccsrmm_t-N8-dense', 'il_rw-N4-dense', 'ccsrmm-N64-dense', 'rowperm-N64-dense',
    'ccsrmm_t-N4-sparse', 'ccsrmm-N3-sparse', 'ccsrmm_t-N64-sparse', 'ccsrmm-N1-sparse', 't_grid_il-N8-sparse', 'ccsrmm-N1-vdense'))


def betas_of(case):
    return (0,) if case.beta0_only else (0, BETA)


def case_dispatch(case, D, beta, x_aligned=True):
    return dispatch(case.entry, D.rows, D.nx, D.N, D.nnz, cf32(beta) == 0, x_aligned=x_aligned)


# ---- the full sub-list ------------------------------------------------------------------------------------------------------------------
def overflow_lens():
    """About 1.05 million rows, one column: every row of the 64-row tasks whose index is = 0 (mod WL_SUB) holds DENSE_THR + 1
    nonzeros, as many such tasks as fill sub-list 0 and one more; every other row is empty (nnz <= 2 rows holds)"""
    ntask = SUB_CAP // 64 + 1
    rows = ((ntask - 1) * WL_SUB + 1) * 64 + 37
    lens = np.zeros(rows, dtype=np.int64)
    for t in range(ntask):
        lens[t * WL_SUB * 64:t * WL_SUB * 64 + 64] = DENSE_THR + 1
    return lens


# ---- scatter cases (ig_ccsrmm, adjoint = 1) ---------------------------------------------------------------------------------------------
SCATTER_CASES = tuple((N, mean, M) for N in (1, 3, 8, 64, 65, 130) for mean, M in ((0.5, 333), (3, 293), (40, 37))) + ((1, 0, 1), (2, 1, 1))


def scatter_case(N, mean, M, exwrite, exact=True, seed=0):
    """A (M x K scipy CSR; exwrite: no column holds two nonzeros), X (M, N), Y0 (K, N)"""
    rng = np.random.default_rng(500 + seed + 7 * N + M)
    draw = exact_values if exact else rounding_values
    lens = rng.poisson(mean, size=M).astype(np.int64) if mean else np.zeros(M, dtype=np.int64)
    if M > 3 and mean:
        lens[0], lens[-1], lens[M // 2] = 0, 4 * int(mean) + 5, 1
    nnz = int(lens.sum())
    K = nnz + 11 if exwrite else max(nnz // 3, 1) + 11
    colind = rng.permutation(K)[:nnz] if exwrite else rng.integers(0, K, size=nnz)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    A = spp.csr_matrix((draw(rng, nnz), colind.astype(np.int32), indptr.astype(np.int32)), shape=(M, K))
    return A, draw(rng, M * N).reshape(M, N), draw(rng, K * N).reshape(K, N)


# =========================================================================================================================================
# a float32 emulation of a row's accumulation in a given lane mapping
# =========================================================================================================================================
def emulate_rows(D, cols, lanes=1, reverse=False, min_len=0, max_len=None):
    """The float32 accumulators alpha is applied to, for the panel columns `cols`, if a row's nonzeros are dealt to `lanes` lanes
    (lane l takes nonzeros l, l + lanes, ... one after the other, two rounded products and two rounded additions per part; the lanes
    are then folded pairwise like the kernels' __shfl_xor trees).  reverse: the nonzeros are taken last first.  -> (rows, len(cols))
    complex64; rows shorter than min_len or longer than max_len are left out (NaN)"""
    conj = ENTRIES[D.case.entry]['conj']
    Xs = (D.X if D.xlist is None else D.X[D.xlist])[:, cols]
    xre, xim = np.ascontiguousarray(Xs.real, dtype=np.float32), np.ascontiguousarray(Xs.imag, dtype=np.float32)
    lens = np.diff(D.indptr.astype(np.int64))
    ptr = D.indptr.astype(np.int64)
    out = np.full((D.rows, len(cols)), np.nan + 1j * np.nan, dtype=C64)
    sg = np.float32(1.0 if conj else -1.0)          # conj(v) x = (vr xr + vi xi) + i (vr xi - vi xr)
    vr, vi = D.vals.real.astype(np.float32), D.vals.imag.astype(np.float32)

    def run(sel):
        L = int(lens[sel].max())
        trips = max((L + lanes - 1) // lanes, 1)
        k = np.arange(trips * lanes, dtype=np.int64)[None, :]
        valid = k < lens[sel][:, None]
        p = np.where(valid, (ptr[sel + 1][:, None] - 1 - k) if reverse else (ptr[sel][:, None] + k), 0)
        w = valid.astype(np.float32)
        a, b = (vr[p] * w)[..., None], (vi[p] * w)[..., None]            # a slot past the row's end adds zero
        col = D.colind[p] if D.nnz else np.zeros_like(p)
        xr, xi = xre[col], xim[col]
        shp = (sel.size, trips, lanes, len(cols))
        t_re1, t_re2 = (a * xr).reshape(shp), (sg * (b * xi)).reshape(shp)
        t_im1, t_im2 = (a * xi).reshape(shp), (-sg * (b * xr)).reshape(shp)
        re = np.zeros((sel.size, lanes, len(cols)), dtype=np.float32)
        im = np.zeros_like(re)
        for t in range(trips):
            re = (re + t_re1[:, t]) + t_re2[:, t]
            im = (im + t_im1[:, t]) + t_im2[:, t]
        n = lanes
        while n > 1:
            h = n // 2
            re, im = re[:, :h] + re[:, h:n], im[:, :h] + im[:, h:n]
            n = h
        assert re.dtype == np.float32
        out[sel] = re[:, 0] + 1j * im[:, 0]

    ok = (lens >= min_len) & (np.ones(D.rows, dtype=bool) if max_len is None else lens <= max_len)
    if D.nnz == 0:
        out[ok] = 0
        return out
    for sel in (np.flatnonzero(ok & (lens <= 64)), np.flatnonzero(ok & (lens > 64))):
        step = max(1, (1 << 22) // (max(lanes, 64) * len(cols)))
        for i in range(0, sel.size, step):
            run(sel[i:i + step])
    return out


def finish_f32(acc, y0, alpha, beta):
    """out = cmul(alpha, acc), then cfma(out, beta, y) unless beta == 0, in float32 operations as the kernels' epilogue does them"""
    a, b = cf32(alpha), cf32(beta)
    ar, ai, br, bi = (np.float32(v) for v in (a.real, a.imag, b.real, b.imag))
    cr, ci = acc.real.astype(np.float32), acc.imag.astype(np.float32)
    re, im = ar * cr - ai * ci, ar * ci + ai * cr
    if b != 0:
        yr, yi = y0.real.astype(np.float32), y0.imag.astype(np.float32)
        re, im = (re + br * yr) - bi * yi, (im + br * yi) + bi * yr
    assert re.dtype == np.float32
    return (re + 1j * im).astype(C64)
