"""No GPU: what tests/test_hip_gridsep64.py rests on.  The float64 reference of tests/gridsep64.py against interp.sep_expand + scipy
and against the stored matrix of the builder; float32 emulations of the kernels' sums (the gather's lane order and shuffle tree, the
scatter's share order per task and its pieces in two orders) that reproduce the reference bit for bit on every exact case; the
exactness bound per case; the seams the tables claim to contain, read off the wave compositions and the task lists; the mirror's
constants, read out of ig_gridsep.hip; and the shares, expanded through their geometry word, against every tap of the hand-built
records."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as spp

import gridsep64 as g
from gridsep64 import ALPHA, BETA, C64, C128, GATHER_CASES, GATHER_ROUNDING, SCATTER_CASES, SCATTER_ROUNDING
from indigo_amd import _lib
from indigo_amd.interp import sep_expand

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "indigo_amd", "csrc")
F32 = np.float32
COMBOS_G = [(NC, tw) for NC in (2, 4, 8) for tw in (4, 6, 8)]
COMBOS_S = [(NC, tw) for NC in (4, 8) for tw in (4, 6, 8)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_mirror_holds_the_constants_of_the_source():
    src = open(os.path.join(CSRC, "ig_gridsep.hip")).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, (pattern, m)
        return m[0]
    assert int(one(r"constexpr int BLK = (\d+);")) == g.BLK
    assert one(r"constexpr int WPB = ([^;]+);") == "BLK / 64"
    assert tuple(int(v) for v in one(r"constexpr int G = (\d+), R = (\d+);")) == (g.G, g.R)
    assert one(r"constexpr int sep_words\(int tw\) \{ return ([^;]+); \}") == "tw == 4 ? 16 : 32"
    assert one(r"constexpr int QL = NC / 2, XL = ([^,]+), LPS = QL \* XL, SPW = 64 / LPS;") == "TW <= 4 ? 4 : 8"
    assert one(r"constexpr int CG = ([^;]+);") == "TW <= 4 ? 4 : 2"
    assert one(r"const int idx = b \* (\d+) \+ lane;") == str(g.HDR) and "hdr_all[WPB][128]" in src
    L = _lib.lib()
    for NC, tw in COMBOS_G:
        assert L.ig_grid_gather_sep_group(NC, tw) == g.gather_geometry(NC, tw)[3]
        assert L.ig_interp3_sep_words(tw) == g.sep_words(tw)
    assert L.ig_grid_gather_sep_group(16, 4) == 0 and L.ig_grid_gather_sep_group(4, 5) == 0


# =========================================================================================================================================
# the reference
# =========================================================================================================================================
def _expanded(rec, tw, dims):
    r, c, v = sep_expand(dict(records=rec, tw=tw, dims=dims, gconst=1.0))
    S = spp.csr_matrix((v.real.astype(np.float64), (r, c)), shape=(rec.shape[0], int(np.prod(dims))))
    S.sort_indices()
    return S


@pytest.mark.parametrize("case", GATHER_CASES[::7] + SCATTER_CASES[::9], ids=repr)
def test_reference_equals_the_expanded_records_exactly(case):
    D = g.build_gather(case) if isinstance(case, g.GCase) else g.build_scatter(case)
    A = D.A.copy()
    A.sort_indices()
    S = _expanded(D.rec, case.tw, case.dims)
    assert np.array_equal(A.indptr, S.indptr) and np.array_equal(A.indices, S.indices) and np.array_equal(A.data, S.data)


@pytest.mark.parametrize("tw", [4, 6, 8])
def test_reference_on_builder_records_is_the_stored_matrix(tw):
    p, sep = g.builder_records(tw)
    dims = tuple(sep['dims'])
    assert dims == (32, 16, 16) and sep['tw'] == tw
    A = g.tap_matrix(sep['records'], tw, dims)
    A.sort_indices()
    S = _expanded(sep['records'], tw, dims)
    assert np.array_equal(A.indptr, S.indptr) and np.array_equal(A.indices, S.indices)
    assert np.abs(A.data - S.data).max() <= 2 * 2.0 ** -24 * np.abs(A.data).max()          # two float32 roundings of the product
    Gs = p.fused_interp(1)
    Gs.sort_indices()
    assert np.array_equal(A.indptr, Gs.indptr) and np.array_equal(A.indices, Gs.indices)
    assert np.abs(A.data * sep['gconst'] - Gs.data).max() <= 4e-7 * np.abs(Gs.data).max()   # (test_gridsep_cpu.py's bar)


@pytest.mark.parametrize("case", GATHER_ROUNDING + SCATTER_ROUNDING, ids=repr)
def test_rounding_cases_stay_clear_of_flush_to_zero(case):
    D = g.build_gather(case) if isinstance(case, g.GCase) else g.build_scatter(case)
    w = np.abs(D.A.data)
    X = np.where(np.isnan(D.X), 0, D.X)
    x = np.concatenate([np.abs(X.real).ravel(), np.abs(X.imag).ravel()])
    assert w[w > 0].min() * x[x > 0].min() >= 2.0 ** -100
    j, cnt, wt = g.unpack(D.rec, case.tw)
    wt = np.abs(wt[wt != 0])
    assert wt.min() ** 2 >= 2.0 ** -100          # (the partial products (w0 w2), (wm x) ws of the kernels)


# =========================================================================================================================================
# exactness
# =========================================================================================================================================
@pytest.mark.parametrize("case", GATHER_CASES + SCATTER_CASES, ids=repr)
def test_exact_inputs_cannot_round(case):
    gather = isinstance(case, g.GCase)
    D = g.build_gather(case) if gather else g.build_scatter(case)
    j, cnt, w = g.unpack(D.rec, case.tw)
    assert D.M <= 4096 and max(case.dims[0], 1) <= 32 and case.dims[1] <= 16 and case.dims[2] <= 16
    assert set(np.unique(np.abs(w)).tolist()) <= {0.0, 1.0, 2.0}
    assert (w[np.arange(case.tw)[None, None, :] >= cnt[:, :, None]] == 0).all() and (D.rec[:, 3 * case.tw + 2:] == 0).all() and (cnt >= 1).all()
    X = np.where(np.isnan(D.X), 0, D.X)
    parts = np.concatenate([X.real.ravel(), X.imag.ravel()])
    assert np.array_equal(parts, np.round(parts)) and np.abs(parts).max() <= g.VMAX
    assert np.abs(D.A.data).max() <= 8
    most_taps = int(cnt.prod(axis=1).max())
    most_hits = int(np.diff(D.A.T.tocsr().indptr).max())
    assert 64 * most_taps <= 2 ** 15 and 64 * most_hits <= 2 ** 18 and most_hits <= D.M
    if gather:
        assert not np.isnan(D.X[D.touched]).any() and np.isnan(D.X[~D.touched]).all()
        assert 4 * float(abs(D.A).sum(axis=1).max()) <= 2 ** 15
        refs = [g.forward_reference(D.A, D.X, D.Y0, ALPHA, b) for b in (0, BETA)]
    else:
        assert 4 * float(abs(D.A).sum(axis=0).max()) <= 2 ** 18
        refs = [g.adjoint_reference(D.A, D.X, ALPHA)]
    for ref in refs:
        assert np.array_equal(ref.astype(C64).astype(C128), ref)
        assert np.array_equal(ref * 4, np.round(ref.real * 4) + 1j * np.round(ref.imag * 4)) and np.abs(ref.real).max() < 2 ** 20


# =========================================================================================================================================
# the gather: wave compositions, float32 emulation
# =========================================================================================================================================
def wave_facts(case, rec):
    """per wave of k_grid_gather_sep: widest slow-axis count, samples with all tw middle-axis taps, distinct count triples"""
    spw = g.gather_geometry(case.NC, case.tw)[2]
    cnt = g.unpack(rec, case.tw)[1]
    out = []
    for lo in range(0, rec.shape[0], spw):
        c = cnt[lo:lo + spw]
        out.append((int(c[:, 2].max()), int((c[:, 1] == case.tw).sum()), len(set(map(tuple, c.tolist()))), c.shape[0]))
    return out


@pytest.mark.parametrize("NC,tw", COMBOS_G)
def test_gather_table_sits_on_its_seams(NC, tw):
    cases = [c for c in GATHER_CASES if (c.NC, c.tw) == (NC, tw)]
    QL, XL, spw, group, CG = g.gather_geometry(NC, tw)
    assert (QL, spw * QL * XL, group) == (NC // 2, 64, 4 * spw) and XL == (4 if tw == 4 else 8)
    Ms = sorted(set(c.M for c in cases))
    assert {1, max(spw - 1, 1), group - 1, group, group + 1} <= set(Ms)
    blocks = {-(-M // group) for M in Ms}
    assert {1, 2, 7, 8, 9} <= blocks and max(blocks) >= 40
    assert {b & 7 for b in blocks} >= {0, 1, 2, 7}          # the remainders of xcd_block
    assert all(M % spw for M in Ms if M not in (group, 1, spw - 1)) or spw == 1
    assert set(c.dims for c in cases) == {(tw, tw, tw), (16, tw, tw), (20, 13, 11)}
    assert all(c.dims[0] <= 32 and c.dims[1] <= 16 and c.dims[2] <= 16 for c in cases)
    assert all(any(c.dims == d and c.M > 4 * group for c in cases) for d in g.gather_grids(tw))          # every grid with an ordered run
    widest, nbt_short, one_full, mixed = set(), 0, 0, 0
    seen = [set(), set(), set()]
    firsts = [set(), set(), set()]
    for c in cases:
        D = g.build_gather(c)
        j, cnt, _ = g.unpack(D.rec, tw)
        for d in range(3):
            seen[d] |= set(cnt[:, d].tolist())
            n = c.dims[d]
            firsts[d] |= {'zero'} if (j[:, d] == 0).any() else set()
            firsts[d] |= {'last'} if ((j[:, d] == n - 1) & (cnt[:, d] > 1)).any() else set()
            firsts[d] |= {'wrap1'} if ((j[:, d] == n - cnt[:, d] + 1) & (cnt[:, d] > 1)).any() else set()
        for top2, full, kinds, size in wave_facts(c, D.rec):
            widest.add(top2)
            nbt_short += full == 0 and size == spw
            one_full += full == 1 and size > 1
            mixed += kinds > 1
    assert all(s == set(range(1, tw + 1)) for s in seen)
    assert all(f == {'zero', 'last', 'wrap1'} for f in firsts)
    assert widest == set(range(1, tw + 1))                  # the nc2u exit: inside (odd) and at the edge (even) of a group of CG = 2 rows
    assert nbt_short > 0 and one_full > 0 and mixed > 0


def emulate_gather(D, alpha, beta):
    """k_grid_gather_sep in float32, lane by lane: lane i of a sample walks the wave's rows (c, b) in order -- a lane past its sample's
    counts re-reads the sample's last tap with weight zero --, then the shuffle tree over the x-tap lanes, alpha and beta"""
    case = D.case
    NC, tw, (n0, nm, ns) = case.NC, case.tw, case.dims
    QL, XL, spw, group, CG = g.gather_geometry(NC, tw)
    j, cnt, w = g.unpack(D.rec, tw)
    M = D.M
    Xf = np.ascontiguousarray(D.X).view(F32).reshape(D.P, 2 * NC)
    wave = np.arange(M) // spw
    nw = int(wave[-1]) + 1
    top2 = np.zeros(nw, np.int64)
    np.maximum.at(top2, wave, cnt[:, 2])
    full = np.zeros(nw, bool)
    np.logical_or.at(full, wave, cnt[:, 1] >= tw)
    rows = (-(-top2 // CG) * CG)[wave]                      # slow-axis rows the wave walks: whole groups of CG
    nbt = np.where(full, tw, tw - 1)[wave]
    i = np.arange(XL)[None, :]
    iv = np.minimum(i, cnt[:, 0, None] - 1)
    w0 = np.where(i < cnt[:, 0, None], np.take_along_axis(w[:, 0], iv, axis=1), F32(0))
    jx = (j[:, 0, None] + iv) % n0
    acc = np.zeros((M, XL, 2 * NC), F32)
    for c in range(tw):
        cc = np.minimum(c, cnt[:, 2] - 1)
        js = (j[:, 2] + cc) % ns
        ws = np.where((c < cnt[:, 2])[:, None], w0 * w[:, 2, c][:, None], F32(0)).astype(F32)
        for b in range(tw):
            bb = np.minimum(b, cnt[:, 1] - 1)
            jm = (j[:, 1] + bb) % nm
            wt = (ws * np.where(b < cnt[:, 1], w[:, 1, b], F32(0))[:, None]).astype(F32)
            v = Xf[jx + n0 * (jm + nm * js)[:, None]]
            live = ((c < rows) & (b < nbt))[:, None, None]
            acc = np.where(live, (wt[:, :, None] * v).astype(F32) + acc, acc)
    off = 1
    while off < XL:
        acc = acc + acc[:, np.arange(XL) ^ off]
        off <<= 1
    s = acc[:, 0].reshape(M, NC, 2)
    a, b_ = g.cf32(alpha), g.cf32(beta)
    ar, ai = F32(a.real), F32(a.imag)
    re, im = ar * s[..., 0] - ai * s[..., 1], ar * s[..., 1] + ai * s[..., 0]
    if b_ != 0:
        y = np.ascontiguousarray(D.Y0).view(F32).reshape(M, NC, 2)
        br, bi = F32(b_.real), F32(b_.imag)
        re, im = re + br * y[..., 0] - bi * y[..., 1], im + br * y[..., 1] + bi * y[..., 0]
    assert re.dtype == F32 and im.dtype == F32
    return (re + 1j * im).astype(C64)


@pytest.mark.parametrize("case", GATHER_CASES, ids=repr)
def test_float32_gather_emulation_is_the_reference_bit_for_bit(case):
    D = g.build_gather(case)
    for beta in (0, BETA):
        emu = emulate_gather(D, ALPHA, beta)
        assert np.isfinite(emu.view(F32)).all(), "a lane read a cell no sample touches"
        assert np.array_equal(bits(emu), bits(g.forward_reference(D.A, D.X, D.Y0, ALPHA, beta).astype(C64)))


# =========================================================================================================================================
# the scatter: shares, task lists, float32 emulation
# =========================================================================================================================================
@pytest.mark.parametrize("case", SCATTER_CASES, ids=repr)
def test_shares_hold_every_tap_of_the_records_exactly_once(case):
    D = g.build_scatter(case)
    E = g.expand_shares(D)
    j, cnt, w = g.unpack(D.rec, case.tw)
    t, cell, _ = g.taps(D.rec, case.tw, case.dims)
    assert E.shape[0] == t.size == int(cnt.prod(axis=1).sum())
    key = lambda tt, cc: np.sort(tt.astype(np.int64) * D.P + cc)
    assert np.array_equal(key(E[:, 1], E[:, 5]), key(t, cell)) and np.unique(key(t, cell)).size == t.size
    # ... and under the tap indices the share names: (a, b, c) of sample t is where the record puts it
    n0, nm, ns = case.dims
    tt = E[:, 1]
    assert np.array_equal(E[:, 5], (j[tt, 0] + E[:, 2]) % n0 + n0 * ((j[tt, 1] + E[:, 3]) % nm + nm * ((j[tt, 2] + E[:, 4]) % ns)))
    assert np.array_equal(D.brick_of[E[:, 5]], D.tab[np.searchsorted(D.tab[:, 1].astype(np.int64), E[:, 0], side='right'), 0])


def test_scatter_table_sits_on_its_seams():
    unshared, pieces, nbricks, boundary = set(), set(), set(), set()
    beside, odd_count, bit63 = 0, 0, set()
    combos = {}
    for c in SCATTER_CASES:
        D = g.build_scatter(c)
        tasks, tab = D.tasks, D.tab
        ln = (tasks[:, 1] - tasks[:, 0]).astype(np.int64)
        sh = ((tasks[:, 3] >> 16) & 1).astype(bool)
        nb = tasks[:, 3] & 0xffff
        assert (ln >= 1).all() and (nb >= 1).all() and (nb <= g.MAX_BRICKS).all() and (nb[sh] == 1).all() and (ln[sh] <= c.chunk).all()
        unshared |= set(ln[~sh].tolist())
        pieces |= set(ln[sh].tolist())
        nbricks |= set(nb[~sh].tolist())
        for lo, bt, n in zip(tasks[~sh, 0], tasks[~sh, 2], nb[~sh]):
            boundary |= set(((tab[bt:bt + n - 1, 1].astype(np.int64) - lo) % g.G).tolist())
        beside += bool(sh.any() and (~sh).any() and D.fmt['nshared'] > 0)
        odd_count += tasks.shape[0] % g.WPB != 0
        combos.setdefault((c.NC, c.tw), set()).add((c.shape, c.tile, c.dims, c.masks))
        inside = g.build_scatter(c._replace(masks='all')).tab if c.masks == 'rand' else tab
        assert ((tab[:, 2:4] & ~inside[:, 2:4]) == 0).all(), "a flagged segment outside the grid"
        if c.shape == (4, 4) and c.tile == 4:
            bit63 |= set(((tab[:, 3] >> 31) & 1)[(inside[:, 3] >> 31) == 1].tolist())
        if c.kind == 'wrap':          # a footprint that wraps on all three axes, inside the one brick along x
            j, cnt, _ = g.unpack(D.rec, c.tw)
            assert c.dims == (16, c.tw, c.tw) and ((j + cnt) > np.asarray(c.dims)).all(axis=1).any()
        if c.kind == 'blob':
            assert np.bincount(D.brick_of[g.taps(D.rec, c.tw, c.dims)[1]]).max() > 3000 and D.fmt['nshared'] > 0
    lengths = unshared | pieces
    assert {v % 8 for v in lengths} == set(range(8)) and {v % 8 for v in unshared} == set(range(8))
    assert set(g.SEAM_LENGTHS) <= unshared and max(unshared) >= 257          # group, ring and header-batch seams in tasks that flush by themselves
    assert {63, 64, 65, 127, 128, 129, 191, 192, 193} <= pieces and max(pieces) >= 257          # ... and in shared pieces
    assert boundary == {0, 1, 2, 3}
    assert 64 in nbricks and 1 in nbricks
    assert beside > 0 and odd_count > 0
    assert bit63 == {0, 1}
    assert set(combos) == set(COMBOS_S)
    for v in combos.values():
        assert {s for s, _, _, _ in v} == set(g.SHAPES) and {t for _, t, _, _ in v} == {16, 8, 4} and {m for _, _, _, m in v} == {'all', 'rand'}
        assert {d for _, _, d, _ in v} >= {(32, 13, 11), (32, 16, 16)}


def emulate_scatter(D, alpha, reverse):
    """k_grid_scatter_mfma in float32: a task adds its shares in order into one brick image -- (wm * x) * ws, times wx, added --, alpha
    on the image; the pieces of a shared brick are added to the zeroed grid in task order or, reverse, the other way round.
    -> (cells, NC) complex64, NaN where nothing is written"""
    case = D.case
    NC, tw = case.NC, case.tw
    _, _, w = g.unpack(D.rec, tw)
    E = g.expand_shares(D)
    E = E[np.argsort(E[:, 0], kind='stable')]
    s, t, a, b, c, cell = E.T
    xf = np.ascontiguousarray(D.X).view(F32).reshape(D.M, 2 * NC)
    contrib = (w[t, 0, a][:, None] * ((w[t, 1, b][:, None] * xf[t]).astype(F32) * w[t, 2, c][:, None]).astype(F32)).astype(F32)
    tasks = D.tasks
    task_of = np.full(D.fmt['nshares'], -1, np.int64)
    for k, (lo, hi) in enumerate(tasks[:, :2]):
        task_of[lo:hi] = k
    assert (task_of >= 0).all()
    shared_task = ((tasks[:, 3] >> 16) & 1).astype(bool)
    aa = g.cf32(alpha)
    ar, ai = F32(aa.real), F32(aa.imag)

    def scaled(img):
        v = img.reshape(img.shape[0], NC, 2)
        return np.stack([ar * v[..., 0] - ai * v[..., 1], ar * v[..., 1] + ai * v[..., 0]], axis=-1).reshape(img.shape[0], 2 * NC).astype(F32)
    own = ~shared_task[task_of[s]]
    img = np.zeros((D.P, 2 * NC), F32)
    np.add.at(img, cell[own], contrib[own])                 # (unbuffered: the additions happen in share order)
    out = scaled(img)
    total = np.zeros((D.P, 2 * NC), F32)
    first = np.searchsorted(s, tasks[:, 0]), np.searchsorted(s, tasks[:, 1])
    order = np.flatnonzero(shared_task)
    for k in (order[::-1] if reverse else order):
        sel = slice(first[0][k], first[1][k])
        cells, inv = np.unique(cell[sel], return_inverse=True)
        piece = np.zeros((cells.size, 2 * NC), F32)
        np.add.at(piece, inv, contrib[sel])
        total[cells] += scaled(piece)
    in_shared = np.isin(D.brick_of, D.shared[:D.fmt['nshared'], 0])
    out[in_shared] = total[in_shared]
    res = out.view(C64).reshape(D.P, NC).copy()
    res[~D.flag] = np.nan
    return res


@pytest.mark.parametrize("case", SCATTER_CASES, ids=repr)
def test_float32_scatter_emulation_is_the_reference_bit_for_bit(case):
    D = g.build_scatter(case)
    ref = g.adjoint_reference(D.A, D.X, ALPHA).astype(C64)
    touched = np.zeros(D.P, bool)
    touched[D.A.indices] = True
    if case.masks == 'all':
        assert not (touched & ~D.flag).any()                # with every segment inside the grid flagged no tap is lost
    for reverse in (False, True):
        emu = emulate_scatter(D, ALPHA, reverse)
        assert np.array_equal(emu[D.flag], ref[D.flag])
        assert np.isfinite(emu[D.flag].view(F32)).all() and np.isnan(emu[~D.flag]).all()
