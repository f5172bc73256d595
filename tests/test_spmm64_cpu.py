"""What makes the comparisons of tests/test_hip_spmm.py legitimate, without a GPU: the exact inputs of tests/spmm64.py really are
exact in float32 whatever the order of a row's sum, the case table reaches every kernel launch_gather can reach (the literal lists
below are what to compare with launch_gather in indigo_amd/csrc/ig_spmm.hip), every case holds row lengths at the seams of the
kernel it reaches, the mirror's constants are the ones in the sources, and a float32 emulation of the rounding cases stays within
the bound the GPU test applies."""
import itertools
import os
import re

import numpy as np
import pytest

import spmm64 as s
from spmm64 import ALPHA, BETA, C64, C128, CASES

eq = np.testing.assert_array_equal
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "indigo_amd", "csrc")
FT = (False, True)

# =========================================================================================================================================
# the kernels the table reaches: (kernel, template arguments in the order of the template's parameter list)
# =========================================================================================================================================
# k_csrmm_gather<CL, NL, CONJ, BMODE>: CL = pow2 >= N; NL from the mean row length, >= 4 below 32 columns because 2 nonzeros per row or
# fewer go to the row-per-lane kernels
GATHER = ((1, 4), (1, 8), (1, 64), (2, 4), (2, 8), (2, 32), (4, 4), (4, 8), (4, 16), (8, 4), (8, 8), (16, 4), (32, 2), (64, 1))
# k_csrmm_gather_v<VW, CLV, NL, CONJ, BMODE, REALW>: 2, 4, 8, 16, 32 columns; 64 columns only behind a result-row permutation (no CONJ entry
# point has one); REALW only through ig_ccsrmm_il_rw (no CONJ)
GATHER_V = ((2, 1, 8), (2, 2, 8), (4, 2, 8), (4, 4, 8), (4, 8, 8))
GATHER_V_ROWPERM = ((4, 16, 4),)
GATHER_V_REALW = ((2, 1, 8), (2, 2, 8), (4, 2, 8))
# k_csrmm_rowlane<NC, CONJ, BMODE, PACKED, U, BUF> as (NC, (BMODE, PACKED, U, BUF)): with beta == 0 a packed panel of 1, 2, 4 or 8 columns
# goes to k_csrmm_dense64 instead, so NC = 1 and 2 have no packed beta == 0 form
ROWLANE = ((1, (1, True, 1, False)),
           (2, (1, True, 1, False)), (2, (0, False, 1, False)), (2, (1, False, 1, False)),
           (4, (0, True, 2, True)), (4, (1, True, 1, False)), (4, (0, False, 1, False)), (4, (1, False, 1, False)),
           (8, (0, True, 2, True)), (8, (1, True, 1, False)), (8, (0, False, 1, False)), (8, (1, False, 1, False)))
# k_csrmm_dense64<NC, CONJ, YIL>: YIL only through ig_ccsrmm_t_grid_il (CONJ, 2 / 4 / 8 columns)
DENSE64 = tuple((nc, conj, False) for nc in (1, 2, 4, 8) for conj in FT) + tuple((nc, True, True) for nc in (2, 4, 8))
ALL_CL = (1, 2, 4, 8, 16, 32, 64)

EXPECTED_MAIN = set(
    [('gather', cl, nl, conj, bm) for cl, nl in GATHER for conj in FT for bm in (0, 1)] +
    [('gather_v', vw, clv, nl, conj, bm, False) for vw, clv, nl in GATHER_V for conj in FT for bm in (0, 1)] +
    [('gather_v', vw, clv, nl, False, bm, False) for vw, clv, nl in GATHER_V_ROWPERM for bm in (0, 1)] +
    [('gather_v', vw, clv, nl, False, bm, True) for vw, clv, nl in GATHER_V_REALW for bm in (0, 1)] +
    [('gather_tile64', conj, bm, 4) for conj in FT for bm in (0, 1)] +
    [('rowlane', nc, conj) + var for nc, var in ROWLANE for conj in FT] +
    [('dense64',) + a for a in DENSE64] +
    [('rowtile64', conj, bm) for conj in FT for bm in (0, 1)])
EXPECTED_DEFERRED = set((k, cl, conj, bm) for k in ('rows_wave', 'rows_block') for cl in ALL_CL for conj in FT for bm in (0, 1))
EXPECTED_SCATTER = set(('scatter', cl, nl, atomic) for cl, nl in
                       ((1, 1), (1, 4), (1, 64), (2, 1), (4, 1), (4, 4), (4, 16), (8, 1), (8, 4), (8, 8), (64, 1)) for atomic in FT)

# Instantiated, but nothing reaches them (listed in DESIGN.md 3.2):
#   k_csrmm_gather_v<4, {4, 8, 16}, 1>   the "short rows" arm of the IG_GV table: both ways into that block need nnz >= 8 rows
#   k_csrmm_gather_v<8, 1, 8>, <2, 4, 8>  the other arms of the compile-time vw (= 4)
#   k_csrmm_gather<CL, NL> for the other 14 pairs with CL NL <= 64: NL < 4 needs <= 2 nonzeros per row (row-per-lane kernels), NL = 16 / 32
#                                         below the cap of the wave needs a mean in (8, 32], which pick_shape holds at NL_CAP
#   k_csrmm_rowlane<NC, ., 0, true, 1, false>   packed, beta == 0 without buffer loads: an array beyond 2 GB (NC = 1: dense64 takes the rest)
#   k_csrmm_rowlane<2, ., 0, true, 2, true>     2 packed columns with beta == 0 are k_csrmm_dense64<2>
GATHER_UNREACHED = sorted(set((cl, nl) for cl in ALL_CL for nl in ALL_CL if cl * nl <= 64) - set(GATHER))


def table_dispatches():
    for c in CASES:
        lens = s.case_lens(c)
        nnz = int(lens.sum())
        for beta in s.betas_of(c):
            yield c, lens, beta, s.dispatch(c.entry, lens.size, nnz + 13 if c.big_x else 97, c.N, nnz, beta == 0)


def test_table_reaches_every_reachable_kernel():
    main, deferred = set(), set()
    for c, lens, beta, d in table_dispatches():
        assert d['error'] is None and d['main'] is not None, c
        assert c.want == '' or d['main'][0] in c.want.split('|'), (c, d['main'])
        main.add(d['main'])
        n = s.deferral(d, np.concatenate([[0], np.cumsum(lens)]))
        assert n['wave_inline'] == 0 and n['block_inline'] == 0
        for k in d['deferred']:
            if n['wave' if k[0] == 'rows_wave' else 'block'] > 0:
                deferred.add(k)
        if not any(k[0] == 'rows_wave' for k in d['deferred']):
            assert n['wave'] == 0, (c, "rows on a list nobody serves")
    assert main == EXPECTED_MAIN, (sorted(main - EXPECTED_MAIN, key=str), sorted(EXPECTED_MAIN - main, key=str))
    assert deferred == EXPECTED_DEFERRED, sorted(EXPECTED_DEFERRED ^ deferred, key=str)
    assert {k[0] for k in main} == {'gather', 'gather_v', 'gather_tile64', 'rowlane', 'dense64', 'rowtile64'}
    assert len(GATHER_UNREACHED) == 14


def test_a_sweep_of_the_mirror_finds_nothing_the_table_misses():
    """every (kernel, arguments) the mirror returns over a grid of entry points, column counts, row counts, mean row lengths, panel
    sizes and betas is in the literal list: the table is complete, and the short-rows arm of the IG_GV table is never taken"""
    seen = set()
    for entry in s.ENTRIES:
        for N in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 64, 65, 130):
            if (entry == 'xrows' and not 2 <= N <= 64) or (entry in ('il', 'il_rw') and (N & (N - 1) or N > 64)) or \
                    (entry == 't_grid_il' and N not in (2, 4, 8)):
                continue
            for rows, mean in itertools.product((1, 100, 1000, 99991), (0, 0.5, 1.9, 2.0, 2.01, 2.5, 3.5, 4.5, 7.9, 8, 8.1, 12, 31, 32, 33, 100, 600)):
                nnz = int(rows * mean)
                for xrows, b0 in itertools.product((10, nnz + 1), FT):
                    if entry == 't_grid_il' and not b0:
                        continue
                    d = s.dispatch(entry, rows, xrows, N, nnz, b0)
                    if d['main']:
                        seen.add(d['main'])
    assert seen == EXPECTED_MAIN, (sorted(seen - EXPECTED_MAIN, key=str), sorted(EXPECTED_MAIN - seen, key=str))
    assert not any(k[0] == 'gather_v' and k[3] == 1 for k in seen)


def test_alignment_only_matters_for_an_interleaved_panel():
    """(X & 15) == 0 in launch_gather: a column-major panel is either repacked (the copy is aligned) or not row-major at all, so only
    a caller of ig_ccsrmm_il could hand over a row-major panel that is 8-byte aligned only; the generic kernel takes it then"""
    for entry, N in itertools.product(('ccsrmm', 'ccsrmm_t', 'rowperm'), (1, 2, 8, 16, 64)):
        for rows, nnz, xrows in ((1000, 12000, 97), (1000, 12000, 20000), (1000, 900, 97)):
            assert s.dispatch(entry, rows, xrows, N, nnz, True, x_aligned=False)['main'] == s.dispatch(entry, rows, xrows, N, nnz, True)['main']
    assert s.dispatch('il', 1000, 97, 8, 12000, True, x_aligned=False)['main'] == ('gather', 8, 8, False, 0)
    assert s.dispatch('il', 1000, 97, 8, 12000, True, x_aligned=True)['main'] == ('gather_v', 4, 2, 8, False, 0, False)


@pytest.mark.parametrize("case", [c for c in CASES if c.lens_fixed is None], ids=repr)
def test_every_case_sits_on_its_seams(case):
    lens = s.case_lens(case)
    rows, nnz, have = lens.size, int(lens.sum()), set(lens.tolist())
    assert rows % 2 == 1 and rows % 64 == 37                                 # partial last wave, 64-row tile and workgroup
    fill, target = s.REGIMES[case.regime]
    assert {'sparse': nnz <= 2 * rows, 'mid3': 3 * rows < nnz <= 4 * rows, 'mid': 2 * rows < nnz < 8 * rows,
            'dense': 8 * rows <= nnz <= 32 * rows, 'vdense': nnz > 32 * rows}[case.regime], (rows, nnz)
    assert case.big_x or nnz >= 97                                           # which side of nnz >= xrows (big_x: nnz + 13 panel rows)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    for beta in s.betas_of(case):
        d = s.dispatch(case.entry, rows, nnz + 13 if case.big_x else 97, case.N, nnz, beta == 0)
        missing = [v for v in s.seam_lengths(d) if v not in have]
        assert not missing, (d['main'], missing)
        for t in d['trips']:
            assert {t - 1, t, t + 1} <= have
        n = s.deferral(d, indptr)
        lim = d['t_inline']
        assert n['block'] == int((lens > d['thr_long']).sum()) >= 7           # thr_long + 1 and the six tail seams
        if lim is not None and lim < d['thr_long']:
            assert any(k[0] == 'rows_wave' for k in d['deferred'])
            assert n['wave'] == int(((lens > lim) & (lens <= d['thr_long'])).sum()) >= 2
            assert {lim, lim + 1, d['thr_long'], d['thr_long'] + 1} <= have
        else:
            assert n['wave'] == 0
    # the long rows: one first, one last, two adjacent inside one 64-row tile (and one wave of every kernel that has several rows a wave)
    order = sorted(have, reverse=True)
    mid = (rows // 2) // 64 * 64 + 5
    assert [lens[0], lens[-1], lens[mid], lens[mid + 1]] == order[:4] and mid // 64 == (mid + 1) // 64 and mid % 2 == 1 or rows < 8


def test_column_counts_and_small_matrices_of_the_issue_are_in_the_table():
    by = lambda f: {c.N for c in CASES if f(c)}
    assert by(lambda c: True) >= {1, 2, 3, 4, 8, 16, 32, 64, 65, 130}
    assert by(lambda c: c.entry == 'il_rw' and c.regime == 'dense') >= {2, 4, 8}
    assert any(c.N == 3 and c.big_x for c in CASES) and any(c.N == 3 and not c.big_x for c in CASES)
    tags = {c.name.rsplit('-', 1)[-1] for c in CASES if c.lens_fixed is not None}
    assert tags == {'onerow0', 'onerow1', 'onerow29', 'empty', 'single'}
    for c in CASES:
        if c.entry == 'il_rw' and c.regime == 'dense' and c.N in (2, 4):       # a real-weight row deferred past thr_mid
            lens = s.case_lens(c)
            d = s.dispatch(c.entry, lens.size, 97, c.N, int(lens.sum()), True)
            assert d['main'][-1] is True and s.deferral(d, np.concatenate([[0], np.cumsum(lens)]))['wave'] > 0


# =========================================================================================================================================
# the mirror against the sources
# =========================================================================================================================================
def test_the_mirror_holds_the_constants_of_the_sources():
    src = open(os.path.join(CSRC, "ig_spmm.hip")).read()
    common = open(os.path.join(CSRC, "ig_spmm_common.h")).read()

    def one(pattern, text=src):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    assert int(one(r"constexpr int BLK = (\d+);", common)) == s.BLK
    assert one(r"constexpr int WAVES_PER_BLOCK = (.+?);", common) == "BLK / 64" and s.WAVES_PER_BLOCK == s.BLK // 64
    assert int(one(r"constexpr int WL_SUB = (\d+);")) == s.WL_SUB
    assert 1 << int(one(r"constexpr uint32_t WL_CAP = 1u << (\d+);")) == s.WL_CAP
    assert one(r"wl\.cap = (.+?);") == "WL_CAP / WL_SUB" and s.SUB_CAP == s.WL_CAP // s.WL_SUB == 32768
    assert one(r"const bool defer = (\w+);") == "true"
    assert one(r"const int nlw = (.+?);") == "64 / s.CL"
    assert int(one(r"const int32_t thr_long = defer \? (\d+) \* nlw : 0x7fffffff;")) == s.THR_LONG_PER_LANE
    assert int(one(r"const int32_t thr_mid = !defer \? 0x7fffffff : \(nlw > s\.NL \? (\d+) \* s\.NL : thr_long\);")) == s.THR_MID_PER_LANE
    assert int(one(r"constexpr int nl_cap = (\d+);")) == s.NL_CAP
    assert one(r"if \(nl_cap > 0 && mean <= (.+?) && cap > nl_cap\) cap = nl_cap;") == "4 * nl_cap"
    assert int(one(r"constexpr int vw = (\d+);")) == s.VW
    assert int(one(r"constexpr int dense_thr = (\d+);")) == s.DENSE_THR
    assert one(r"const int32_t td = defer \? \((.+?)\) : 0x7fffffff;") == "thr_long < dense_thr ? thr_long : dense_thr"
    assert tuple(int(v) for v in one(r"const int32_t tm_want = nnz <= 2 \* rows \? (\d+) : (\d+);")) == (s.TM_SPARSE, s.TM_WIDE)
    assert one(r"const int32_t tm = defer \? \((.+?)\) : 0x7fffffff;") == "thr_long < tm_want ? thr_long : tm_want"
    assert one(r"const int32_t tt = defer \? \((.+?)\) : 0x7fffffff;") == "thr_long < %d ? thr_long : %d" % (s.TM_WIDE, s.TM_WIDE)
    assert int(one(r"constexpr int TLD = 65, U = (\d+), RPW = 64 / NW;")) == s.TILE64_U
    assert int(one(r"constexpr int UT = (\d+);")) == s.ROWTILE_UT
    # the conditions of the decision tree, as written
    for text in ("const bool wide_v = vw > 0 && packed && sxc == 1 && N == sxr && (N == 64 || N == 32 || N == 16) && !y_il &&",
                 "nnz >= 8 * rows && (reinterpret_cast<uintptr_t>(X) & 15u) == 0;",
                 "const bool rowlane = !wide_v && (nnz <= 2 * rows || (packed && N >= 16 && nnz <= 8 * rows));",
                 "if (!x_il && ((N >= 2 && N <= 64 && nnz >= xrows) || (xperm && N <= 64))) {",
                 "if (packed && sxc == 1 && N == 64 && sxr == 64 && !y_il && !mask.bits) {",
                 "if (dense_thr > 0 && packed && b0 && bufok && nnz <= 2 * rows && N == sxr && (sxr == 8 || sxr == 4 || sxr == 2 || sxr == 1)) {",
                 "if (wide_v || (vw > 0 && packed && sxc == 1 && N == sxr && (N == 8 || N == 4 || N == 2) &&",
                 "if (thr_mid < thr_long || rowlane) {",
                 "if (s.CL >= 8) IG_ROWLANE(8);",
                 "for (; p + 3 * NLW < p1; p += 4 * NLW) {", "for (; p + 3 * NLB < p1; p += 4 * NLB) {",
                 "constexpr int NLW = 64 / CL;", "constexpr int NLB = 1024 / CL;",
                 "for (int32_t p = p0 + i; p < p1; p += 4 * NL) {"):
        assert text in src, text
    # the IG_GV table: every instantiation it names, reached or not
    gv = sorted(set(tuple(int(v) for v in m) for m in re.findall(r"IG_GV\((\d+), (\d+), (\d+)\);", src)))
    gvr = sorted(set(tuple(int(v) for v in m) for m in re.findall(r"IG_GVR\((\d+), (\d+), (\d+)\);", src)))
    short_arm, other_vw = [(4, 4, 1), (4, 8, 1), (4, 16, 1)], [(8, 1, 8), (2, 4, 8)]
    assert gv == sorted(list(GATHER_V) + list(GATHER_V_ROWPERM) + short_arm + other_vw), gv
    assert gvr == sorted(GATHER_V_REALW), gvr
    # the profiling scopes bench.py keys on
    for name in ('"csrmm_rowlane_conj" : "csrmm_rowlane"', '"csrmm_gather_conj" : "csrmm_gather"', '"csrmm_rows_wave"', '"csrmm_rows_block"',
                 '"csrmm_scatter_atomic" : "csrmm_scatter_exwrite"', '"panel_scale"', '"pack_panel"'):
        assert name in src, name


def test_the_full_sub_list_case_overflows_one_sub_list_by_64_rows():
    lens = s.overflow_lens()
    rows, nnz = lens.size, int(lens.sum())
    assert 1.04e6 < rows < 1.06e6 and nnz <= 2 * rows and rows % 64 == 37
    indptr = np.concatenate([[0], np.cumsum(lens)])
    for beta, main in ((0, ('dense64', 1, True, False)), (BETA, ('rowlane', 1, True, 1, True, 1, False))):
        d = s.dispatch('ccsrmm_t', rows, 97, 1, nnz, beta == 0)
        assert d['main'] == main and d['t_inline'] == (32 if beta == 0 else 16)
        n = s.deferral(d, indptr)
        assert n == dict(wave=s.SUB_CAP, wave_inline=64, block=0, block_inline=0), n
        assert int((lens > d['t_inline']).sum()) == s.SUB_CAP + 64 == 513 * 64
        assert set(s.sub_list(d, np.flatnonzero(lens)).tolist()) == {0}


# =========================================================================================================================================
# the exact inputs are exact
# =========================================================================================================================================
def lane_orders(case, lens, nnz):
    """(lanes, reverse, min_len, max_len): one after the other, last first, and dealt to the NL nonzero lanes of the row-slot kernels, the
    NLW = 64 / CL of k_csrmm_rows_wave and the NLB = 1024 / CL of k_csrmm_rows_block (the long rows only), folded pairwise"""
    CL, NL = s.pick_shape(lens.size, case.N, nnz)
    out = [(1, False, 0, 4200), (1, True, 0, 4200), (NL, False, 0, None), (64 // CL, True, 0, None), (1024 // CL, False, 65, None)]
    return sorted(set(out), key=str)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_exact_inputs_have_no_rounding_in_any_order(case):
    D = s.build(case)
    Xs = D.X if D.xlist is None else D.X[D.xlist]
    for a in (D.vals, D.X, D.Y0):
        parts = a.view(np.float32)
        assert np.all(parts == np.round(parts)) and np.all(np.abs(parts) <= s.VMAX)
    assert np.all(D.X.view(np.float32) != 0) and np.all(D.vals.real != 0)
    assert np.all(D.vals.imag == 0) if s.ENTRIES[case.entry].get('rvals') else np.all(D.vals.imag != 0)
    # 1. the bound next to the generator: the sum of the magnitudes of a row's products stays below 2^24, so every partial sum of any
    #    subset in any order is an integer float32 holds
    l1 = lambda z: np.abs(z.real) + np.abs(z.imag)
    lens = np.diff(D.indptr.astype(np.int64))
    assert 2 * s.VMAX * s.VMAX * max(int(lens.max()), 1) < 2 ** 20
    mags = s.spp.csr_matrix((l1(D.vals.astype(C128)), D.colind, D.indptr), shape=(D.rows, D.nx)) @ l1(Xs.astype(C128))
    assert mags.max(initial=0.0) < s.EXACT_LIMIT / 16
    prod = s.csr_of(D) @ Xs.astype(C128)
    assert s.is_f32(prod)
    for beta in s.betas_of(case):
        ref = s.gather_reference(D, ALPHA, beta)
        assert s.is_f32(ref)
        # the epilogue in float32 operations gives the reference's bits
        if D.yperm is None:
            eq(s.finish_f32(prod.astype(C64), D.Y0, ALPHA, beta), ref.astype(C64))
        else:
            eq(s.finish_f32(prod.astype(C64), D.Y0[D.yperm], ALPHA, beta), ref.astype(C64)[D.yperm])
    # 2. float32 accumulations in several lane mappings, first and last column
    cols = sorted({0, D.N - 1})
    want = prod[:, cols].astype(C64)
    for lanes, reverse, lo, hi in lane_orders(case, lens, D.nnz):
        got = s.emulate_rows(D, cols, lanes=lanes, reverse=reverse, min_len=lo, max_len=hi)
        done = ~np.isnan(got.real)
        assert done.any() or lo > 0 or D.rows == 0
        eq(got[done], want[done])


@pytest.mark.parametrize("spec", s.SCATTER_CASES, ids=repr)
@pytest.mark.parametrize("exwrite", FT)
def test_exact_scatter_inputs_have_no_rounding_in_a_random_order(spec, exwrite):
    """k_panel_scale, then conj(v) (alpha x) added to Y one nonzero at a time in a random order, all in float32 operations"""
    N, mean, M = spec
    A, X, Y0 = s.scatter_case(N, mean, M, exwrite)
    if exwrite:
        assert np.bincount(A.indices, minlength=A.shape[1]).max(initial=0) <= 1
    rng = np.random.default_rng(5)
    for beta in (0, BETA):
        ref = s.scatter_reference(A, X, Y0, ALPHA, beta)
        assert s.is_f32(ref)
        y = s.finish_f32(np.zeros_like(Y0), Y0, 0, beta)
        yr, yi = y.real.copy(), y.imag.copy()
        ax = s.finish_f32(X, X, ALPHA, 0)
        row = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        order = rng.permutation(A.nnz)
        vr, vi = A.data.real[order, None], A.data.imag[order, None]
        xr, xi = ax.real[row[order]], ax.imag[row[order]]
        np.add.at(yr, A.indices[order], vr * xr + vi * xi)
        np.add.at(yi, A.indices[order], vr * xi - vi * xr)
        assert yr.dtype == np.float32
        eq(yr + 1j * yi, ref.astype(C64))


def test_scatter_cases_reach_the_scatter_shapes():
    seen, pre = set(), set()
    for (N, mean, M), exwrite, beta in itertools.product(s.SCATTER_CASES, FT, (0, BETA)):
        A, X, Y0 = s.scatter_case(N, mean, M, exwrite)
        p, k = s.scatter_dispatch(M, N, A.nnz, beta, exwrite, A.shape[1] + 3, A.shape[1])
        pre.add(p)
        if k:
            seen.add(k)
    assert seen == EXPECTED_SCATTER, sorted(seen ^ EXPECTED_SCATTER, key=str)
    assert pre == {('panel_scale', True), ('panel_scale', False)}


# =========================================================================================================================================
# the rounding bound
# =========================================================================================================================================
@pytest.mark.parametrize("case", s.ROUNDING_CASES, ids=repr)
def test_float32_emulations_keep_within_the_rounding_bound(case):
    D = s.build(case, False)
    lens = np.diff(D.indptr.astype(np.int64))
    cols = sorted({0, D.N - 1})
    pos = np.arange(D.rows) if D.yperm is None else D.yperm.astype(np.int64)
    worst = 0.0
    for beta in s.betas_of(case):
        ref, bound = s.gather_reference(D, ALPHA, beta)[pos][:, cols], s.gather_bound(D, ALPHA, beta)[pos][:, cols]
        for lanes, reverse, lo, hi in lane_orders(case, lens, D.nnz):
            acc = s.emulate_rows(D, cols, lanes=lanes, reverse=reverse, min_len=lo, max_len=hi)
            done = ~np.isnan(acc.real)
            got = s.finish_f32(np.where(done, acc, 0), D.Y0[pos][:, cols], ALPHA, beta).astype(C128)
            err = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
            assert np.all(err[done] <= bound[done])
            worst = max(worst, float((err[done] / np.maximum(bound[done], 1e-300)).max(initial=0.0)))
    assert worst < 1.0
    print("%s: largest error / bound = %.3f" % (case, worst))
