"""What makes the comparisons of tests/test_hip_wide64.py legitimate, without a GPU: the exact inputs of tests/wide64.py are exact in
float32 for every case, every case holds the seams its table entry claims (read from the host formats grid_formats.runs and
grid_formats.wide_bricks themselves), the constants the cases are built on are the ones in the sources, the float32 emulations that
walk the device formats in the kernels' order give the float64 reference element for element, the formats regroup into the CSR they
came from, and the host builders refuse what they document."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as spp

import wide64 as w
from wide64 import ALPHA, BETA, C64, C128, RUNS_CASES, WIDE_CASES

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "indigo_amd", "csrc")
FT = (False, True)


def holds(claims, found):
    """the claims of a case that the format does not show"""
    return {k: (v, found[k]) for k, v in claims.items() if not (found[k] is True if v is True else v <= found[k])}


# =========================================================================================================================================
# the constants
# =========================================================================================================================================
def test_the_constants_are_the_ones_in_the_sources():
    runs = open(os.path.join(CSRC, "ig_spmm_runs.hip")).read()
    bricks = open(os.path.join(CSRC, "ig_spmm_bricks.hip")).read()
    fmts = open(os.path.join(ROOT, "indigo_amd", "grid_formats.py")).read()

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    assert int(one(r"constexpr int RUN_ROWS = (\d+);", runs)) == w.RUN_ROWS
    assert int(one(r"uint32_t wr_\[(\d+)\];", runs)) == w.RING
    assert [int(v) for v in re.findall(r"static_for_runs<0, (\d+)>\((?:fill|step)\)", runs)] == [w.RING, w.RING]
    assert int(one(r"for \(int32_t d = 0; d < nd; d \+= (\d+)\)", runs)) == w.RING
    assert int(one(r"if \(ei >= (\d+)\) \{", runs)) == w.WINDOW
    assert int(one(r"const int avail = (\d+) - ei;", runs)) == w.WINDOW
    assert [int(v) for v in re.findall(r"prefetch_(?:entries|rows)\((\d+)\);", runs)] == [w.WINDOW, w.WINDOW]
    assert int(one(r"if \(since < (\d+)\) asm volatile\(\"s_waitcnt vmcnt\(0\)\"", runs)) == w.RING
    assert set(int(v) for v in re.findall(r"s_waitcnt vmcnt\((\d+)\)", runs)) == {0, w.RING - 1}
    assert int(one(r"int cnt = \(int\)\(w >> (\d+)\) \+ 1;", runs)) == w.COL_BITS
    assert int(one(r"if \(K > \(1LL << (\d+)\)\)", runs)) == w.COL_BITS
    assert int(one(r"constexpr int WIDE_LD = (\d+);", bricks)) == w.WIDE_LD
    assert one(r"constexpr int TRIP = (\d+), TQ = TRIP / 4;", bricks) == str(w.TRIP) and w.TQ == w.TRIP // 4
    assert one(r"constexpr int AHEAD = (TQ - 1);", bricks) and w.AHEAD == w.TQ - 1
    assert set(int(v) for v in re.findall(r"s_waitcnt vmcnt\((\d+)\)", bricks)) == {0, w.AHEAD}
    assert int(one(r"const int64_t r0 = \(int64_t\)blockIdx.x \* (\d+);", bricks)) == w.ZERO_BLOCK
    assert int(one(r"for \(int gi = 0; gi < ngroup; gi \+= (\d+)\)", bricks)) == w.ROTATION
    assert int(one(r"const int ngroup = \(nent \+ 3\) / (\d+);", bricks)) == w.GROUP
    assert int(one(r"cur_end = __builtin_amdgcn_readlane\(my_end, cur & (\d+)\);\n    \};\n    // quad k", bricks)) == w.MAX_BRICKS - 1
    assert int(one(r"tasks, table, shared = brick_tasks\(counts, ptr, chunk, run, max_bricks=(\d+), longest_first=True\)", fmts)) == w.MAX_BRICKS


# =========================================================================================================================================
# the forward cases
# =========================================================================================================================================
@pytest.mark.parametrize("case", RUNS_CASES, ids=repr)
def test_forward_case(case):
    for real in FT:
        D = w.runs_data(case, True, real)
        n = int(np.diff(D.indptr).max())
        assert 32 * n < w.EXACT_LIMIT and n <= 1024
        assert D.fmt['all_real'] == int(real or D.A.nnz == 0)
        assert not holds(case.claims, w.runs_seams(D)), (case, holds(case.claims, w.runs_seams(D)))
        assert (D.fmt['order'] is None) == (case.order == 'none' or len(case.runs) == 1)
        # the format regroups into the CSR
        B = w.runs_to_csr(D.fmt, D.indptr, D.M, w.NX)
        assert (B != D.A).nnz == 0 and B.nnz == D.A.nnz
        acc, _ = w.emulate_runs(D)
        for beta in (0, BETA):
            ref = w.forward_reference(D, ALPHA, beta)
            assert w.is_f32(ref)
            assert np.array_equal(w.finish_f32(acc, D.Y0, ALPHA, beta).astype(C128), ref), (case, real, beta)
    if D.A.nnz and len(case.runs) > 1:                     # panel row 0 and the last panel row are both used
        used = np.unique(D.A.indices)
        assert used[0] == 0 and used[-1] == w.NX - 1 and w.TOUCHED[0] == 0 and w.TOUCHED[-1] == w.XTOTAL - 1 and w.TOUCHED.size < w.XTOTAL


def test_forward_table_holds_every_seam():
    union = {}
    for case in RUNS_CASES:
        for k, v in w.runs_seams(w.runs_data(case)).items():
            union[k] = union.get(k, set()) | v if isinstance(v, set) else union.get(k, False) or v
    assert set(w.ND_SEAMS) <= union['nd'] and max(union['nd']) > 192
    assert set(w.NE_SEAMS) <= union['ne'] and max(union['ne']) >= 300
    assert set(w.CNT_SEAMS) <= union['cnt']
    assert {1, 15, 16, 17} <= union['m'] and {1, 15} <= union['m_mod16']
    assert {1, 2, 3} <= union['left_at_row_of_4'] and all(union[k] for k in
                                                          ('row_at_window_end', 'switch_inside_row', 'since_lt_16', 'since_ge_16',
                                                           'quad_path', 'single_path', 'empty_run', 'empty_rows', 'partial_block'))
    assert 0 in union['nnz']
    assert {c.order for c in RUNS_CASES} == {'none', 'perm', 'dims'}
    built = w.runs_data(w.RUNS_BY_NAME['windows']).fmt['order']
    assert np.array_equal(np.sort(built), np.arange(built.size)) and not np.array_equal(built, np.arange(built.size))


def test_emulated_rounding_stays_inside_the_forward_bound():
    for real in FT:
        D = w.runs_data(w.RUNS_BY_NAME[w.RUNS_ROUNDING], False, real)
        acc, _ = w.emulate_runs(D)
        for beta in (0, BETA):
            err = np.abs(w.finish_f32(acc, D.Y0, ALPHA, beta).astype(C128) - w.forward_reference(D, ALPHA, beta))
            frac = float((err / w.forward_bound(D, ALPHA, beta)).max())
            assert 0 < frac < 1, frac


def test_ig_csr_runs_build_refuses_what_it_documents():
    from indigo_amd import _lib, grid_formats
    L = _lib.lib()

    def build(M, K, indptr, colind):
        indptr, colind = np.asarray(indptr, dtype=np.int32), np.asarray(colind, dtype=np.int32)
        vals = np.ones(max(colind.size, 1), dtype=C64)
        dptr = np.zeros((M + 15) // 16 + 1, dtype=np.int32)
        rc = L.ig_csr_runs_build(M, K, indptr.ctypes.data, colind.ctypes.data, vals.ctypes.data, dptr.ctypes.data, None, None, None)
        return rc, _lib.last_error(None)
    assert build(2, 8, [0, 2, 3], [1, 5, 1])[0] == 0                       # the same column in two rows of a run: fine
    rc, msg = build(2, 8, [0, 2, 3], [5, 5, 1])
    assert rc != 0 and "holds a column twice" in msg
    rc, msg = build(2, 8, [0, 2, 3], [1, 8, 1])
    assert rc != 0 and "outside the matrix" in msg
    rc, msg = build(2, 8, [0, 2, 3], [1, -1, 1])
    assert rc != 0 and "outside the matrix" in msg
    assert build(1, 1 << 27, [0, 1], [(1 << 27) - 1])[0] == 0
    rc, msg = build(1, (1 << 27) + 1, [0, 1], [0])
    assert rc != 0 and "more than 27 bits" in msg
    ones = np.ones(3, dtype=C64)
    assert grid_formats.runs(np.array([0, 2, 3]), np.array([5, 5, 1]), ones, np.arange(8, dtype=np.int32)) is None


# =========================================================================================================================================
# the adjoint cases
# =========================================================================================================================================
@pytest.mark.parametrize("case", WIDE_CASES, ids=repr)
def test_adjoint_case(case):
    for real in FT:
        D = w.wide_data(case, True, real)
        assert D.fmt is not None
        n0, nm, ns = case.dims if case.dims is not None else (case.K, 1, 1)
        assert D.fmt['geom'] == (n0, nm) + case.shape and D.fmt['words'] == (2 if real and case.NT > 1 else 3)
        n = int(np.bincount(D.A.indices).max())
        assert 32 * n < w.EXACT_LIMIT and n <= 1024
        found = w.wide_seams(D)
        assert not holds(case.claims, found), (case, holds(case.claims, found))
        B = w.wide_to_csr(D)
        assert (B != D.A).nnz == 0 and B.nnz == D.A.nnz
        ref = w.adjoint_reference(D, ALPHA)
        assert w.is_f32(ref)
        untouched = np.setdiff1d(np.arange(D.K), D.A.indices)
        assert not np.any(ref[untouched])
        for aligned in FT:                                    # k_wide_zero_unowned by the bitmap / a memset of everything
            ev = {}
            assert np.array_equal(w.emulate_wide(D, ALPHA, y_aligned=aligned, events=ev).astype(C128), ref), (case, real, aligned)
        # every owned tile is stored exactly once, by a task that is not shared; no unowned tile is stored
        tasks, table = w.wide_tasks(D.fmt)
        stored = np.bincount([r0 // 16 for ti, cur, r0 in ev['stored'] if not tasks[ti, 3] >> 16], minlength=D.K // 16)
        assert np.array_equal(stored, w.owned_bits(D).astype(np.int64))
        assert all((tasks[:, 1] - tasks[:, 0]) % (4 if case.NT > 1 else 1) == 0) and all(tasks[:, 0] % (4 if case.NT > 1 else 1) == 0)


def test_adjoint_table_holds_every_seam():
    per = {}
    for case in WIDE_CASES:
        for real in FT:
            D = w.wide_data(case, True, real)
            s = w.wide_seams(D)
            u = per.setdefault((case.NT, real and case.NT > 1), dict(nent=set(), nquad=set(), boundary=set(), bricks=set(), pad=set(), taps=set(), shapes=set()))
            u['nent'] |= s['nent']; u['nquad'] |= s['nquad']; u['boundary'] |= s['boundary_quad']; u['bricks'] |= s['bricks_per_task']
            u['pad'] |= s['pad']; u['taps'] |= s['taps']; u['shapes'].add(case.shape)
    for NT in (2, 4):
        for real in FT:                                       # the four instantiations of k_bricks_wide64r
            u = per[(NT, real)]
            assert set(w.NENT_SEAMS) <= u['nent'] and max(u['nent']) >= 288, (NT, real)
            assert {1, w.AHEAD - 1, w.AHEAD, w.TQ, 2 * w.TQ, 2 * w.TQ + 1, 4 * w.TQ, 4 * w.TQ + 1, 5 * w.TQ} <= u['nquad']
            assert {0, w.AHEAD} <= u['boundary'] and u['boundary'] - {0, w.AHEAD}
            assert {1, 2, 3, w.MAX_BRICKS} <= u['bricks'] and u['pad'] == {0, 1, 2, 3}
    assert per[(2, False)]['shapes'] >= {(2, 1), (1, 2)} and per[(4, False)]['taps'] >= {27, 36, 48, 64}
    assert set(w.PLAIN_NENT) <= per[(1, False)]['nent'] and {1, 2, w.MAX_BRICKS} <= per[(1, False)]['bricks']
    # tiles 31 and 32 -- the last bit of a bitmap word and the first of the next -- with different owners
    assert any(w.owned_bits(w.wide_data(c))[31] != w.owned_bits(w.wide_data(c))[32] for c in WIDE_CASES if c.K >= 33 * 16)
    assert min(c.task for c in WIDE_CASES) == (4, 4)


def test_emulated_rounding_stays_inside_the_adjoint_bound():
    for name in w.WIDE_ROUNDING:
        for real in FT:
            D = w.wide_data(w.WIDE_BY_NAME[name], False, real)
            err = np.abs(w.emulate_wide(D, ALPHA).astype(C128) - w.adjoint_reference(D, ALPHA))
            bound = w.adjoint_bound(D, ALPHA)
            assert np.all(err[bound == 0] == 0)
            frac = float((err[bound > 0] / bound[bound > 0]).max())
            assert 0 < frac < 1, (name, real, frac)


def test_a_row_that_touches_more_than_64_bricks_has_no_wide_format():
    from indigo_amd import grid_formats
    K = 16 * 70
    for n, ok in ((64, True), (65, False)):
        cols = 16 * np.arange(n, dtype=np.int32) + 3
        A = spp.csr_matrix((np.ones(n, dtype=C64), cols, np.array([0, n], dtype=np.int32)), shape=(1, K))
        fmt = grid_formats.wide_bricks(A.indptr, A.indices, A.data, K)
        assert (fmt is not None) == ok


def test_cases_per_instantiation():
    """the counts the GPU file runs (printed with -s)"""
    print("k_csrmm_runs64r: %d exact cases for each of <0, false>, <0, true>, <1, false>, <1, true>" % len(RUNS_CASES))
    for NT in (2, 4):
        print("k_bricks_wide64r<%d, .>: %d exact cases for each of real and complex entries" % (NT, sum(c.NT == NT for c in WIDE_CASES)))
    print("k_bricks_wide64: %d exact case(s)" % sum(c.NT == 1 for c in WIDE_CASES))
    assert len(RUNS_CASES) >= 8 and all(sum(c.NT == NT for c in WIDE_CASES) >= 3 for NT in (2, 4))
