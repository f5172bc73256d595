"""What makes the comparisons of tests/test_hip_slots64.py legitimate, without a GPU: every case of tests/slots64.py holds the seams its
table entry claims (read from the slot format grid_formats.slots built, not from the recipe), the cases between them hold every seam
of k_grid_slots / k_grid_bricks_zero, the constants they are built on are the ones in the sources, the restatement taken from the
format equals scipy's conj(A)^T X, the float32 emulation that walks the format in the kernel's order gives it exactly on the exact
inputs, and the host builder ig_grid_slots_build does what the format promises on hand-made brick lists."""
import ctypes
import os
import re

import numpy as np
import pytest

import slots64 as w
from slots64 import ALPHA, C64, C128, SLOT_CASES

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "indigo_amd", "csrc")
FT = (False, True)
NCS = (1, 2, 4)
SENTINEL = 7 - 3j


def holds(claims, found):
    """the claims of a case that the format does not show"""
    return {k: (v, found[k]) for k, v in claims.items() if not (found[k] is True if v is True else v <= found[k])}


# =========================================================================================================================================
# the constants
# =========================================================================================================================================
def test_the_constants_are_the_ones_in_the_sources():
    spmm = open(os.path.join(CSRC, "ig_spmm.hip")).read()
    common = open(os.path.join(CSRC, "ig_spmm_common.h")).read()
    fmts = open(os.path.join(ROOT, "indigo_amd", "grid_formats.py")).read()
    from indigo_amd import grid_formats

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    kernel = spmm[spmm.index("\nk_grid_slots(const BrickTask"):spmm.index("\nk_grid_bricks_zero(const int32_t")]
    entry = spmm[spmm.index("\nint ig_ccsrmm_t_slots("):spmm.index("// ---- host-side structure analysis")]
    # the window of 63 slots: a window of 64 offsets, a slot needs its end too
    assert int(one(r"for \(int32_t base = 0; base < nslot; base \+= (\d+)\)", kernel)) == w.WINDOW
    assert one(r"cnt = left < (\d+) \? left : (\d+);", kernel) == (str(w.WINDOW),) * 2 and w.WINDOW == w.WAVE - 1
    assert one(r"if \(base \+ i >= cur_end\) (flush\(\));", kernel)
    assert int(one(r"cur_end = __builtin_amdgcn_readlane\(my_end, cur & (\d+)\);", kernel)) == w.WAVE - 1
    # the mask lookup: 8 passes of 64 pairs, and the brick cap that keeps a run inside them
    assert [int(v) for v in re.findall(r"for \(int p = 0; p < (\d+); \+\+p\)", kernel)] == [w.MASK_PASSES] * 2
    assert int(one(r"uint32_t w\[(\d+)\];", kernel)) == w.MASK_PASSES
    assert int(one(r"const int pair = p \* (\d+) \+ lane,", kernel)) == w.WAVE
    assert one(r"return min\((\d+), (\d+) // \(\(16 // tile\) \* bm \* bs\)\)", fmts) == (str(w.WAVE), str(w.MASK_PASSES * w.WAVE))
    for tile, bm, bs in ((16, 1, 1), (16, 2, 2), (4, 1, 1), (4, 2, 2), (8, 4, 4), (4, 2, 4), (8, 2, 4)):
        assert grid_formats._max_bricks(tile, bm, bs) == min(w.WAVE, w.MASK_PASSES * w.WAVE // ((16 // tile) * bm * bs))
    # the launch: four tasks per workgroup
    assert one(r"constexpr int WAVES_PER_BLOCK = (.+?);", common) == "BLK / 64" and int(one(r"constexpr int BLK = (\d+);", common)) == 64 * w.WAVES_PER_BLOCK
    assert one(r"const int task = blockIdx.x \* (\w+) \+ wv;", kernel) == "WAVES_PER_BLOCK"
    assert one(r"const unsigned blocks = \(unsigned\)\(\(ntasks \+ (\w+) - 1\) / \w+\);", entry) == "WAVES_PER_BLOCK"
    # the entries: 16 bytes {cell, re, im, row}, 12 bytes {cell, re, row}
    assert one(r"struct SlotEntry \{ (uint32_t cell; float re, im; uint32_t row;) \};", spmm)
    assert sorted(int(v) for v in re.findall(r"\(unsigned\)\(off \+ lane\) \* (\d+)u", kernel)) == sorted(w.ENTRY_BYTES.values())
    assert one(r"entry_words == (\d) \|\| entry_words == (\d), \"ig_ccsrmm_t_slots", entry) == ("4", "3") and w.ENTRY_BYTES == {4: 16, 3: 12}
    # at most 32 segments per brick: the bits of my_mask
    assert int(one(r"\(16 / support_tile\) \* bm \* bs <= (\d+), \"ig_ccsrmm_t_slots", entry)) == w.MAX_SEGMENTS
    assert one(r"IG_REQUIRE\(ctx, N == 1 \|\| N == 2 \|\| N == 4, \"(ig_ccsrmm_t_slots)", entry)


# =========================================================================================================================================
# the cases
# =========================================================================================================================================
@pytest.mark.parametrize("case", SLOT_CASES, ids=repr)
def test_slot_case(case):
    for real in FT:
        D = w.slot_data(case, real)
        fmt = D.fmt
        assert fmt['words'] == (3 if real else 4) and fmt['entries'].size == max(D.A.nnz, 1) * fmt['words'] and 4 * fmt['words'] == w.ENTRY_BYTES[fmt['words']]
        assert (fmt['bm'], fmt['bs']) == case.shape and case.nseg <= w.MAX_SEGMENTS
        assert (fmt['support'] is None) == (not case.table)
        n = int(w.hits(fmt).max())
        assert 32 * n < w.EXACT_LIMIT and n <= 1024 and D.M <= 320
        found = w.slot_seams(D)
        assert not holds(case.claims, found), (case, holds(case.claims, found))
        # the format keeps its promises: non-empty slots of at most 64 distinct cells (the emulation asserts the cells), tasks over
        # consecutive table rows that tile the slots, every brick of the table in exactly one owner or in shared pieces only
        per = np.diff(fmt['slot_ptr'])
        assert per.min() >= 1 and per.max() <= w.WAVE and fmt['slot_ptr'][0] == 0 and fmt['slot_ptr'][-1] == D.A.nnz
        tasks, table = w.slot_tasks(fmt)
        t = tasks[np.argsort(tasks[:, 0], kind='stable')]
        assert t[0, 0] == 0 and t[-1, 1] == fmt['nslots'] and np.array_equal(t[1:, 0], t[:-1, 1])
        assert all((nbf & 0xffff) <= w.max_bricks(case.tile, *case.shape) for nbf in tasks[:, 3])
        assert found['pairs'] <= w.MASK_PASSES * w.WAVE
        # the precondition: no nonzero weight in an unflagged segment (the zero weights there are the case's own)
        W = w.slot_walk(fmt)
        flags = w.cell_flags(fmt)
        assert not np.any(W.w[~flags[W.grid]]) and (np.count_nonzero(~flags[W.grid]) > 0) == bool(case.unflag)
        assert np.all(W.w[flags[W.grid]] != 0)
        # the format expands to the matrix, the restatement taken from it is scipy's product
        B, A0 = w.slot_csr(fmt, D.M), D.A.copy()
        A0.eliminate_zeros()
        assert (B != A0).nnz == 0 and B.nnz == A0.nnz
        mask = w.write_mask(fmt)
        assert mask.any() and (not mask.all() or case.name == 'entries')
        feeders = w.slot_feeders(fmt)
        assert sum(len(v) for v in feeders.values()) == D.A.nnz
        for nc in NCS:
            X = w.panel(D, nc)
            ref, m2 = w.slot_reference(fmt, X, ALPHA)
            assert np.array_equal(m2, mask) and w.is_f32(ref)
            sci = w.cf32(ALPHA) * (D.A.astype(C128).conj().T @ X.astype(C128))
            assert np.array_equal(ref[mask], sci[mask]) and not np.any(sci[~mask]), (case, real, nc)
            # the emulation in the kernel's order: the reference exactly, the caller's bytes elsewhere
            Y0 = np.full((D.K, nc), SENTINEL, dtype=C64)
            em = w.emulate_slots(fmt, X, ALPHA, Y0)
            assert np.array_equal(em[mask].astype(C128), ref[mask]), (case, real, nc)
            assert np.array_equal(em[~mask].view(np.uint32), Y0[~mask].view(np.uint32))
            assert not np.any(np.signbit(em[mask].real) & (em[mask].real == 0)) and not np.any(np.signbit(em[mask].imag) & (em[mask].imag == 0))


def test_the_table_holds_every_seam():
    """the seams of the issue's list, each read from some case's format, for real and complex entries alike"""
    for real in FT:
        u = {}
        for case in SLOT_CASES:
            for k, v in w.slot_seams(w.slot_data(case, real)).items():
                u[k] = u.get(k, set()) | v if isinstance(v, set) else max(u.get(k, 0), v)
        # the slot window
        assert {1, 2, 62, 63, 64, 126, 127} <= u['task_slots'] and u['boundary'] == {'first', 'last', 'middle'}
        # the entry and row lookahead
        assert {1, 2, w.WINDOW} <= u['window_cnt'] and {1, 63, 64} <= u['slot_entries'] and u['one_by_64'] and u['cut_64']
        assert u['sample_ends'] and u['cell_ends']
        # cell multiplicity
        assert {1, 2} <= u['mult'] and max(u['mult']) >= 200 and u['single_second_group']
        # brick runs and the mask lookup
        caps = {1: 64, 4: 64, 16: 32, 32: 16}
        for case in SLOT_CASES:
            if case.name.startswith('cap-'):
                s = w.slot_seams(w.slot_data(case, real))
                C = caps.pop(case.nseg)
                assert C == w.max_bricks(case.tile, *case.shape) and {C, C - 1} <= s['bricks_per_task']
                assert {(n, e, f) for n in (C, C - 1) for e in ('first', 'last') for f in FT} <= s['cap_flags'], case
                assert (s['pairs'] == C * case.nseg) and (case.nseg < 16 or s['pairs'] == w.MASK_PASSES * w.WAVE)
        assert not caps
        # the support tables
        assert u['tile_pts'] == {16, 8, 4} and {0, 1, 2, 3} <= u['zw_bit'] and u['nm_gt_zw'] and u['no_table']
        assert {c.zw for c in SLOT_CASES if c.table} >= {16, 4}
        assert any(c.zw == 16 and c.dims[1] > 16 for c in SLOT_CASES) and any(c.zw < 16 and c.dims[1] > c.zw for c in SLOT_CASES)
        assert u['partial_segment'] and u['unflagged_beside_flagged']
        # shared pieces, the launch tail
        assert u['shared'] and u['owned'] and max(u['pieces']) >= 3 and u['shared_unflagged'] and u['shared_partial'] and u['piece_of_one']
        assert u['ntasks_mod4'] and u['one_task']
    assert all(c.K <= 64 * 16 * 16 for c in SLOT_CASES) and sum(c.dims == w.DIMS for c in SLOT_CASES) >= 4
    assert all(c.dims == w.CAP_DIMS for c in SLOT_CASES if c.name.startswith('cap-')) and all(c.dims[1] < 32 or c.name == 'zw16-nm64' for c in SLOT_CASES)
    for name, fine in w.ROUTE_CASES:
        assert (w.SLOT_BY_NAME[name].tile < 16) == fine and w.SLOT_BY_NAME[name].zw == 16


def test_emulated_rounding_stays_inside_the_bound():
    case = w.SLOT_BY_NAME[w.SLOT_ROUNDING]
    for real in FT:
        D = w.slot_data(case, real, exact=False)
        for nc in NCS:
            X = w.panel(D, nc)
            ref, mask = w.slot_reference(D.fmt, X, ALPHA)
            em = w.emulate_slots(D.fmt, X, ALPHA, np.zeros((D.K, nc), dtype=C64))
            err, bound = np.abs(em.astype(C128) - ref)[mask], w.adjoint_bound(D.fmt, X, ALPHA)[mask]
            assert np.all(err[bound == 0] == 0)
            frac = float((err[bound > 0] / bound[bound > 0]).max())
            assert 0 < frac < 1, (real, nc, frac)


def test_cases_per_instantiation():
    """the counts the GPU file runs (printed with -s)"""
    print("k_grid_slots<NC, REALW>: %d exact cases and one rounding case for each of NC = 1, 2, 4 x real and complex entries; "
          "k_grid_bricks_zero<NC>: %d of them with shared bricks" % (len(SLOT_CASES), sum(w.slot_data(c).fmt['nshared'] > 0 for c in SLOT_CASES)))
    assert len(SLOT_CASES) >= 10 and sum(w.slot_data(c).fmt['nshared'] > 0 for c in SLOT_CASES) >= 6


# =========================================================================================================================================
# ig_grid_slots_build on hand-made brick lists
# =========================================================================================================================================
def build_slots(bricks, ncell, poison=0):
    """bricks: a list of lists of cells, in input order.  -> (rc, entries16 (n, 4), brick_slots, slot_ptr[:nslots + 1], nslots); the
    sample of an entry is its position in the input, its weight (position + 1, -position - 2)"""
    from indigo_amd import _lib
    nb = len(bricks)
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in bricks])]).astype(np.int64)
    n = int(ptr[-1])
    e12 = np.zeros((max(n, 1), 3), dtype=np.uint32)
    cells = np.asarray([c for b in bricks for c in b], dtype=np.uint32)
    e12[:n, 0] = cells
    e12[:n, 1] = (np.arange(n) + 1).astype(np.float32).view(np.uint32)
    e12[:n, 2] = (-np.arange(n) - 2).astype(np.float32).view(np.uint32)
    rows = np.arange(max(n, 1), dtype=np.uint32)
    e16 = np.full((max(n, 1), 4), poison, dtype=np.uint32)
    brick_slots = np.full(max(nb, 1), poison, dtype=np.int32)
    slot_ptr = np.full(n + 1, poison, dtype=np.int32)
    nslots = ctypes.c_int64(-1)
    rc = _lib.lib().ig_grid_slots_build(nb, ptr.ctypes.data, e12.ctypes.data, rows.ctypes.data, ncell, e16.ctypes.data, brick_slots.ctypes.data,
                                        slot_ptr.ctypes.data, ctypes.byref(nslots))
    return rc, e16[:n], brick_slots[:nb], slot_ptr[:max(int(nslots.value), 0) + 1], int(nslots.value)


def _hand_made_bricks():
    rng = np.random.default_rng(11)
    return [[],
            list(rng.permutation(256)[:130]) + [5, 5, 9, 200, 5],          # 130 distinct cells: 64 + 64 + 2, then later hits in input order
            [17],
            [],
            [3] * 5,
            list(rng.integers(0, 256, size=700)),                           # a random multiset: groups of every size
            list(range(64)) + [63],                                         # a group of exactly 64 and a group of one
            list(range(65)) * 2,                                            # two groups of 65: 64 + 1 each
            []]


def test_ig_grid_slots_build_groups_by_occurrence_in_input_order():
    bricks = _hand_made_bricks()
    rc, e16, brick_slots, slot_ptr, nslots = build_slots(bricks, 256)
    n = sum(len(b) for b in bricks)
    assert rc == 0 and nslots == brick_slots.sum() and slot_ptr[0] == 0 and slot_ptr[nslots] == n
    assert np.all(np.diff(slot_ptr) >= 1) and np.all(np.diff(slot_ptr) <= w.WAVE)
    p0, s0 = 0, 0
    for b, cells in enumerate(bricks):
        if not cells:
            assert brick_slots[b] == 0
            continue
        cells = np.asarray(cells)
        # the occurrence of every input entry: how many earlier entries of the brick name its cell
        occ = np.asarray([np.count_nonzero(cells[:i] == c) for i, c in enumerate(cells)])
        sizes = np.bincount(occ)
        assert brick_slots[b] == sum((g + 63) // 64 for g in sizes)
        out = e16[p0:p0 + cells.size]
        start = np.concatenate([[0], np.cumsum(sizes)])
        for k, g in enumerate(sizes):
            grp = out[start[k]:start[k + 1]]
            inp = np.flatnonzero(occ == k)                                  # the (k + 1)-th occurrence of each cell, input order
            assert np.array_equal(np.sort(grp[:, 3]), p0 + inp) and np.unique(grp[:, 0]).size == g
            assert np.array_equal(grp[:, 0], cells[grp[:, 3].astype(np.int64) - p0])
            assert np.array_equal(grp[:, 1].view(np.float32), grp[:, 3] + 1.0) and np.array_equal(grp[:, 2].view(np.float32), -(grp[:, 3] + 2.0))
            # its slots: contiguous, 64 entries each but the last, none across the group's end
            ns_g = (g + 63) // 64
            want = p0 + start[k] + 64 * np.arange(ns_g)
            assert np.array_equal(slot_ptr[s0:s0 + ns_g], want) and slot_ptr[s0 + ns_g] == p0 + start[k + 1]
            s0 += ns_g
        # a cell's entries keep their input order from group to group
        for c in np.unique(cells):
            where = np.flatnonzero(out[:, 0] == c)
            assert np.all(np.diff(out[where, 3].astype(np.int64)) > 0)
        p0 += cells.size
    assert s0 == nslots


def test_ig_grid_slots_build_edges_and_refusals():
    from indigo_amd import _lib
    rc, e16, brick_slots, slot_ptr, nslots = build_slots([[], [], []], 64)
    assert rc == 0 and nslots == 0 and not brick_slots.any() and slot_ptr[0] == 0
    rc, e16, brick_slots, slot_ptr, nslots = build_slots([[63]], 64)
    assert rc == 0 and nslots == 1 and list(slot_ptr) == [0, 1] and list(e16[0, [0, 3]]) == [63, 0]
    rc = build_slots([[1, 2], [0, 64, 3]], 64)[0]
    assert rc != 0 and "a cell index outside the brick" in _lib.last_error(None)
    rc = build_slots([[1, 0xffffffff]], 64)[0]                              # the padding cell of the round format is no slot entry
    assert rc != 0 and "a cell index outside the brick" in _lib.last_error(None)
    assert build_slots([[0]], 0)[0] != 0 and build_slots([[0]], 1025)[0] != 0 and build_slots([[1023]], 1024)[0] == 0


def test_ig_grid_slots_build_twice_gives_identical_bytes():
    bricks = _hand_made_bricks() * 40                                       # enough bricks for several host threads
    a, b = build_slots(bricks, 256, poison=0), build_slots(bricks, 256, poison=0x5a5a5a5a)
    assert a[0] == 0 and b[0] == 0 and a[4] == b[4]
    for x, y in zip(a[1:4], b[1:4]):
        assert x.tobytes() == y.tobytes()
