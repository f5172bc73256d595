"""The brick scatter k_grid_bricks (ig_ccsrmm_t_bricks) at the sizes where its lane roles can go wrong.

The 8-coil kernel hands entries and panel rows from the loading lanes to the accumulating lanes in registers (DPP row broadcasts and
the half/row swaps of gfx950); the 4-coil kernel keeps ds_bpermute.  A wrong lane in either shows as a wrong cell, a wrong coil or a
wrong sample, so every case is checked three ways:

  * against conj(G)^T K formed with scipy in complex128, by the comparisons and bounds of tests/stress_adjoint.py: relative 2-norm
    error <= 1e-7 over the bricks one task owns, largest deviation <= 2e-6 of the grid's largest value on bricks whose pieces add
    with float atomics;
  * the grid is poisoned with NaN beforehand and every unflagged segment must still be NaN;
  * bit for bit against the output of the kernel before the register hand-off, on the cases without a shared brick (plain stores in
    a fixed order: a deviation is a wrong lane, not rounding).  Those outputs are fixtures under tests/golden/bricks_handoff_*.npy:
    the whole grid for the headline instantiation <8, 8, true, true>, and for the other cases one 64-bit digest per grid cell over
    its 2 x NC words (the fixtures stay under a quarter of a megabyte).  They were written ONCE, with the library built from the
    parent commit, by

        python tests/test_hip_bricks_handoff.py --write-golden

The grid is 32 x 8 x 8 with about 250 samples of half-width 2 (3 taps on an axis where the coordinate is an integer, else 4); the
footprints wrap all three grid edges and thin out towards large kx and km (light bricks beside heavy ones), the plane ks = 6 and
the columns kx = 20..28 are never touched (unflagged segments).
test_cases_reach_the_edges_of_the_lane_roles (no GPU) asserts from the formats themselves that the cases contain what they are
there for: partial last super-trips down to one round, tasks shorter than a super-trip and longer than the four-set rotation, brick
boundaries at round 0, at round 7 and in between, runs of three and more bricks, shared pieces beside unshared runs, shares of two
rounds.  Panels of 16 columns have no brick format (set_grid_bricks takes 4 or 8) and so no path through this kernel."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as spp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from indigo_amd.util import rand64c  # noqa: E402

C64 = np.dtype('complex64')
GOLDEN = os.path.join(ROOT, "tests", "golden")
GRID = (32, 8, 8)                       # n0 (fastest), nm, ns
ALPHA = 0.5 - 0.25j

# name: panel width, real weights, kx points per support-table entry (None: no table), brick bm x bs, chunk, run, sample set,
#       the instantiation it runs, golden ('full' / 'digest' / None: a shared brick, not deterministic)
CASES = {
    "pair_real_runs":      dict(nc=8, real=True,  tile=4,    bm=2, bs=2, chunk=1 << 20, run=2048, blob=False, kernel="<8, 8, true, true>",   golden="full"),
    "pair_real_bricks":    dict(nc=8, real=True,  tile=4,    bm=2, bs=2, chunk=1 << 20, run=8,    blob=False, kernel="<8, 8, true, true>",   golden="digest"),
    "pair_real_shared":    dict(nc=8, real=True,  tile=4,    bm=2, bs=2, chunk=256,     run=512,  blob=True,  kernel="<8, 8, true, true>",   golden=None),
    "pair_cplx_runs":      dict(nc=8, real=False, tile=4,    bm=2, bs=2, chunk=1 << 20, run=1024, blob=False, kernel="<8, 8, true, false>",  golden="digest"),
    "seg8_real_runs":      dict(nc=8, real=True,  tile=8,    bm=2, bs=2, chunk=1 << 20, run=1024, blob=False, kernel="<8, 8, false, true>",  golden="digest"),
    "seg4_cplx_runs":      dict(nc=8, real=False, tile=16,   bm=2, bs=2, chunk=1 << 20, run=512,  blob=False, kernel="<8, 4, false, false>", golden="digest"),
    "generic_real_runs":   dict(nc=8, real=True,  tile=8,    bm=1, bs=1, chunk=1 << 20, run=256,  blob=False, kernel="<8, 0, false, true>",  golden="digest"),
    "generic_cplx_shared": dict(nc=8, real=False, tile=None, bm=4, bs=4, chunk=1024,    run=4096, blob=True,  kernel="<8, 0, false, false>", golden=None),
    "nc4_real_runs":       dict(nc=4, real=True,  tile=16,   bm=2, bs=2, chunk=1 << 20, run=1024, blob=False, kernel="<4, 0, false, true>",  golden="digest"),
    "nc4_cplx_shared":     dict(nc=4, real=False, tile=8,    bm=2, bs=2, chunk=512,     run=256,  blob=True,  kernel="<4, 0, false, false>", golden=None),
}

_memo = {}


def gridding_matrix(blob, real):
    """(T x P csr, complex64) of samples with half-width-2 footprints on GRID: kx in [30, 50) mod 32, km anywhere, ks in [0, 4); every
    third kx, fifth km and seventh ks coordinate an integer (3 taps), the rest 4; `blob`: 60 % of the samples within one cell of a
    point (a heavy brick)"""
    key = ("A", blob, real)
    if key not in _memo:
        n0, nm, ns = GRID
        rng = np.random.default_rng(11 + blob)
        T = 250
        pos = np.stack([30 + 20 * rng.random(T) ** 2.5, nm * rng.random(T) ** 2, 4 * rng.random(T)], axis=1)
        if blob:
            heavy = rng.random(T) < 0.6
            pos[heavy] = np.array([37.3, 5.4, 1.6]) + rng.random((int(heavy.sum()), 3)) - 0.5
        pos[::3, 0] = np.floor(pos[::3, 0])
        pos[::5, 1] = np.floor(pos[::5, 1])
        pos[::7, 2] = np.floor(pos[::7, 2])
        rows, cols = [], []
        for t in range(T):
            ax = []
            for p, n in zip(pos[t], GRID):
                i = np.arange(int(np.floor(p)) - 2, int(np.floor(p)) + 3)
                ax.append(i[np.abs(i - p) < 2] % n)
            c = (ax[0][None, None, :] + n0 * (ax[1][None, :, None] + nm * ax[2][:, None, None])).reshape(-1)
            assert np.unique(c).size == c.size and c.size in (27, 36, 48, 64)
            rows.append(np.full(c.size, t)); cols.append(c)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        vals = rng.standard_normal(rows.size).astype(np.float32).astype(C64) if real else (rand64c(rows.size, seed=3) - (0.5 + 0.5j)).astype(C64)
        A = spp.csr_matrix((vals, (rows, cols)), shape=(T, n0 * nm * ns))
        A.sort_indices()
        _memo[key] = A
    return _memo[key]


def panel(nc):
    return rand64c(250, nc, seed=5)


def expected(blob, real, nc):
    """alpha conj(G)^T K in complex128, computed once per (matrix, panel width)"""
    key = ("E", blob, real, nc)
    if key not in _memo:
        A = gridding_matrix(blob, real)
        _memo[key] = ALPHA * (A.conj().T.astype(np.complex128) @ panel(nc).astype(np.complex128))
    return _memo[key]


def flagged_segments(A, tile):
    """seg[ks][km][kx tile]: the segments the matrix touches"""
    n0, nm, ns = GRID
    seg = np.zeros((ns, nm, n0 // tile), dtype=bool)
    uc = np.unique(A.indices)
    seg[uc // (n0 * nm), (uc // n0) % nm, (uc % n0) // tile] = True
    return seg


def host_format(name):
    from indigo_amd import grid_formats
    c = CASES[name]
    A = gridding_matrix(c['blob'], c['real'])
    return grid_formats.bricks(A.indptr, A.indices, A.data, *GRID, c['nc'], c['bm'], c['bs'], c['chunk'], c['run'],
                               tile=c['tile'] or 16, real_entries=c['real'])


def digest(out):
    """one uint64 per grid cell over the 2 x NC words of its panel row (odd multipliers, arithmetic modulo 2^64)"""
    w = np.ascontiguousarray(out).view(np.uint32).astype(np.uint64)
    mult = np.random.default_rng(99).integers(1, 2 ** 62, size=w.shape[1], dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return (w * mult[None, :]).sum(axis=1, dtype=np.uint64)


def scatter(hip, name):
    """the case's adjoint into a NaN-poisoned grid: (got (P, NC) row-major, segments flagged or None, cells of shared bricks)"""
    c = CASES[name]
    n0, nm, ns = GRID
    P, nc = n0 * nm * ns, c['nc']
    A = gridding_matrix(c['blob'], c['real'])
    A_d = hip.csr_matrix(hip, A)
    seg = None
    if c['tile']:
        from test_hip_operators import support_table_from_segments
        seg = flagged_segments(A, c['tile'])
        flat, _ = support_table_from_segments(seg)
        if c['tile'] == 16:
            A_d.set_grid_support(flat, n0, nm)
        else:
            A_d.set_grid_support_fine(flat, c['tile'])
    A_d.set_grid_interleaved(True)
    A_d.set_grid_bricks(n0, nm, ns, ncols=nc, bm=c['bm'], bs=c['bs'], chunk=c['chunk'], run=c['run'])
    f = A_d._bricks
    assert f is not None and f['words'] == (2 if c['real'] else 3) and A_d.adjoint_route(nc, 0, hip.zero_array((P, nc), C64)) == 'bricks'
    assert (f['nshared'] > 0) == (c['golden'] is None)
    y_d = hip.copy_array(np.full((P, nc), np.nan + 1j * np.nan, dtype=C64, order='F'))
    A_d.adjoint(y_d, hip.copy_array(panel(nc)), alpha=ALPHA)
    got = y_d.to_host().reshape(-1, order='F').reshape(P, nc)                     # row-major (interleaved) memory
    shared = np.zeros((ns, nm, n0), dtype=bool)
    if f['nshared']:
        sb = f['shared'].to_host()[:f['nshared']].astype(np.int64)
        nbx, nbm = n0 // 16, nm // c['bm']
        for b in sb:
            bx, bmi, bsi = b % nbx, (b // nbx) % nbm, b // (nbx * nbm)
            shared[bsi * c['bs']:(bsi + 1) * c['bs'], bmi * c['bm']:(bmi + 1) * c['bm'], bx * 16:(bx + 1) * 16] = True
    return got, seg, shared.reshape(-1)


def golden_path(name):
    return os.path.join(GOLDEN, "bricks_handoff_%s.npy" % name)


def scattered(hip, name):
    """scatter(), evaluated once per case and shared by the tests below"""
    if ("S", name) not in _memo:
        _memo[("S", name)] = scatter(hip, name)
    return _memo[("S", name)]


def inside_cells(c, got, seg):
    return np.ones(got.shape[0], dtype=bool) if seg is None else np.repeat(seg, c['tile'], axis=2).reshape(-1)


def errors(c, got, seg, shared):
    """(relative 2-norm error over the cells of owned bricks, largest deviation on shared bricks over the grid's largest value,
    the same largest-deviation figure on owned bricks -- printed only)"""
    exp = expected(c['blob'], c['real'], c['nc'])
    inside = inside_cells(c, got, seg)
    assert np.abs(exp[~inside]).max(initial=0.0) == 0
    own, sh, scale = inside & ~shared, inside & shared, np.abs(exp).max()
    e_own = np.linalg.norm((got[own] - exp[own]).ravel()) / np.linalg.norm(exp[own].ravel())
    e_sh = np.abs(got[sh] - exp[sh]).max(initial=0.0) / scale
    return e_own, e_sh, np.abs(got[own] - exp[own]).max() / scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_brick_scatter_writes_what_it_wrote_before_the_hand_off(hip, name):
    """unflagged segments still NaN; without a shared brick, bit for bit the output of the parent commit's kernel"""
    c = CASES[name]
    got, seg, shared = scattered(hip, name)
    inside = inside_cells(c, got, seg)
    if seg is not None:
        assert (~inside).any() and np.isnan(got[~inside].real).all() and np.isnan(got[~inside].imag).all(), "an unflagged segment was written"
    assert not np.isnan(got[inside].real).any() and not np.isnan(got[inside].imag).any(), "a flagged segment was not written"
    if c['golden']:
        ref = np.load(golden_path(name), allow_pickle=False)
        if c['golden'] == "full":
            bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1))
        else:
            bad = np.flatnonzero(digest(got) != ref)
        assert bad.size == 0, "%d cells differ bitwise from the kernel before the hand-off; first (kx, km, ks): %s" % (
            bad.size, [(int(p % GRID[0]), int(p // GRID[0] % GRID[1]), int(p // (GRID[0] * GRID[1]))) for p in bad[:6]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_brick_scatter_against_scipy(hip, name):
    """conj(G)^T K in complex128, by the two comparisons of tests/stress_adjoint.py: the relative 2-norm error over the cells of bricks
    one task owns (its comparison with scipy) <= 1e-7, the largest deviation on shared bricks over the grid's largest value (its bound
    on bricks whose pieces add with atomics) <= 2e-6.
    Measured on MI355X, parent commit and this kernel alike (the owned cells are bit-identical): see profiles/bricks_handoff_ab.txt."""
    c = CASES[name]
    got, seg, shared = scattered(hip, name)
    e_own, e_sh, m_own = errors(c, got, seg, shared)
    print("%s k_grid_bricks%s: owned bricks %.3e (2-norm; largest deviation %.3e of the grid's largest value), shared bricks %.3e"
          % (name, c['kernel'], e_own, m_own, e_sh))
    assert e_own <= 1e-7, e_own
    assert e_sh <= 2e-6, e_sh


def test_sixteen_columns_have_no_brick_format():
    """the brick format exists for panels of 4 and 8 columns only (ig_ccsrmm_t_bricks takes no other): 16 columns end on no path of
    k_grid_bricks, hand-off or not"""
    from indigo_amd import grid_formats
    A = gridding_matrix(False, True)
    with pytest.raises(AssertionError):
        grid_formats.bricks(A.indptr, A.indices, A.data, *GRID, 16, 2, 2)


def test_cases_reach_the_edges_of_the_lane_roles():
    """from the host formats alone (no GPU): what the cases above are there for is in them"""
    seen = set()
    for name, c in CASES.items():
        f = host_format(name)
        unit = 64 // c['nc']
        tasks, table, rounds = f['tasks'].reshape(-1, 4), f['table'].reshape(-1, 2), f['rounds']
        kinds = set()
        for lo, hi, bt, nbf in tasks[:f['ntasks']]:
            nent, nb, sh = int(hi - lo), int(nbf) & 0xffff, (int(nbf) >> 16) & 1
            assert nent > 0 and nent % unit == 0 and lo % unit == 0
            kinds.add('shared' if sh else 'owned')
            if nent % 64:
                seen.add((c['nc'], 'partial'))
            if nent % 64 == unit:
                seen.add((c['nc'], 'one round left'))
            if nent < 64:
                seen.add((c['nc'], 'short'))
            if nent > 4 * 64:
                seen.add((c['nc'], 'beyond the rotation'))
            if nb >= 3:
                seen.add((c['nc'], 'three bricks'))
            if not sh:
                for j in range(1, nb):
                    r = ((int(table[bt + j - 1, 1]) - int(lo)) // unit) % (64 // unit)
                    seen.add((c['nc'], 'boundary at round 0' if r == 0 else 'boundary at the last round' if r == 64 // unit - 1 else 'boundary inside'))
            # two rounds of one sample in one brick (a share of more than `unit` entries)
            r0 = rounds[lo // unit:hi // unit]
            if sh:
                if (r0[1:] == r0[:-1]).any():
                    seen.add((c['nc'], 'two rounds'))
            else:
                ends = set(((table[bt:bt + nb, 1] - lo) // unit).tolist())
                if any(r0[i] == r0[i - 1] and i not in ends for i in range(1, r0.size)):
                    seen.add((c['nc'], 'two rounds'))
        if c['golden'] is None:
            assert kinds == {'shared', 'owned'}, (name, kinds)
            seen.add((c['nc'], 'shared beside owned'))
        else:
            assert f['nshared'] == 0
    A = gridding_matrix(False, True)
    per_row = np.diff(A.indptr)
    assert {27, 36, 48, 64} <= set(per_row.tolist())                              # 3 and 4 taps on every axis
    kx = A.indices % GRID[0]
    assert {0, 31} <= set(kx.tolist()) and not (set(range(20, 29)) & set(kx.tolist())) and 6 not in set((A.indices // (GRID[0] * GRID[1])).tolist())
    want = {'partial', 'one round left', 'short', 'beyond the rotation', 'three bricks', 'boundary at round 0', 'boundary at the last round',
            'boundary inside', 'two rounds', 'shared beside owned'}
    for nc in (8, 4):               # (a 4-column round holds 16 entries, all a sample can leave in a 16 x 2 x 2 brick)
        need = want - ({'two rounds'} if nc == 4 else set())
        assert need <= {k for n, k in seen if n == nc}, (nc, sorted(need - {k for n, k in seen if n == nc}))


def _write_golden():
    from indigo_amd.backends import get_backend
    hip = get_backend("hip")
    os.makedirs(GOLDEN, exist_ok=True)
    for name, c in CASES.items():
        got, seg, shared = scatter(hip, name)
        print("%-20s owned %.3e (2-norm; largest deviation %.3e) shared %.3e" % ((name,) + tuple(np.array(errors(c, got, seg, shared))[[0, 2, 1]])), flush=True)
        if c['golden']:
            np.save(golden_path(name), got if c['golden'] == "full" else digest(got))


if __name__ == "__main__":
    if "--write-golden" in sys.argv:
        _write_golden()
