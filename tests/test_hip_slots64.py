"""The slot scatter of the adjoint gridding path -- k_grid_slots<NC, REALW> for NC = 1, 2, 4 with its zero-fill k_grid_bricks_zero<NC>
(ig_ccsrmm_t_slots) -- called through the C ABI on the formats grid_formats.slots builds, against the float64 restatement in
tests/slots64.py: every cell of the grid, every column.

Exact cases: the hand-built matrices of slots64.SLOT_CASES, whose seams tests/test_slots64_cpu.py reads back from the formats, on integer
inputs with a dyadic alpha where nothing rounds -- not the fused multiply-adds, not the read-add-writes of the image, not the float
atomics of shared pieces.  The device must give the reference by value in every cell of the write mask (the flagged segments of the
bricks of the table) and the float32 emulation of the kernel BIT FOR BIT on the bricks a task owns; every cell outside the write mask,
every guard item and the input panel must come back bit-identical.  The grid lies between guard items and starts as a NaN pattern (as
zeros where `support` is NULL: the caller zeroes it then).  A failure names the case, what it was built for and the first wrong cells
as (kx, km, ks, column) with the (task, brick, slot, lane, sample) that feed them.

Rounding cases: one uniform-random case per instantiation inside the derived worst case of slots64.adjoint_bound; the largest
fraction of the bound reached is printed."""
import ctypes

import numpy as np
import pytest

import slots64 as w
from slots64 import ALPHA, C64, C128, SLOT_CASES

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
NAN32 = 0x7fc0dead                  # the sentinel: a quiet NaN that any arithmetic would also spread into the results
GUARD = 8                           # sentinel items on either side
FT = (False, True)
NCS = (1, 2, 4)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Guarded:
    """n complex64 items on the device between sentinels; view(host) is the payload inside a host image of the whole allocation"""

    def __init__(self, hip, n, view, data=None):
        self.n, self._view = n, view
        host = np.empty(GUARD + n + GUARD, dtype=C64)
        bits(host)[:] = NAN32
        if data is not None:
            self.payload(host)[...] = data
        self.before = host
        self.dev = hip.copy_array(host)
        self.ptr = VP(self.dev._arr + 8 * GUARD)

    def payload(self, host):
        return self._view(host[GUARD:GUARD + self.n])

    def read(self):
        """the payload; the guards (and what the view leaves out: padding rows) must be bit-identical"""
        h = self.dev.to_host()
        keep = np.ones(h.size, dtype=bool)
        keep[self.payload(np.arange(h.size)).reshape(-1)] = False
        assert np.array_equal(bits(h)[np.repeat(keep, 2)], bits(self.before)[np.repeat(keep, 2)]), "a guard item or a padding row was overwritten"
        return self.payload(h).copy()

    def untouched(self):
        return np.array_equal(bits(self.dev.to_host()), bits(self.before))


def grid_panel(hip, K, nc, data=None):
    """the result: K grid rows of nc interleaved columns"""
    return Guarded(hip, K * nc, lambda a: a.reshape(K, nc), data)


def x_panel(hip, X, pad=3):
    """the input: column-major (M, nc) with `pad` sentinel rows below every column (ldx = M + pad > M)"""
    M, nc = X.shape
    p = Guarded(hip, (M + pad) * nc, lambda a: a.reshape(nc, M + pad).T[:M], X)
    p.ld = M + pad
    return p


def up(hip, a):
    return hip.copy_array(np.ascontiguousarray(a))


def explain(case, fmt, got, want, rows, what):
    """the first wrong cells among `rows` (a mask over the grid) and what feeds them"""
    n0, nm, ns = w.fmt_dims(fmt)[0]
    bad = np.argwhere(rows[:, None] & ~((got == want) | (np.isnan(got) & np.isnan(want))))
    feeders = w.slot_feeders(fmt)
    brick = w.brick_of_cells(fmt)
    lines = ["%s (%s): %s: %d of %d cells x columns differ" % (case.name, case.purpose, what, bad.shape[0], int(rows.sum()) * got.shape[1])]
    for r, c in bad[:6]:
        fed = feeders.get(int(r), [])
        if fed:
            src = "fed by (task, brick, slot, lane, sample) %s" % fed[:6]
        else:
            near = sorted(set(f[:3] for q in np.flatnonzero(brick == brick[r]) for f in feeders.get(int(q), [])))
            src = "fed by nothing; its brick %d by (task, brick, slot) %s" % (brick[r], near[:6])
        lines.append("  (kx %d, km %d, ks %d, column %d): got %r, want %r; %s" % (r % n0, (r // n0) % nm, r // (n0 * nm), c, complex(got[r, c]), complex(want[r, c]), src))
    return "\n".join(lines)


# ---- per (case, entries): the device copy of the format, the reference and the emulation for four columns (a product of NC columns
# is the first NC of them: the columns do not meet) -----------------------------------------------------------------------------------------
_dev, _ref = {}, {}


def device_format(hip, case, real, exact=True):
    key = (case.name, real, exact)
    if key not in _dev:
        if len(_dev) > 4:
            _dev.clear()
        D = w.slot_data(case, real, exact)
        f = D.fmt
        _dev[key] = D, dict(entries=up(hip, f['entries']), slot_ptr=up(hip, f['slot_ptr']), tasks=up(hip, f['tasks']), table=up(hip, f['table']),
                            shared=up(hip, f['shared']), support=None if f['support'] is None else up(hip, f['support']))
    return _dev[key]


def expected(case, real, exact=True):
    """(reference (K, 4) complex128, write mask, emulation (K, 4) complex64 over a zero grid, owned rows)"""
    key = (case.name, real, exact)
    if key not in _ref:
        D = w.slot_data(case, real, exact)
        ref, mask = w.slot_reference(D.fmt, D.X4, ALPHA)
        _ref[key] = ref, mask, w.emulate_slots(D.fmt, D.X4, ALPHA, np.zeros((D.K, 4), dtype=C64)) if exact else None, w.owned_rows(D.fmt)
    return _ref[key]


def call_slots(hip, D, dev, X, Y, nc, **kw):
    a = w.cf32(ALPHA)
    f = D.fmt
    p = lambda k: None if dev[k] is None else VP(dev[k]._arr)
    arg = dict(M=D.M, K=D.K, N=nc, ldx=X.ld, n0=f['n0'], nm=f['nm'], bm=f['bm'], bs=f['bs'], ntasks=f['ntasks'], nshared=f['nshared'], tile=f['tile'],
               zw=f['zw'], words=f['words'])
    arg.update(kw)
    return hip._L.ig_ccsrmm_t_slots(hip._ctx, arg['M'], arg['K'], arg['N'], a.real, a.imag, p('entries'), p('slot_ptr'), X.ptr, arg['ldx'], Y.ptr, p('support'),
                                    arg['n0'], arg['nm'], arg['bm'], arg['bs'], p('tasks'), arg['ntasks'], p('table'), p('shared'), arg['nshared'],
                                    arg['tile'], arg['zw'], arg['words'])


def start_of_grid(D, nc):
    """what the caller's grid holds before the product: the NaN sentinel, or zeros where there is no table (the caller zeroes it)"""
    return None if D.fmt['support'] is not None else np.zeros((D.K, nc), dtype=C64)


def check_against_reference(case, D, got, before, nc, real):
    ref, mask, em, owned = expected(case, real)
    want = ref[:, :nc].astype(C64)
    assert np.all(np.isfinite(got[mask].view(np.float32))), explain(case, D.fmt, got, want, mask & ~np.isfinite(got.view(np.float32)).reshape(D.K, -1).all(axis=1),
                                                                    "a cell of the write mask was not written (or a NaN reached it)")
    assert np.array_equal(got[mask], want[mask]), explain(case, D.fmt, got, want, mask, "the write mask against the float64 reference")
    assert np.array_equal(bits(got[owned]), bits(em[owned][:, :nc])), explain(case, D.fmt, got, em[:, :nc], owned, "owned bricks against the float32 emulation, bit for bit")
    assert np.array_equal(bits(got[~mask]), bits(before[~mask])), explain(case, D.fmt, got, before, ~mask, "a cell outside the write mask was written")


@pytest.mark.parametrize("real", FT, ids=("complex", "real"))
@pytest.mark.parametrize("nc", NCS, ids=("nc1", "nc2", "nc4"))
@pytest.mark.parametrize("case", SLOT_CASES, ids=repr)
def test_exact_case_cell_for_cell(hip, case, nc, real):
    D, dev = device_format(hip, case, real)
    X = x_panel(hip, w.panel(D, nc))
    Y = grid_panel(hip, D.K, nc, start_of_grid(D, nc))
    before = Y.payload(Y.before).copy()
    hip._check(call_slots(hip, D, dev, X, Y, nc), case.name)
    check_against_reference(case, D, Y.read(), before, nc, real)
    assert X.untouched(), "the input panel was modified"


@pytest.mark.parametrize("real", FT, ids=("complex", "real"))
@pytest.mark.parametrize("nc", NCS, ids=("nc1", "nc2", "nc4"))
def test_rounding_stays_inside_the_derived_bound(hip, nc, real):
    case = w.SLOT_BY_NAME[w.SLOT_ROUNDING]
    D, dev = device_format(hip, case, real, exact=False)
    X = x_panel(hip, w.panel(D, nc))
    Y = grid_panel(hip, D.K, nc)
    before = Y.payload(Y.before).copy()
    hip._check(call_slots(hip, D, dev, X, Y, nc), case.name)
    got = Y.read()
    ref, mask, _, _ = expected(case, real, exact=False)
    assert np.array_equal(bits(got[~mask]), bits(before[~mask])), "a cell outside the write mask was written"
    err = np.abs(got[mask].astype(C128) - ref[mask][:, :nc])
    bound = w.adjoint_bound(D.fmt, w.panel(D, nc), ALPHA)[mask]
    assert np.all(err[bound == 0] == 0)
    frac = float((err[bound > 0] / bound[bound > 0]).max())
    print("k_grid_slots<%d, %s>: largest fraction of the bound %.3f" % (nc, str(real).lower(), frac))
    assert frac <= 1.0, frac


def test_refusals_leave_the_result_untouched(hip):
    L = hip._L
    for name, real, nc in (('zw4', False, 2), ('zw16-nm64', True, 1)):
        case = w.SLOT_BY_NAME[name]
        D, dev = device_format(hip, case, real)
        X = x_panel(hip, w.panel(D, nc))
        Y = grid_panel(hip, D.K, nc)

        def refused(needle, **kw):
            assert call_slots(hip, D, dev, X, Y, nc, **kw) != 0
            assert needle in L.ig_last_error(hip._ctx), L.ig_last_error(hip._ctx)
            assert Y.untouched(), "a refused call wrote to its result"
        refused(b"1, 2 or 4 columns", N=3)
        refused(b"1, 2 or 4 columns", N=8)
        refused(b"entries of 4 words", words=2)
        refused(b"support_tile 5", tile=5)
        refused(b"short leading dimension", ldx=D.M - 1)
        refused(b"bad dimensions", M=-1)
        refused(b"bad task list", ntasks=-1)
        refused(b"are not a grid of", n0=24)
        if name == 'zw4':
            refused(b"at most 32 segments per brick", tile=4, bm=4, bs=4)          # 4 x 4 x 4 = 64 segments
        else:
            refused(b"the support bitmaps hold 32 bits in each of 1 words", zw=1)   # nm = 64 > 32 x 1
        assert X.untouched()


def test_empty_calls_succeed_and_touch_nothing(hip):
    case = w.SLOT_BY_NAME['zw4']
    D, dev = device_format(hip, case, False)
    for nc in NCS:
        X = x_panel(hip, w.panel(D, nc))
        Y = grid_panel(hip, D.K, nc)
        for kw in (dict(ntasks=0), dict(ntasks=0, nshared=0), dict(K=0)):
            hip._check(call_slots(hip, D, dev, X, Y, nc, **kw), case.name)
            hip._L.ig_sync(hip._ctx)
            assert Y.untouched() and X.untouched(), kw


@pytest.mark.parametrize("nc", NCS, ids=("nc1", "nc2", "nc4"))
@pytest.mark.parametrize("name,fine", w.ROUTE_CASES, ids=("support", "support-fine"))
def test_route_of_csr_matrix_leads_to_the_slots(hip, monkeypatch, name, fine, nc):
    """csr_matrix.adjoint through set_grid_slots, by the 16-point table of set_grid_support (complex weights) and by a 4-point table
    of set_grid_support_fine (real weights): the same comparison against the same reference"""
    case, real = w.SLOT_BY_NAME[name], fine
    D = w.slot_data(case, real)
    n0, nm, ns = case.dims
    monkeypatch.setitem(hip.tuning, "real_entries", True)
    A_d = hip.csr_matrix(hip, D.A)
    if fine:
        A_d.set_grid_support_fine(D.fmt['support'], case.tile)
    else:
        A_d.set_grid_support(D.fmt['support'], n0, nm, zw=case.zw)
    if nc > 1:
        A_d.set_grid_interleaved(True)
    A_d.set_grid_slots(n0, nm, ns, ncols=nc, bm=case.shape[0], bs=case.shape[1], chunk=case.chunk, run=case.run)
    sl = A_d._slots
    assert sl is not None and (sl['words'], sl['ntasks'], sl['nshared'], sl['nslots'], sl['nentries']) == tuple(D.fmt[k] for k in ('words', 'ntasks', 'nshared', 'nslots', 'nentries'))
    before = np.empty((D.K, nc), dtype=C64)
    bits(before)[:] = NAN32
    y_d = hip.copy_array(np.asfortranarray(before.reshape(-1).reshape(D.K, nc, order='F')))
    assert A_d.adjoint_route(nc, 0, y_d) == 'slots'
    A_d.adjoint(y_d, hip.copy_array(np.asfortranarray(w.panel(D, nc))), alpha=ALPHA)
    got = y_d.to_host().reshape(-1, order='F').reshape(D.K, nc)               # row-major (interleaved) memory
    check_against_reference(case, D, got, before, nc, real)
