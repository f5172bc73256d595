"""The 64-column routes of BASELINE config 3 -- k_csrmm_runs64r (ig_ccsrmm_xrows_runs) and k_bricks_wide64r / k_bricks_wide64 /
k_wide_zero_unowned (ig_ccsrmm_t_bricks_wide[_grid]) -- called through the C ABI on the formats grid_formats builds, against the
float64 restatement in tests/wide64.py: every element of every row.

Exact cases: the hand-built tables of wide64.RUNS_CASES and wide64.WIDE_CASES, whose seams tests/test_wide64_cpu.py reads back from the
formats, on integer inputs with dyadic alpha and beta where nothing rounds -- not the fused multiply-adds, not the float atomics of
shared pieces: the device must give the reference by value, element for element.  A failure names the case, what it was built for
and the first wrong elements with the run / panel row / entry (forward) or the task / brick / quad (adjoint) that feed them.
Results lie between guard items with padded leading dimensions; guards and padding hold a NaN pattern that must come back untouched,
with beta == 0 the payload starts as that NaN and must come back finite (rows no nonzero touches as 0).

Rounding cases: one uniform-random case per instantiation inside the derived worst case of wide64.forward_bound / adjoint_bound; the
largest fraction of the bound reached is printed."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as spp

import wide64 as w
from wide64 import ALPHA, BETA, C64, C128, RUNS_CASES, WIDE_CASES

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
NAN32 = 0x7fc0dead                  # the sentinel: a quiet NaN that any arithmetic would also spread into the results
GUARD = 8                           # sentinel items on either side (even: the item behind them is 16-byte aligned)
FT = (False, True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Panel:
    """A (rows, 64) complex64 column-major panel on the device between sentinels, `pad` sentinel rows below every column
    (ld = rows + pad); data None: the payload is sentinels too; off = 1 passes the address one item behind a 16-byte boundary"""

    def __init__(self, hip, rows, data=None, pad=6, off=0):
        self.rows, self.ld, self.lo = rows, rows + pad, GUARD + off
        host = np.empty(GUARD + 1 + self.ld * 64 + GUARD, dtype=C64)
        bits(host)[:] = NAN32
        self.before = host
        if data is not None:
            self.payload(host)[...] = data
        self.dev = hip.copy_array(host)
        assert self.dev._arr % 16 == 0
        self.ptr = VP(self.dev._arr + 8 * self.lo)

    def payload(self, host):
        return host[self.lo:self.lo + self.ld * 64].reshape(64, self.ld).T[:self.rows]

    def read(self):
        """the payload; guards and padding rows must be bit-identical"""
        h = self.dev.to_host()
        keep = np.ones(h.size, dtype=bool)
        keep[self.payload(np.arange(h.size)).reshape(-1)] = False
        assert np.array_equal(bits(h)[np.repeat(keep, 2)], bits(self.before)[np.repeat(keep, 2)]), "a guard item or a padding row of the panel was overwritten"
        return self.payload(h).copy()

    def untouched(self):
        return np.array_equal(bits(self.dev.to_host()), bits(self.before))


def explain(case, got, want, feeders, labels):
    """the first wrong elements of a result and what feeds their rows"""
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    lines = ["%s (%s): %d of %d elements differ" % (case.name, case.purpose, bad.shape[0], got.size)]
    for r, c in bad[:5]:
        fed = feeders.get(int(r), [])
        if fed:
            src = "fed by %s %s" % (labels, fed[:6])
        else:                                                   # nothing adds into the row: what feeds the 16 rows around it
            near = sorted(set(f for q in range(int(r) // 16 * 16, int(r) // 16 * 16 + 16) for f in feeders.get(q, [])))
            src = "fed by nothing; its 16 rows by %s %s" % (labels, near[:6])
        lines.append("  (row %d, column %d): got %r, want %r; %s" % (r, c, complex(got[r, c]), complex(want[r, c]), src))
    return "\n".join(lines)


def up(hip, a):
    return hip.copy_array(np.ascontiguousarray(a))


# =========================================================================================================================================
# the forward product by runs
# =========================================================================================================================================
_fwd = {}


def forward_device(hip, case, exact, real):
    key = (case, exact, real)
    if key not in _fwd:
        if len(_fwd) > 4:
            _fwd.clear()
        D = w.runs_data(case, exact, real)
        f = D.fmt
        _fwd[key] = D, dict(indptr=up(hip, D.indptr), dptr=up(hip, f['dptr']), dcols=up(hip, f['dcols']), entries=up(hip, f['entries']),
                            order=None if f['order'] is None else up(hip, f['order']), touched=up(hip, w.TOUCHED))
    return _fwd[key]


def call_forward(hip, D, dev, beta, X, Y, M=None, K=w.XTOTAL, ldx=None, ldy=None, nxrows=w.NX, nnz=None):
    a, b = w.cf32(ALPHA), w.cf32(beta)
    p = lambda k: None if dev[k] is None else VP(dev[k]._arr)
    return hip._L.ig_ccsrmm_xrows_runs(hip._ctx, D.M if M is None else M, K, D.A.nnz if nnz is None else nnz, a.real, a.imag, p('indptr'), p('dptr'),
                                       p('dcols'), p('entries'), D.fmt['all_real'], p('order'), X.ptr, X.ld if ldx is None else ldx, b.real, b.imag,
                                       Y.ptr, Y.ld if ldy is None else ldy, p('touched'), nxrows)


def run_forward(hip, case, real, beta, exact=True):
    D, dev = forward_device(hip, case, exact, real)
    X = Panel(hip, w.XTOTAL, D.X, pad=3)
    Y = Panel(hip, D.M, None if w.cf32(beta) == 0 else D.Y0, pad=5)
    hip._check(call_forward(hip, D, dev, beta, X, Y), case.name)
    out = Y.read()
    assert X.untouched(), "the input panel was modified"
    return D, out


@pytest.mark.parametrize("beta", (0, BETA), ids=("beta0", "beta"))
@pytest.mark.parametrize("real", FT, ids=("complex", "real"))
@pytest.mark.parametrize("case", RUNS_CASES, ids=repr)
def test_forward_exact_case_element_for_element(hip, case, real, beta):
    D, out = run_forward(hip, case, real, beta)
    want = w.forward_reference(D, ALPHA, beta).astype(C64)
    assert np.all(np.isfinite(out.view(np.float32))), "a result row was not written (or a NaN of the padding reached it)"
    assert np.array_equal(out, want), explain(case, out, want, w.runs_feeders(D.fmt, D.indptr, D.M), "(run, panel row, entry)")


@pytest.mark.parametrize("beta", (0, BETA), ids=("beta0", "beta"))
@pytest.mark.parametrize("real", FT, ids=("complex", "real"))
def test_forward_rounding_stays_inside_the_derived_bound(hip, real, beta):
    case = w.RUNS_BY_NAME[w.RUNS_ROUNDING]
    D, out = run_forward(hip, case, real, beta, exact=False)
    err = np.abs(out.astype(C128) - w.forward_reference(D, ALPHA, beta))
    frac = float((err / w.forward_bound(D, ALPHA, beta)).max())
    print("k_csrmm_runs64r<%d, %s>: largest fraction of the bound %.3f" % (beta != 0, str(real).lower(), frac))
    assert frac <= 1.0, frac


def test_forward_refusals_and_empty_calls(hip):
    L = hip._L
    case = w.RUNS_BY_NAME['m17']
    D, dev = forward_device(hip, case, True, False)
    X = Panel(hip, w.XTOTAL, D.X, pad=3)
    Y = Panel(hip, D.M, None, pad=5)

    def refused(needle, **kw):
        assert call_forward(hip, D, dev, 0, X, Y, **kw) != 0
        assert needle in L.ig_last_error(hip._ctx), L.ig_last_error(hip._ctx)
        assert Y.untouched(), "a refused call wrote to its result"
    refused(b"bad dimensions", M=-1)
    refused(b"bad dimensions", nnz=-1)
    refused(b"short leading dimension", ldy=D.M - 1)
    refused(b"short leading dimension", ldx=w.XTOTAL - 1)
    refused(b"bad row list", nxrows=0)
    refused(b"bad row list", nxrows=w.XTOTAL + 1)
    refused(b"2 GB window", nnz=(1 << 31) // 12 + 1)
    # no rows: nothing is launched, nothing written
    assert call_forward(hip, D, dev, 0, X, Y, M=0) == 0
    L.ig_sync(hip._ctx)
    assert Y.untouched()


def test_forward_route_of_csr_matrix_leads_to_the_runs(hip):
    D = w.runs_data(w.RUNS_BY_NAME['windows'])
    A = spp.csr_matrix((D.A.data, w.TOUCHED[D.A.indices], D.A.indptr), shape=(D.M, w.XTOTAL))
    A_d = hip.csr_matrix(hip, A)
    assert A_d.forward_route(64) == 'xrows_runs'
    xfull = np.asfortranarray(np.concatenate([D.X, D.X[:4]]))
    yfull = np.asfortranarray(np.concatenate([D.Y0, D.Y0[:3]]))
    x_d, y_d = hip.copy_array(xfull)[0:w.XTOTAL, :], hip.copy_array(yfull)[0:D.M, :]
    A_d.forward(y_d, x_d, alpha=ALPHA, beta=BETA)
    assert A_d._runs_fmt is not None
    assert np.array_equal(y_d.to_host(), w.forward_reference(D, ALPHA, BETA).astype(C64))


# =========================================================================================================================================
# the adjoint by wide bricks
# =========================================================================================================================================
_adj = {}


def adjoint_device(hip, case, exact, real):
    key = (case, exact, real)
    if key not in _adj:
        if len(_adj) > 4:
            _adj.clear()
        D = w.wide_data(case, exact, real)
        f = D.fmt
        _adj[key] = D, dict(entries=up(hip, f['entries']), rows=up(hip, f['rows']), tasks=up(hip, f['tasks']), table=up(hip, f['table']),
                            owned=up(hip, f['owned']))
    return _adj[key]


def call_adjoint(hip, D, dev, X, Y, plain_entry=False, **kw):
    a = w.cf32(ALPHA)
    f = D.fmt
    p = lambda k: VP(dev[k]._arr)
    arg = dict(M=D.M, K=D.K, ldx=X.ld, ldy=Y.ld, ntasks=f['ntasks'], geom=f['geom'], words=f['words'])
    arg.update(kw)
    head = (hip._ctx, arg['M'], arg['K'], a.real, a.imag, p('entries'), p('rows'), X.ptr, arg['ldx'], Y.ptr, arg['ldy'], p('tasks'), arg['ntasks'],
            p('table'), p('owned'))
    if plain_entry:
        return hip._L.ig_ccsrmm_t_bricks_wide(*head)
    return hip._L.ig_ccsrmm_t_bricks_wide_grid(*head, *arg['geom'], arg['words'])


LAYOUTS = dict(even=dict(pad=6, off=0), odd=dict(pad=5, off=0), offset=dict(pad=6, off=1))      # k_wide_zero_unowned / the memset twice


@pytest.mark.parametrize("real", FT, ids=("complex", "real"))
@pytest.mark.parametrize("case", WIDE_CASES, ids=repr)
def test_adjoint_exact_case_element_for_element(hip, case, real):
    D, dev = adjoint_device(hip, case, True, real)
    assert D.fmt['geom'][2:] == case.shape
    want = w.adjoint_reference(D, ALPHA).astype(C64)
    X = Panel(hip, D.M, D.X, pad=3)
    for name, lay in LAYOUTS.items():
        Y = Panel(hip, D.K, None, **lay)                        # a sentinel everywhere: untouched tiles must come back as zero
        assert (Y.ld % 2 == 0 and (Y.dev._arr + 8 * Y.lo) % 16 == 0) == (name == 'even')
        for again in range(2 if name == 'even' else 1):         # a second product into the same result equals the first
            hip._check(call_adjoint(hip, D, dev, X, Y, plain_entry=case.NT == 1 and name == 'odd'), case.name)
            out = Y.read()
            assert np.array_equal(out, want), "result layout '%s', product %d: " % (name, again + 1) + \
                explain(case, out, want, w.wide_feeders(D), "(task, brick, quad)")
    assert X.untouched(), "the input panel was modified"


@pytest.mark.parametrize("real", FT, ids=("complex", "real"))
@pytest.mark.parametrize("name", w.WIDE_ROUNDING)
def test_adjoint_rounding_stays_inside_the_derived_bound(hip, name, real):
    case = w.WIDE_BY_NAME[name]
    D, dev = adjoint_device(hip, case, False, real)
    X, Y = Panel(hip, D.M, D.X, pad=3), Panel(hip, D.K, None)
    hip._check(call_adjoint(hip, D, dev, X, Y), case.name)
    err = np.abs(Y.read().astype(C128) - w.adjoint_reference(D, ALPHA))
    bound = w.adjoint_bound(D, ALPHA)
    assert np.all(err[bound == 0] == 0)
    frac = float((err[bound > 0] / bound[bound > 0]).max())
    kernel = "k_bricks_wide64" if case.NT == 1 else "k_bricks_wide64r<%d, %s>" % (case.NT, str(real).lower())
    print("%s: largest fraction of the bound %.3f" % (kernel, frac))
    assert frac <= 1.0, frac


def test_adjoint_refusals_and_empty_calls(hip):
    L = hip._L
    grid, plain = w.WIDE_BY_NAME['one-brick'], w.WIDE_BY_NAME['plain']
    for case, real in ((grid, True), (plain, False)):
        D, dev = adjoint_device(hip, case, True, real)
        X, Y = Panel(hip, D.M, D.X, pad=3), Panel(hip, D.K, None)

        def refused(needle, **kw):
            assert call_adjoint(hip, D, dev, X, Y, **kw) != 0
            assert needle in L.ig_last_error(hip._ctx), L.ig_last_error(hip._ctx)
            assert Y.untouched(), "a refused call wrote to its result"
        refused(b"entries of 3 words", words=4)
        refused(b"short leading dimension", ldy=D.K - 1)
        refused(b"short leading dimension", ldx=D.M - 1)
        refused(b"bad task list", ntasks=-1)
        refused(b"exceeds the 2 GB window", M=1 << 22, ldx=1 << 22)
        if case is grid:
            n0, nm, bm, bs = D.fmt['geom']
            refused(b"are not a grid of", geom=(24, nm, bm, bs))
            refused(b"are not a grid of", geom=(n0, nm, 4, 2))
            refused(b"are not a grid of", geom=(n0, 3, bm, bs))
            refused(b"are not a grid of", geom=(0, nm, bm, bs))
        else:
            refused(b"entries of 3 words", words=2)            # 8-byte entries are a form of the grid bricks only
            refused(b"must be a multiple of 16", K=D.K - 8)
            # no rows of Y: nothing to do
            assert call_adjoint(hip, D, dev, X, Y, K=0) == 0
            L.ig_sync(hip._ctx)
            assert Y.untouched()
        # no tasks, or no rows of X: the result is zero, its padding untouched
        for kw in (dict(ntasks=0), dict(M=0)):
            Y = Panel(hip, D.K, None)
            hip._check(call_adjoint(hip, D, dev, X, Y, **kw), case.name)
            assert not np.any(bits(Y.read())), kw


def test_adjoint_route_of_csr_matrix_leads_to_the_wide_bricks(hip, monkeypatch):
    case = w.WIDE_BY_NAME['taps-2x2']
    D = w.wide_data(case)
    monkeypatch.setitem(hip.tuning, "wide_brick_shape", case.shape)
    monkeypatch.setitem(hip.tuning, "wide_task_shape", case.task)
    A_d = hip.csr_matrix(hip, D.A)
    A_d.set_grid_dims(*case.dims)
    yfull = np.full((D.K + 6, 64), w.SENTINEL, dtype=C64, order='F')
    y_d = hip.copy_array(yfull)[0:D.K, :]
    assert A_d.adjoint_route(64, 0, y_d) == 'wide'
    A_d.adjoint(y_d, hip.copy_array(np.asfortranarray(D.X)), alpha=ALPHA)
    assert A_d._wide['geom'] == case.dims[:2] + case.shape and A_d._wide['words'] == 3
    assert np.array_equal(y_d.to_host(), w.adjoint_reference(D, ALPHA).astype(C64))
