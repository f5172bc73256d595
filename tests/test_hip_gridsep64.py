"""GPU: the separable gridding kernels (ig_grid_gather_sep -> k_grid_gather_sep, ig_grid_scatter_sep -> k_sep_pack_recx,
k_grid_sep_zero, k_grid_scatter_mfma) through the C ABI with ctypes -- no csr_matrix, so no route layer moves a case elsewhere --
against the float64 restatement in tests/gridsep64.py: every element of every sample and of every grid cell.

Exact cases: the tables of gridsep64 (hand-built records with every tap count, wrap-around first taps, the smallest legal grids;
sample counts at the seams of the gather's launch; task lists at the seams of the scatter's pipeline; redrawn segment masks) on
integer inputs with dyadic alpha and beta, where no kernel rounds anything (tests/test_gridsep64_cpu.py shows it per case and
emulates the sums in float32): the device must give the reference as numbers, element by element, shared bricks included.  Panels sit
between NaN sentinels, padding rows and every grid cell no sample touches hold NaN, and results start as NaN where nothing reads them.

Rounding cases: builder-made records and uniform-random panels, one per (NC, tw) and direction, within the worst-case bound
gridsep64 derives per element."""

import numpy as np
import pytest

import gridsep64 as g
from gridsep64 import ALPHA, BETA, C64, GATHER_CASES, GATHER_ROUNDING, SCATTER_CASES, SCATTER_ROUNDING
from indigo_amd import grid_formats
from test_hip_spmm import NAN32, Panel, VP, bits, same_bits

pytestmark = pytest.mark.gpu
eq = np.testing.assert_array_equal


def ids(v):
    return repr(v) if isinstance(v, (g.GCase, g.SCase)) else ('beta0' if v == 0 else 'beta' if isinstance(v, complex) else str(v))


def upload(hip, a):
    d = hip.copy_array(np.ascontiguousarray(a).reshape(-1))
    assert d._arr % 16 == 0
    return d


def wide_records(rec):
    """the records at the stride of the share scatter, the words behind them poisoned"""
    recx, rs = grid_formats.records_with_rows(rec)
    recx = recx.reshape(rec.shape[0], rs).copy()
    recx[:, rec.shape[1]:] = NAN32
    return recx, rs


# =========================================================================================================================================
# the gather
# =========================================================================================================================================
def call_gather(hip, D, rec_d, rs, X, Y, alpha, beta, order=None, **over):
    c = D.case
    a, b = g.cf32(alpha), g.cf32(beta)
    p = dict(M=D.M, NC=c.NC, tw=c.tw, rec_ptr=VP(rec_d._arr), stride=rs, x_ptr=X.ptr, n0=c.dims[0], nm=c.dims[1], ns=c.dims[2], y_ptr=Y.ptr, ldy=Y.ld)
    p.update(over)
    return hip._L.ig_grid_gather_sep(hip._ctx, p['M'], p['NC'], p['tw'], p['rec_ptr'], p['stride'], p['x_ptr'], p['n0'], p['nm'], p['ns'],
                                     a.real, a.imag, b.real, b.imag, p['y_ptr'], p['ldy'], None if order is None else VP(order._arr))


def run_gather(hip, D, alpha, beta, wide=False, order=None):
    rec, stride = wide_records(D.rec) if wide else (D.rec, D.rec.shape[1])
    rec_d = upload(hip, rec)
    X = Panel(hip, D.P, D.case.NC, D.X, il=True)
    Y = Panel(hip, D.M, D.case.NC, None if g.cf32(beta) == 0 else D.Y0)          # beta == 0: NaN all over
    hip._check(call_gather(hip, D, rec_d, stride, X, Y, alpha, beta, None if order is None else upload(hip, order)), repr(D.case))
    out = Y.read()
    X.unchanged()
    assert same_bits(rec_d.to_host(), rec.reshape(-1)), "the records were modified"
    return out


@pytest.mark.parametrize("beta", [0, BETA], ids=ids)
@pytest.mark.parametrize("case", GATHER_CASES, ids=ids)
def test_gather_is_exact_sample_by_sample(hip, case, beta):
    D = g.build_gather(case)
    ref = g.forward_reference(D.A, D.X, D.Y0, ALPHA, beta).astype(C64)
    outs = [run_gather(hip, D, ALPHA, beta, wide) for wide in (False, True)]
    group = g.gather_geometry(case.NC, case.tw)[3]
    morton = grid_formats.gather_order(D.rec, case.tw, case.NC)
    assert (morton is not None) == (D.M > 4 * group)
    if morton is not None:
        nblocks = -(-D.M // group)
        assert morton.size == nblocks
        outs += [run_gather(hip, D, ALPHA, beta, order=o) for o in (morton, np.random.default_rng(case.seed).permutation(nblocks).astype(np.uint32))]
    for out in outs:
        assert np.all(np.isfinite(out.view(np.float32))), "a sample was not written (or a NaN of an untouched cell reached it)"
        eq(out, ref)
        assert same_bits(out, outs[0])


@pytest.mark.parametrize("case", GATHER_ROUNDING, ids=ids)
def test_random_gather_within_the_worst_case_bound(hip, case):
    D = g.build_gather(case)
    for beta in (0, BETA):
        out = run_gather(hip, D, ALPHA, beta)
        ref, bound = g.forward_reference(D.A, D.X, D.Y0, ALPHA, beta), g.forward_bound(D.A, D.X, D.Y0, ALPHA, beta)
        err = np.maximum(np.abs(out.real - ref.real), np.abs(out.imag - ref.imag))
        print("%r beta %s: largest error / bound = %.3f" % (case, beta, float((err / np.maximum(bound, 1e-300)).max())))
        assert np.all(err <= bound), np.argwhere(~(err <= bound))[:8]


# =========================================================================================================================================
# the scatter
# =========================================================================================================================================
class Shares:
    """a case's share format and widened records on the device"""

    def __init__(self, hip, D):
        f = D.fmt
        self.recx = upload(hip, D.recx)
        self.dev = {k: upload(hip, f[k]) for k in ('shares', 'tasks', 'table', 'shared')}

    def call(self, hip, D, X, Y, alpha, **over):
        c, f = D.case, D.fmt
        a = g.cf32(alpha)
        p = dict(M=D.M, NC=c.NC, tw=c.tw, stride=D.rs, ldx=X.ld, n0=c.dims[0], nm=c.dims[1], ns=c.dims[2], bm=f['bm'], bs=f['bs'],
                 ntasks=f['ntasks'], nshared=f['nshared'], tile=f['tile'])
        p.update(over)
        d = self.dev
        return hip._L.ig_grid_scatter_sep(hip._ctx, p['M'], p['NC'], p['tw'], VP(self.recx._arr), p['stride'], VP(d['shares']._arr), X.ptr, p['ldx'],
                                          Y.ptr, p['n0'], p['nm'], p['ns'], p['bm'], p['bs'], VP(d['tasks']._arr), p['ntasks'], VP(d['table']._arr),
                                          VP(d['shared']._arr), p['nshared'], p['tile'], a.real, a.imag)


def run_scatter(hip, D, alpha, evaluations=2):
    """-> the grid panel (cells, NC) after each evaluation into the same poisoned grid"""
    c = D.case
    S = Shares(hip, D)
    X = Panel(hip, D.M, c.NC, D.X)                          # ldx = M + 5, NaN below every column
    Y = Panel(hip, D.P, c.NC, None, il=True)
    outs = []
    for _ in range(evaluations):
        hip._check(S.call(hip, D, X, Y, alpha), repr(c))
        outs.append(Y.read())
    X.unchanged()
    after = S.recx.to_host().reshape(D.M, D.rs)
    rw = g.sep_words(c.tw)
    assert same_bits(after[:, :rw], D.recx[:, :rw]), "the records were modified"
    assert same_bits(after[:, rw + 2 * c.NC:], D.recx[:, rw + 2 * c.NC:]), "a word behind the panel row was written"
    assert same_bits(after[:, rw:rw + 2 * c.NC], bits(np.ascontiguousarray(D.X)).reshape(D.M, 2 * c.NC)), "the packed panel rows"
    for k in ('shares', 'tasks', 'table', 'shared'):
        assert same_bits(S.dev[k].to_host(), np.ascontiguousarray(D.fmt[k]).reshape(-1))
    return outs


@pytest.mark.parametrize("case", SCATTER_CASES, ids=ids)
def test_scatter_is_exact_cell_by_cell(hip, case):
    D = g.build_scatter(case)
    ref = g.adjoint_reference(D.A, D.X, ALPHA).astype(C64)
    outs = run_scatter(hip, D, ALPHA)
    for out in outs:
        assert np.all(bits(out[~D.flag]) == NAN32), "a cell outside the flagged segments was written"
        assert np.all(np.isfinite(out[D.flag].view(np.float32))), "a flagged cell was not written (or a NaN of the padding reached it)"
        eq(out[D.flag], ref[D.flag])
    eq(outs[1], outs[0])


@pytest.mark.parametrize("case", SCATTER_ROUNDING, ids=ids)
def test_random_scatter_within_the_worst_case_bound(hip, case):
    D = g.build_scatter(case)
    assert D.fmt['nshared'] > 0 and D.flag[np.unique(D.A.indices)].all()
    out = run_scatter(hip, D, ALPHA, evaluations=1)[0]
    ref, bound = g.adjoint_reference(D.A, D.X, ALPHA), g.adjoint_bound(D.A, D.X, ALPHA, D.pieces)
    assert np.all(bits(out[~D.flag]) == NAN32)
    err = np.maximum(np.abs(out.real - ref.real), np.abs(out.imag - ref.imag))[D.flag]
    print("%r: largest error / bound = %.3f" % (case, float((err / np.maximum(bound[D.flag], 1e-300)).max())))
    assert np.all(err <= bound[D.flag]), np.argwhere(~(err <= bound[D.flag]))[:8]


# =========================================================================================================================================
# empties and refusals
# =========================================================================================================================================
G_SMALL = g.GCase(4, 6, (16, 6, 6), 37, 901, True)
S_SMALL = g.SCase(4, 6, 'wrap', (16, 6, 6), (2, 4), 8, 16, 16, 'all', 902, True)


def test_empty_calls_write_nothing(hip):
    D = g.build_gather(G_SMALL)
    rec_d = upload(hip, D.rec)
    X, Y = Panel(hip, D.P, 4, D.X, il=True), Panel(hip, D.M, 4, None)
    assert call_gather(hip, D, rec_d, D.rec.shape[1], X, Y, ALPHA, BETA, M=0) == 0
    assert same_bits(Y.dev.to_host(), Y.before)
    D = g.build_scatter(S_SMALL)
    S = Shares(hip, D)
    X, Y = Panel(hip, D.M, 4, D.X), Panel(hip, D.P, 4, None, il=True)
    for over in (dict(ntasks=0), dict(M=0), dict(ntasks=0, nshared=0)):
        assert S.call(hip, D, X, Y, ALPHA, **over) == 0
        hip._check(hip._L.ig_sync(hip._ctx), "ig_sync")
        assert same_bits(Y.dev.to_host(), Y.before) and same_bits(S.recx.to_host(), D.recx.reshape(-1))


def test_refusals_leave_the_result_untouched(hip):
    L = hip._L
    D = g.build_gather(G_SMALL)
    wide, rs = wide_records(D.rec)
    rec_d, wide_d = upload(hip, D.rec), upload(hip, wide)
    X, Y = Panel(hip, D.P, 4, D.X, il=True), Panel(hip, D.M, 4, D.Y0)
    assert call_gather(hip, D, rec_d, 32, X, Y, ALPHA, BETA) == 0          # the call every refusal below spoils in one argument
    Y = Panel(hip, D.M, 4, D.Y0)
    for over in (dict(NC=16), dict(tw=5), dict(n0=5), dict(nm=5), dict(ns=5), dict(x_ptr=VP(X.ptr.value + 8)), dict(rec_ptr=VP(rec_d._arr + 8)),
                 dict(stride=18), dict(stride=16), dict(ldy=D.M - 1), dict(n0=65536)):
        assert call_gather(hip, D, rec_d, 32, X, Y, ALPHA, BETA, **over) != 0, over
        assert b"ig_grid_gather_sep" in L.ig_last_error(hip._ctx), over
        assert same_bits(Y.dev.to_host(), Y.before), over
    assert call_gather(hip, D, wide_d, rs, X, Y, ALPHA, BETA, stride=2048) != 0
    assert same_bits(Y.dev.to_host(), Y.before)
    X.unchanged()

    D = g.build_scatter(S_SMALL)
    S = Shares(hip, D)
    X, Y = Panel(hip, D.M, 4, D.X), Panel(hip, D.P, 4, None, il=True)
    rw = g.sep_words(6)
    for over in (dict(NC=16), dict(NC=2), dict(tw=5), dict(nm=5), dict(ns=5), dict(stride=rw + 2 * 4 - 4), dict(stride=rw + 2 * 4 + 2), dict(ldx=D.M - 1),
                 dict(bm=8), dict(bs=8), dict(bm=3), dict(n0=24), dict(n0=8), dict(tile=2), dict(tile=32), dict(ntasks=-1)):
        assert S.call(hip, D, X, Y, ALPHA, **over) != 0, over
        assert b"ig_grid_scatter_sep" in L.ig_last_error(hip._ctx), over
        assert same_bits(Y.dev.to_host(), Y.before) and same_bits(S.recx.to_host(), D.recx.reshape(-1)), over
    hip._check(S.call(hip, D, X, Y, ALPHA), "the call the refusals spoil")
    out = Y.read()
    eq(out[D.flag], g.adjoint_reference(D.A, D.X, ALPHA).astype(C64)[D.flag])


# =========================================================================================================================================
# through the route layer
# =========================================================================================================================================
def test_csr_matrix_routes_reach_the_same_kernels(hip):
    """HipBackend.csr_matrix + set_grid_interleaved + set_grid_separable + set_grid_shares on a hand-built exact `sep` dict with
    gconst = -1j: the forward and the adjoint equal the direct calls (alpha times gconst, and times its conjugate)"""
    gconst = -1j
    for NC, tw in ((8, 6), (4, 8)):
        case = g.SCase(NC, tw, 'odd', (32, 13, 11), (4, 4), 16, 32, 48, 'all', 903, True)
        D = g.build_scatter(case)
        sep = dict(records=D.rec, tw=tw, gconst=gconst, dims=case.dims)
        A_d = hip.csr_matrix(hip, (D.A.astype(np.complex128) * gconst).astype(C64).tocsr())
        A_d.set_grid_interleaved(True)
        A_d.set_grid_separable(sep)
        A_d.set_grid_shares(NC, 4, 4, 32, 48)
        # forward: a grid panel with a value in every cell (the route layer has no NaN to step around)
        rng = np.random.default_rng(11)
        Xg, Y0 = g.exact_panel(rng, (D.P, NC)), g.exact_panel(rng, (D.M, NC))
        Dg = g.GatherData(g.GCase(NC, tw, case.dims, D.M, 0, True), D.rec, Xg, Y0, D.A, D.M, D.P, np.ones(D.P, dtype=bool))
        x_d = hip.copy_array(np.asfortranarray(Xg.reshape(-1).reshape(D.P, NC, order='F')))          # row-major memory
        for beta in (0, BETA):
            assert A_d.forward_route(NC) == 'sep'
            y_d = hip.copy_array(np.asfortranarray(Y0))
            A_d.forward(y_d, x_d, alpha=ALPHA, beta=beta)
            direct = run_gather(hip, Dg, ALPHA * gconst, beta)
            eq(y_d.to_host(), direct)
            eq(direct, g.forward_reference(D.A, Xg, Y0, ALPHA * gconst, beta).astype(C64))
        # adjoint: the route zeroes the grid first (no support table), the direct call writes the bricks that hold a share
        y_d = hip.copy_array(np.full((D.P, NC), np.nan + 0j, dtype=C64))
        assert A_d.adjoint_route(NC, 0, y_d) == 'shares'
        A_d.adjoint(y_d, hip.copy_array(np.asfortranarray(D.X)), alpha=ALPHA)
        got = y_d.to_host().reshape(-1, order='F').reshape(D.P, NC)
        direct = run_scatter(hip, D, ALPHA * np.conj(gconst), evaluations=1)[0]
        eq(got[D.flag], direct[D.flag])
        eq(got[~D.flag], 0)
        eq(direct[D.flag], g.adjoint_reference(D.A, D.X, ALPHA * np.conj(gconst)).astype(C64)[D.flag])
