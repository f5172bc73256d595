"""The gather / scatter kernels of indigo_amd/csrc/ig_spmm.hip, called leaf by leaf through the C ABI (no csr_matrix, so no route layer
moves a case elsewhere), against the float64 restatement in tests/spmm64.py: every element of every row.

Exact cases: the table of spmm64.CASES -- built through the mirror of launch_gather so that every reachable kernel meets row lengths
at its own seams -- on integer inputs with dyadic alpha and beta, where no kernel rounds anything (tests/test_spmm64_cpu.py shows
it): the device must give the reference BIT FOR BIT, with beta == 0 and beta != 0.  Every result panel has ldy > rows and lies
between guard items; padding and guards hold a NaN pattern that must come back untouched, with beta == 0 the payload starts as NaN
and must come back finite (empty rows as 0, deferred rows written once), and the panel's own NaN padding (ldx > rows) must never
reach a result.

Rounding cases: one uniform-random case per kernel family within the classical worst-case bound of spmm64.gather_bound (a half
precision intermediate would pass the integer cases)."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import spmm64 as s
from spmm64 import ALPHA, BETA, C64, C128, CASES, CASE_BY_NAME
from indigo_amd import fused

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
NAN32 = 0x7fc0dead                  # the sentinel: a quiet NaN that any arithmetic would also spread into the results
GUARD = 8                           # sentinel items on either side (even: the item behind them is 16-byte aligned)
eq = np.testing.assert_array_equal
FT = (False, True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Panel:
    """A (rows, N) complex64 panel on the device between sentinels.  Column-major with `pad` sentinel rows below every column
    (ld = rows + pad), or, il = True, row-major without padding.  data None: the payload is sentinels too.  off = 1 passes the
    address one item behind a 16-byte boundary."""

    def __init__(self, hip, rows, N, data=None, pad=5, off=0, il=False):
        self.rows, self.N, self.il = rows, N, il
        self.ld = rows if il else rows + pad
        self.lo = GUARD + off
        n = rows * N if il else self.ld * N
        host = np.empty(GUARD + 1 + n + GUARD, dtype=C64)
        bits(host)[:] = NAN32
        self.before = host
        if data is not None:
            self.payload(host)[...] = data
        self.dev = hip.copy_array(host)
        assert self.dev._arr % 16 == 0
        self.ptr = VP(self.dev._arr + 8 * self.lo)

    def payload(self, host):
        body = host[self.lo:self.lo + (self.rows * self.N if self.il else self.ld * self.N)]
        return body.reshape(self.rows, self.N) if self.il else body.reshape(self.N, self.ld).T[:self.rows]

    def read(self):
        """the payload; guards and padding rows must be bit-identical"""
        h = self.dev.to_host()
        keep = np.ones(h.size, dtype=bool)
        view = self.payload(np.arange(h.size))
        keep[view.reshape(-1)] = False
        assert np.array_equal(bits(h)[np.repeat(keep, 2)], bits(self.before)[np.repeat(keep, 2)]), "a guard item or a padding row of the panel was overwritten"
        return self.payload(h).copy()

    def unchanged(self):
        assert same_bits(self.dev.to_host(), self.before), "an input panel was modified"


@functools.lru_cache(maxsize=2)
def device_matrix(hip, case, exact=True):
    D = s.build(case, exact)
    dev = dict(indptr=hip.copy_array(D.indptr), colind=hip.copy_array(D.colind if D.nnz else np.zeros(1, dtype=np.int32)),
               vals=hip.copy_array(D.vals if D.nnz else np.zeros(1, dtype=C64)),
               vals_re=hip.copy_array(np.ascontiguousarray(D.vals.real, dtype=np.float32) if D.nnz else np.zeros(1, dtype=np.float32)))
    if D.xlist is not None:
        dev['xlist'] = hip.copy_array(D.xlist)
    if D.yperm is not None:
        dev['yperm'] = hip.copy_array(D.yperm)
    return D, dev


def call_entry(hip, D, dev, alpha, beta, X, Y, support=None, n0=0, nm=0):
    """the case's entry point on the device panels X and Y; -> its return code"""
    L, ctx, e = hip._L, hip._ctx, D.case.entry
    a, b = s.cf32(alpha), s.cf32(beta)
    p = lambda k: VP(dev[k]._arr)
    head = (a.real, a.imag, p('vals'), p('colind'), p('indptr'))
    if e == 'ccsrmm':
        return L.ig_ccsrmm(ctx, 0, 0, D.rows, D.xtotal, D.N, D.nnz, *head, X.ptr, X.ld, b.real, b.imag, Y.ptr, Y.ld)
    if e == 'ccsrmm_t':
        return L.ig_ccsrmm_t(ctx, D.xtotal, D.rows, D.N, D.nnz, *head, X.ptr, X.ld, b.real, b.imag, Y.ptr, Y.ld)
    if e == 'rowperm':
        return L.ig_ccsrmm_rowperm(ctx, D.rows, D.xtotal, D.N, D.nnz, *head, X.ptr, X.ld, b.real, b.imag, Y.ptr, Y.ld, p('yperm'))
    if e == 'xrows':
        return L.ig_ccsrmm_xrows(ctx, D.rows, D.xtotal, D.N, D.nnz, *head, X.ptr, X.ld, b.real, b.imag, Y.ptr, Y.ld, p('xlist'), D.nx)
    if e in ('t_grid', 't_grid_xp'):
        return L.ig_ccsrmm_t_grid(ctx, D.xtotal, D.rows, D.N, D.nnz, *head, X.ptr, X.ld, b.real, b.imag, Y.ptr, Y.ld,
                                  support, n0, nm, p('xlist') if e == 't_grid_xp' else None)
    if e == 'il':
        return L.ig_ccsrmm_il(ctx, D.rows, D.xtotal, D.N, D.nnz, *head, X.ptr, b.real, b.imag, Y.ptr, Y.ld)
    if e == 'il_rw':
        return L.ig_ccsrmm_il_rw(ctx, D.rows, D.xtotal, D.N, D.nnz, a.real, a.imag, p('vals'), p('vals_re'), p('colind'), p('indptr'),
                                 X.ptr, b.real, b.imag, Y.ptr, Y.ld)
    if e == 't_grid_il':
        assert b == 0
        return L.ig_ccsrmm_t_grid_il(ctx, D.xtotal, D.rows, D.N, D.nnz, *head, X.ptr, X.ld, Y.ptr, support, n0, nm)
    raise KeyError(e)


def run_case(hip, case, beta, exact=True, offx=0, offy=0, y_start=None):
    """-> (D, the result panel as the device left it)"""
    D, dev = device_matrix(hip, case, exact)
    e = s.ENTRIES[case.entry]
    X = Panel(hip, D.xtotal, D.N, D.X, off=offx, il=e.get('x_il', False))
    start = y_start if y_start is not None else (None if s.cf32(beta) == 0 else D.Y0)         # beta == 0: NaN all over
    Y = Panel(hip, D.rows, D.N, start, off=offy, il=e.get('y_il', False))
    rc = call_entry(hip, D, dev, ALPHA, beta, X, Y)
    hip._check(rc, case.name)
    out = Y.read()
    X.unchanged()
    return D, out


def ids(v):
    return repr(v) if isinstance(v, s.Case) else ('beta0' if v == 0 else 'beta' if isinstance(v, complex) else str(v))


CASE_BETAS = [(c, b) for c in CASES for b in s.betas_of(c)]


# =========================================================================================================================================
# the exact cases
# =========================================================================================================================================
@pytest.mark.parametrize("case,beta", CASE_BETAS, ids=ids)
def test_exact_case_is_reproduced_bit_for_bit(hip, case, beta):
    D, out = run_case(hip, case, beta)
    assert np.all(np.isfinite(out.view(np.float32))), "a result row was not written (or a NaN of the padding reached it)"
    eq(out, s.gather_reference(D, ALPHA, beta).astype(C64))


ALIGN_CASES = ('ccsrmm-N1-mid', 'ccsrmm_t-N1-sparse', 'ccsrmm-N4-dense', 'ccsrmm_t-N8-sparse', 'ccsrmm-N3-sparse-bigx', 'rowperm-N3-mid',
               'ccsrmm_t-N16-dense', 'ccsrmm-N64-dense', 'ccsrmm_t-N64-sparse', 'rowperm-N64-dense', 'ccsrmm-N65-mid')


@pytest.mark.parametrize("offx,offy", ((1, 0), (0, 1), (1, 1)))
@pytest.mark.parametrize("name", ALIGN_CASES)
def test_panels_that_are_8_byte_aligned_only(hip, name, offx, offy):
    """ig_ccsrmm, ig_ccsrmm_t, ig_ccsrmm_rowperm with X and / or Y one item behind a 16-byte boundary.  A column-major panel of 2..64
    columns reaches the 16-byte kernels only as the library's own repacked (aligned) copy, and a single column is read 8 bytes at a
    time, so the kernel is the same (test_spmm64_cpu.py::test_alignment_only_matters_for_an_interleaved_panel) and so must be the bits"""
    case = CASE_BY_NAME[name]
    for beta in s.betas_of(case):
        D, out = run_case(hip, case, beta, offx=offx, offy=offy)
        eq(out, s.gather_reference(D, ALPHA, beta).astype(C64))


def test_backend_methods_take_the_same_leaves(hip):
    """hip.ccsrmm / hip.ccsrmm_t on the backend's own arrays: the same bits as through ctypes"""
    for name, beta in (('ccsrmm-N3-mid', BETA), ('ccsrmm_t-N8-sparse', 0)):
        D, dev = device_matrix(hip, CASE_BY_NAME[name])
        x_d, y_d = hip.copy_array(np.asfortranarray(D.X)), hip.copy_array(np.asfortranarray(D.Y0))
        if name.startswith('ccsrmm_t'):
            hip.ccsrmm_t(y_d, (D.nx, D.rows), dev['colind'], dev['indptr'], dev['vals'], x_d, alpha=ALPHA, beta=beta)
        else:
            hip.ccsrmm(y_d, (D.rows, D.nx), dev['colind'], dev['indptr'], dev['vals'], x_d, alpha=ALPHA, beta=beta)
        eq(y_d.to_host(), s.gather_reference(D, ALPHA, beta).astype(C64))


# =========================================================================================================================================
# a full sub-list: "list full -> compute inline"
# =========================================================================================================================================
@pytest.mark.parametrize("beta", (0, BETA), ids=ids)
def test_rows_that_find_their_sub_list_full_are_computed_inline(hip, beta):
    """513 tasks of 64 rows with 33 nonzeros each all hash to sub-list 0 (32768 entries): 64 rows find it full and stay with the main
    kernel (k_csrmm_dense64<1> with beta == 0, k_csrmm_rowlane with beta != 0), the others go through k_csrmm_rows_wave -- whichever
    64 they are, every row is exact"""
    case = s.Case('ccsrmm_t', 1, 'sparse', 'dense64|rowlane', lens=s.overflow_lens(), seed=901, tag='-overflow')
    D = s.build(case)
    d = s.case_dispatch(case, D, beta)
    n = s.deferral(d, D.indptr)
    assert d['main'][0] == ('dense64' if beta == 0 else 'rowlane') and n['wave'] == s.SUB_CAP and n['wave_inline'] == 64 and n['block'] == 0
    X = Panel(hip, D.xtotal, 1, D.X)
    Y = Panel(hip, D.rows, 1, None if beta == 0 else D.Y0)
    dev = dict(indptr=hip.copy_array(D.indptr), colind=hip.copy_array(D.colind), vals=hip.copy_array(D.vals))
    hip._check(call_entry(hip, D, dev, ALPHA, beta, X, Y), case.name)
    eq(Y.read(), s.gather_reference(D, ALPHA, beta).astype(C64))


# =========================================================================================================================================
# a support mask
# =========================================================================================================================================
N0 = NM = 16
NS = 2


@functools.lru_cache(maxsize=1)
def masked_case_lens():
    """512 result rows = the smallest grid grid_mask accepts (16 x 16 x 2); 11 of its 32 segments of 16 rows hold nonzeros, among them a
    row for each deferred list of the narrow kernels, the others are empty"""
    rng = np.random.default_rng(31)
    lens = np.zeros(N0 * NM * NS, dtype=np.int64)
    segs = np.sort(rng.choice(32, size=11, replace=False))
    for sgm in segs:
        lens[16 * sgm:16 * sgm + 16] = rng.choice((0, 0, 1, 1, 2, 3), size=16)
        lens[16 * sgm + rng.integers(16)] = 1                      # at least one nonzero
    lens[16 * segs[2] + 3], lens[16 * segs[5] + 15], lens[16 * segs[7]] = 17, 33, 40
    return lens, segs


@pytest.mark.parametrize("entry,N", [('t_grid', n) for n in (1, 3, 8, 64)] + [('t_grid_il', n) for n in (2, 4, 8)])
def test_support_mask_writes_flagged_segments_only(hip, entry, N):
    lens, segs = masked_case_lens()
    case = s.Case(entry, N, 'sparse', '', lens=lens, seed=77 + N, tag='-masked')
    D = s.build(case)
    assert D.nnz <= 2 * D.rows and D.nnz >= D.nx
    # the support table from the matrix whose transpose this CSR is: its touched columns are this CSR's non-empty rows
    table = fused.grid_support_numpy(s.csr_of(D, C64, conj=False).T.tocsr(), (N0, NS, NM))
    flagged = np.zeros(D.rows, dtype=bool)
    for sgm in segs:
        flagged[16 * sgm:16 * sgm + 16] = True
    table_d = hip.copy_array(table)
    dev = dict(indptr=hip.copy_array(D.indptr), colind=hip.copy_array(D.colind), vals=hip.copy_array(D.vals))
    for beta in s.betas_of(case):
        d = s.dispatch(entry, D.rows, D.nx, N, D.nnz, beta == 0, masked=True)
        assert d['main'][0] in ('dense64', 'rowlane') and s.deferral(d, D.indptr, live=flagged)['wave'] >= 2
        X = Panel(hip, D.xtotal, N, D.X)
        start = np.empty((D.rows, N), dtype=C64)
        bits(start)[:] = NAN32
        if beta != 0:
            start[flagged] = D.Y0[flagged]                       # unflagged rows keep the sentinel
        Y = Panel(hip, D.rows, N, start, il=entry == 't_grid_il')
        hip._check(call_entry(hip, D, dev, ALPHA, beta, X, Y, VP(table_d._arr), N0, NM), case.name)
        out = Y.read()
        eq(out[flagged], s.gather_reference(D, ALPHA, beta).astype(C64)[flagged])
        assert same_bits(out[~flagged], Y.payload(Y.before)[~flagged]), "a row outside the support was written"


# =========================================================================================================================================
# refusals
# =========================================================================================================================================
def test_refusals_leave_the_result_untouched(hip):
    L = hip._L

    def refused(case, needle, beta=0):
        D, dev = device_matrix(hip, case)
        X = Panel(hip, D.xtotal, D.N, D.X)
        Y = Panel(hip, D.rows, D.N, None, il=s.ENTRIES[case.entry].get('y_il', False))
        assert call_entry(hip, D, dev, ALPHA, beta, X, Y) != 0
        assert needle in L.ig_last_error(hip._ctx), L.ig_last_error(hip._ctx)
        assert same_bits(Y.dev.to_host(), Y.before), "a refused call wrote to its result"

    # an interleaved result for a matrix whose rows are not mostly empty
    lens = s.case_lens(CASE_BY_NAME['ccsrmm_t-N4-dense'])
    assert s.dispatch('t_grid_il', lens.size, 97, 4, int(lens.sum()), True)['error'] is not None
    refused(s.Case('t_grid_il', 4, 'dense', '', lens=lens, seed=5, tag='-refused'), b"mostly empty rows")
    # ... and for mostly empty rows over a panel with more rows than the matrix has nonzeros, which is not repacked
    lens = s.case_lens(CASE_BY_NAME['ccsrmm_t-N4-sparse'])
    assert s.dispatch('t_grid_il', lens.size, int(lens.sum()) + 13, 4, int(lens.sum()), True)['error'] is not None
    refused(s.Case('t_grid_il', 4, 'sparse', '', big_x=True, lens=lens, seed=6, tag='-refused'), b"dense-lane kernel")
    # a panel-row list with more than 64 columns
    small = [3, 0, 1, 2, 0, 5, 1] * 11
    assert s.dispatch('t_grid_xp', len(small), 97, 65, sum(small), True)['error'] is not None
    refused(s.Case('t_grid_xp', 65, 'sparse', '', lens=small, seed=7, tag='-refused'), b"panel-row list")
    refused(s.Case('xrows', 65, 'sparse', '', lens=small, seed=8, tag='-refused'), b"2..64 panel columns", beta=BETA)


# =========================================================================================================================================
# the adjoint of ig_ccsrmm: k_panel_scale, then k_csrmm_scatter
# =========================================================================================================================================
def run_scatter(hip, A, X, Y0, alpha, beta, exwrite, offx=0, offy=0, pad=5):
    M, K = A.shape
    N = X.shape[1]
    Xp = Panel(hip, M, N, X, off=offx)
    Yp = Panel(hip, K, N, None if s.cf32(beta) == 0 else Y0, off=offy, pad=pad)
    a, b = s.cf32(alpha), s.cf32(beta)
    one = lambda arr, dt: hip.copy_array(arr.astype(dt) if arr.size else np.zeros(1, dtype=dt))
    v_d, c_d, p_d = one(A.data, C64), one(A.indices, np.int32), hip.copy_array(A.indptr.astype(np.int32))
    hip._check(hip._L.ig_ccsrmm(hip._ctx, 1, 1 if exwrite else 0, M, K, N, A.nnz, a.real, a.imag, VP(v_d._arr), VP(c_d._arr), VP(p_d._arr),
                                Xp.ptr, Xp.ld, b.real, b.imag, Yp.ptr, Yp.ld), "ig_ccsrmm(adjoint)")
    out = Yp.read()
    Xp.unchanged()
    return out


@pytest.mark.parametrize("exwrite", FT, ids=("atomic", "exwrite"))
@pytest.mark.parametrize("spec", s.SCATTER_CASES, ids=repr)
def test_scatter_adjoint_is_exact(hip, spec, exwrite):
    N, mean, M = spec
    A, X, Y0 = s.scatter_case(N, mean, M, exwrite)
    for beta, (offx, offy), pad in ((0, (0, 0), 5), (BETA, (0, 0), 5), (1, (1, 1), 5), (0, (0, 1), 0), (BETA, (1, 0), 0)):
        out = run_scatter(hip, A, X, Y0, ALPHA, beta, exwrite, offx, offy, pad)        # pad = 0, beta = 0: the memset form of the pre-pass
        assert np.all(np.isfinite(out.view(np.float32)))
        eq(out, s.scatter_reference(A, X, Y0, ALPHA, beta).astype(C64))


# =========================================================================================================================================
# the coarse route: first-level profiling scopes
# =========================================================================================================================================
ROUTE_CASES = ('ccsrmm-N3-mid', 'ccsrmm_t-N8-sparse', 'ccsrmm-N64-dense', 'ccsrmm_t-N1-vdense', 'ccsrmm-N3-sparse-bigx', 'ccsrmm_t-N64-sparse',
               'ccsrmm-N16-dense-bigx', 'ccsrmm_t-N2-dense')
MAIN_SCOPES = {'csrmm_rowlane', 'csrmm_rowlane_conj', 'csrmm_gather', 'csrmm_gather_conj', 'csrmm_scatter_atomic', 'csrmm_scatter_exwrite'}


def profiled(hip, fn):
    hip.profile(True)
    try:
        hip.profile_report()
        fn()
        return hip.profile_report()
    finally:
        hip.profile(False)


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_first_level_scopes_are_the_ones_the_mirror_predicts(hip, name):
    case = CASE_BY_NAME[name]
    D, dev = device_matrix(hip, case)
    for beta in (0, BETA):
        d = s.case_dispatch(case, D, beta)
        x_d, y_d = hip.copy_array(np.asfortranarray(D.X)), hip.copy_array(np.asfortranarray(D.Y0))
        if case.entry == 'ccsrmm_t':
            fn = lambda: hip.ccsrmm_t(y_d, (D.nx, D.rows), dev['colind'], dev['indptr'], dev['vals'], x_d, alpha=ALPHA, beta=beta)
        else:
            fn = lambda: hip.ccsrmm(y_d, (D.rows, D.nx), dev['colind'], dev['indptr'], dev['vals'], x_d, alpha=ALPHA, beta=beta)
        rep = profiled(hip, fn)
        assert set(rep) & MAIN_SCOPES == {d['scope']}, (rep.keys(), d['scope'])
        assert ('pack_panel' in rep) == d['packs']
        assert ('csrmm_rows_wave' in rep) == any(k[0] == 'rows_wave' for k in d['deferred']) and 'csrmm_rows_block' in rep
        assert all(v['launches'] == 1 for v in rep.values()), rep
        eq(y_d.to_host(), s.gather_reference(D, ALPHA, beta).astype(C64))


@pytest.mark.parametrize("exwrite", FT, ids=("atomic", "exwrite"))
def test_scatter_scopes(hip, exwrite):
    A, X, Y0 = s.scatter_case(8, 3, 293, exwrite)
    dev = [hip.copy_array(a) for a in (A.indices.astype(np.int32), A.indptr.astype(np.int32), A.data.astype(C64))]
    for beta in (0, 1, BETA):
        x_d, y_d = hip.copy_array(np.asfortranarray(X)), hip.copy_array(np.asfortranarray(Y0))
        rep = profiled(hip, lambda: hip.ccsrmm(y_d, A.shape, dev[0], dev[1], dev[2], x_d, alpha=ALPHA, beta=beta, adjoint=True, exwrite=exwrite))
        assert set(rep) & MAIN_SCOPES == {'csrmm_scatter_exwrite' if exwrite else 'csrmm_scatter_atomic'}
        assert ('panel_scale' in rep) == (beta != 1)
        eq(y_d.to_host(), s.scatter_reference(A, X, Y0, ALPHA, beta).astype(C64))


# =========================================================================================================================================
# rounding cases
# =========================================================================================================================================
@pytest.mark.parametrize("case", s.ROUNDING_CASES, ids=repr)
def test_random_case_within_the_worst_case_bound(hip, case):
    for beta in s.betas_of(case):
        D, out = run_case(hip, case, beta, exact=False)
        ref, bound = s.gather_reference(D, ALPHA, beta), s.gather_bound(D, ALPHA, beta)
        err = np.maximum(np.abs(out.real - ref.real), np.abs(out.imag - ref.imag))
        print("%s beta %s: largest error / bound = %.3f" % (case, beta, float((err / np.maximum(bound, 1e-300)).max(initial=0.0))))
        assert np.all(err <= bound), np.argwhere(err > bound)[:8]


@pytest.mark.parametrize("exwrite", FT, ids=("atomic", "exwrite"))
def test_random_scatter_within_the_worst_case_bound(hip, exwrite):
    """(n_k + 4) 2^-23 (|alpha|_1 (|A|_1^T |X|_1)_kj + |beta|_1 |y_kj|_1) with n_k the nonzeros of column k: the same bound, the order of the
    atomic additions being free"""
    l1 = lambda z: np.abs(z.real) + np.abs(z.imag)
    for N, mean, M in ((3, 40, 37), (64, 3, 293)):
        A, X, Y0 = s.scatter_case(N, mean, M, exwrite, exact=False)
        for beta in (0, BETA):
            out = run_scatter(hip, A, X, Y0, ALPHA, beta, exwrite)
            ref = s.scatter_reference(A, X, Y0, ALPHA, beta)
            A1 = s.spp.csr_matrix((l1(A.data.astype(C128)), A.indices, A.indptr), shape=A.shape)
            n_k = np.bincount(A.indices, minlength=A.shape[1])[:, None]
            bound = (n_k + 4) * 2.0 ** -23 * (l1(s.cf32(ALPHA)) * (A1.T @ l1(X.astype(C128))) + l1(s.cf32(beta)) * l1(Y0.astype(C128)))
            err = np.maximum(np.abs(out.real - ref.real), np.abs(out.imag - ref.imag))
            assert np.all(err <= bound)
