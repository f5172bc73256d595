"""The BLAS-1 glue and the fused CG passes of ig_blas.hip, called through the C ABI, against the float64 restatement in tests/blas64.py.

Exact cases: on vectors of small integers with dyadic scalars no kernel rounds anything (tests/test_blas64_cpu.py shows it), so the
outputs must equal the reference BIT FOR BIT at any length, alignment and grid: a dropped, doubled or mis-signed element shows among
8 million where a relative tolerance would hide it.  The lengths sit around one workgroup (blas64.SMALL_N), in the capped grid where
every workgroup loops (N_MID) and where the float32 runs are flushed and restarted (N_BIG); every vector is passed 16-byte aligned and
8-byte aligned only, lies between NaN sentinels, and every scalar output lies between sentinel slots.

Rounding cases: the same calls once more on rand64c data at N_MID, within bounds that follow from the kernels' operation counts
(a bf16 or half intermediate would pass the integer cases)."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import blas64 as b64
from blas64 import C64, C128, N_BIG, N_MID, SMALL_N
from indigo_amd import _lib
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
EPS = 2.0 ** -24                    # unit roundoff of float32
NAN32 = 0x7fc0dead                  # the sentinel: a quiet NaN that any arithmetic would also spread into the results
GUARD = 8                           # sentinel items on either side (even: the item behind them is 16-byte aligned)
eq = np.testing.assert_array_equal
OFFS2 = tuple(itertools.product((0, 1), (0, 1)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Buf:
    """n items on the device between sentinels, with one spare item in front: off = 0 passes the 16-byte aligned address, off = 1
    the next item (8-byte aligned for complex64, 4-byte for float32)"""

    def __init__(self, hip, data, off=0):
        data = np.ascontiguousarray(data).reshape(-1)
        self.n, self.lo = data.size, GUARD + off
        host = np.empty(GUARD + 1 + self.n + GUARD, dtype=data.dtype)
        bits(host)[:] = NAN32
        host[self.lo:self.lo + self.n] = data
        self.before = host
        self.dev = hip.copy_array(host)
        assert self.dev._arr % 16 == 0
        self.addr = self.dev._arr + self.lo * data.dtype.itemsize
        assert self.addr % 16 == (0 if off == 0 else data.dtype.itemsize)
        self.ptr = VP(self.addr)

    def read(self):
        """the payload; the sentinels around it must be bit-identical"""
        h = self.dev.to_host()
        lo, hi = self.lo, self.lo + self.n
        assert same_bits(h[:lo], self.before[:lo]), "sentinel in front of the vector overwritten"
        assert same_bits(h[hi:], self.before[hi:]), "sentinel behind the vector overwritten"
        return h[lo:hi]

    def unchanged(self):
        assert same_bits(self.read(), self.before[self.lo:self.lo + self.n]), "an input vector was modified"


class Slots:
    """96 of the context's scalar slots, far from the ones HipBackend.cg uses, filled with NaN sentinels that carry their index"""
    BASE, COUNT = 400, 96

    def __init__(self, hip):
        self.hip = hip
        base, nslots = hip._slots()
        assert nslots >= self.BASE + self.COUNT
        self.base = base + 8 * self.BASE
        self.reset()

    def ptr(self, i):
        assert 0 <= i < self.COUNT
        return VP(self.base + 8 * i)

    def _h2d(self, i, arr):
        self.hip._check(self.hip._L.ig_copy2d(self.hip._ctx, self.ptr(i), arr.nbytes, VP(arr.ctypes.data), arr.nbytes, arr.nbytes, 1, _lib.IG_H2D),
                        "ig_copy2d(H2D)")

    def reset(self):
        self.expect = np.uint64(0x7ff8dead00000000) + np.arange(self.COUNT, dtype=np.uint64)
        self._h2d(0, self.expect)

    def put(self, i, value):
        v = np.array([value], dtype=np.float64)
        self.expect[i] = v.view(np.uint64)[0]
        self._h2d(i, v)

    def get(self, written=()):
        """all slots as doubles (ig_scalar_read); every slot outside `written` must hold the bits last put there"""
        host = np.zeros(self.COUNT, dtype=np.float64)
        self.hip._check(self.hip._L.ig_scalar_read(self.hip._ctx, self.ptr(0), self.COUNT, VP(host.ctypes.data)), "ig_scalar_read")
        keep = np.ones(self.COUNT, dtype=bool)
        keep[list(written)] = False
        bad = np.nonzero((host.view(np.uint64) != self.expect) & keep)[0]
        assert bad.size == 0, "scalar slots %s overwritten" % (bad + self.BASE).tolist()
        return host


@pytest.fixture(scope="module")
def slots(hip):
    return Slots(hip)


def call(hip, name, *args):
    hip._check(getattr(hip._L, name)(hip._ctx, *args), name)


def nan_like(n):
    return np.full(n, np.nan + 1j * np.nan, dtype=C64)


# =========================================================================================================================================
# the fused CG iteration
# =========================================================================================================================================
RR, R0, ALPHA, RRN, HIST = 11, 21, 31, 41, 51          # every one between sentinel slots
CG_MASKS = ((), ('x',), ('p',), ('r',), ('Ap',), ('x', 'p', 'r', 'Ap'))


def run_cg(hip, S, case, mask=(), with_hist=True, **over):
    """ig_cg_dot -> ig_cg_step_r -> ig_cg_step_xp on the case's vectors (those named in `mask` 8-byte aligned only); -> every output"""
    c = dict(case, **over)
    n = c['p'].size
    v = {k: Buf(hip, c[k], 1 if k in mask else 0) for k in ('p', 'Ap', 'r', 'x')}
    S.reset()
    S.put(RR, c['rr'])
    S.put(R0, c['r0'])
    call(hip, 'ig_cg_dot', n, v['p'].ptr, v['Ap'].ptr, ctypes.c_float(c['lamda']))
    out = dict(Ap=v['Ap'].read())
    v['p'].unchanged()
    call(hip, 'ig_cg_step_r', n, v['r'].ptr, v['Ap'].ptr, S.ptr(RR), S.ptr(R0), ctypes.c_double(c['tol2']), S.ptr(ALPHA))
    assert same_bits(v['Ap'].read(), out['Ap'])
    call(hip, 'ig_cg_step_xp', n, v['x'].ptr, v['p'].ptr, v['r'].ptr, S.ptr(ALPHA), S.ptr(RR), S.ptr(RRN), S.ptr(R0),
         S.ptr(HIST) if with_hist else None)
    s = S.get(written=(ALPHA, RRN, HIST) if with_hist else (ALPHA, RRN))
    out.update(r=v['r'].read(), x=v['x'].read(), p=v['p'].read(), alpha=s[ALPHA], rr_next=s[RRN], hist=s[HIST] if with_hist else None)
    return out


def check_cg_exact(out, ref, case):
    eq(out['Ap'], ref['Ap'].astype(C64))
    if case['lamda'] == 0:
        assert same_bits(out['Ap'], case['Ap'])                            # not written at all
    eq(out['r'], ref['r'].astype(C64))
    eq(out['x'], ref['x'].astype(C64))
    assert out['alpha'] == ref['alpha'] and out['alpha'] != 0
    assert case['rr'] / out['alpha'] == ref['pap']                          # <p, Ap>, recovered from the step length
    assert out['rr_next'] == ref['r2']
    assert b64.ulp64(out['hist'], ref['hist']) <= 2                         # a double division on the device
    assert b64.ulp32(out['p'], ref['p']) <= 1                               # beta is not dyadic: one correctly rounded fma per component


def cg_reference(n, lamda, k):
    c = b64.exact_cg_case(n, 7 * n + k, lamda, k)
    return c, b64.cg_iteration(n, c['p'], c['Ap'], c['r'], c['x'], lamda, c['rr'], c['r0'], c['tol2'])


cg_reference_cached = functools.lru_cache(maxsize=8)(cg_reference)


@pytest.mark.parametrize("n", SMALL_N)
def test_cg_iteration_exact_small(hip, slots, n):
    for lamda, k in itertools.product(b64.CG_LAMDAS, b64.CG_KS):
        case, ref = cg_reference_cached(n, lamda, k)
        for mask in CG_MASKS:
            check_cg_exact(run_cg(hip, slots, case, mask), ref, case)


@pytest.mark.parametrize("lamda,k", list(itertools.product(b64.CG_LAMDAS, b64.CG_KS)))
def test_cg_iteration_exact_capped_grid(hip, slots, lamda, k):
    """N_MID: 2048 workgroups, every thread loops, a partial second trip and an odd tail; the three calls of an iteration take
    different 16-byte / 8-byte paths under the masks and must still agree on the number of block partials"""
    case, ref = cg_reference_cached(N_MID, lamda, k)
    for mask in CG_MASKS:
        check_cg_exact(run_cg(hip, slots, case, mask), ref, case)


def test_cg_iteration_exact_float_runs_restart(hip, slots):
    """N_BIG: some threads make a ninth trip, so the 8-trip float32 run is flushed into the double and a second run starts"""
    case, ref = cg_reference(N_BIG, 0.5, 3)
    check_cg_exact(run_cg(hip, slots, case, ()), ref, case)
    check_cg_exact(run_cg(hip, slots, case, ('x', 'p', 'r', 'Ap')), ref, case)


def test_cg_iteration_is_deterministic(hip, slots):
    case, _ = cg_reference_cached(N_MID, 0.5, 3)
    a = run_cg(hip, slots, case, ('r',))
    b = run_cg(hip, slots, case, ('r',))
    for name in ('Ap', 'r', 'x', 'p'):
        assert same_bits(a[name], b[name]), name
    for name in ('alpha', 'rr_next', 'hist'):
        assert np.float64(a[name]).view(np.uint64) == np.float64(b[name]).view(np.uint64), name


def test_cg_gates(hip, slots):
    n = 1000
    case = b64.exact_cg_case(n, 3, 0.5, 1)
    ref = lambda **over: (lambda c: b64.cg_iteration(n, c['p'], c['Ap'], c['r'], c['x'], c['lamda'], c['rr'], c['r0'], c['tol2']))(dict(case, **over))
    # stopped by the tolerance: rr just below tol2 * r0 -> alpha is exactly 0, r and x keep their bits, rr_next is the exact ||r||^2
    tol2, r0 = 2.0 ** -10, case['rr'] * 2.0 ** 10
    below = dict(rr=float(np.nextafter(case['rr'], 0)), r0=r0, tol2=tol2)
    out = run_cg(hip, slots, case, **below)
    assert out['alpha'] == 0.0 and same_bits(out['r'], case['r']) and same_bits(out['x'], case['x'])
    assert out['rr_next'] == b64.nrm2sq(case['r']) == ref(**below)['rr_next']
    eq(out['Ap'], ref(**below)['Ap'].astype(C64))
    assert b64.ulp32(out['p'], ref(**below)['p']) <= 1
    # rr exactly tol2 * r0 is not stopped
    at = dict(r0=r0, tol2=tol2)
    out = run_cg(hip, slots, case, **at)
    assert out['alpha'] == 0.5
    check_cg_exact(out, ref(**at), case)
    # <p, Ap> == 0 (Ap = 0, lamda = 0): a zero step, nothing NaN or Inf anywhere
    zero = dict(Ap=np.zeros(n, dtype=C64), lamda=0.0)
    out = run_cg(hip, slots, case, **zero)
    assert out['alpha'] == 0.0 and same_bits(out['r'], case['r']) and same_bits(out['x'], case['x']) and not out['Ap'].any()
    assert all(np.isfinite(out[name]).all() for name in ('Ap', 'r', 'x', 'p', 'alpha', 'rr_next', 'hist'))
    assert out['rr_next'] == b64.nrm2sq(case['r']) and b64.ulp32(out['p'], ref(**zero)['p']) <= 1
    # rr == 0: beta = 0 and p' == r' bitwise
    out = run_cg(hip, slots, case, rr=0.0, tol2=0.0)
    assert out['alpha'] == 0.0 and same_bits(out['p'], out['r']) and same_bits(out['r'], case['r']) and np.isfinite(out['hist'])
    # r0 == 0: the history entry is 0 and the step is taken as usual
    out = run_cg(hip, slots, case, r0=0.0)
    assert out['hist'] == 0.0 and np.float64(out['hist']).view(np.uint64) == 0 and out['alpha'] == 0.5
    eq(out['r'], ref(r0=0.0)['r'].astype(C64))
    # d_hist == NULL is accepted and changes nothing else (run_cg sees the HIST slot keep its sentinel)
    full, nohist = run_cg(hip, slots, case), run_cg(hip, slots, case, with_hist=False)
    for name in ('Ap', 'r', 'x', 'p'):
        assert same_bits(full[name], nohist[name]), name
    assert full['alpha'] == nohist['alpha'] and full['rr_next'] == nohist['rr_next'] and nohist['hist'] is None


def test_cg_error_returns_leave_the_vectors_alone(hip, slots):
    L, ctx = hip._L, hip._ctx
    n = 513
    case = b64.exact_cg_case(n, 4, 0.5, 0)
    v = {k: Buf(hip, case[k]) for k in ('p', 'Ap', 'r', 'x')}
    slots.reset()
    slots.put(RR, case['rr'])
    slots.put(R0, case['r0'])
    slots.put(ALPHA, 0.5)
    S, lam, tol2 = slots.ptr, ctypes.c_float(0.5), ctypes.c_double(case['tol2'])
    bad = [
        lambda: L.ig_cg_dot(ctx, 0, v['p'].ptr, v['Ap'].ptr, lam),
        lambda: L.ig_cg_dot(ctx, -1, v['p'].ptr, v['Ap'].ptr, lam),
        lambda: L.ig_cg_dot(ctx, n, None, v['Ap'].ptr, lam),
        lambda: L.ig_cg_dot(ctx, n, v['p'].ptr, None, lam),
        lambda: L.ig_cg_step_r(ctx, 0, v['r'].ptr, v['Ap'].ptr, S(RR), S(R0), tol2, S(ALPHA)),
        lambda: L.ig_cg_step_r(ctx, n, None, v['Ap'].ptr, S(RR), S(R0), tol2, S(ALPHA)),
        lambda: L.ig_cg_step_r(ctx, n, v['r'].ptr, None, S(RR), S(R0), tol2, S(ALPHA)),
        lambda: L.ig_cg_step_xp(ctx, -5, v['x'].ptr, v['p'].ptr, v['r'].ptr, S(ALPHA), S(RR), S(RRN), S(R0), S(HIST)),
        lambda: L.ig_cg_step_xp(ctx, n, None, v['p'].ptr, v['r'].ptr, S(ALPHA), S(RR), S(RRN), S(R0), S(HIST)),
        lambda: L.ig_cg_step_xp(ctx, n, v['x'].ptr, None, v['r'].ptr, S(ALPHA), S(RR), S(RRN), S(R0), S(HIST)),
        lambda: L.ig_cg_step_xp(ctx, n, v['x'].ptr, v['p'].ptr, None, S(ALPHA), S(RR), S(RRN), S(R0), S(HIST)),
        lambda: L.ig_cg_step_xp(ctx, n, v['x'].ptr, v['p'].ptr, v['r'].ptr, S(ALPHA), S(RR), S(RR), S(R0), S(HIST)),      # rr == rr_next
    ]
    for i, f in enumerate(bad):
        assert f() != 0, i
        msg = L.ig_last_error(ctx)
        assert msg and b"ig_cg_" in msg, (i, msg)
    hip.barrier()
    for b in v.values():
        b.unchanged()
    slots.get()                                                             # no slot written either


# =========================================================================================================================================
# reductions
# =========================================================================================================================================
DOT, NRM = 61, 71


def check_reductions(hip, S, x, y, offsets):
    n = x.size
    ref_dot, ref_nrm = b64.dotc(x, y), b64.nrm2sq(x)
    for xo, yo in offsets:
        bx, by = Buf(hip, x, xo), Buf(hip, y, yo)
        S.reset()
        host = []
        for _ in range(2):
            out, nrm = (ctypes.c_double * 2)(np.nan, np.nan), ctypes.c_double(np.nan)
            call(hip, 'ig_cdotc', n, bx.ptr, by.ptr, out)
            call(hip, 'ig_scnrm2sq', n, bx.ptr, ctypes.byref(nrm))
            call(hip, 'ig_cdotc_dev', n, bx.ptr, by.ptr, S.ptr(DOT))
            call(hip, 'ig_scnrm2sq_dev', n, bx.ptr, S.ptr(NRM))
            s = S.get(written=(DOT, DOT + 1, NRM))            # the dot writes exactly two doubles, the norm exactly one
            host.append((out[0], out[1], nrm.value, s[DOT], s[DOT + 1], s[NRM]))
        assert host[0] == host[1]                             # two calls, the same bits (all finite: == is bitwise up to the sign of 0)
        assert host[0][:2] == ref_dot and host[0][2] == ref_nrm, (n, xo, yo, host[0], ref_dot, ref_nrm)
        assert host[0][3:5] == ref_dot and host[0][5] == ref_nrm
        bx.unchanged()
        by.unchanged()


@pytest.mark.parametrize("n", SMALL_N + (N_MID,))
def test_reductions_exact(hip, slots, n):
    x, y = b64.exact_inputs(n, n + 1, 2)
    check_reductions(hip, slots, x, y, OFFS2)


def test_reductions_exact_second_float_run(hip, slots):
    """N_BIG > 16 * 2048 * 256: k_reduce flushes its 16-element float32 run and starts another"""
    x, y = b64.exact_inputs(N_BIG, N_BIG + 1, 2)
    check_reductions(hip, slots, x, y, ((0, 0),))


def test_reductions_of_nothing(hip, slots):
    out, nrm = (ctypes.c_double * 2)(np.nan, np.nan), ctypes.c_double(np.nan)
    call(hip, 'ig_cdotc', 0, None, None, out)
    call(hip, 'ig_scnrm2sq', 0, None, ctypes.byref(nrm))
    assert (out[0], out[1], nrm.value) == (0.0, 0.0, 0.0)
    slots.reset()
    call(hip, 'ig_cdotc_dev', 0, None, None, slots.ptr(DOT))
    call(hip, 'ig_scnrm2sq_dev', 0, None, slots.ptr(NRM))
    s = slots.get(written=(DOT, DOT + 1, NRM))
    assert not s[[DOT, DOT + 1, NRM]].view(np.uint64).any()


# =========================================================================================================================================
# elementwise: ig_caxpby / ig_cscal / ig_caxpby_dev / ig_cmax
# =========================================================================================================================================
def run_axpby(hip, beta, by, alpha, bx):
    if alpha == 0 and bx is None:
        call(hip, 'ig_cscal', by.n, *_lib.cplx(beta), by.ptr)
    else:
        call(hip, 'ig_caxpby', by.n, *_lib.cplx(beta), by.ptr, *_lib.cplx(alpha), bx.ptr)
    return by.read()


@pytest.mark.parametrize("n", SMALL_N + (N_MID,))
def test_axpby_and_scal_exact(hip, n):
    """the four kernel modes (beta = 0 over a NaN-filled y, beta = 1, general, alpha = 0), x and y aligned and not in every combination"""
    x, y = b64.exact_inputs(n, n, 2)
    for xo in (0, 1):
        bx = Buf(hip, x, xo)
        for (beta, alpha), yo in itertools.product(b64.AXPBY_SCALARS, (0, 1)):
            ref = b64.axpby(beta, y, alpha, x).astype(C64)
            by = Buf(hip, nan_like(n) if beta == 0 else y, yo)
            # (alpha = 0 ignores x: once through ig_caxpby, once through ig_cscal, which passes no x)
            got = run_axpby(hip, beta, by, alpha, None if (alpha == 0 and xo == 1) else bx)
            assert not np.isnan(got).any(), (beta, alpha, xo, yo)
            eq(got, ref, err_msg=str((beta, alpha, xo, yo)))
        bx.unchanged()


def test_axpby_exact_eight_million(hip):
    x, y = b64.exact_inputs(N_BIG, 5, 2)
    beta, alpha = 1.5 - 0.25j, 0.5j
    eq(run_axpby(hip, beta, Buf(hip, y), alpha, Buf(hip, x)), b64.axpby(beta, y, alpha, x).astype(C64))


@pytest.mark.parametrize("n", (3, 513))
def test_axpby_paths_without_a_kernel(hip, n):
    x = b64.exact_inputs(n, n, 1)[0]
    for yo in (0, 1):
        # both scalars zero: zeros, whatever y held
        by = Buf(hip, nan_like(n), yo)
        got = run_axpby(hip, 0, by, 0, Buf(hip, x))
        assert not bits(got).any()
        by = Buf(hip, nan_like(n), yo)
        assert not bits(run_axpby(hip, 0, by, 0, None)).any()
        # alpha = 0, beta = 1: y keeps its bits, NaNs included
        y = x.copy()
        y[::2] = np.nan
        by = Buf(hip, y, yo)
        run_axpby(hip, 1, by, 0, Buf(hip, x))
        by.unchanged()
        run_axpby(hip, 1, by, 0, None)
        by.unchanged()


SB, SA = 81, 85


@pytest.mark.parametrize("n", (3, 513, N_MID))
def test_axpby_with_device_scalars_exact(hip, slots, n):
    x, y = b64.exact_inputs(n, n + 2, 2)
    slots.reset()
    slots.put(SB, b64.DEV_BETA)
    slots.put(SA, b64.DEV_ALPHA)
    for xo, yo in ((0, 0), (1, 1), (1, 0)):
        bx = Buf(hip, x, xo)
        for d_beta, bs, d_alpha in b64.DEV_COMBOS:
            by = Buf(hip, y, yo)
            call(hip, 'ig_caxpby_dev', n, None if d_beta is None else slots.ptr(SB), ctypes.c_float(bs), by.ptr,
                 None if d_alpha is None else slots.ptr(SA), ctypes.c_float(b64.DEV_ALPHA_SCALE), bx.ptr)
            eq(by.read(), b64.axpby_dev(d_beta, bs, y, d_alpha, b64.DEV_ALPHA_SCALE, x).astype(C64), err_msg=str((d_beta, bs, d_alpha, xo, yo)))
        bx.unchanged()
    slots.get()


@pytest.mark.parametrize("nfloats", (1, 3, 5, 1025, 4 * 2048 * 256 + 7))
def test_cmax_bitwise(hip, nfloats):
    rng = np.random.default_rng(nfloats)
    a = rng.standard_normal(nfloats).astype(np.float32)
    a[a == 0] = 1.0
    for off, val in itertools.product((0, 1), (0.25, -0.5)):
        b = Buf(hip, a, off)
        call(hip, 'ig_cmax', nfloats, ctypes.c_float(val), b.ptr)
        assert same_bits(b.read(), b64.smax(val, a)), (off, val)
        assert same_bits(b64.smax(val, a), np.maximum(a, np.float32(val)))


# =========================================================================================================================================
# scalar programs
# =========================================================================================================================================
def test_scalar_ratio_programs(hip, slots):
    NUM, DEN, OUT, GN, GD = 3, 5, 7, 9, 13
    S = slots

    def ratio(num, den, scale):
        S.reset()
        S.put(NUM, num)
        S.put(DEN, den)
        call(hip, 'ig_scalar_ratio', S.ptr(OUT), S.ptr(NUM), S.ptr(DEN), ctypes.c_double(scale))
        return S.get(written=(OUT,))[OUT]

    def gated(num, den, scale, gn, gd, tol):
        S.reset()
        for i, v in ((NUM, num), (DEN, den), (GN, gn), (GD, gd)):
            S.put(i, v)
        call(hip, 'ig_scalar_ratio_gated', S.ptr(OUT), S.ptr(NUM), S.ptr(DEN), ctypes.c_double(scale), S.ptr(GN), S.ptr(GD), ctypes.c_double(tol))
        return S.get(written=(OUT,))[OUT]

    for num, den, scale in ((3.0, 4.0, 1.0), (3.0, 4.0, -2.0), (1.0, 3.0, -0.7), (3.0, 0.0, 1.0), (0.0, 0.0, -1.0)):
        got = ratio(num, den, scale)
        assert got == b64.scalar_ratio(num, den, scale) and np.isfinite(got), (num, den, scale)
    assert ratio(3.0, 0.0, 1.0) == 0.0 and ratio(3.0, 4.0, -2.0) == -1.5
    edge = float(np.nextafter(1.0, 0))
    for gn in (2.0, 1.0, edge, 0.0):                       # above the gate, at equality (not stopped), just below, far below
        got = gated(1.0, 3.0, 2.0, gn, 4.0, 0.25)
        assert got == b64.scalar_ratio_gated(1.0, 3.0, 2.0, gn, 4.0, 0.25), gn
        assert (got == 0.0) == (gn < 1.0)
    assert gated(1.0, 0.0, 2.0, 2.0, 4.0, 0.25) == 0.0
    # bad arguments
    L, ctx = hip._L, hip._ctx
    assert L.ig_scalar_ratio(ctx, None, S.ptr(NUM), S.ptr(DEN), 1.0) != 0 and b"ig_scalar_ratio" in L.ig_last_error(ctx)
    assert L.ig_scalar_ratio_gated(ctx, S.ptr(OUT), S.ptr(NUM), S.ptr(DEN), 1.0, None, S.ptr(GD), 1.0) != 0


def test_scalar_copy_and_read(hip, slots):
    L, ctx = hip._L, hip._ctx
    src = np.arange(1, 1001, dtype=np.float64) * 0.37
    bs = Buf(hip, src)
    for count in (0, 1, 65, 1000):
        bd = Buf(hip, -src)
        call(hip, 'ig_scalar_copy', bd.ptr, bs.ptr, count)
        got = bd.read()
        assert same_bits(got[:count], src[:count]) and same_bits(got[count:], -src[count:]), count
    bd = Buf(hip, np.zeros(5000))
    big = Buf(hip, np.ones(5000))
    assert L.ig_scalar_copy(ctx, bd.ptr, big.ptr, 4097) != 0 and b"ig_scalar_copy" in L.ig_last_error(ctx)
    assert L.ig_scalar_copy(ctx, bd.ptr, big.ptr, -1) != 0
    hip.barrier()
    assert not bd.read().any()
    call(hip, 'ig_scalar_copy', bd.ptr, big.ptr, 4096)
    assert bd.read()[:4096].all() and not bd.read()[4096:].any()
    bs.unchanged()
    # reading nothing leaves the host buffer alone
    host = np.full(4, -3.5)
    call(hip, 'ig_scalar_read', bs.ptr, 0, VP(host.ctypes.data))
    eq(host, np.full(4, -3.5))
    call(hip, 'ig_scalar_read', bs.ptr, 3, VP(host.ctypes.data))
    eq(host, np.concatenate([src[:3], [-3.5]]))


# =========================================================================================================================================
# coil sums
# =========================================================================================================================================
def run_csum_il(hip, X, y_in, alpha, beta, xo, yo):
    rows, ncols = X.shape
    bX, by = Buf(hip, X, xo), Buf(hip, y_in, yo)              # (C order: the rows are contiguous)
    call(hip, 'ig_csum_il', rows, ncols, bX.ptr, *_lib.cplx(alpha), *_lib.cplx(beta), by.ptr)
    got = by.read()
    bX.unchanged()
    return got


def check_csum_il(hip, rows, ncols):
    X = b64.exact_inputs(rows * ncols, rows + ncols, 1)[0].reshape(rows, ncols)
    y = b64.exact_inputs(rows, rows, 1)[0]
    for beta, alpha in b64.CSUM_SCALARS:
        ref = b64.csum_il(X, alpha, beta, y).astype(C64)
        y_in = nan_like(rows) if beta == 0 else y
        # X offset by one element cannot take a 16-byte path: the generic kernel, the same bits
        first = None
        for xo, yo in OFFS2:
            got = run_csum_il(hip, X, y_in, alpha, beta, xo, yo)
            assert not np.isnan(got).any()
            eq(got, ref, err_msg=str((rows, ncols, beta, alpha, xo, yo)))
            first = got if first is None else first
            assert same_bits(got, first), (rows, ncols, beta, alpha, xo, yo)


@pytest.mark.parametrize("ncols", b64.CSUM_NCOLS)
def test_csum_il_exact(hip, ncols):
    """1, 3, 7: odd; 6, 64: the generic 16-byte path; 2 ... 32: PARTS lanes per row and shuffles, rows * PARTS no multiple of 64"""
    for rows in b64.CSUM_ROWS:
        check_csum_il(hip, rows, ncols)


def test_csum_il_exact_rows_beyond_the_grid(hip):
    check_csum_il(hip, 40000, 32)                               # 40000 * 16 lanes > 2048 * 256: the shuffle kernel loops


def run_csum_cols(hip, panel, rows, ncols, ldx, y_in, alpha, beta, yo=0):
    bX, by = Buf(hip, panel), Buf(hip, y_in, yo)
    call(hip, 'ig_csum_cols', rows, ncols, bX.ptr if ncols else None, ldx, *_lib.cplx(alpha), *_lib.cplx(beta), by.ptr)
    got = by.read()
    bX.unchanged()
    return got


@pytest.mark.parametrize("rows,ncols", [(257, 1), (257, 7), (1001, 64), (600001, 2)])
def test_csum_cols_exact(hip, rows, ncols):
    ldx = rows + 3
    X = b64.exact_inputs(rows * ncols, rows + ncols, 1)[0].reshape(rows, ncols, order='F')
    panel = np.full((ldx, ncols), np.nan + 1j * np.nan, dtype=C64, order='F')          # NaN rows between the columns
    panel[:rows] = X
    y = b64.exact_inputs(rows, rows, 1)[0]
    for (beta, alpha), yo in itertools.product(b64.CSUM_SCALARS, (0, 1)):
        got = run_csum_cols(hip, panel.reshape(-1, order='F'), rows, ncols, ldx, nan_like(rows) if beta == 0 else y, alpha, beta, yo)
        eq(got, b64.csum_cols(X, alpha, beta, y).astype(C64), err_msg=str((beta, alpha, yo)))


def test_csum_cols_of_no_columns(hip):
    rows = 257
    y = b64.exact_inputs(rows, 1, 1)[0]
    got = run_csum_cols(hip, np.zeros(4, C64), rows, 0, rows, y, 0.5 - 1j, 0.5)
    eq(got, (0.5 * y.astype(C128)).astype(C64))
    got = run_csum_cols(hip, np.zeros(4, C64), rows, 0, rows, nan_like(rows), 0.5 - 1j, 0)
    assert not got.any()


# =========================================================================================================================================
# the Python layer: a row-sliced 2-d view is handled column by column
# =========================================================================================================================================
def test_axpby_and_scale_on_row_sliced_views(hip):
    rows, ncols, lo, hi = 37, 5, 3, 30
    X = b64.exact_inputs(rows * ncols, 1, 1)[0].reshape(rows, ncols, order='F')
    Y = b64.exact_inputs(rows * ncols, 2, 1)[0].reshape(rows, ncols, order='F')
    Y[:lo] = np.nan                                                                     # rows between the columns: must keep their bits
    beta, alpha = 1.5 - 0.25j, 0.5j
    x_d, y_d = hip.copy_array(np.asfortranarray(X)), hip.copy_array(np.asfortranarray(Y))
    xv, yv = x_d[lo:hi, :], y_d[lo:hi, :]
    assert not yv.contiguous and yv._leading_dim == rows > hi - lo

    def check(exp):
        got = y_d.to_host()
        eq(got[lo:hi], exp[lo:hi])                                                      # (values: an exact zero may carry either sign)
        assert same_bits(got[:lo], Y[:lo]) and same_bits(got[hi:], Y[hi:])              # the rows outside the view keep their bits

    hip.axpby(beta, yv, alpha, xv)
    exp = Y.copy()
    exp[lo:hi] = b64.axpby(beta, Y[lo:hi], alpha, X[lo:hi]).astype(C64)
    check(exp)
    hip.scale(yv, -2)
    exp[lo:hi] = b64.axpby(-2, exp[lo:hi], 0, None).astype(C64)
    check(exp)
    assert same_bits(x_d.to_host(), X)


# =========================================================================================================================================
# rounding on real-valued data, N_MID elements
# =========================================================================================================================================
def within(got, ref, bound, what):
    err = np.abs(np.asarray(got, dtype=C128) - ref)
    worst = float(np.max(err / bound))
    print("%s: worst |got - ref| / bound = %.3f" % (what, worst))
    assert worst <= 1.0, what


def elementwise_bound(beta, y, alpha, x):
    """8 * 2^-24 * (|beta||y| + |alpha||x|) on the complex difference: each component is a sum of four real products built with at
    most four roundings (one for a product, one per fused multiply-add), each at most 2^-24 times the sum of the products'
    magnitudes, which is at most |beta||y| + |alpha||x|; sqrt(2) for the two components: 4 sqrt(2) < 8.  ig_caxpby_dev rounds
    the product scale * slot once more (5 sqrt(2) < 8)."""
    return 8 * EPS * (abs(beta) * np.abs(y.astype(C128)) + abs(alpha) * np.abs(x.astype(C128)))


def test_elementwise_rounding(hip, slots):
    n = N_MID
    x, y = rand64c(n, seed=31), rand64c(n, seed=32)
    bx = Buf(hip, x)
    for beta, alpha in ((0, 1.2 + 3j), (1, -2.1), (1.5 - 1j, 1.2 + 3j), (0.3 - 0.7j, 0)):
        got = run_axpby(hip, beta, Buf(hip, y), alpha, bx)
        within(got, b64.axpby(beta, y, alpha, x), elementwise_bound(b64.cf32(beta), y, b64.cf32(alpha), x), "axpby %s %s" % (beta, alpha))
    slots.reset()
    slots.put(SB, 0.7)
    slots.put(SA, 1.3)
    by = Buf(hip, y, 1)
    call(hip, 'ig_caxpby_dev', n, slots.ptr(SB), ctypes.c_float(0.5), by.ptr, slots.ptr(SA), ctypes.c_float(-0.3), bx.ptr)
    within(by.read(), b64.axpby_dev(0.7, 0.5, y, 1.3, -0.3, x), elementwise_bound(0.5 * 0.7, y, 0.3 * 1.3, x), "axpby_dev")


def test_reduction_rounding(hip):
    """64 * 2^-24 * sum |terms|: a float32 run is 16 elements of two fused multiply-adds per component, 32 roundings, each at most
    2^-24 times the run's sum of magnitudes; doubled for margin.  From the runs upwards the sums are double."""
    n = N_MID
    x, y = rand64c(n, seed=33), rand64c(n, seed=34)
    bx, by = Buf(hip, x, 1), Buf(hip, y)
    out, nrm = (ctypes.c_double * 2)(), ctypes.c_double()
    call(hip, 'ig_cdotc', n, bx.ptr, by.ptr, out)
    call(hip, 'ig_scnrm2sq', n, bx.ptr, ctypes.byref(nrm))
    re, im = b64.dotc(x, y)
    bound = 64 * EPS * float(np.sum(np.abs(x.astype(C128)) * np.abs(y.astype(C128))))
    print("dot: errors %.3e %.3e, bound %.3e;  norm: error %.3e, bound %.3e" % (abs(out[0] - re), abs(out[1] - im), bound, abs(nrm.value - b64.nrm2sq(x)),
                                                                                 64 * EPS * b64.nrm2sq(x)))
    assert abs(out[0] - re) <= bound and abs(out[1] - im) <= bound
    assert abs(nrm.value - b64.nrm2sq(x)) <= 64 * EPS * b64.nrm2sq(x)


def test_cg_rounding(hip, slots):
    """Each pass against the restatement of THAT pass on the device's own inputs to it (the previous pass's output as read back), so
    that every bound is one kernel's.  Reductions: a float32 run of the CG passes is 8 trips of two elements, per element one
    product, one fused multiply-add and one addition to the run: 48 roundings, each at most 2^-24 times the run's sum of magnitudes;
    64 * 2^-24 * sum |terms| covers them.  <p, Ap> is recovered as rr / alpha: two double divisions, 2^-50 relative."""
    n, lamda = N_MID, 0.05
    p, Ap, r, x = (rand64c(n, seed=s) for s in (41, 42, 43, 44))
    rr = b64.nrm2sq(r)
    case = dict(p=p, Ap=Ap, r=r, x=x, lamda=lamda, rr=rr, r0=4.0 * rr, tol2=1e-20)
    out = run_cg(hip, slots, case, ('x',))
    lam32 = b64.f32(lamda)
    within(out['Ap'], b64.cg_dot(p, Ap, lamda)[0], elementwise_bound(1, Ap, lam32, p), "cg_dot Ap")
    pap_ref = b64.cg_dot(p, out['Ap'], 0.0)[1]
    pap_dev = rr / out['alpha']
    bound = (64 * EPS + 2.0 ** -50) * float(np.sum(np.abs(p.astype(C128)) * np.abs(out['Ap'].astype(C128))))
    print("pap: error %.3e, bound %.3e" % (abs(pap_dev - pap_ref), bound))
    assert abs(pap_dev - pap_ref) <= bound
    a32 = b64.f32(out['alpha'])
    within(out['r'], b64.axpby_dev(None, 1.0, r, out['alpha'], -1.0, out['Ap']), elementwise_bound(1, r, a32, out['Ap']), "cg_step_r r")
    r2_ref = b64.nrm2sq(out['r'])
    print("r2: error %.3e, bound %.3e" % (abs(out['rr_next'] - r2_ref), 64 * EPS * r2_ref))
    assert abs(out['rr_next'] - r2_ref) <= 64 * EPS * r2_ref
    beta = out['rr_next'] / rr
    within(out['x'], b64.axpby_dev(None, 1.0, x, out['alpha'], 1.0, p), elementwise_bound(1, x, a32, p), "cg_step_xp x")
    within(out['p'], b64.axpby_dev(beta, 1.0, p, None, 1.0, out['r']), elementwise_bound(b64.f32(beta), p, 1, out['r']), "cg_step_xp p")
    assert b64.ulp64(out['hist'], out['rr_next'] / case['r0']) <= 2


def test_coil_sum_rounding(hip):
    """2 (ncols + 4) * 2^-24 * (|alpha| sum_j |X_kj| + |beta||y_k|): summing a row takes at most ncols roundings per component
    (one per column in the sequential kernels, fewer in the shuffle tree), alpha times the sum two, beta y two more, each at most
    2^-24 times the magnitudes' sum; sqrt(2) < 2 for the two components"""
    beta, alpha = 0.3 - 0.7j, 1.2 + 3j
    for rows, ncols in ((N_MID // 32 + 1, 32), (N_MID // 6 + 1, 6), (N_MID // 7, 7)):
        X, y = rand64c(rows, ncols, seed=rows, order='C'), rand64c(rows, seed=ncols)
        bound = 2 * (ncols + 4) * EPS * (abs(alpha) * np.abs(X.astype(C128)).sum(axis=1) + abs(beta) * np.abs(y.astype(C128)))
        within(run_csum_il(hip, X, y, alpha, beta, 0, 0), b64.csum_il(X, alpha, beta, y), bound, "csum_il %d" % ncols)
        Xf = np.asfortranarray(X)
        got = run_csum_cols(hip, Xf.reshape(-1, order='F'), rows, ncols, rows, y, alpha, beta)
        within(got, b64.csum_cols(X, alpha, beta, y), bound, "csum_cols %d" % ncols)
