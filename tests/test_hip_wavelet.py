"""The wavelet transform, the soft threshold and pics --l1 on the MI355X: ig_dwt3_c64 / ig_csoft_c64 against the float64
restatement in tests/dwt64.py, and the FISTA driver against the same driver on the numpy oracle backend."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

import dwt64
import dwt_cases
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _dwt(hip, x, dims, wavelet, levels, inverse=False, alpha=1, beta=0, y0=None, pad=0):
    """dwt3 of the panel x (n x ncols) into a panel with `pad` extra rows (leading dimension n + pad); y starts as y0 or NaN"""
    n, ncols = x.shape
    xp = np.zeros((n + pad, ncols), dtype=C64, order='F')
    xp[:n] = x
    yp = np.full((n + pad, ncols), np.nan, dtype=C64, order='F')
    if y0 is not None:
        yp[:n] = y0
    x_d, y_d = hip.copy_array(xp), hip.copy_array(yp)
    hip.dwt3(y_d[:n], x_d[:n], dims, wavelet, levels, inverse=inverse, alpha=alpha, beta=beta)
    out = y_d.to_host()
    if pad:
        assert np.array_equal(out[n:], yp[n:], equal_nan=True)          # the rows between columns are left alone
    return out[:n]


@pytest.mark.parametrize("dims", [(16, 16, 16), (64, 48, 40)])
@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("wavelet", ["haar", "db2", "db4"])
def test_dwt3_matches_the_float64_transform(hip, wavelet, levels, dims):
    n = int(np.prod(dims))
    x = rand64c(n, 1, seed=levels) - (0.5 + 0.5j)
    ref = dwt64.dwt(x, dims, wavelet, levels)
    fwd = _dwt(hip, x, dims, wavelet, levels)                           # y starts as NaN: beta == 0 does not read it
    assert np.isfinite(fwd).all()
    assert _rel(fwd, ref) < 2e-6, _rel(fwd, ref)
    inv = _dwt(hip, ref.astype(C64), dims, wavelet, levels, inverse=True)
    assert _rel(inv, x) < 2e-6, _rel(inv, x)
    back = _dwt(hip, fwd, dims, wavelet, levels, inverse=True)
    assert _rel(back, x) < 2e-6, _rel(back, x)
    # in place, both directions
    x_d = hip.copy_array(x)
    hip.dwt3(x_d, x_d, dims, wavelet, levels)
    assert _rel(x_d.to_host(), ref) < 2e-6
    hip.dwt3(x_d, x_d, dims, wavelet, levels, inverse=True)
    assert _rel(x_d.to_host(), x) < 2e-6
    # adjoint identity <W x, y> = <x, W^H y>
    y = rand64c(n, 1, seed=7 + levels) - (0.5 + 0.5j)
    wy = _dwt(hip, y, dims, wavelet, levels, inverse=True)
    lhs, rhs = np.vdot(y.astype(np.complex128), fwd), np.vdot(wy.astype(np.complex128), x)
    assert abs(lhs - rhs) < 1e-6 * np.linalg.norm(x) * np.linalg.norm(y)


def test_dwt3_panels_with_leading_dimension_alpha_and_beta(hip):
    dims, wavelet, levels = (64, 48, 40), "db2", 3
    n = int(np.prod(dims))
    x = rand64c(n, 2, seed=3) - (0.5 + 0.5j)
    y0 = rand64c(n, 2, seed=4) - (0.5 + 0.5j)
    alpha, beta = 0.75 - 0.5j, -0.25 + 1.5j
    for inverse in (False, True):
        ref = alpha * dwt64.dwt(x, dims, wavelet, levels, inverse=inverse)
        out = _dwt(hip, x, dims, wavelet, levels, inverse=inverse, alpha=alpha, pad=37)
        assert _rel(out, ref) < 2e-6, (inverse, _rel(out, ref))
        ref = ref + beta * y0
        out = _dwt(hip, x, dims, wavelet, levels, inverse=inverse, alpha=alpha, beta=beta, y0=y0, pad=37)
        assert _rel(out, ref) < 2e-6, (inverse, _rel(out, ref))


@pytest.mark.parametrize("dims,wavelet", [((480, 208, 308), "db4"), ((256, 256, 256), "db4"),
                                          ((480, 208, 308), "haar"), ((480, 208, 308), "db2")])
def test_dwt3_on_large_volumes(hip, dims, wavelet):
    """the reference's scan size (axes of 208 and 308 = 4 x 77 split unevenly) and 256^3; the float64 transform only for db4,
    the other filters by their round trip"""
    n = int(np.prod(dims))
    x = rand64c(n, 1, seed=11) - (0.5 + 0.5j)
    x_d, y_d = hip.copy_array(x), hip.zero_array((n, 1), C64)
    hip.dwt3(y_d, x_d, dims, wavelet, 3)
    fwd = y_d.to_host()
    hip.dwt3(x_d, y_d, dims, wavelet, 3, inverse=True)
    assert _rel(x_d.to_host(), x) < 2e-6
    if wavelet == "db4":
        ref = dwt64.dwt(x, dims, wavelet, 3)
        assert _rel(fwd, ref) < 2e-6, _rel(fwd, ref)
        y_d.copy_from(np.asfortranarray(ref.astype(C64)))
        hip.dwt3(x_d, y_d, dims, wavelet, 3, inverse=True)
        assert _rel(x_d.to_host(), x) < 2e-6


def test_soft_threshold_zeros_and_the_coarse_box(hip):
    dims, tau = (64, 48, 40), 0.3
    keep = dwt64.coarse_box(dims, "db2", 3)
    n = int(np.prod(dims))
    u = (rand64c(n, 2, seed=5) - (0.5 + 0.5j)).astype(C64)
    r = np.abs(u.astype(np.complex128))
    near = np.abs(r / tau - 1) < 1e-4                                   # keep float32 rounding away from the edge ...
    u[near] *= np.float32(1.01)
    u[-120:-80, 0] = 0                                                  # ... but for the exact cases |u| = 0 and |u| = tau
    u[-80:-40, 0] = np.float32(tau)                                     # (the last rows lie outside the coarse box)
    u[-40:, 1] = np.complex64(1j * np.float32(tau))
    u_d = hip.copy_array(u)
    hip.soft_threshold(u_d, np.float32(tau), dims, keep)
    out = u_d.to_host()
    ref = dwt64.soft(u, np.float32(tau), dims, keep)
    vol_in, vol_out = (a.reshape(dims + (2,), order='F') for a in (u, out))
    box = tuple(slice(0, c) for c in keep)
    assert np.array_equal(vol_out[box].view(np.uint64), vol_in[box].view(np.uint64))       # untouched, bit for bit
    inside = np.zeros(dims + (2,), dtype=bool)
    inside[box] = True
    zero = (np.abs(u.astype(np.complex128)).reshape(dims + (2,), order='F') <= np.float32(tau)) & ~inside
    assert zero.sum() > 1000 and zero.reshape((n, 2), order='F')[-120:-40, 0].all() and zero.reshape((n, 2), order='F')[-40:, 1].all()
    assert np.array_equal(vol_out[zero].view(np.uint64), np.zeros(zero.sum(), np.uint64))   # exact (+0) zeros
    rest = ~zero & ~inside
    assert np.abs(vol_out[rest] - ref.reshape(dims + (2,), order='F')[rest]).max() < 1e-6


# ---- the case table (tests/dwt_cases.py) against the elementwise bound of dwt64.dwt_bound -----------------------------------------
PAD_X, PAD_Y = 37, 11                                                       # NaN rows under every column of x and of y: ldx != ldy
ALPHA, BETA = 0.75 - 0.5j, -0.25 + 1.5j


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _panel(hip, a, pad):
    """the panel a on the device with `pad` NaN rows under every column, and the host copy"""
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _run(hip, x, case, inverse=False, alpha=1, beta=0, y0=None):
    """dwt3 out of place between two padded panels; y starts as y0 or NaN; the pad rows of y and all of x come back bit-identical"""
    dims, wavelet, levels = case
    n = x.shape[0]
    x_d, xp = _panel(hip, x, PAD_X)
    y_d, yp = _panel(hip, np.full(x.shape, np.nan, dtype=C64) if y0 is None else y0, PAD_Y)
    hip.dwt3(y_d[:n], x_d[:n], dims, wavelet, levels, inverse=inverse, alpha=alpha, beta=beta)
    out = y_d.to_host()
    assert _same_bits(out[n:], yp[n:])
    assert _same_bits(x_d.to_host(), xp)
    return out[:n]


def _ratio(out, ref, bound):
    assert np.isfinite(out).all()
    return dwt64.worst_ratio(np.abs(out - ref), bound)


@pytest.fixture(scope="module", params=dwt_cases.CASES, ids=dwt_cases.case_id)
def table(request):
    """three-column inputs of one case and their float64 transforms, computed once"""
    dims, wavelet, levels = request.param
    x, y0 = dwt_cases.make_input(dims, dwt_cases.NCOLS, seed=1), dwt_cases.make_input(dims, dwt_cases.NCOLS, seed=2)
    ref = {inverse: dwt64.dwt(x, dims, wavelet, levels, inverse) for inverse in (False, True)}
    return dict(case=request.param, x=x, y0=y0, ref=ref, npasses=len(dwt64.passes(dims, wavelet, levels)[0]))


def test_dwt3_inside_the_elementwise_bound(hip, table):
    """plain, scaled and accumulated, both directions, out of place with ldx != ldy: every element within dwt64.dwt_bound of the
    float64 transform.  The bound is derived (dwt64.dwt_abs), not fitted: a float32 restatement of the arithmetic stays below 0.4 of
    it on the CPU (tests/test_wavelet_cpu.py), and the MI355X gave the same figures, 0.23 at worst on the cases with passes and
    0.40 on (16, 16, 16) db2 0, where alpha x + beta y is all there is to do"""
    case, x, y0 = table["case"], table["x"], table["y0"]
    worst = 0.0
    for inverse in (False, True):
        ref = table["ref"][inverse]
        for alpha in (1, ALPHA):                                        # y starts as NaN: beta == 0 does not read it
            out = _run(hip, x, case, inverse=inverse, alpha=alpha)
            worst = max(worst, _ratio(out, alpha * ref, dwt64.dwt_bound(x, *case, inverse, alpha=alpha)))
        out = _run(hip, x, case, inverse=inverse, alpha=ALPHA, beta=BETA, y0=y0)
        worst = max(worst, _ratio(out, ALPHA * ref + BETA * y0, dwt64.dwt_bound(x, *case, inverse, alpha=ALPHA, beta=BETA, y0=y0)))
    print("dwt3 %s: worst error / bound %.3f" % (dwt_cases.case_id(case), worst))
    assert worst <= 1, worst


def test_dwt3_in_place_and_layouts_give_the_same_bits(hip, table):
    case, x = table["case"], table["x"]
    dims, wavelet, levels = case
    n, ncols = x.shape
    for inverse in (False, True):
        for alpha in (1, ALPHA):
            out = _run(hip, x, case, inverse=inverse, alpha=alpha)
            assert _same_bits(_run(hip, x, case, inverse=inverse, alpha=alpha), out)           # a second call
            x_d, xp = _panel(hip, x, PAD_X)                                                    # in place
            hip.dwt3(x_d[:n], x_d[:n], dims, wavelet, levels, inverse=inverse, alpha=alpha)
            got = x_d.to_host()
            assert _same_bits(got[:n], out) and _same_bits(got[n:], xp[n:])
            x_d, y_d = hip.copy_array(x), hip.zero_array((n, ncols), C64)                      # no padding
            hip.dwt3(y_d, x_d, dims, wavelet, levels, inverse=inverse, alpha=alpha)
            assert _same_bits(y_d.to_host(), out)
            x_d = hip.copy_array(np.asfortranarray(x.reshape((n * ncols, 1), order='F')))      # the columns stacked in one vector
            y_d = hip.zero_array((n * ncols, 1), C64)
            hip.dwt3(y_d, x_d, dims, wavelet, levels, inverse=inverse, alpha=alpha)
            assert _same_bits(y_d.to_host().reshape((n, ncols), order='F'), out)
            hip.dwt3(x_d, x_d, dims, wavelet, levels, inverse=inverse, alpha=alpha)
            assert _same_bits(x_d.to_host().reshape((n, ncols), order='F'), out)
    if not table["npasses"]:                                            # nothing to do and nothing done
        x_d, xp = _panel(hip, x, PAD_X)
        for inverse in (False, True):
            hip.dwt3(x_d[:n], x_d[:n], dims, wavelet, levels, inverse=inverse)
            assert _same_bits(x_d.to_host(), xp)
            assert _same_bits(_run(hip, x, case, inverse=inverse), x)  # out of place: a copy


def test_dwt3_adjoint_identity_on_the_case_table(hip, table):
    """<W x, y> = <x, W^H y> on the device results"""
    case, x, y = table["case"], table["x"], table["y0"]
    fwd, wy = _run(hip, x, case), _run(hip, y, case, inverse=True)
    lhs, rhs = np.vdot(y.astype(np.complex128), fwd), np.vdot(wy.astype(np.complex128), x)
    assert abs(lhs - rhs) < 1e-6 * np.linalg.norm(x) * np.linalg.norm(y)


def test_dwt3_strides_over_more_columns_than_a_grid_holds(hip):
    dims, wavelet, levels, ncols = dwt_cases.MANY_COLUMNS
    case = (dims, wavelet, levels)
    x = dwt_cases.make_input(dims, ncols, seed=3)
    worst = 0.0
    for inverse in (False, True):
        out = _run(hip, x, case, inverse=inverse)
        worst = max(worst, _ratio(out, dwt64.dwt(x, *case, inverse), dwt64.dwt_bound(x, *case, inverse)))
    print("dwt3 %s, %d columns: worst error / bound %.3f" % (dwt_cases.case_id(case), ncols, worst))
    assert worst <= 1, worst


@pytest.mark.parametrize("case", [((12, 10, 3), "haar", 3), ((9, 16, 4), "db2", 3), ((1, 1, 64), "db4", 5)], ids=dwt_cases.case_id)
def test_dwt3_of_the_unit_vectors_is_the_dense_matrix(hip, case):
    """every coefficient's position and sign: a coefficient of a unit vector is a sum of products of single taps, the bound is
    relative to those, and where the matrix has a zero the result is a zero"""
    dims, wavelet, levels = case
    n = int(np.prod(dims))
    npasses = len(dwt64.passes(dims, wavelet, levels)[0])
    eye = np.asfortranarray(np.eye(n, dtype=C64))
    W = dwt64.dense(dims, wavelet, levels)
    worst = 0.0
    for inverse in (False, True):
        ref = W.T if inverse else W
        out = _run(hip, eye, case, inverse=inverse)
        assert np.abs(out - ref).max() <= npasses * (dwt64.TAPS[wavelet] + 2) * 2.0 ** -24
        worst = max(worst, _ratio(out, ref, dwt64.dwt_bound(eye, dims, wavelet, levels, inverse)))
    print("dwt3 %s, unit vectors: worst error / bound %.3f" % (dwt_cases.case_id(case), worst))
    assert worst <= 1, worst


def test_wavelet_in_an_operator_product(hip):
    case = dims, wavelet, levels = (9, 16, 4), "db2", 3
    W = hip.Wavelet(dims, wavelet=wavelet, levels=levels)
    x, k = dwt_cases.make_input(dims, 2, seed=5), dwt_cases.make_input(dims, 2, seed=6)
    wx = W * x
    worst = _ratio(wx, dwt64.dwt(x, *case), dwt64.dwt_bound(x, *case))
    # W^H of the float32 W x: its own bound (the error of W x is in its input, not in the comparison)
    worst = max(worst, _ratio(W.H * wx, dwt64.dwt(wx, *case, inverse=True), dwt64.dwt_bound(wx, *case, inverse=True)))
    assert _rel(W.H * wx, x) < 2e-6
    a = np.conj(0.5j)
    worst = max(worst, _ratio((0.5j * W).H * k, a * dwt64.dwt(k, *case, inverse=True), dwt64.dwt_bound(k, *case, inverse=True, alpha=a)))
    print("Wavelet operator %s: worst error / bound %.3f" % (dwt_cases.case_id(case), worst))
    assert worst <= 1, worst


def _raw_dwt3(hip, dims, wavelet_id, levels, ncols, x, ldx, y, ldy, inverse=0, alpha=1, beta=0):
    """ig_dwt3_c64 on raw device addresses -> status"""
    return hip._L.ig_dwt3_c64(hip._ctx, *dims, wavelet_id, levels, inverse, ncols, ctypes.c_void_p(x), ldx,
                              *(float(v) for c in (complex(alpha), complex(beta)) for v in (c.real, c.imag)), ctypes.c_void_p(y), ldy)


def test_dwt3_contract_errors_leave_both_arrays_alone(hip):
    hx, hy = dwt_cases.make_input((1025, 1, 2), 1, seed=1), dwt_cases.make_input((1025, 1, 2), 1, seed=2)
    x_d, y_d = hip.copy_array(hx), hip.copy_array(hy)
    for dims in ((1025, 1, 1), (1, 1025, 1), (1, 1, 1025)):            # 1024 is served: the case table has it on axes 0 and 2
        with pytest.raises(RuntimeError, match="longer than 1024"):
            hip.dwt3(y_d[:1025], x_d[:1025], dims, "haar", 1)
    dims, n = (8, 4, 2), 64
    with pytest.raises(RuntimeError, match="negative"):
        hip.dwt3(y_d[:n], x_d[:n], dims, "haar", -1)
    with pytest.raises(RuntimeError, match="beta != 0"):
        hip.dwt3(x_d[:n], x_d[:n], dims, "haar", 1, beta=1)
    for wavelet_id in (3, -1):
        with pytest.raises(RuntimeError, match="unknown wavelet"):
            hip._check(_raw_dwt3(hip, dims, wavelet_id, 1, 2, x_d._arr, n, y_d._arr, n), "ig_dwt3_c64")
    for ldx, ldy in ((n - 1, n), (n, n - 1)):
        with pytest.raises(RuntimeError, match="leading dimension"):
            hip._check(_raw_dwt3(hip, dims, 0, 1, 2, x_d._arr, ldx, y_d._arr, ldy), "ig_dwt3_c64")
    with pytest.raises(RuntimeError, match="different leading dimensions"):
        hip._check(_raw_dwt3(hip, dims, 0, 1, 2, x_d._arr, n, x_d._arr, n + 5), "ig_dwt3_c64")
    # empty input: nothing to do is no error
    for dims0, ncols in (((0, 4, 2), 2), ((8, 0, 2), 2), ((8, 4, 0), 2), (dims, 0)):
        for y in (y_d._arr, x_d._arr):
            hip._check(_raw_dwt3(hip, dims0, 0, 1, ncols, x_d._arr, n, y, n, alpha=ALPHA), "ig_dwt3_c64")
    assert _same_bits(x_d.to_host(), hx) and _same_bits(y_d.to_host(), hy)


def test_dwt3_rejects_panels_that_overlap_without_being_equal(hip):
    case = dims, wavelet, levels = (4, 4, 4), "haar", 3
    n, ncols = 64, 2
    host = dwt_cases.make_input((600, 1, 1), 1, seed=9)                 # elements: x = [192, 320); y may start anywhere
    buf = hip.copy_array(host)

    def at(y_off, alpha=1):
        return _raw_dwt3(hip, dims, 0, levels, ncols, buf._arr + 8 * 192, n, buf._arr + 8 * y_off, n, alpha=alpha)
    # shifted by one element either way; y's first column is x's last; x's last element; y's last element is x's first
    for off in (193, 191, 256, 319, 65):
        with pytest.raises(RuntimeError, match="y overlaps x"):
            hip._check(at(off), "ig_dwt3_c64")
    assert _same_bits(buf.to_host(), host)
    x = host[192:320, 0].reshape((n, ncols), order='F')
    ref, bound = dwt64.dwt(x, *case), dwt64.dwt_bound(x, *case)
    for off in (64, 320):                                               # adjacent on either side, not overlapping
        hip._check(at(off), "ig_dwt3_c64")
        after = buf.to_host()
        assert _ratio(after[off:off + 128, 0].reshape((n, ncols), order='F'), ref, bound) <= 1
        keep = np.ones(600, dtype=bool)
        keep[off:off + 128] = False
        assert _same_bits(after[keep], host[keep])
        host = after
    hip._check(at(192, alpha=ALPHA), "ig_dwt3_c64")                     # y == x is the in-place form
    assert _ratio(buf.to_host()[192:320, 0].reshape((n, ncols), order='F'), ALPHA * ref, dwt64.dwt_bound(x, *case, alpha=ALPHA)) <= 1


# ---- the soft threshold against dwt64.soft, elementwise -----------------------------------------------------------------------
# (dims, keep, columns)
SOFT_CASES = [
    ((17, 5, 3), (5, 5, 2), 3),            # the whole middle axis is inside: every axis's test decides somewhere on its own
    ((17, 5, 3), (17, 5, 0), 3),           # one empty side is an empty box: everything is thresholded
    ((17, 5, 3), (0, 5, 3), 3),
    ((17, 5, 3), (17, 0, 3), 3),
    ((17, 5, 3), (17, 5, 3), 3),           # the box is the volume: nothing changes
    ((17, 5, 3), (0, 0, 0), 3),
    ((8, 1, 6), (3, 1, 2), 3),             # unit axes, a partial box
    ((1, 1, 9), (1, 1, 4), 3),
    ((128, 96, 90), (16, 12, 45), 2),      # 1 105 920 elements a column: more than 4096 x 256, so the kernel strides
]


def _soft(hip, u, tau, dims, keep):
    """soft_threshold on a panel with PAD_X NaN rows under every column, which come back bit-identical"""
    n = u.shape[0]
    u_d, up = _panel(hip, u, PAD_X)
    hip.soft_threshold(u_d[:n], tau, dims, keep)
    out = u_d.to_host()
    assert _same_bits(out[n:], up[n:])
    return out[:n]


@pytest.mark.parametrize("dims,keep,ncols", SOFT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_soft_threshold_elementwise(hip, dims, keep, ncols):
    """|out - ref| <= 6 * 2^-24 |u|: r2, the square root, the division and the subtraction leave f = 1 - tau / |u| within 4 roundings
    absolute (f <= 1), the product adds one; an element that the float32 comparison puts on the other side of |u| = tau than float64
    does is within the same bound, its exact result being that close to 0 -- so nothing is moved away from the edge"""
    n = int(np.prod(dims))
    u = np.array(dwt_cases.make_input(dims, ncols, seed=5))
    tau = np.float32(np.median(np.abs(u)))
    u[-3, 0], u[-2, 0], u[-1, 0] = 0, tau, np.complex64(1j * tau)      # the exact cases: |u| = 0, u = tau, u = i tau
    mag = np.abs(u.astype(np.complex128))
    assert 0.2 <= (mag > tau).mean() <= 0.8
    out = _soft(hip, u, tau, dims, keep)
    ref = dwt64.soft(u, tau, dims, keep)
    assert np.isfinite(out).all()
    assert (np.abs(out - ref) <= 6 * 2.0 ** -24 * mag).all(), dwt64.worst_ratio(np.abs(out - ref), 6 * 2.0 ** -24 * mag)
    inside = np.zeros(tuple(dims) + (ncols,), dtype=bool)
    inside[tuple(slice(0, c) for c in keep)] = True
    inside = inside.reshape((n, ncols), order='F')
    assert inside.sum() == int(np.prod(keep)) * ncols
    assert _same_bits(out[inside], u[inside])                           # the box: untouched, bit for bit
    if keep == dims:
        assert _same_bits(out, u)
    else:
        assert not inside[-3:, 0].any() and _same_bits(out[-3:, 0], np.zeros(3, C64))          # exact (+0) zeros
        assert (inside | (u == 0) | (_bits(out) != _bits(u))).all()     # tau > 0 moves every element outside that is not 0


def test_soft_threshold_exact_properties(hip):
    dims, keep = (17, 5, 3), (5, 5, 2)
    u = np.array(dwt_cases.make_input(dims, 3, seed=6))
    for part in (u.real, u.imag):                                       # components of at least 1e-3 ...
        part[np.abs(part) < 1e-3] = 1e-3
    u[-2:, 1] = [0, np.complex64(complex(-0.0, 0.0))]                   # ... and zeros of both signs
    # tau = 0 returns the input bit for bit; zeros stay (or become) +0
    want = u.copy()
    want[-2:, 1] = 0
    assert _same_bits(_soft(hip, u, 0.0, dims, keep), want)
    # power-of-two scaling commutes with every float32 operation of the kernel while nothing leaves the normal range
    tau = np.float32(np.median(np.abs(u)))
    out = _soft(hip, u, tau, dims, keep)
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    for s in (2.0 ** 40, 2.0 ** -40):
        for a in (u, out):
            comp = np.abs(np.concatenate([a.real.ravel(), a.imag.ravel()]).astype(np.float64))
            comp = comp[comp > 0]
            assert ((comp * s) ** 2 >= tiny).all() and 2 * (comp.max() * s) ** 2 <= huge
        assert (float(tau) * s) ** 2 >= tiny
        scaled = _soft(hip, u * np.float32(s), np.float32(tau * np.float32(s)), dims, keep)
        assert _same_bits(scaled, out * np.float32(s)), s


def test_soft_threshold_limits(hip):
    dims, keep, n = (17, 5, 3), (5, 5, 2), 255
    u = dwt_cases.make_input(dims, 2, seed=7)
    u_d = hip.copy_array(u)
    with pytest.raises(RuntimeError, match="negative threshold"):
        hip.soft_threshold(u_d, -0.5, dims, keep)
    with pytest.raises(RuntimeError, match="leading dimension"):
        hip._check(hip._L.ig_csoft_c64(hip._ctx, *dims, *keep, 2, ctypes.c_float(0.5), ctypes.c_void_p(u_d._arr), n - 1), "ig_csoft_c64")
    assert _same_bits(u_d.to_host(), u)


def _scan(tmpdir, B, N, C, nro, nsp, osf, width=2):
    """a synthetic radial scan built the way test_hip_pics builds its scans"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j)).astype(np.complex64)
    img[(np.abs(g[0]) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5                 # an edge for the wavelets to see
    centres = [(-1, 0, 0.3), (1, 0.5, -0.4)][:C]
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph) for cx, cy, ph in centres],
                   axis=3).astype(np.complex64)
    coord = radial_trajectory(nsp, nro, seed=2)
    traj = coord * np.array(N, dtype=np.float64)[:, None, None]
    F1 = B.NUFFT((1, nro, nsp), N, coord, width=width, oversamp=(osf, osf, osf), dtype=C64)
    A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
    ksp = (A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F')
    path = os.path.join(str(tmpdir), "scan.npz")
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path


def _logged(caplog, pattern):
    return [float(m.group(1)) for r in caplog.records for m in [re.search(pattern, r.getMessage())] if m]


def test_pics_l1_on_the_gpu_matches_the_oracle_backend(tmp_path, hip, oracle_backend, caplog):
    N = (64, 64, 64)
    path = _scan(tmp_path, hip, N, 2, nro=128, nsp=200, osf=2.0)
    args = ["--osf", "2.0", "--width", "2", "--lamda", "1e-3", "--l1", "0.02", "--debug", "40", path]
    # the two power iterations' estimates of the largest eigenvalue of A^H A + lamda I
    est = {}
    for name, B in (("hip", hip), ("oracle", oracle_backend)):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="pics"):
            pics.main(["-i", "0", "--power-iters", "6"] + args, backend=B)
        oracle_backend._scratch = None
        est[name] = _logged(caplog, r"largest eigenvalue of A\^H A \+ lamda I (\S+)")[0]
    assert abs(est["hip"] - est["oracle"]) < 1e-4 * est["oracle"], est
    step = ["--step", "%.8e" % (0.9 / est["oracle"])]
    for iters, tol in (("1", 1e-5), ("10", 1e-4)):
        out = pics.main(["-i", iters] + step + args, backend=hip)
        ref = pics.main(["-i", iters, "--no-fuse"] + step + args, backend=oracle_backend)
        oracle_backend._scratch = None
        assert _rel(out, ref) < tol, (iters, _rel(out, ref))
    # the objective falls (fixed-step FISTA is not monotone step by step, but 5 -> 30 iterations must gain)
    obj = {}
    for iters in ("5", "30"):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="pics"):
            pics.main(["-i", iters] + args, backend=hip)
        obj[iters] = _logged(caplog, r"fista iter \d+, objective (\S+)")[-1]
    assert obj["30"] < obj["5"], obj
