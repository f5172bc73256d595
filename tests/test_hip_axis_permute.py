"""The image-axis permutation on the MI355X: the ig_permute3_c64 kernel against numpy, the fused SENSE leaf on grids whose x axis
is chirp-z (image 52 x 120 x 77 at the reference driver's oversampling 640/480: grid 69 x 160 x 102, run as 160 x 69 x 102 after
a permutation of the image) against the oracle on the unpermuted problem, and pics.py -O3 on such a scan."""
import ctypes
import itertools

import numpy as np
import pytest

from conftest import rel_err
from indigo_amd import fused
from indigo_amd import operators as op
from indigo_amd.sense import SenseProblem, normal_operator
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu

C64 = np.dtype('complex64')
RTOL = 1e-5
PERMS = list(itertools.permutations(range(3)))


def _host_permute(x, dims, perm):
    n = int(np.prod(dims))
    return x.reshape(tuple(dims) + (-1,), order='F').transpose(tuple(perm) + (3,)).reshape((n, -1), order='F')


def _run(hip, x, dims, perm, alpha=1, beta=0, y0=None, pad=0):
    """permute3 of the panel x (n x ncols) into a panel with `pad` extra rows (leading dimension n + pad); returns the n rows"""
    n, ncols = x.shape
    xp = np.zeros((n + pad, ncols), dtype=C64, order='F')
    xp[:n] = x
    yp = np.full((n + pad, ncols), np.nan, dtype=C64, order='F') if y0 is None else np.zeros((n + pad, ncols), dtype=C64, order='F')
    if y0 is not None:
        yp[:n] = y0
    x_d, y_d = hip.copy_array(xp), hip.copy_array(yp)
    hip.permute3(y_d[:n], x_d[:n], dims, perm, alpha=alpha, beta=beta)
    out = y_d.to_host()
    if pad:
        assert np.array_equal(out[n:], yp[n:], equal_nan=True)          # the rows between columns are left alone
    return out[:n]


@pytest.mark.parametrize("dims", [(69, 160, 102), (7, 5, 3), (277, 3, 5)])
def test_permute3_all_perms_bit_identical(hip, dims):
    x = rand64c(int(np.prod(dims)), 1, seed=11)
    for perm in PERMS:
        assert np.array_equal(_run(hip, x, dims, perm), _host_permute(x, dims, perm)), perm


def test_permute3_256_cubed(hip):
    dims = (256, 256, 256)
    x = rand64c(int(np.prod(dims)), 1, seed=12)
    assert np.array_equal(_run(hip, x, dims, (2, 0, 1)), _host_permute(x, dims, (2, 0, 1)))


@pytest.mark.parametrize("perm", PERMS)
def test_permute3_panels_with_leading_dimension_and_complex_scalars(hip, perm):
    dims = (69, 16, 11)
    n = int(np.prod(dims))
    x = rand64c(n, 3, seed=13)
    ref = _host_permute(x, dims, perm)
    assert np.array_equal(_run(hip, x, dims, perm, pad=5), ref)
    a, b = 0.5 - 1.25j, -0.75 + 0.5j
    y0 = rand64c(n, 3, seed=14)
    got = _run(hip, x, dims, perm, alpha=a, beta=b, y0=y0, pad=5)
    assert rel_err(got, np.complex64(b) * y0 + np.complex64(a) * ref) < 1e-6
    got = _run(hip, x, dims, perm, alpha=a, beta=0, pad=1)            # beta = 0: the NaN in y is not read
    assert rel_err(got, np.complex64(a) * ref) < 1e-6


def test_permute3_rejects_bad_arguments(hip):
    dims = (7, 5, 3)
    x_d = hip.copy_array(rand64c(105, 1, seed=1))
    y_d = hip.zero_array((105, 1), C64)
    with pytest.raises(RuntimeError, match="ig_permute3_c64"):
        hip.permute3(x_d, x_d, dims, (1, 0, 2))
    with pytest.raises(RuntimeError, match="ig_permute3_c64"):
        hip.permute3(y_d, x_d, dims, (1, 1, 2))
    L = hip._L
    perm = (ctypes.c_int * 3)(1, 0, 2)
    rc = L.ig_permute3_c64(hip._ctx, 7, 5, 3, perm, 1, ctypes.c_void_p(x_d._arr), 104, 1.0, 0.0, 0.0, 0.0, ctypes.c_void_p(y_d._arr), 105)
    assert rc == 2
    rc = L.ig_permute3_c64(hip._ctx, 7, 5, 3, (ctypes.c_int * 3)(0, 1, 3), 1, ctypes.c_void_p(x_d._arr), 105, 1.0, 0.0, 0.0, 0.0,
                           ctypes.c_void_p(y_d._arr), 105)
    assert rc == 2
    assert np.array_equal(y_d.to_host(), np.zeros((105, 1), dtype=C64))


def _zpad_leaves(A):
    out, stack = [], [A]
    while stack:
        n = stack.pop()
        if isinstance(n, op.ZpadFFT):
            out.append(n)
        stack.extend(getattr(n, '_children', []))
    return out


def _sense_case(hip, oracle_backend, N, C, width, grid, pgrid, perm):
    p = SenseProblem.synthetic(N, C, nspokes=300, nreadout=160, width=width, ntable=128, oversamp=640 / 480, seed=6)
    assert p.oN == grid and not hip.supports_padded_fft(grid, C)
    assert fused.image_permutation(hip, grid, C) == perm
    hip._scratch = None
    oracle_backend._scratch = None
    A = p.build_zpadfft(hip)
    assert isinstance(A.right, op.AxisPermute) and A.right._perm == perm
    zs = _zpad_leaves(A)
    assert zs and all(z._grid == pgrid for z in zs), [z._grid for z in zs]
    x = rand64c(A.shape[1], 1, seed=1)
    k = rand64c(A.shape[0], 1, seed=2)
    A_o = p.build_zpadfft(oracle_backend, layout=0, support=False)
    assert not A_o.has(op.AxisPermute)
    assert rel_err(A * x, A_o * x) < RTOL
    assert rel_err(A.H * k, A_o.H * k) < RTOL
    y_d = hip.zero_array((A.shape[1], 1), C64)
    normal_operator(A, lamda=0.2).eval(y_d, hip.copy_array(x))
    exp = A_o.H * (A_o * x) + np.float32(0.2) * x
    assert rel_err(y_d.to_host(), exp) < RTOL
    hip._scratch = None
    oracle_backend._scratch = None
    return A


@pytest.mark.parametrize("width", [2, 3])
def test_sense_on_a_chirp_z_x_axis_through_a_permutation(hip, oracle_backend, width):
    _sense_case(hip, oracle_backend, (52, 120, 77), 8, width, (69, 160, 102), (160, 69, 102), (1, 0, 2))


def test_sense_through_a_swap_with_z(hip, oracle_backend):
    _sense_case(hip, oracle_backend, (52, 77, 120), 8, 2, (69, 102, 160), (160, 102, 69), (2, 1, 0))


def test_sense_through_a_permutation_with_12_coils(hip, oracle_backend):
    A = _sense_case(hip, oracle_backend, (52, 120, 77), 12, 2, (69, 160, 102), (160, 69, 102), (1, 0, 2))
    assert isinstance(A.left, op.VStack) and [c[2] for c in A.left._coil_chunks] == [8, 4]


def test_pics_on_a_chirp_z_x_axis_takes_the_fused_leaf(tmp_path, hip, oracle_backend, caplog):
    """image 52 x 120 x 77 at the reference driver's default oversampling: grid 69 x 160 x 102, x = 69 = 3 * 23 is chirp-z.
    FuseZpadFFT runs the fused leaf on 160 x 69 x 102 after a permutation of the image; the image equals the unfused -O3 leaves'
    and the oracle backend's"""
    import logging
    from indigo_amd import pics
    from test_hip_pics import _rel, _scan
    N, C = (52, 120, 77), 4
    path, img = _scan(tmp_path, hip, N, C, nro=160, nsp=300, osf=640 / 480, width=3)
    args = ["-i", "4", "--width", "3", "--lamda", "1e-3", "--debug", "40", path]
    assert not hip.supports_padded_fft((69, 160, 102), C)
    with caplog.at_level(logging.INFO, logger="pics"):
        out = pics.main(["-O", "3"] + args, backend=hip)
    tree = [r.getMessage() for r in caplog.records if r.getMessage().startswith("tree:")][-1]
    assert "ZpadFFT" in tree and "AxisPermute" in tree and "UnscaledFFT" not in tree, tree
    plain = pics.main(["-O", "3", "--no-fuse"] + args, backend=hip)
    assert _rel(out, plain) < 2e-4
    oracle_backend._scratch = None
    ref = pics.main(["-O", "3", "--no-fuse"] + args, backend=oracle_backend)
    oracle_backend._scratch = None
    assert _rel(out, ref) < 1e-3
