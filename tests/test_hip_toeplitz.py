"""The Toeplitz normal operator on the MI355X: ig_psf_mix_c64 against the float64 restatement in tests/toep64.py,
operators.ToeplitzNormal against the numpy oracle backend with the same kernel, and pics --basis --toeplitz against the same
driver on the oracle backend."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

import basis64
import toep64
from indigo_amd import pics
from indigo_amd.toeplitz import pack_planes
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
TOL = 1e-5          # the project's bar on the relative 2-norm; sums of at most 8 float32 products land near 5e-7
PAD = 37

NS = (1, 105, 2048, 5049)                       # one point; 7 * 5 * 3; whole workgroups; 33 * 17 * 9: several workgroups and a tail
KS = (1, 2, 3, 4, 5, 8)                         # both sides of every register image: 1 | 2, 2 | 3, 4 | 5, and the limit
NCS = (1, 3, 8)


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _bits(a):
    """the bit patterns of a complex64 array (NaN payloads included), whatever its memory order"""
    return np.ascontiguousarray(a).view(np.uint32)


def _kernel(K, n, seed):
    """K^2 planes of n floats: a random Hermitian matrix per grid point"""
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((K, K, n, 1, 1)) + 1j * rng.standard_normal((K, K, n, 1, 1))
    return pack_planes(H + np.conj(H.transpose(1, 0, 2, 3, 4)))


def _panel(x, interleaved, width, pad):
    """x (n, C, K) as the host panel of K columns in the layout's memory order: `width` coil slots per grid point when interleaved,
    `pad` rows under every column; whatever is not an element of x is NaN"""
    n, C, K = x.shape
    if interleaved:
        mem = np.full((width, n, K), np.nan, dtype=C64)
        mem[:C] = x.transpose(1, 0, 2)
    else:
        mem = x
    rows = mem.shape[0] * mem.shape[1]
    p = np.full((rows + pad, K), np.nan, dtype=C64, order='F')
    p[:rows] = mem.reshape((rows, K), order='F')
    return p, rows


def _unpanel(p, rows, n, C, K, interleaved, width):
    mem = p[:rows].reshape(((width, n, K) if interleaved else (n, C, K)), order='F')
    return mem[:C].transpose(1, 0, 2) if interleaved else mem


WORST = {"err": 0.0}


@pytest.mark.parametrize("n,K", [(n, K) for n in NS for K in KS], ids=lambda v: str(v))
def test_kernel_matches_the_float64_restatement(hip, n, K):
    kern = _kernel(K, n, seed=K * 10 + 1)
    kern_d = hip.copy_array(np.ascontiguousarray(kern).reshape(-1))
    for C in NCS:
        x = rand64c(n * C * K, 1, seed=n + C).reshape((n, C, K), order='F')
        want = toep64.mix(kern, x)
        for interleaved, width, pad in ((False, C, PAD), (False, C, 0), (True, C, PAD), (True, C + 1, 2), (True, C, 0)):
            xp, rows = _panel(x, interleaved, width, pad)
            mask = np.isnan(xp)                                           # padding rows and padding coil slots
            for in_place in (False, True):
                x_d = hip.copy_array(xp)
                y_d = x_d if in_place else hip.copy_array(np.full_like(xp, np.nan))
                hip.psf_mix(y_d[:rows], x_d[:rows], kern_d, n, C, interleaved=interleaved, width=width)
                out = y_d.to_host()
                if not in_place:
                    assert np.array_equal(_bits(x_d.to_host()), _bits(xp))
                assert np.array_equal(_bits(out[mask]), _bits(xp[mask])), "padding was touched"
                got = _unpanel(out, rows, n, C, K, interleaved, width)
                err = _rel(got, want)
                WORST["err"] = max(WORST["err"], err)
                assert np.isfinite(got).all() and err < TOL, (C, interleaved, width, pad, in_place, err)
    print("psf_mix n %d K %d: worst relative error so far %.3e" % (n, K, WORST["err"]))


def test_stacked_vectors_and_panels_give_the_same_bits(hip):
    n, C, K = 2048, 8, 4
    kern_d = hip.copy_array(np.ascontiguousarray(_kernel(K, n, 3)).reshape(-1))
    x = rand64c(n * C * K, 1, seed=4).reshape((n, C, K), order='F')
    for interleaved in (False, True):
        outs = []
        for pad in (PAD, 0, 2):
            xp, rows = _panel(x, interleaved, C, pad)
            x_d = hip.copy_array(xp)
            hip.psf_mix(x_d[:rows], x_d[:rows], kern_d, n, C, interleaved=interleaved)
            outs.append(x_d.to_host()[:rows])
        xs = hip.copy_array(np.asfortranarray(_panel(x, interleaved, C, 0)[0].reshape((-1, 1), order='F')))
        hip.psf_mix(xs, xs, kern_d, n, C, interleaved=interleaved)
        outs.append(xs.to_host().reshape((n * C, K), order='F'))
        for o in outs[1:]:
            assert np.array_equal(_bits(o), _bits(outs[0]))


def test_contract_errors(hip):
    n, C, K = 64, 2, 2
    host = rand64c(1200, 1, seed=9)
    buf = hip.copy_array(host)
    kern_d = hip.copy_array(np.ascontiguousarray(_kernel(9, n, 5)).reshape(-1))
    rows = n * C

    def call(nn, kk, x_off, y_off):
        return hip._L.ig_psf_mix_c64(hip._ctx, nn, C, kk, ctypes.c_void_p(kern_d._arr), ctypes.c_void_p(buf._arr + 8 * x_off), rows,
                                     ctypes.c_void_p(buf._arr + 8 * y_off), rows, 1, nn)
    with pytest.raises(RuntimeError, match="9 coefficients"):
        hip._check(call(n, 9, 0, 0), "ig_psf_mix_c64")
    with pytest.raises(RuntimeError, match="0 grid points"):
        hip._check(call(0, K, 0, 600), "ig_psf_mix_c64")
    for off in (1, rows, K * rows - 1):                                   # x = [0, 256): shifted by one, by a column, its last element
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(call(n, K, 0, off), "ig_psf_mix_c64")
    assert np.array_equal(buf.to_host(), host)
    hip._check(call(n, K, 0, K * rows), "ig_psf_mix_c64")                 # adjacent, not overlapping
    after = buf.to_host()
    assert np.array_equal(after[:K * rows], host[:K * rows]) and np.array_equal(after[2 * K * rows:], host[2 * K * rows:])
    want = toep64.mix(kern_d.to_host().reshape(-1)[:K * K * n].reshape((K * K, n)), host[:K * rows, 0].reshape((n, C, K), order='F'))
    assert _rel(after[K * rows:2 * K * rows, 0].reshape((n, C, K), order='F'), want) < TOL


def _hermitian(K, grid, seed):
    rng = np.random.default_rng(seed)
    H = (rng.standard_normal((K, K) + tuple(grid), dtype=np.float32) + 1j * rng.standard_normal((K, K) + tuple(grid), dtype=np.float32))
    return H + np.conj(H.transpose(1, 0, 2, 3, 4))


@pytest.mark.parametrize("dims,C,K,path", [((64, 64, 64), 3, 2, 'xzy'), ((64, 64, 64), 8, 2, 'xzy'), ((12, 10, 8), 2, 3, 'xyz')],
                         ids=["128^3-3coils", "128^3-8coils", "unfused"])
def test_toeplitz_normal_matches_the_oracle_backend(hip, oracle_backend, dims, C, K, path):
    """the SAME kernel on both backends: the fused ZpadFFT path in coil chunks of 4 (one zero-weight coil) and 8, and the unfused
    composition on a grid the leaf does not take"""
    N = int(np.prod(dims))
    grid = tuple(2 * n for n in dims)
    maps = rand64c(N, C, seed=4).reshape(dims + (C,), order='F')
    kern = pack_planes(_hermitian(K, grid, 1))
    x, y = rand64c(N * K, 1, seed=5), rand64c(N * K, 1, seed=6)
    hip._scratch = oracle_backend._scratch = None
    T = hip.ToeplitzNormal(dims, maps, kern, K)
    assert T._order == path and T.H is T
    Tx = T * x
    want = oracle_backend.ToeplitzNormal(dims, maps, kern, K) * x
    err = _rel(Tx, want)
    print("ToeplitzNormal %s x %d coils, K %d: relative difference to the oracle backend %.3e" % (dims, C, K, err))
    assert err < TOL, err
    # Hermitian on the device, and alpha / beta
    Ty = T * y
    lhs, rhs = np.vdot(y.astype(np.complex128), Tx.astype(np.complex128)), np.vdot(Ty.astype(np.complex128), x.astype(np.complex128))
    assert abs(lhs - rhs) < 1e-5 * abs(lhs), (lhs, rhs)
    alpha, beta = 0.7 - 0.3j, 0.5 + 0.25j
    y_d = hip.copy_array(y)
    T.eval(y_d, hip.copy_array(x), alpha=alpha, beta=beta)
    assert _rel(y_d.to_host(), alpha * Tx + beta * y) < TOL


@pytest.fixture(scope="module")
def scan(tmp_path_factory, hip, oracle_backend):
    """32^3, 2 coils, 5 frames in the span of 2 decaying exponentials; the step of the proximal solver from the oracle's power
    iteration"""
    tmp = tmp_path_factory.mktemp("toeplitz_scan")
    phi = basis64.exponential_basis(5)
    np.save(os.path.join(str(tmp), "phi.npy"), phi)
    hip._scratch = None
    path = basis64.subspace_scan(tmp, hip, (32, 32, 32), 2, phi, nro=64, nsp=100, osf=2.0, width=2)
    args = ["--toeplitz", "--basis", os.path.join(str(tmp), "phi.npy"), "--osf", "2.0", "--width", "2", "--lamda", "1e-3", path]
    records = []

    class Keep(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())
    keep = Keep(level=logging.INFO)
    plog = logging.getLogger("pics")
    old = plog.level
    plog.addHandler(keep)
    plog.setLevel(logging.INFO)
    try:
        oracle_backend._scratch = None
        pics.main(["-i", "0", "--power-iters", "6", "--no-fuse", "--l1", "0.01", "--debug", "40"] + args, backend=oracle_backend)
    finally:
        plog.removeHandler(keep)
        plog.setLevel(old)
    oracle_backend._scratch = None
    est = [float(m.group(1)) for s in records for m in [re.search(r"largest eigenvalue of A\^H A \+ lamda I (\S+)", s)] if m][0]
    return args, ["--step", "%.8e" % (0.9 / est)]


@pytest.mark.parametrize("extra", [[], ["--llr", "0.02", "--llr-block", "8"]], ids=["cg", "llr"])
def test_pics_basis_toeplitz_on_the_gpu_matches_the_oracle_backend(scan, hip, oracle_backend, caplog, extra):
    """the bar of test_hip_basis.py's driver cases: 1e-5 after one iteration, 1e-4 after ten"""
    args, step = scan
    with caplog.at_level(logging.WARNING):
        for iters, tol in (("1", 1e-5), ("10", 1e-4)):
            argv = extra + ["-i", iters, "--debug", "40"] + (step if extra else []) + args
            hip._scratch = None
            out = pics.main(argv, backend=hip)
            oracle_backend._scratch = None
            ref = pics.main(["--no-fuse"] + argv, backend=oracle_backend)
            oracle_backend._scratch = None
            assert out.shape == (32, 32, 32, 1, 1, 1, 2)
            print("pics --basis --toeplitz %s, %s iterations: relative difference %.3e" % (extra, iters, _rel(out, ref)))
            assert _rel(out, ref) < tol, (extra, iters, _rel(out, ref))
    assert not any("scratch arena too small" in r.getMessage() for r in caplog.records)
