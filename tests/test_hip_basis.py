"""The temporal-subspace kernels and pics --basis on the MI355X: ig_basis_c64 against the float64 restatement in tests/basis64.py,
operators.FrameBasis inside a product, and the driver against the same driver on the numpy oracle backend."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

import basis64
from indigo_amd import pics
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
TOL = 1e-5          # the project's bar on the relative 2-norm; sums of at most 40 float32 products land near 1e-6
ALPHA, BETA = 0.7 - 0.3j, 0.5 + 0.25j
PAD = 37

NS = (1, 105, 2048, 5049)                       # one voxel; 5 * 7 * 3; whole workgroups; 33 * 17 * 9: several workgroups and a tail
KS = (1, 3, 4, 5, 8, 9, 16, 17, 32)             # both sides of every register image: 4 | 5, 8 | 9, 16 | 17, and the limit


def _frames(K):
    return (1, K, 7, 40)                        # 40 rows of a 32-column basis need two fillings of the LDS copy


# every (n, K) once, with T rotating through its four values, and the corners that the rotation misses
CASES = [(n, K, _frames(K)[(i + j) % 4]) for i, K in enumerate(KS) for j, n in enumerate(NS)]
CASES += [c for c in [(2048, 4, 40), (2048, 32, 40), (5049, 17, 7), (5049, 32, 32), (1, 32, 40)] if c not in CASES]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _bits(a):
    """the bit patterns of a complex64 array (NaN payloads included), whatever its memory order"""
    return np.ascontiguousarray(a).view(np.uint32)


def _padded(hip, a, pad):
    """the panel a on the device with `pad` extra rows of NaN under every column, and the host copy"""
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _run(hip, phi_d, n, x, y, adjoint, alpha, beta, pad):
    """frame_basis on panels with `pad` NaN rows under every column of x and y, which must come back bit-identical"""
    x_d, xp = _padded(hip, x, pad)
    y_d, yp = _padded(hip, y, pad)
    hip.frame_basis(y_d[:n], x_d[:n], phi_d, n, adjoint=adjoint, alpha=alpha, beta=beta)
    out = y_d.to_host()
    assert np.array_equal(_bits(x_d.to_host()), _bits(xp))
    assert np.array_equal(_bits(out[n:]), _bits(yp[n:]))
    return out[:n]


WORST = {"err": 0.0}


@pytest.mark.parametrize("n,K,T", CASES, ids=lambda v: str(v))
def test_kernel_matches_the_float64_restatement(hip, n, K, T):
    phi = rand64c(T, K, seed=K * 100 + T)
    phi_d, _ = _padded(hip, phi, 3)                                       # ldphi = T + 3, the padding NaN
    for adjoint in (False, True):
        cols_x, cols_y = (T, K) if adjoint else (K, T)
        x, y = rand64c(n, cols_x, seed=n + 1), rand64c(n, cols_y, seed=n + 2)
        for beta, y0 in ((0, np.full_like(y, np.nan)), (BETA, y)):
            got = _run(hip, phi_d[:T], n, x, y0, adjoint, ALPHA, beta, PAD)
            err = _rel(got, basis64.apply(phi, x, y, adjoint, ALPHA, beta))
            WORST["err"] = max(WORST["err"], err)
            assert np.isfinite(got).all() and err < TOL, (adjoint, beta, err)
    print("frame_basis n %d K %d T %d: worst relative error so far %.3e" % (n, K, T, WORST["err"]))


@pytest.mark.parametrize("n,K,T", [(2048, 4, 7), (2048, 9, 40), (5049, 5, 7), (2048, 32, 40)], ids=lambda v: str(v))
def test_layout_forms_give_the_same_bits(hip, n, K, T):
    """the stacked vectors, the plain panels (both with 16-byte accesses when n is even) and panels with an odd leading
    dimension (8-byte accesses) hold the same bits"""
    phi = rand64c(T, K, seed=3)
    phi_d = hip.copy_array(phi)
    for adjoint in (False, True):
        cols_x, cols_y = (T, K) if adjoint else (K, T)
        x, y = rand64c(n, cols_x, seed=4), rand64c(n, cols_y, seed=5)
        outs = []
        for pad in (PAD, 0, 2):
            outs.append(_run(hip, phi_d, n, x, y, adjoint, ALPHA, BETA, pad))
        xs, ys = (hip.copy_array(np.asfortranarray(a.reshape((-1, 1), order='F'))) for a in (x, y))
        hip.frame_basis(ys, xs, phi_d, n, adjoint=adjoint, alpha=ALPHA, beta=BETA)
        outs.append(ys.to_host().reshape((n, cols_y), order='F'))
        for o in outs[1:]:
            assert np.array_equal(_bits(o), _bits(outs[0]))


def test_adjointness_on_the_device(hip):
    n, K, T = 5049, 5, 7
    phi_d = hip.copy_array(rand64c(T, K, seed=6))
    x, y = rand64c(n, K, seed=7), rand64c(n, T, seed=8)
    px, phy = hip.zero_array((n, T), C64), hip.zero_array((n, K), C64)
    hip.frame_basis(px, hip.copy_array(x), phi_d, n)
    hip.frame_basis(phy, hip.copy_array(y), phi_d, n, adjoint=True)
    lhs = np.vdot(y.astype(np.complex128), px.to_host().astype(np.complex128))
    rhs = np.vdot(phy.to_host().astype(np.complex128), x.astype(np.complex128))
    assert abs(lhs - rhs) < 1e-5 * abs(lhs), (lhs, rhs)


def test_limits(hip):
    n = 64
    x33, y = hip.copy_array(rand64c(n, 33, seed=1)), hip.copy_array(rand64c(n, 3, seed=2))
    before = y.to_host()
    with pytest.raises(RuntimeError, match="33 coefficients"):
        hip.frame_basis(y, x33, hip.copy_array(rand64c(3, 33, seed=3)), n)
    with pytest.raises(RuntimeError, match="33 coefficients"):
        hip.frame_basis(x33, y, hip.copy_array(rand64c(3, 33, seed=3)), n, adjoint=True)
    assert np.array_equal(y.to_host(), before)
    phi = rand64c(3, 32, seed=4)                                          # the limit itself is served
    x32 = rand64c(n, 32, seed=5)
    hip.frame_basis(y, hip.copy_array(x32), hip.copy_array(phi), n)
    assert _rel(y.to_host(), basis64.forward(phi, x32)) < TOL


def test_overlapping_panels_raise(hip):
    n, K, T = 64, 2, 3
    # elements: y may start anywhere; x = [192, 320); phi = [520, 526)
    host = rand64c(600, 1, seed=9)
    buf = hip.copy_array(host)

    def at(y_off):
        return hip._L.ig_basis_c64(hip._ctx, n, K, T, ctypes.c_void_p(buf._arr + 8 * 520), T, 0, ctypes.c_void_p(buf._arr + 8 * 192), n,
                                   1.0, 0.0, 0.0, 0.0, ctypes.c_void_p(buf._arr + 8 * y_off), n)
    for off in (1, 319, 200, 329, 525):          # x's first element, its last, inside it; phi's first element, its last
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(at(off), "ig_basis_c64")
    assert np.array_equal(buf.to_host(), host)
    hip._check(at(0), "ig_basis_c64")                                     # adjacent to x, not overlapping
    after = buf.to_host()
    assert np.array_equal(after[192:], host[192:])
    want = basis64.forward(host[520:526, 0].reshape((T, K), order='F'), host[192:320, 0].reshape((n, K), order='F'))
    assert _rel(after[:192, 0].reshape((n, T), order='F'), want) < TOL


def test_frame_basis_inside_a_product(hip):
    n, K, T = 105, 3, 2
    phi = rand64c(T, K, seed=10)
    d = [rand64c(n, 1, seed=11 + t) for t in range(T)]
    P = hip.BlockDiag([hip.Diag(v) for v in d]) * hip.FrameBasis(phi, n)
    assert P.shape == (n * T, n * K)
    x = rand64c(n * K, 1, seed=20)
    want = basis64.forward(phi, x.reshape((n, K), order='F')) * np.concatenate(d, axis=1)
    assert _rel(P * x, want.reshape((-1, 1), order='F')) < TOL
    z = rand64c(n * T, 1, seed=21)
    want = basis64.adjoint(phi, z.reshape((n, T), order='F') * np.conj(np.concatenate(d, axis=1)))
    assert _rel(P.H * z, want.reshape((-1, 1), order='F')) < TOL


@pytest.fixture(scope="module")
def scan(tmp_path_factory, hip, oracle_backend):
    """32^3, 2 coils, 5 frames in the span of 2 decaying exponentials; the step of the proximal solvers from the oracle's power
    iteration"""
    tmp = tmp_path_factory.mktemp("basis_scan")
    phi = basis64.exponential_basis(5)
    np.save(os.path.join(str(tmp), "phi.npy"), phi)
    path = basis64.subspace_scan(tmp, hip, (32, 32, 32), 2, phi, nro=64, nsp=100, osf=2.0, width=2)
    args = ["--basis", os.path.join(str(tmp), "phi.npy"), "--osf", "2.0", "--width", "2", "--lamda", "1e-3", path]
    handler_records = []

    class Keep(logging.Handler):
        def emit(self, record):
            handler_records.append(record.getMessage())
    keep = Keep(level=logging.INFO)
    plog = logging.getLogger("pics")
    old = plog.level
    plog.addHandler(keep)
    plog.setLevel(logging.INFO)
    try:
        pics.main(["-i", "0", "--power-iters", "6", "--no-fuse", "--l1", "0.01", "--debug", "40"] + args, backend=oracle_backend)
    finally:
        plog.removeHandler(keep)
        plog.setLevel(old)
    oracle_backend._scratch = None
    est = [float(m.group(1)) for s in handler_records for m in [re.search(r"largest eigenvalue of A\^H A \+ lamda I (\S+)", s)] if m][0]
    return args, ["--step", "%.8e" % (0.9 / est)]


@pytest.mark.parametrize("extra", [[], ["--llr", "0.02", "--llr-block", "8"], ["--tv", "0.01"], ["--l1", "0.01"]],
                         ids=["cg", "llr", "tv", "l1"])
def test_pics_basis_on_the_gpu_matches_the_oracle_backend(scan, hip, oracle_backend, caplog, extra):
    args, step = scan
    with caplog.at_level(logging.WARNING):
        for iters, tol in (("1", 1e-5), ("10", 1e-4)):
            argv = extra + ["-i", iters, "--debug", "40"] + (step if extra else []) + args
            out = pics.main(argv, backend=hip)
            ref = pics.main(["--no-fuse"] + argv, backend=oracle_backend)
            oracle_backend._scratch = None
            assert out.shape == (32, 32, 32, 1, 1, 1, 2)
            print("pics --basis %s, %s iterations: relative difference %.3e" % (extra, iters, _rel(out, ref)))
            assert _rel(out, ref) < tol, (extra, iters, _rel(out, ref))
    assert not any("scratch arena too small" in r.getMessage() for r in caplog.records)
