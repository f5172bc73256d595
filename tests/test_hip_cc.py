"""Coil compression and noise prewhitening on the MI355X: ig_coil_gram_c64 and Backend.coil_mix against the float64 restatement in
tests/cc64.py, the cc driver against the same driver on the numpy oracle backend, and pics --cc."""
import ctypes
import os

import numpy as np
import pytest

import cc64
from indigo_amd import cc, pics
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
TOL = 1e-5          # the project's bar on the relative 2-norm
PAD = 37            # NaN rows under every column of the sample panel
PAD_PARTS = 3       # NaN rows below the partial sums

NS = (1, 105, 2048, 5049)
CS = (1, 2, 3, 5, 8, 12, 16, 17, 32, 33, 64)          # every padded width (8, 16, 32, 64), both sides of each threshold
SLABS = ("one", 1000, 64)                             # one row (slab >= n), a ragged last row, many rows

# every (coils, slab) once with n rotating through its four values; slab = 1 (a row per sample) at n = 105 only; the corners
CASES = [(NS[(i + j) % 4], C, slab) for i, C in enumerate(CS) for j, slab in enumerate(SLABS)]
CASES += [(105, C, 1) for C in CS]
CASES += [c for c in [(5049, 64, 1000), (1, 64, "one")] if c not in CASES]
CASES += [(70001, 64, None)]                          # the backend's default slab, several rows of it


def _rel(a, b):
    return np.linalg.norm((np.asarray(a) - np.asarray(b)).ravel()) / np.linalg.norm(np.asarray(b).ravel())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _padded(hip, a, pad):
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


WORST = {"row": 0.0, "sum": 0.0}


@pytest.mark.parametrize("n,C,slab", CASES, ids=lambda v: str(v))
def test_gram_kernel_matches_the_float64_restatement(hip, n, C, slab):
    y = rand64c(n, C, seed=1000 * C + n)
    x_d, x_h = _padded(hip, y, PAD)
    s = n + 11 if slab == "one" else hip.tuning['gram_slab'] if slab is None else slab
    rows, ntri = -(-n // s), C * (C + 1) // 2
    parts_h = np.full((rows + PAD_PARTS, ntri), np.nan, dtype=C64, order='F')
    got = []
    for call in range(2):
        parts_d = hip.copy_array(parts_h)
        hip._check(hip._L.ig_coil_gram_c64(hip._ctx, n, C, ctypes.c_void_p(x_d._arr), n + PAD, s, ctypes.c_void_p(parts_d._arr),
                                           rows + PAD_PARTS), "ig_coil_gram_c64")
        got.append(parts_d.to_host())
    out = got[0]
    assert np.array_equal(_bits(out), _bits(got[1]))                               # a second call returns the same bits
    assert np.array_equal(_bits(x_d.to_host()), _bits(x_h))                        # the input and its padding
    assert np.array_equal(_bits(out[rows:]), _bits(parts_h[rows:]))                # the rows below the partial sums
    assert np.isfinite(out[:rows]).all()
    G = cc64.unpack(out[:rows], C)
    assert np.array_equal(G.imag[:, np.arange(C), np.arange(C)], np.zeros((rows, C)))
    want = cc64.slab_grams(y, s)
    err_row = max(_rel(G[j], want[j]) for j in range(rows))
    err_sum = _rel(G.sum(axis=0), cc64.gram(y))
    WORST["row"], WORST["sum"] = max(WORST["row"], err_row), max(WORST["sum"], err_sum)
    print("coil_gram n %d C %d slab %s (%d rows): worst row %.3e, sum %.3e; worst so far %.3e / %.3e"
          % (n, C, slab, rows, err_row, err_sum, WORST["row"], WORST["sum"]))
    assert err_row <= TOL and err_sum <= TOL
    # the backend method: the same rows, added in float64 and unpacked
    Gb = hip.coil_gram(x_d[:n], n, C, slab=s)
    assert Gb.dtype == np.complex128 and np.array_equal(Gb, Gb.conj().T) and _rel(Gb, cc64.gram(y)) <= TOL
    assert np.array_equal(_bits(x_d.to_host()), _bits(x_h))


def test_gram_more_slabs_than_workgroups(hip):
    """2^20 + 7 slabs of one sample: the launch is capped at 2^20 workgroups, the first seven take a second slab"""
    n, C = (1 << 20) + 7, 2
    y = rand64c(n, C, seed=77)
    parts = hip.coil_gram_parts(hip.copy_array(y), n, C, slab=1)
    y = y.astype(np.complex128)
    want = np.stack([np.abs(y[:, 0]) ** 2, y[:, 0] * np.conj(y[:, 1]), np.abs(y[:, 1]) ** 2], axis=1)
    assert parts.shape == (n, 3) and np.isfinite(parts).all()
    err = np.abs(parts - want).max() / np.abs(want).max()
    print("coil_gram, %d slabs of one sample: largest element error %.3e" % (n, err))
    assert err <= 1e-6 and np.array_equal(parts.imag[:, [0, 2]], np.zeros((n, 2), dtype=np.float32))


def test_gram_limits(hip):
    n = 64
    buf = hip.copy_array(rand64c(n * 70, 1, seed=1))
    before = buf.to_host()
    parts = hip.copy_array(rand64c(3000, 1, seed=2))

    def call(nc, slab, ldx=n, ldp=1, p=None):
        return hip._L.ig_coil_gram_c64(hip._ctx, n, nc, ctypes.c_void_p(buf._arr), ldx, slab,
                                       ctypes.c_void_p(parts._arr if p is None else p), ldp)
    for args, text in (((65, 16), "65 coils, between 1 and 64"), ((0, 16), "0 coils"), ((4, 0), "slab of 0"), ((4, 16, n - 1), "leading dimension"),
                       ((4, 16, n, 3), "leading dimension"), ((4, 16, n, 4, buf._arr + 8 * 100), "overlaps")):
        with pytest.raises(RuntimeError, match=text):
            hip._check(call(*args), "ig_coil_gram_c64")
    assert np.array_equal(buf.to_host(), before)


@pytest.mark.parametrize("n,C,V", [(5049, 33, 7), (2048, 64, 32), (105, 12, 12), (1, 64, 1)], ids=lambda v: str(v))
def test_coil_mix_matches_the_float64_restatement(hip, n, C, V):
    y, A = rand64c(n, C, seed=C + n), rand64c(V, C, seed=V).astype(np.complex128)
    x_d, x_h = _padded(hip, y, PAD)
    o_d, o_h = _padded(hip, np.full((n, V), np.nan, dtype=C64), PAD)
    hip.coil_mix(o_d[:n], x_d[:n], A, n)
    out = o_d.to_host()
    assert np.array_equal(_bits(x_d.to_host()), _bits(x_h)) and np.array_equal(_bits(out[n:]), _bits(o_h[n:]))
    err = _rel(out[:n], cc64.mix(A, y, coil_axis=1))
    print("coil_mix n %d, %d -> %d: %.3e" % (n, C, V, err))
    assert np.isfinite(out[:n]).all() and err <= TOL
    with pytest.raises(RuntimeError, match="33 virtual coils"):
        hip.coil_mix(o_d[:n], x_d[:n], np.zeros((33, C)), n)


# ---- the drivers --------------------------------------------------------------------------------------------------------------------

def _cc(B, argv):
    return cc.main(argv + ["--debug", "40"], backend=B)


def test_cc_driver_on_the_gpu_matches_the_oracle_backend(hip, oracle_backend, tmp_path):
    """the rank-deficient scan of tests/test_cc_cpu.py (4 true coils seen through 12 channels), 1920 samples in three chunks.
    Measured: lambda_1 ... lambda_3 within 1.3e-07, lambda_4 within 5.4e-06 -- it is 1/1600 of lambda_1, so the float32 rounding of
    G's entries (6e-08 of entries of the size of lambda_1) shows there first --, projectors 1.7e-05 apart (bound 2.3e-02)"""
    path = cc64.rank_deficient_scan(tmp_path, oracle_backend, (16, 16, 16), 32, 60, 2.0, 2)
    stem = os.path.splitext(path)[0]
    A_o, lam_o = _cc(oracle_backend, ["-p", "4", path])
    data_o = np.load(stem + ".cc.npz")['data']
    A_h, lam_h = _cc(hip, ["-p", "4", "--chunk", "700", path])
    out = np.load(stem + ".cc.npz")
    G = cc64.gram(cc64.samples_of(path))
    lam64 = cc64.matrix(G, 4)[1]
    err_lam = np.abs(lam_h[:4] - lam_o[:4]) / lam_o[:4]
    err_p, bound = np.linalg.norm(cc64.projector(A_h) - cc64.projector(A_o)), cc64.davis_kahan(G, lam64, 4)
    print("cc on the device against the oracle: eigenvalues %s, projector %.3e (Davis-Kahan bound %.3e)" % (err_lam, err_p, bound))
    assert err_lam.max() <= 1e-5 and err_p <= bound
    assert out['data'].shape == data_o.shape and out['maps'].shape[1] == 4
    z = np.load(path)
    assert _rel(out['data'].T, cc64.mix(A_h, z['data'].T)) <= TOL and _rel(out['maps'].T, cc64.mix(A_h, z['maps'].T)) <= TOL
    assert cc.matrix(G, energy=0.999999)[0].shape[0] == _cc(hip, ["-e", "0.999999", path])[0].shape[0] == 4


N32, NRO, NSP = (32, 32, 32), 64, 100
OPTS = ["--osf", "2.0", "--width", "2"]


@pytest.fixture(scope="module")
def scan32(tmp_path_factory, oracle_backend):
    """32^3, 12 channels of 4 true coils, 100 spokes x 64; lamda = a tenth of the largest eigenvalue of A^H A (power iteration on the
    oracle, on the 4 virtual coils), the rule of tests/test_hip_softsense.py for comparing two realisations of one operator"""
    path = cc64.rank_deficient_scan(tmp_path_factory.mktemp("cc32"), oracle_backend, N32, NRO, NSP, 2.0, 2)
    L = cc64.largest_eigenvalue(oracle_backend, ["--no-fuse", "--cc", "4"] + OPTS + ["--lamda", "0", path])
    return path, OPTS + ["--lamda", "%.8e" % (L / 10), path]


def _pics(B, argv):
    B._scratch = None
    try:
        return pics.main(argv + ["--debug", "40"], backend=B)
    finally:
        B._scratch = None


def test_pics_cc_on_the_gpu_matches_the_oracle_backend(hip, oracle_backend, scan32):
    path, args = scan32
    for iters, tol in (("1", 1e-5), ("10", 1e-4)):
        out = _pics(hip, ["-i", iters, "--cc", "4"] + args)
        ref = _pics(oracle_backend, ["--no-fuse", "-i", iters, "--cc", "4"] + args)
        print("pics --cc 4 on the device against the oracle, %s iterations: %.3e" % (iters, _rel(out, ref)))
        assert out.shape == N32 + (1,) and _rel(out, ref) < tol


def test_pics_cc_full_rank_equals_no_compression_on_the_gpu(hip, scan32):
    path, args = scan32
    for iters, tol in (("1", 1e-5), ("10", 1e-4)):
        out = _pics(hip, ["-i", iters, "--cc", "12"] + args)
        ref = _pics(hip, ["-i", iters] + args)
        print("pics --cc 12 against pics on the device, %s iterations: %.3e" % (iters, _rel(out, ref)))
        assert out.shape == N32 + (1,) and _rel(out, ref) < tol
