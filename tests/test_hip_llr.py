"""Block-wise singular-value thresholding, the blocks' nuclear norms and pics --llr on the MI355X: ig_llr_svt_c64 /
ig_llr_nuc_c64 against the float64 restatement in tests/llr64.py, and the driver on three time frames against the same driver on
the numpy oracle backend."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

import llr64
from llr_cases import CASES, INPUTS, case_id, make_input, share_above, threshold
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
TOL = 5e-6          # of the float64 result: 5 x the float64-Gram model's worst value, half the project's 1e-5


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _bits(a):
    """the bit patterns of a complex64 array (NaN payloads included), whatever its memory order"""
    return np.ascontiguousarray(a).view(np.uint32)


def _padded(hip, a, pad):
    """the panel a (rows x frames) on the device with `pad` extra rows of NaN under every column, and the host copy"""
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


@pytest.fixture(scope="module", params=[(c, k) for c in CASES for k in INPUTS], ids=lambda p: case_id(p[0]) + "_" + p[1])
def case(request):
    """one shape and one input, its singular values, threshold and float64 results, computed once"""
    (dims, block, T, shift), kind = request.param
    x = make_input(kind, dims, block, T, shift)
    x.setflags(write=False)
    sv = llr64.singular_values(x, dims, T, block, shift)
    tau = threshold(sv)
    return dict(dims=dims, block=block, T=T, shift=shift, n=int(np.prod(dims)), x=x, sv=sv, tau=tau,
                svt=llr64.svt(x, tau, dims, T, block, shift), nuc=np.array([s.sum() for s in sv]))


def _svt(hip, c, tau, pad):
    """llr_threshold on the panel with `pad` NaN rows under every column, which must come back bit-identical"""
    x_d, xp = _padded(hip, c["x"], pad)
    hip.llr_threshold(x_d[:c["n"]], tau, c["dims"], c["T"], c["block"], c["shift"])
    out = x_d.to_host()
    assert np.array_equal(_bits(out[c["n"]:]), _bits(xp[c["n"]:]))
    return out[:c["n"]]


def test_the_threshold_bites(case):
    share = share_above(case["sv"], case["tau"])
    assert 0.2 <= share <= 0.8, share


def test_svt_matches_the_float64_svt(hip, case):
    c = case
    dims, block, T, shift, n, x, tau = (c[k] for k in ("dims", "block", "T", "shift", "n", "x", "tau"))
    out = _svt(hip, c, tau, pad=37)
    err = _rel(out, c["svt"])
    print("svt: relative error %.3e" % err)
    assert np.isfinite(out).all() and err < TOL, err
    assert np.array_equal(_svt(hip, c, tau, pad=11), out)                # another leading dimension, the same bits
    stacked = hip.copy_array(np.asfortranarray(x.reshape((-1, 1), order='F')))
    hip.llr_threshold(stacked, tau, dims, T, block, shift)
    assert np.array_equal(stacked.to_host().reshape((n, T), order='F'), out)
    # no singular value of a block's result exceeds sigma - tau by more than TOL * sigma_max
    for s_in, s_out in zip(c["sv"], llr64.singular_values(out, dims, T, block, shift)):
        assert np.all(s_out <= np.maximum(s_in - tau, 0.0) + TOL * s_in[0]), (s_in, s_out, tau)


def test_svt_at_the_ends_of_the_threshold(hip, case):
    c = case
    same = _svt(hip, c, 0.0, pad=5)                                      # tau = 0 still goes through P = V V^H
    assert _rel(same, c["x"]) < 2e-6, _rel(same, c["x"])
    smax = max(s[0] for s in c["sv"])
    assert not _svt(hip, c, 2.0 * smax, pad=5).any()                     # tau above every singular value: exact zeros


def test_nuc_matches_the_float64_norms(hip, case):
    c = case
    x_d, xp = _padded(hip, c["x"], 23)
    got = hip.llr_block_norms(x_d[:c["n"]], c["dims"], c["T"], c["block"], c["shift"])
    assert np.array_equal(_bits(x_d.to_host()), _bits(xp))     # x is only read
    assert got.dtype == np.float32 and got.shape == c["nuc"].shape
    err = np.abs(got - c["nuc"]) / c["nuc"]
    print("nuc: worst block %.3e" % err.max())
    assert err.max() < TOL, err.max()
    total = hip.llr_norm(x_d[:c["n"]], c["dims"], c["T"], c["block"], c["shift"])
    assert isinstance(total, float) and abs(total - c["nuc"].sum()) < TOL * c["nuc"].sum()
    stacked = hip.copy_array(np.asfortranarray(c["x"].reshape((-1, 1), order='F')))
    assert np.array_equal(hip.llr_block_norms(stacked, c["dims"], c["T"], c["block"], c["shift"]), got)


def test_unsupported_sizes_raise(hip):
    dims = (16, 16, 8)
    n = int(np.prod(dims))
    x33 = hip.copy_array(rand64c(n, 33, seed=1))
    with pytest.raises(RuntimeError, match="33 frames"):
        hip.llr_threshold(x33, 0.1, dims, 33, (8, 8, 8))
    with pytest.raises(RuntimeError, match="33 frames"):
        hip.llr_norm(x33, dims, 33, (8, 8, 8))
    x2 = hip.copy_array(rand64c(n, 2, seed=1))
    before = x2.to_host()
    with pytest.raises(RuntimeError, match="2048 voxels"):
        hip.llr_threshold(x2, 0.1, dims, 2, (16, 16, 8))
    with pytest.raises(RuntimeError, match="2048 voxels"):
        hip.llr_norm(x2, dims, 2, (16, 16, 8))
    with pytest.raises(RuntimeError, match="shift"):
        hip.llr_threshold(x2, 0.1, dims, 2, (8, 8, 8), (8, 0, 0))
    with pytest.raises(RuntimeError, match="threshold"):
        hip.llr_threshold(x2, -1.0, dims, 2, (8, 8, 8))
    assert np.array_equal(x2.to_host(), before)
    hip.llr_threshold(x2, 0.0, (16, 16, 8), 2, (16, 8, 8))               # 1024 voxels: the limit itself is served
    assert _rel(x2.to_host(), before) < 2e-6


def test_nuc_overlapping_x_raises(hip):
    dims, T, block = (8, 4, 2), 2, (4, 4, 2)
    n, nb = 64, 2
    buf = hip.copy_array(rand64c(2 * n + 1, 1, seed=1))                  # x = rows [0, 2N), one more element behind it
    before = buf.to_host()

    def nuc_at(byte_offset):
        return hip._L.ig_llr_nuc_c64(hip._ctx, *dims, T, *block, 0, 0, 0, ctypes.c_void_p(buf._arr), n,
                                     ctypes.c_void_p(buf._arr + byte_offset))
    for off in (0, 8 * n, 8 * 2 * n - 4):                                # the first frame, the second, the panel's last float
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(nuc_at(off), "ig_llr_nuc_c64")
    assert np.array_equal(buf.to_host(), before)
    hip._check(nuc_at(8 * 2 * n), "ig_llr_nuc_c64")                      # adjacent, not overlapping: nb floats = one element
    after = buf.to_host()
    assert np.array_equal(after[:2 * n], before[:2 * n])
    np.testing.assert_allclose(np.ascontiguousarray(after[2 * n:]).view(np.float32).ravel(), llr64.nuc(before[:2 * n, 0], dims, T, block), rtol=TOL)
    assert nb == np.ascontiguousarray(after[2 * n:]).view(np.float32).size


def _scan(tmpdir, B, N, C, T, nro, nsp, osf, width=2):
    """a synthetic radial scan of T frames (a box that moves) with a trajectory per frame"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    centres = [(-1, 0, 0.3), (1, 0.5, -0.4)][:C]
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph) for cx, cy, ph in centres],
                   axis=3).astype(np.complex64)
    ksps, trajs = [], []
    for t in range(T):
        img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j)).astype(np.complex64)
        img[(np.abs(g[0] - 0.1 * t) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5
        coord = radial_trajectory(nsp, nro, seed=2 + t)
        F1 = B.NUFFT((1, nro, nsp), N, coord, width=width, oversamp=(osf, osf, osf), dtype=C64)
        A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
        ksps.append((A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F'))
        trajs.append(coord * np.array(N, dtype=np.float64)[:, None, None])
    ksp = np.stack(ksps, axis=-1).reshape(ksps[0].shape + (1,) * 6 + (T,))
    traj = np.stack(trajs, axis=-1).reshape(trajs[0].shape + (1,) * 7 + (T,))
    path = os.path.join(str(tmpdir), "scan.npz")
    np.savez(path, data=ksp.T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path


def test_pics_llr_on_the_gpu_matches_the_oracle_backend(tmp_path, hip, oracle_backend, caplog):
    N, T = (64, 64, 64), 3
    path = _scan(tmp_path, hip, N, 2, T, nro=128, nsp=200, osf=2.0)
    args = ["--osf", "2.0", "--width", "2", "--lamda", "1e-3", "--llr", "0.02", "--llr-block", "8", "--debug", "40", path]
    # the step from the oracle's power-iteration estimate of the largest eigenvalue of A^H A + lamda I
    with caplog.at_level(logging.INFO, logger="pics"):
        pics.main(["-i", "0", "--power-iters", "6", "--no-fuse"] + args, backend=oracle_backend)
    oracle_backend._scratch = None
    est = [float(m.group(1)) for r in caplog.records
           for m in [re.search(r"largest eigenvalue of A\^H A \+ lamda I (\S+)", r.getMessage())] if m][0]
    step = ["--step", "%.8e" % (0.9 / est)]
    for extra, iters, tol in (([], "1", 1e-5), ([], "10", 1e-4), (["--llr-shifts"], "10", 1e-4), (["--tv-time", "0.02"], "10", 1e-4)):
        out = pics.main(extra + ["-i", iters] + step + args, backend=hip)
        ref = pics.main(extra + ["-i", iters, "--no-fuse"] + step + args, backend=oracle_backend)
        oracle_backend._scratch = None
        assert out.shape == N + (1,) * 7 + (T,)
        print("pics --llr %s, %s iterations: relative difference %.3e" % (extra, iters, _rel(out, ref)))
        assert _rel(out, ref) < tol, (extra, iters, _rel(out, ref))
