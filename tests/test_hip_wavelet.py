"""The wavelet transform, the soft threshold and pics --l1 on the MI355X: ig_dwt3_c64 / ig_csoft_c64 against the float64
restatement in tests/dwt64.py, and the FISTA driver against the same driver on the numpy oracle backend."""
import logging
import os
import re

import numpy as np
import pytest

import dwt64
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
