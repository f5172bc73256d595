"""The gradient, its adjoint, the fused total-variation dual step and pics --tv on the MI355X: ig_grad3_c64 / ig_grad3h_c64 /
ig_tv_dual_c64 against the float64 restatement in tests/tv64.py, and the primal-dual driver against the same driver on the numpy
oracle backend."""
import logging
import os
import re

import numpy as np
import pytest

import tv64
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
# nothing a multiple of a wave or a line; several workgroups; unit axes; the smallest; 67 600 rows (more groups of rows than
# the kernels' grid holds, so they stride)
DIMS = [(17, 5, 3), (64, 48, 40), (8, 1, 6), (1, 1, 9), (2, 2, 2), (8, 260, 260)]
PAD = 37


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _padded(hip, a, fill=0.0):
    """the panel a (rows x ncols) on the device with PAD extra rows of `fill` under every column, and the host copy"""
    p = np.full((a.shape[0] + PAD, a.shape[1]), fill, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _grad(hip, x, dims, adjoint=False, alpha=1, beta=0, y0=None):
    """grad3 of the panel x into a panel with PAD extra rows (which must come back untouched); y starts as y0 or NaN"""
    n = int(np.prod(dims))
    rows_y = n if adjoint else 3 * n
    x_d, _ = _padded(hip, x)
    y_d, yp = _padded(hip, np.full((rows_y, x.shape[1]), np.nan, dtype=C64) if y0 is None else y0, fill=np.nan)
    hip.grad3(y_d[:rows_y], x_d[:x.shape[0]], dims, adjoint=adjoint, alpha=alpha, beta=beta)
    out = y_d.to_host()
    assert np.array_equal(out[rows_y:], yp[rows_y:], equal_nan=True)
    return out[:rows_y]


@pytest.fixture(scope="module", params=DIMS, ids=lambda d: "x".join(map(str, d)))
def case(request):
    """two-column inputs of one volume shape and their float64 gradients, computed once"""
    dims = request.param
    n = int(np.prod(dims))
    x = rand64c(n, 2, seed=1) - (0.5 + 0.5j)
    u = rand64c(3 * n, 2, seed=2) - (0.5 + 0.5j)
    xo = rand64c(n, 2, seed=3) - (0.5 + 0.5j)
    for a in (x, u, xo):
        a.setflags(write=False)
    return dict(dims=dims, n=n, x=x, u=u, xo=xo, Dx=tv64.grad(x, dims), DHu=tv64.gradh(u, dims))


def test_grad3_matches_the_float64_gradient(hip, case):
    dims, x, u = case["dims"], case["x"], case["u"]
    alpha, beta = 0.75 - 0.5j, -0.25 + 1.5j
    fwd = _grad(hip, x, dims)                                           # y starts as NaN: beta == 0 does not read it
    adj = _grad(hip, u, dims, adjoint=True)
    assert np.isfinite(fwd).all() and np.isfinite(adj).all()
    assert _rel(fwd, case["Dx"]) < 2e-6, _rel(fwd, case["Dx"])
    assert _rel(adj, case["DHu"]) < 2e-6, _rel(adj, case["DHu"])
    for adjoint, src, ref in ((False, x, case["Dx"]), (True, u, case["DHu"])):
        y0 = rand64c(ref.shape[0], 2, seed=4) - (0.5 + 0.5j)
        out = _grad(hip, src, dims, adjoint=adjoint, alpha=alpha, beta=beta, y0=y0)
        assert _rel(out, alpha * ref + beta * y0) < 2e-6, (adjoint, _rel(out, alpha * ref + beta * y0))
    # adjoint identity <D x, u> = <x, D^H u> on the device results
    lhs, rhs = np.vdot(u.astype(np.complex128), fwd), np.vdot(adj.astype(np.complex128), x)
    assert abs(lhs - rhs) < 1e-6 * np.linalg.norm(x) * np.linalg.norm(u)


def test_grad3_rejects_overlapping_panels(hip):
    dims = (8, 4, 2)
    n = 64
    buf = hip.copy_array(rand64c(4 * n, 1, seed=1))
    before = buf.to_host()
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.grad3(buf[:3 * n], buf[2 * n:3 * n], dims)                  # y = rows [0, 3N) holds x = rows [2N, 3N)
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.grad3(buf[3 * n - 1:4 * n - 1], buf[:3 * n], dims, adjoint=True)
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tv_dual_step(buf[:3 * n], buf[3 * n:], buf[n:2 * n], 1.0, 1.0, dims)
    assert np.array_equal(buf.to_host(), before)
    hip.grad3(buf[:3 * n], buf[3 * n:], dims)                           # adjacent, not overlapping: fine
    np.testing.assert_allclose(buf.to_host()[:3 * n], tv64.grad(before[3 * n:], dims), atol=1e-6)


def test_tv_dual_step_matches_the_float64_step(hip, case):
    dims, n, x, u, xo = (case[k] for k in ("dims", "n", "x", "u", "xo"))
    sigma = 0.7
    unprojected = u.astype(np.complex128) + sigma * tv64.grad(2.0 * x.astype(np.complex128) - xo, dims)
    r = tv64.radius(unprojected, dims)
    mu = float(np.float32(np.median(r)))                               # the ball that clips about half of the voxels
    ref = tv64.dual_step(u, x, xo, sigma, mu, dims)
    clipped = (r > mu).mean()
    assert 0.2 <= clipped <= 0.8, clipped
    x_d, xo_d = hip.copy_array(x), hip.copy_array(xo)

    def step(mu_):
        u_d, up = _padded(hip, u, fill=np.nan)
        hip.tv_dual_step(u_d[:3 * n], x_d, xo_d, sigma, mu_, dims)
        out = u_d.to_host()
        assert np.array_equal(out[3 * n:], up[3 * n:], equal_nan=True)  # the rows between columns are left alone
        return out[:3 * n]
    out = step(mu)
    assert _rel(out, ref) < 2e-6, _rel(out, ref)
    assert tv64.radius(out, dims).max() <= mu * (1 + 1e-6)
    assert not step(0.0).any()                                          # mu = 0: exact zeros
    big = step(1e6)                                                     # nothing clips: the unprojected step
    assert _rel(big, unprojected) < 2e-6, _rel(big, unprojected)


def test_gradient_in_an_operator_product(hip):
    dims = (17, 5, 3)
    G = hip.Gradient(dims)
    x = rand64c(G.shape[1], 2, seed=6) - (0.5 + 0.5j)
    ref = tv64.gradh(tv64.grad(x, dims), dims)
    out = (G.H * G) * x
    assert _rel(out, ref) < 2e-6, _rel(out, ref)


def _scan(tmpdir, B, N, C, nro, nsp, osf, width=2):
    """a synthetic radial scan built the way test_hip_pics builds its scans"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j)).astype(np.complex64)
    img[(np.abs(g[0]) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5                 # an edge for the differences to see
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


def test_pics_tv_on_the_gpu_matches_the_oracle_backend(tmp_path, hip, oracle_backend, caplog):
    N = (64, 64, 64)
    path = _scan(tmp_path, hip, N, 2, nro=128, nsp=200, osf=2.0)
    args = ["--osf", "2.0", "--width", "2", "--lamda", "1e-3", "--tv", "0.02", "--debug", "40", path]
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
    for extra, iters, tol in (([], "1", 1e-5), ([], "10", 1e-4), (["--l1", "0.02"], "10", 1e-4)):
        out = pics.main(extra + ["-i", iters] + step + args, backend=hip)
        ref = pics.main(extra + ["-i", iters, "--no-fuse"] + step + args, backend=oracle_backend)
        oracle_backend._scratch = None
        assert _rel(out, ref) < tol, (extra, iters, _rel(out, ref))
    # the objective falls
    obj = {}
    for iters in ("5", "30"):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="pics"):
            pics.main(["-i", iters] + args, backend=hip)
        obj[iters] = _logged(caplog, r"tv iter \d+, objective (\S+)")[-1]
    assert obj["30"] < obj["5"], obj
