"""The gradient with a temporal difference, its adjoint, the fused spatio-temporal dual step and pics --tv-time on the MI355X:
ig_grad4_c64 / ig_grad4h_c64 / ig_tv4_dual_c64 against the float64 restatement in tests/tv4_64.py, and the primal-dual driver on
two time frames against the same driver on the numpy oracle backend."""
import logging
import os
import re

import numpy as np
import pytest

import tv4_64
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
# nothing a multiple of a wave or a line; several workgroups; unit axes; one frame; 67 600 rows (more groups of rows than the
# kernels' grid holds, so they stride)
CASES = [((17, 5, 3), 3), ((64, 48, 40), 2), ((8, 1, 6), 4), ((1, 1, 9), 2), ((2, 2, 2), 1), ((8, 260, 260), 2)]
PAD = 37


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _padded(hip, a, fill=0.0, pad=PAD):
    """the panel a (rows x frames) on the device with `pad` extra rows of `fill` under every column, and the host copy"""
    p = np.full((a.shape[0] + pad, a.shape[1]), fill, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _grad(hip, x, dims, T, adjoint=False, alpha=1, beta=0, y0=None):
    """grad4 of the panel x into a panel with PAD extra rows (which must come back untouched); y starts as y0 or NaN"""
    n = int(np.prod(dims))
    rows_y = n if adjoint else 4 * n
    x_d, _ = _padded(hip, x)
    y_d, yp = _padded(hip, np.full((rows_y, T), np.nan, dtype=C64) if y0 is None else y0, fill=np.nan)
    hip.grad4(y_d[:rows_y], x_d[:x.shape[0]], dims, T, adjoint=adjoint, alpha=alpha, beta=beta)
    out = y_d.to_host()
    assert np.array_equal(out[rows_y:], yp[rows_y:], equal_nan=True)
    return out[:rows_y]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "x".join(map(str, c[0])) + "x%d" % c[1])
def case(request):
    """the frames of one volume shape as panels and their float64 gradients, computed once"""
    dims, T = request.param
    n = int(np.prod(dims))
    x = rand64c(n, T, seed=1) - (0.5 + 0.5j)
    u = rand64c(4 * n, T, seed=2) - (0.5 + 0.5j)
    xo = rand64c(n, T, seed=3) - (0.5 + 0.5j)
    for a in (x, u, xo):
        a.setflags(write=False)
    return dict(dims=dims, T=T, n=n, x=x, u=u, xo=xo, Dx=tv4_64.grad(x, dims, T).reshape((4 * n, T), order='F'),
                DHu=tv4_64.gradh(u, dims, T).reshape((n, T), order='F'))


def test_grad4_matches_the_float64_gradient(hip, case):
    dims, T, n, x, u = (case[k] for k in ("dims", "T", "n", "x", "u"))
    alpha, beta = 0.75 - 0.5j, -0.25 + 1.5j
    fwd = _grad(hip, x, dims, T)                                        # y starts as NaN: beta == 0 does not read it
    adj = _grad(hip, u, dims, T, adjoint=True)
    assert np.isfinite(fwd).all() and np.isfinite(adj).all()
    assert _rel(fwd, case["Dx"]) < 2e-6, _rel(fwd, case["Dx"])
    assert _rel(adj, case["DHu"]) < 2e-6, _rel(adj, case["DHu"])
    assert not fwd[3 * n:, T - 1].any()                                 # the temporal component of the last frame: exactly zero
    for adjoint, src, ref in ((False, x, case["Dx"]), (True, u, case["DHu"])):
        y0 = rand64c(ref.shape[0], T, seed=4) - (0.5 + 0.5j)
        out = _grad(hip, src, dims, T, adjoint=adjoint, alpha=alpha, beta=beta, y0=y0)
        assert _rel(out, alpha * ref + beta * y0) < 2e-6, (adjoint, _rel(out, alpha * ref + beta * y0))
    # adjoint identity <D4 x, u> = <x, D4^H u> on the device results
    lhs, rhs = np.vdot(u.astype(np.complex128), fwd), np.vdot(adj.astype(np.complex128), x)
    assert abs(lhs - rhs) < 1e-6 * np.linalg.norm(x) * np.linalg.norm(u)
    # the adjoint does not read the temporal component of the last frame
    u_nan = u.copy()
    u_nan[3 * n:, T - 1] = np.nan
    assert np.array_equal(_grad(hip, u_nan, dims, T, adjoint=True), adj)


def test_one_frame_is_the_3d_kernels_with_a_zero_component(hip):
    dims, n = (17, 5, 3), 255
    x, xo = (hip.copy_array(rand64c(n, 1, seed=s) - (0.5 + 0.5j)) for s in (1, 3))
    u = rand64c(4 * n, 1, seed=2) - (0.5 + 0.5j)
    u[3 * n:] = 0
    y4, y3 = hip.zero_array((4 * n, 1), C64), hip.zero_array((3 * n, 1), C64)
    hip.grad4(y4, x, dims, 1)
    hip.grad3(y3, x, dims)
    assert np.array_equal(y4.to_host()[:3 * n], y3.to_host()) and not y4.to_host()[3 * n:].any()
    h4, h3 = hip.zero_array((n, 1), C64), hip.zero_array((n, 1), C64)
    hip.grad4(h4, hip.copy_array(u), dims, 1, adjoint=True)
    hip.grad3(h3, hip.copy_array(np.asfortranarray(u[:3 * n])), dims, adjoint=True)
    assert np.array_equal(h4.to_host(), h3.to_host())
    u4, u3 = hip.copy_array(u), hip.copy_array(np.asfortranarray(u[:3 * n]))
    hip.tv4_dual_step(u4, x, xo, 0.7, 0.9, 0.5, dims, 1)
    hip.tv_dual_step(u3, x, xo, 0.7, 0.9, dims)
    assert np.array_equal(u4.to_host()[:3 * n], u3.to_host()) and not u4.to_host()[3 * n:].any()


def test_grad4_rejects_overlapping_panels(hip):
    dims, T = (8, 4, 2), 2
    n = 64
    # x as the panel (N, 2) in rows [0, 2N), then room for y (4N, 2) in rows [2N, 10N)
    buf = hip.copy_array(rand64c(10 * n, 1, seed=1))
    before = buf.to_host()
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.grad4(buf[n:9 * n], buf[:2 * n], dims, T)                   # y = rows [N, 9N) holds frame 1 of x = rows [N, 2N)
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.grad4(buf[8 * n - 1:10 * n - 1], buf[:8 * n], dims, T, adjoint=True)
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tv4_dual_step(buf[:8 * n], buf[8 * n:], buf[n:3 * n], 1.0, 1.0, 1.0, dims, T)       # u holds xo
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tv4_dual_step(buf[:8 * n], buf[7 * n:9 * n], buf[8 * n:], 1.0, 1.0, 1.0, dims, T)   # u holds the first frame of xn
    assert np.array_equal(buf.to_host(), before)
    hip.grad4(buf[2 * n:], buf[:2 * n], dims, T)                        # adjacent, not overlapping: fine
    np.testing.assert_allclose(buf.to_host()[2 * n:, 0], tv4_64.grad(before[:2 * n, 0], dims, T), atol=1e-6)


def test_tv4_dual_step_matches_the_float64_step(hip, case):
    dims, T, n, x, u, xo = (case[k] for k in ("dims", "T", "n", "x", "u", "xo"))
    sigma = 0.7
    unprojected = u.astype(np.complex128) + sigma * tv4_64.grad(2.0 * x.astype(np.complex128) - xo, dims, T).reshape(u.shape, order='F')
    r, m = tv4_64.radius(unprojected, dims, T), tv4_64.modulus_t(unprojected, dims, T)
    mu = float(np.float32(np.median(r)))                               # the ball that clips about half of the voxels
    clipped = (r > mu).mean()
    assert 0.2 <= clipped <= 0.8, clipped
    if T > 1:
        mu_t = float(np.float32(np.median(m[..., :T - 1])))            # and the disc that clips about half of the differences
        clipped_t = (m[..., :T - 1] > mu_t).mean()
        assert 0.2 <= clipped_t <= 0.8, clipped_t
    else:
        mu_t = float(np.float32(np.median(m)))                         # no differences: u_3 kept where |u_3| <= mu_t, else scaled
    ref = tv4_64.dual_step(u, x, xo, sigma, mu, mu_t, dims, T)
    # three different leading dimensions: a kernel that took the next frame N rows on, or with xn's stride in xo, fails here
    x_d, xo_d = _padded(hip, x, fill=np.nan)[0], _padded(hip, xo, fill=np.nan, pad=11)[0]

    def step(mu_, mu_t_):
        u_d, up = _padded(hip, u, fill=np.nan, pad=23)
        hip.tv4_dual_step(u_d[:4 * n], x_d[:n], xo_d[:n], sigma, mu_, mu_t_, dims, T)
        out = u_d.to_host()
        assert np.array_equal(out[4 * n:], up[4 * n:], equal_nan=True)  # the rows between columns are left alone
        return out[:4 * n]
    out = step(mu, mu_t)
    assert _rel(out, ref) < 2e-6, _rel(out, ref)
    assert tv4_64.radius(out, dims, T).max() <= mu * (1 + 1e-6)
    assert tv4_64.modulus_t(out, dims, T).max() <= mu_t * (1 + 1e-6)
    if T == 1:
        u3, o3 = u[3 * n:, 0], out[3 * n:, 0]
        kept = np.abs(u3.astype(np.complex128)) <= mu_t
        assert np.array_equal(o3[kept], u3[kept]) and 0 < kept.sum() < n
        np.testing.assert_allclose(np.abs(o3[~kept]), mu_t, rtol=1e-6)
    zs = step(0.0, mu_t)                                                # mu = 0: exact zeros in the spatial part, the rest as before
    assert not zs[:3 * n].any() and _rel(zs[3 * n:], ref.reshape(u.shape, order='F')[3 * n:]) < 2e-6
    zt = step(mu, 0.0)                                                  # mu_t = 0: exact zeros in the temporal part
    assert not zt[3 * n:].any() and _rel(zt[:3 * n], ref.reshape(u.shape, order='F')[:3 * n]) < 2e-6
    big = step(1e6, 1e6)                                                # nothing clips: the unprojected step
    assert _rel(big, unprojected) < 2e-6, _rel(big, unprojected)


def test_gradient_t_in_an_operator_product(hip):
    dims, T = (17, 5, 3), 3
    G = hip.GradientT(dims, T)
    x = rand64c(G.shape[1], 2, seed=6) - (0.5 + 0.5j)                    # two stacked vectors side by side: one product per column
    ref = np.stack([tv4_64.gradh(tv4_64.grad(x[:, j], dims, T), dims, T) for j in range(2)], axis=1)
    out = (G.H * G) * x
    assert out.shape == ref.shape and _rel(out, ref) < 2e-6, _rel(out, ref)


def _scan(tmpdir, B, N, C, T, nro, nsp, osf, width=2):
    """a synthetic radial scan of T frames (a box that moves) with a trajectory per frame, built the way test_hip_tv builds its scan"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    centres = [(-1, 0, 0.3), (1, 0.5, -0.4)][:C]
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph) for cx, cy, ph in centres],
                   axis=3).astype(np.complex64)
    ksps, trajs = [], []
    for t in range(T):
        img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j)).astype(np.complex64)
        img[(np.abs(g[0] - 0.1 * t) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5    # an edge for the differences to see; it moves
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


def _logged(caplog, pattern):
    return [float(m.group(1)) for r in caplog.records for m in [re.search(pattern, r.getMessage())] if m]


def test_pics_tv_time_on_the_gpu_matches_the_oracle_backend(tmp_path, hip, oracle_backend, caplog):
    N, T = (64, 64, 64), 2
    path = _scan(tmp_path, hip, N, 2, T, nro=128, nsp=200, osf=2.0)
    args = ["--osf", "2.0", "--width", "2", "--lamda", "1e-3", "--tv", "0.02", "--tv-time", "0.02", "--debug", "40", path]
    # the step from the oracle's power-iteration estimate of the largest eigenvalue of A^H A + lamda I
    with caplog.at_level(logging.INFO, logger="pics"):
        pics.main(["-i", "0", "--power-iters", "6", "--no-fuse"] + args, backend=oracle_backend)
    oracle_backend._scratch = None
    assert "frames 2, distinct trajectories 2" in [r.getMessage() for r in caplog.records]
    est = _logged(caplog, r"largest eigenvalue of A\^H A \+ lamda I (\S+)")[0]
    step = ["--step", "%.8e" % (0.9 / est)]
    for extra, iters, tol in (([], "1", 1e-5), ([], "10", 1e-4), (["--l1", "0.02"], "10", 1e-4)):
        out = pics.main(extra + ["-i", iters] + step + args, backend=hip)
        ref = pics.main(extra + ["-i", iters, "--no-fuse"] + step + args, backend=oracle_backend)
        oracle_backend._scratch = None
        assert out.shape == N + (1,) * 7 + (T,)
        assert _rel(out, ref) < tol, (extra, iters, _rel(out, ref))
