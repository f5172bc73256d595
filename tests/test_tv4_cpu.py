"""pics on several time frames on the CPU: the float64 restatement (tests/tv4_64.py) against its definition,
the host forms of Backend.grad4 / tv4_dual_step and operators.GradientT against it, and the driver on a tiny multi-frame scan
against a complex128 Condat-Vu loop on the dense block-diagonal matrix of the same operator -- all on the numpy oracle backend."""
import logging
import os
import re

import numpy as np
import pytest

import dwt64
import tv4_64
import tv64
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
CASES = [((17, 5, 3), 3), ((8, 1, 6), 4), ((1, 1, 9), 2), ((2, 2, 2), 1)]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _c128(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def test_float64_gradient_voxel_by_voxel_and_its_adjoint():
    dims, T = (5, 4, 3), 3
    rng = np.random.default_rng(1)
    n = 60
    x, u = _c128(rng, n, T), _c128(rng, 4 * n, T)
    v = x.reshape(dims + (T,), order='F')
    d = tv4_64.grad(x, dims, T)
    assert d.shape == (4 * n, T)
    d = d.reshape(dims + (4, T), order='F')
    shape4 = dims + (T,)
    for i in np.ndindex(*shape4):
        for a in range(4):
            j = tuple(i[b] + (b == a) for b in range(4))
            assert d[i[:3] + (a, i[3])] == (v[j] - v[i] if i[a] < shape4[a] - 1 else 0)
    # the adjoint, voxel by voxel from its formula
    c = u.reshape(dims + (4, T), order='F')
    h = tv4_64.gradh(u, dims, T).reshape(shape4, order='F')
    for i in np.ndindex(*shape4):
        s = 0
        for a in range(4):
            lo = tuple(i[b] - (b == a) for b in range(4))
            if i[a] > 0:
                s += c[lo[:3] + (a, lo[3])]
            if i[a] < shape4[a] - 1:
                s -= c[i[:3] + (a, i[3])]
        assert abs(h[i] - s) < 1e-14
    # stacked vectors are the same thing
    xs, us = x.reshape(-1, order='F'), u.reshape(-1, order='F')
    assert np.array_equal(tv4_64.grad(xs, dims, T), tv4_64.grad(x, dims, T).reshape(-1, order='F'))
    assert np.array_equal(tv4_64.gradh(us, dims, T), tv4_64.gradh(u, dims, T).reshape(-1, order='F'))
    assert np.array_equal(tv4_64.grad(np.full(n * T, 2 - 3j), dims, T), np.zeros(4 * n * T))
    for dm, Tm in CASES + [(dims, T)]:
        nm = int(np.prod(dm))
        xm, um = _c128(rng, nm * Tm), _c128(rng, 4 * nm * Tm)
        lhs, rhs = np.vdot(um, tv4_64.grad(xm, dm, Tm)), np.vdot(tv4_64.gradh(um, dm, Tm), xm)
        assert abs(lhs - rhs) < 1e-12 * np.linalg.norm(xm) * np.linalg.norm(um), (dm, Tm)


def test_float64_one_frame_is_the_3d_restatement():
    dims = (5, 4, 3)
    rng = np.random.default_rng(3)
    x, u = _c128(rng, 60), _c128(rng, 240)
    g = tv4_64.grad(x, dims, 1)
    assert np.array_equal(g[:180], tv64.grad(x, dims)) and not g[180:].any()
    assert np.array_equal(tv4_64.gradh(u, dims, 1), tv64.gradh(u[:180], dims))


def test_float64_gradient_norm():
    lam = tv4_64.norm2_estimate((9, 8, 7), 5)
    assert 12 < lam <= 16, lam                             # 4 per axis longer than 1, time included (and the estimate is not trivially small)
    lam = tv4_64.norm2_estimate((1, 1, 1), 9)
    assert 3 < lam <= 4, lam


def test_float64_projections():
    dims, T, mu, mu_t = (5, 4, 3), 3, 2.4, 1.2
    u = _c128(np.random.default_rng(2), 4 * 60, T)
    p = tv4_64.proj(u, mu, mu_t, dims, T)
    r, rp = tv4_64.radius(u, dims, T), tv4_64.radius(p, dims, T)
    m, mp = tv4_64.modulus_t(u, dims, T), tv4_64.modulus_t(p, dims, T)
    assert 0.1 < (r > mu).mean() < 0.9 and 0.1 < (m > mu_t).mean() < 0.9
    np.testing.assert_allclose(rp, np.minimum(r, mu), atol=1e-14)
    np.testing.assert_allclose(mp, np.minimum(m, mu_t), atol=1e-14)
    c, cp = u.reshape(dims + (4, T), order='F'), p.reshape(dims + (4, T), order='F')
    inside = np.broadcast_to((r <= mu)[:, :, :, None, :], dims + (3, T))
    assert np.array_equal(cp[:, :, :, :3][inside], c[:, :, :, :3][inside])
    assert np.array_equal(cp[:, :, :, 3][m <= mu_t], c[:, :, :, 3][m <= mu_t])
    # the two constraints are separate: each part is what it would be alone
    assert np.array_equal(tv4_64.proj(u, mu, 1e9, dims, T).reshape(cp.shape, order='F')[:, :, :, :3], cp[:, :, :, :3])
    assert np.array_equal(tv4_64.proj(u, 1e9, mu_t, dims, T).reshape(cp.shape, order='F')[:, :, :, 3], cp[:, :, :, 3])
    np.testing.assert_allclose(tv4_64.proj(p, mu, mu_t, dims, T), p, atol=1e-14)
    z = tv4_64.proj(u, 0.0, 0.0, dims, T)
    assert np.array_equal(z, np.zeros_like(u))


@pytest.mark.parametrize("dims,T", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_host_forms_match_the_float64_restatement(oracle_backend, dims, T):
    B = oracle_backend
    n = int(np.prod(dims))
    alpha, beta = 0.75 - 0.5j, -0.25 + 1.5j
    x = rand64c(n, T, seed=1) - (0.5 + 0.5j)
    u = rand64c(4 * n, T, seed=2) - (0.5 + 0.5j)
    for adjoint, src, ref in ((False, x, tv4_64.grad(x, dims, T)), (True, u, tv4_64.gradh(u, dims, T))):
        ref = ref.reshape((-1, T), order='F')
        y0 = rand64c(ref.shape[0], T, seed=3)
        y = B.copy_array(np.full(ref.shape, np.nan, dtype=C64, order='F'))
        B.grad4(y, B.copy_array(src), dims, T, adjoint=adjoint)
        np.testing.assert_allclose(y.to_host(), ref, atol=1e-6)
        y = B.copy_array(y0)
        B.grad4(y, B.copy_array(src), dims, T, adjoint=adjoint, alpha=alpha, beta=beta)
        np.testing.assert_allclose(y.to_host(), alpha * ref + beta * y0, atol=1e-6)
        # the frames stacked in one column
        y = B.copy_array(np.full((ref.size, 1), np.nan, dtype=C64, order='F'))
        B.grad4(y, B.copy_array(np.asfortranarray(src.reshape((-1, 1), order='F'))), dims, T, adjoint=adjoint)
        np.testing.assert_allclose(y.to_host(), ref.reshape((-1, 1), order='F'), atol=1e-6)
    xo = rand64c(n, T, seed=4) - (0.5 + 0.5j)
    sigma = 0.7
    for mu, mu_t in ((0.0, 0.0), (0.9, 0.5), (0.0, 0.5), (0.9, 0.0), (1e3, 1e3)):
        ref = tv4_64.dual_step(u, x, xo, sigma, mu, mu_t, dims, T)
        u_d = B.copy_array(u)
        B.tv4_dual_step(u_d, B.copy_array(x), B.copy_array(xo), sigma, mu, mu_t, dims, T)
        out = u_d.to_host()
        np.testing.assert_allclose(out, ref, atol=1e-6)
        c = out.reshape(dims + (4, T), order='F')
        assert mu > 0 or not c[:, :, :, :3].any()
        assert mu_t > 0 or not c[:, :, :, 3].any()
    if n > 1:
        unprojected = u + sigma * tv4_64.grad(2.0 * x - xo, dims, T)
        assert 0 < (tv4_64.radius(unprojected, dims, T) > 0.9).mean() < 1       # the balls above clip some entries and leave others
        assert 0 < (tv4_64.modulus_t(unprojected, dims, T) > 0.5).mean() < 1
    if T == 1:
        # one frame: grad3 / tv_dual_step with a zero fourth component
        y4, y3 = B.zero_array((4 * n, 1), C64), B.zero_array((3 * n, 1), C64)
        B.grad4(y4, B.copy_array(x), dims, 1)
        B.grad3(y3, B.copy_array(x), dims)
        assert np.array_equal(y4.to_host()[:3 * n], y3.to_host()) and not y4.to_host()[3 * n:].any()
        u0 = u.copy(order='F')
        u0[3 * n:] = 0
        h4, h3 = B.zero_array((n, 1), C64), B.zero_array((n, 1), C64)
        B.grad4(h4, B.copy_array(u), dims, 1, adjoint=True)               # u_3 of the last frame is not read
        B.grad3(h3, B.copy_array(np.asfortranarray(u[:3 * n])), dims, adjoint=True)
        assert np.array_equal(h4.to_host(), h3.to_host())
        u4, u3 = B.copy_array(u0), B.copy_array(np.asfortranarray(u[:3 * n]))
        B.tv4_dual_step(u4, B.copy_array(x), B.copy_array(xo), sigma, 0.9, 0.5, dims, 1)
        B.tv_dual_step(u3, B.copy_array(x), B.copy_array(xo), sigma, 0.9, dims)
        assert np.array_equal(u4.to_host()[:3 * n], u3.to_host()) and not u4.to_host()[3 * n:].any()


def test_gradient_t_operator(oracle_backend):
    B = oracle_backend
    dims, T = (17, 5, 3), 3
    G = B.GradientT(dims, T)
    n = 17 * 5 * 3 * T
    assert G.shape == (4 * n, n) and G.H.shape == (n, 4 * n)
    x = rand64c(n, 2, seed=4) - (0.5 + 0.5j)
    u = rand64c(4 * n, 2, seed=5) - (0.5 + 0.5j)
    for j in range(2):
        np.testing.assert_allclose((G * x)[:, j], tv4_64.grad(x[:, j], dims, T), atol=1e-6)
        np.testing.assert_allclose((G.H * u)[:, j], tv4_64.gradh(u[:, j], dims, T), atol=1e-6)
        np.testing.assert_allclose(((G.H * G) * x)[:, j], tv4_64.gradh(tv4_64.grad(x[:, j], dims, T), dims, T), atol=1e-5)
    for bad in [((17, 5), 3), ((17, 5, 0), 3), ((17, 5, 3, 1), 3), ((4, -1, 4), 3), ((17, 5, 3), 0)]:
        with pytest.raises(ValueError):
            B.GradientT(*bad)


def test_dense_rows_of_one_column_are_contiguous(oracle_backend):
    B = oracle_backend
    a = B.copy_array(rand64c(12, 1, seed=1))
    v = a.dense_rows(4, 9)
    assert v.shape == (5, 1) and v.contiguous and np.array_equal(v.to_host(), a.to_host()[4:9])
    v.copy_from(np.asfortranarray(np.full((5, 1), 2 - 1j, dtype=C64)))         # a view: writes reach the parent
    assert np.array_equal(a.to_host()[4:9], np.full((5, 1), 2 - 1j, dtype=C64))
    p = B.copy_array(rand64c(12, 3, seed=2))
    w = p.dense_rows(4, 9)
    assert w.shape == (5, 3) and np.array_equal(w.to_host(), p.to_host()[4:9])


def test_pics_parses_the_tv_time_option():
    a = pics.parse(["--tv", "0.01", "--tv-time", "0.03", "x.npz"])
    assert (a.tv, a.tv_time) == (0.01, 0.03)
    assert pics.parse(["x.npz"]).tv_time == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------------
N16, NRO, OSF = (16, 16, 16), 16, 1.5


def _maps():
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N16)]
    return np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph)
                     for cx, cy, ph in [(-1, 0, 0.3), (1, 0.5, -0.4)]], axis=3).astype(C64)


def _frame(shift):
    """the 16^3 image of test_tv_cpu's scan with its box moved by `shift`"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N16)]
    img = (np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + g[2] ** 2)) * (1 + 0.3j)).astype(C64)
    img[(np.abs(g[0] - shift) < 0.4) & (np.abs(g[1]) < 0.3)] += 0.5
    return img


def _operator(B, mps, coord):
    F1 = B.NUFFT((1,) + coord.shape[1:], N16, coord, width=3, oversamp=(OSF,) * 3, dtype=C64)
    return B.KronI(mps.shape[3], F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(mps.shape[3])])


def _save(path, ksps, mps, coords):
    """ksps: per frame (1, nro, nsp, C); coords: per frame (3, nro, nsp), or one such array for a traj without a TIME axis"""
    T = len(ksps)
    ksp = np.stack(ksps, axis=-1).reshape(ksps[0].shape + (1,) * 6 + (T,))
    scale = np.array(N16, dtype=np.float64)[:, None, None]
    if isinstance(coords, list):
        traj = np.stack([c * scale for c in coords], axis=-1).reshape(coords[0].shape + (1,) * 7 + (T,))
    else:
        traj = coords * scale
    np.savez(path, data=ksp.T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path


def _pics(B, argv):
    B._scratch = None
    out = pics.main(argv, backend=B)
    B._scratch = None
    return out


@pytest.fixture(scope="module")
def scan16x3(tmp_path_factory, oracle_backend):
    """three frames of a 16^3 two-coil scan (the box moves), a radial trajectory of 30 spokes per frame, each frame's own; the
    k-space data and the dense matrix of every frame's SENSE operator (built as test_tv_cpu's is)"""
    B = oracle_backend
    B._scratch = None
    mps = _maps()
    coords = [radial_trajectory(30, NRO, seed=2 + t) for t in range(3)]
    ksps, dense = [], []
    for t, coord in enumerate(coords):
        A = _operator(B, mps, coord)
        img = _frame(0.15 * t)
        ksps.append((A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, NRO, 30, 2), order='F'))
        m = A.shape[0]
        AdH = np.concatenate([A.H * np.asfortranarray(np.eye(m, dtype=C64)[:, j:j + 480]) for j in range(0, m, 480)], axis=1)
        dense.append(AdH.conj().T.astype(np.complex128))
    B._scratch = None
    path = _save(os.path.join(str(tmp_path_factory.mktemp("scan16x3")), "scan.npz"), ksps, mps, coords)
    return path, ksps, dense


TV_MU, TV_MU_T, L1 = 0.02, 0.02, 0.05     # on the float64 loop below both constraints are active on some entries and not on others


def test_pics_frames_match_a_float64_condat_vu(scan16x3, oracle_backend, caplog):
    path, ksps, dense = scan16x3
    N, T = N16, 3
    n = int(np.prod(N))
    lamda, mu, mu_t, l1, iters = 1e-3, TV_MU, TV_MU_T, L1, 10
    y = np.concatenate([k.reshape(-1, order='F').astype(np.complex128) for k in ksps])
    AHy = np.concatenate([Ad.conj().T @ k.reshape(-1, order='F') for Ad, k in zip(dense, ksps)])
    scale = np.abs(AHy).max()                              # one scale: the maximum over all frames
    b = AHy / scale

    def blocks(z, f):
        return np.concatenate([f(Ad, z[t * n:(t + 1) * n]) for t, Ad in enumerate(dense)])

    def AHA(z):
        return blocks(z, lambda Ad, zt: Ad.conj().T @ (Ad @ zt)) + lamda * z
    L = max(np.linalg.norm(Ad, 2) ** 2 for Ad in dense) + lamda     # the largest eigenvalue of the block-diagonal A^H A + lamda I
    tau, sigma = 0.9 / L, L / 32
    keep = dwt64.coarse_box(N, 'db2', 3)

    def prox(v, t):                                        # per frame
        return np.concatenate([dwt64.dwt(dwt64.soft(dwt64.dwt(v[f * n:(f + 1) * n], N, 'db2', 3), t * l1, N, keep), N, 'db2', 3, inverse=True)
                               for f in range(T)])
    seen, u = tv4_64.condat_vu(lambda z: AHA(z) - b, prox, tau, sigma, mu, mu_t, N, T, np.zeros_like(b), iters)
    x = seen[-1]
    on_ball = (tv4_64.radius(u, N, T) >= mu * (1 - 1e-9)).mean()
    on_disc = (tv4_64.modulus_t(u, N, T)[..., :-1] >= mu_t * (1 - 1e-9)).mean()
    print("share of dual vectors on the spatial ball %.3f, on the temporal disc %.3f after %d iterations" % (on_ball, on_disc, iters))
    assert 0.1 < on_ball < 0.9 and 0.1 < on_disc < 0.9, (on_ball, on_disc)
    argv = ["--osf", "1.5", "--lamda", str(lamda), "--tv", str(mu), "--tv-time", str(mu_t), "--l1", str(l1), "--step", "%.12e" % tau,
            "--debug", "40", path]
    with caplog.at_level(logging.INFO, logger="pics"):
        out = _pics(oracle_backend, ["-i", str(iters)] + argv)
    assert out.shape == N + (1,) * 7 + (T,)
    assert _rel(out.reshape(-1, order='F'), x) < 1e-4, _rel(out.reshape(-1, order='F'), x)
    msgs = [r.getMessage() for r in caplog.records]
    assert "frames 3, distinct trajectories 3" in msgs
    steps = [m for m in msgs if m.startswith("tv: tau")]
    assert len(steps) == 1
    got = dict(zip(("tau", "sigma", "mu"), (float(w.rstrip(",")) for w in steps[0].split()[2:7:2])))
    assert abs(got["tau"] - tau) < 1e-6 * tau and abs(got["sigma"] - sigma) < 1e-6 * sigma and got["mu"] == mu, (steps, tau, sigma)
    logged = [m for m in msgs if "objective" in m]
    assert logged and logged[-1].startswith("tv iter %d, objective" % iters)
    resid = blocks(x, lambda Ad, zt: Ad @ zt) - y / scale
    obj = (0.5 * np.linalg.norm(resid) ** 2 + 0.5 * lamda * np.linalg.norm(x) ** 2 + mu * tv4_64.tv(x, N, T)
           + mu_t * tv4_64.tv_time(x, N, T))
    inside = np.zeros(N, dtype=bool)
    inside[tuple(slice(0, c) for c in keep)] = True
    for f in range(T):
        obj += l1 * np.abs(dwt64.dwt(x[f * n:(f + 1) * n], N, 'db2', 3).reshape(N, order='F')[~inside]).sum()
    assert abs(float(logged[-1].split()[-1]) - obj) < 1e-4 * abs(obj), (logged[-1], obj)
    # the objective falls
    val = {}
    for it in (5, 30):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="pics"):
            _pics(oracle_backend, ["-i", str(it)] + argv)
        val[it] = [float(m.split()[-1]) for m in (r.getMessage() for r in caplog.records) if "objective" in m][-1]
    assert val[30] < val[5], val


def test_pics_frames_without_a_regulariser_solve_every_frame_by_cg(scan16x3, oracle_backend, tmp_path):
    """the block system solved jointly: with a fixed iteration count that is not CG on each frame alone (one step length for all
    frames), but it converges to the same solution"""
    path, ksps, dense = scan16x3
    n = int(np.prod(N16))
    lamda = 0.05 * max(np.linalg.norm(Ad, 2) ** 2 for Ad in dense)       # condition number <= 21: 60 iterations converge
    out = _pics(oracle_backend, ["-i", "60", "--osf", "1.5", "--lamda", "%.6e" % lamda, "--debug", "40", path])
    AHy = [Ad.conj().T @ k.reshape(-1, order='F') for Ad, k in zip(dense, ksps)]
    scale = max(np.abs(v).max() for v in AHy)
    for t, Ad in enumerate(dense):
        ref = np.linalg.solve(Ad.conj().T @ Ad + float("%.6e" % lamda) * np.eye(n), AHy[t] / scale)
        got = out.reshape((n, 3), order='F')[:, t]
        assert _rel(got, ref) < 1e-4, (t, _rel(got, ref))


def test_pics_shared_trajectory(scan16x3, oracle_backend, tmp_path, caplog):
    ksps = scan16x3[1]
    mps = _maps()
    coord = radial_trajectory(30, NRO, seed=2)
    shared = _save(str(tmp_path / "shared.npz"), ksps, mps, coord)
    tiled = _save(str(tmp_path / "tiled.npz"), ksps, mps, [coord] * 3)
    argv = ["-i", "4", "--osf", "1.5", "--lamda", "1e-3", "--tv", "0.02", "--tv-time", "0.02", "--power-iters", "8", "--debug", "40"]
    with caplog.at_level(logging.INFO, logger="pics"):
        a = _pics(oracle_backend, argv + [shared])
    assert "frames 3, distinct trajectories 1" in [r.getMessage() for r in caplog.records]
    b = _pics(oracle_backend, argv + [tiled])
    assert a.shape == b.shape == N16 + (1,) * 7 + (3,)
    assert _rel(a, b) <= 1e-6, _rel(a, b)
    assert np.linalg.norm(a) > 0


def test_pics_one_frame_ignores_tv_time(scan16x3, oracle_backend, tmp_path, caplog):
    ksps = scan16x3[1]
    one = _save(str(tmp_path / "one.npz"), ksps[:1], _maps(), [radial_trajectory(30, NRO, seed=2)])
    argv = ["-i", "4", "--osf", "1.5", "--lamda", "1e-3", "--debug", "40", one]
    a = _pics(oracle_backend, ["--tv", "0.02"] + argv)
    with caplog.at_level(logging.INFO, logger="pics"):
        b = _pics(oracle_backend, ["--tv", "0.02", "--tv-time", "0.05"] + argv)
    assert any(re.search(r"--tv-time .* no effect", r.getMessage()) for r in caplog.records)
    assert a.shape == b.shape == N16 + (1,) * 7 + (1,)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # and --tv-time alone on one frame is the CG driver
    c = _pics(oracle_backend, argv)
    d = _pics(oracle_backend, ["--tv-time", "0.05"] + argv)
    assert np.array_equal(c.view(np.uint64), d.view(np.uint64))


def test_scratch_arena_of_three_frames_is_that_of_one(scan16x3, oracle_backend, tmp_path):
    """the frames' operators run one after the other on the same arena: it is reserved for the most demanding frame once, not
    for the T times larger block"""
    B = oracle_backend
    path, ksps = scan16x3[:2]
    one = _save(str(tmp_path / "one.npz"), ksps[:1], _maps(), [radial_trajectory(30, NRO, seed=2)])
    size = {}
    for name, scan in (("one", one), ("three", path)):
        B._scratch = None
        pics.main(["-i", "1", "--osf", "1.5", "--debug", "40", scan], backend=B)
        size[name] = B._scratch.size
        B._scratch = None
    assert size["three"] == size["one"] > 0, size


def test_tv_time_couples_the_frames(oracle_backend, tmp_path, caplog):
    """two frames of one image, each sampled with its own 12 spokes: alone, each frame shows its own undersampling artefacts;
    the temporal term pulls the two reconstructions together"""
    B = oracle_backend
    B._scratch = None
    mps = _maps()
    coords = [radial_trajectory(12, NRO, seed=11 + t) for t in range(2)]
    img = np.asfortranarray(_frame(0.0).reshape(-1, 1, order='F'))
    ksps = [(_operator(B, mps, c) * img).reshape((1, NRO, 12, 2), order='F') for c in coords]
    path = _save(str(tmp_path / "two.npz"), ksps, mps, coords)
    argv = ["--osf", "1.5", "--lamda", "1e-3", "--debug", "40", path]
    with caplog.at_level(logging.INFO, logger="pics"):
        _pics(B, ["-i", "0", "--tv", "0.005"] + argv)
    L = [float(m.group(1)) for r in caplog.records for m in [re.search(r"largest eigenvalue of A\^H A \+ lamda I (\S+)", r.getMessage())] if m][0]
    argv = ["-i", "15", "--step", "%.8e" % (0.9 / L)] + argv
    diff = {}
    for mu_t in ("0", "0.05"):
        out = _pics(B, ["--tv", "0.005", "--tv-time", mu_t] + argv).reshape((-1, 2), order='F')
        diff[mu_t] = np.linalg.norm(out[:, 1] - out[:, 0])
    assert diff["0"] > 0 and diff["0.05"] < diff["0"], diff
