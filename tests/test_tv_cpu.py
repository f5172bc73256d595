"""pics --tv on the CPU: the float64 restatement (tests/tv64.py) against its definition, the host forms of Backend.grad3 /
tv_dual_step, operators.Gradient, Backend.primal_dual against a plain complex128 Condat-Vu loop, and the driver against the
same loop on the dense matrix of the same operator -- all on the numpy oracle backend."""
import logging
import os

import numpy as np
import pytest

import dwt64
import tv64
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
SHAPES = [(17, 5, 3), (8, 1, 6), (1, 1, 9), (2, 2, 2)]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _c128(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("dims", SHAPES + [(6, 4, 1)])
def test_float64_gradient_and_its_adjoint(dims):
    rng = np.random.default_rng(1)
    n = int(np.prod(dims))
    x, u = _c128(rng, n, 2), _c128(rng, 3 * n, 2)
    lhs, rhs = np.vdot(u, tv64.grad(x, dims)), np.vdot(tv64.gradh(u, dims), x)
    assert abs(lhs - rhs) < 1e-12 * np.linalg.norm(x) * np.linalg.norm(u)
    assert np.array_equal(tv64.grad(np.full(n, 2 - 3j), dims), np.zeros(3 * n))
    # the definition, voxel by voxel
    v = x[:, 0].reshape(dims, order='F')
    d = tv64.grad(x[:, 0], dims).reshape(dims + (3,), order='F')
    for i in np.ndindex(*dims):
        for a in range(3):
            j = tuple(i[b] + (b == a) for b in range(3))
            assert d[i + (a,)] == (v[j] - v[i] if i[a] < dims[a] - 1 else 0)


def test_float64_gradient_norm():
    for dims in [(9, 8, 7), (17, 5, 3), (8, 1, 6), (1, 1, 9)]:
        assert tv64.norm2_estimate(dims) <= 12
    lam = tv64.norm2_estimate((12, 12, 1))
    assert 6 < lam <= 8, lam                               # 4 per axis longer than 1 (and the estimate is not trivially small)
    assert tv64.norm2_estimate((1, 1, 9)) <= 4


def test_float64_projection():
    dims, mu = (5, 4, 3), 2.4
    u = _c128(np.random.default_rng(2), 3 * 60, 2)
    p = tv64.proj(u, mu, dims)
    r, rp = tv64.radius(u, dims), tv64.radius(p, dims)
    assert 0.1 < (r > mu).mean() < 0.9
    np.testing.assert_allclose(rp, np.minimum(r, mu), atol=1e-14)
    inside = np.broadcast_to((r <= mu)[:, :, :, None, :], dims + (3, 2))
    assert np.array_equal(p.reshape(dims + (3, 2), order='F')[inside], u.reshape(dims + (3, 2), order='F')[inside])
    np.testing.assert_allclose(tv64.proj(p, mu, dims), p, atol=1e-14)
    assert np.array_equal(tv64.proj(u, 0.0, dims), np.zeros_like(u))


@pytest.mark.parametrize("dims", SHAPES)
def test_host_forms_match_the_float64_restatement(oracle_backend, dims):
    B = oracle_backend
    n = int(np.prod(dims))
    alpha, beta = 0.75 - 0.5j, -0.25 + 1.5j
    x = rand64c(n, 2, seed=1) - (0.5 + 0.5j)
    u = rand64c(3 * n, 2, seed=2) - (0.5 + 0.5j)
    for adjoint, src, ref in ((False, x, tv64.grad(x, dims)), (True, u, tv64.gradh(u, dims))):
        y0 = rand64c(ref.shape[0], 2, seed=3)
        y = B.copy_array(np.full(ref.shape, np.nan, dtype=C64, order='F'))
        B.grad3(y, B.copy_array(src), dims, adjoint=adjoint)
        np.testing.assert_allclose(y.to_host(), ref, atol=1e-6)
        y = B.copy_array(y0)
        B.grad3(y, B.copy_array(src), dims, adjoint=adjoint, alpha=alpha, beta=beta)
        np.testing.assert_allclose(y.to_host(), alpha * ref + beta * y0, atol=1e-6)
    xo = rand64c(n, 2, seed=4) - (0.5 + 0.5j)
    sigma = 0.7
    for mu in (0.0, 0.9, 1e3):
        ref = tv64.dual_step(u, x, xo, sigma, mu, dims)
        u_d = B.copy_array(u)
        B.tv_dual_step(u_d, B.copy_array(x), B.copy_array(xo), sigma, mu, dims)
        np.testing.assert_allclose(u_d.to_host(), ref, atol=1e-6)
    if n > 1:
        clipped = tv64.radius(u + sigma * tv64.grad(2.0 * x - xo, dims), dims) > 0.9
        assert 0 < clipped.mean() < 1                      # mu = 0.9 above projects some voxels and leaves others


def test_gradient_operator(oracle_backend):
    B = oracle_backend
    dims = (17, 5, 3)
    G = B.Gradient(dims)
    n = 17 * 5 * 3
    assert G.shape == (3 * n, n) and G.H.shape == (n, 3 * n)
    x = rand64c(n, 2, seed=4) - (0.5 + 0.5j)
    u = rand64c(3 * n, 2, seed=5) - (0.5 + 0.5j)
    np.testing.assert_allclose(G * x, tv64.grad(x, dims), atol=1e-6)
    np.testing.assert_allclose(G.H * u, tv64.gradh(u, dims), atol=1e-6)
    np.testing.assert_allclose((G.H * G) * x, tv64.gradh(tv64.grad(x, dims), dims), atol=1e-5)
    for bad in [(17, 5), (17, 5, 0), (17, 5, 3, 1), (4, -1, 4)]:
        with pytest.raises(ValueError):
            B.Gradient(bad)


@pytest.mark.parametrize("with_prox", [False, True])
def test_primal_dual_reproduces_a_numpy_loop(oracle_backend, with_prox):
    B = oracle_backend
    dims, mu = (6, 4, 1), 6.0          # (on the float64 loop below: the projection acts on some voxels and not on others)
    rng = np.random.default_rng(2)
    M = _c128(rng, 40, 24).astype(C64)
    b = _c128(rng, 40, 1).astype(C64)
    A = B.DenseMatrix(M)
    AH_b = B.copy_array(np.asfortranarray(M.conj().T @ b))
    tmp = B.zero_array((40, 1), C64)
    G = B.Gradient(dims)

    def gradf(g, z):                                  # grad of 1/2 ||M z - b||^2
        A.eval(tmp, z)
        A.H.eval(g, tmp)
        B.axpby(1, g, -1, AH_b)

    def proxg(v, tau):                                # prox of 0.3 ||v||_1 (complex soft threshold, no box kept)
        B.soft_threshold(v, tau * 0.3, (24, 1, 1), (0, 0, 0))

    L = np.linalg.norm(M.astype(np.complex128), 2) ** 2
    tau, sigma = 0.9 / L, L / 24
    seen = []
    x0 = rand64c(24, 1, seed=1)
    x = x0.copy(order='F')
    u = B.zero_array((72, 1), C64)
    B.primal_dual(gradf, proxg if with_prox else None, lambda g, v: G.eval(g, v, alpha=1, beta=1, forward=False),
                  lambda v, xn, xo: B.tv_dual_step(v, xn, xo, sigma, mu, dims), tau, x, u, maxiter=12,
                  callback=lambda k, xk: seen.append(xk.to_host().copy()))
    # the same iteration in numpy, complex128
    Md = M.astype(np.complex128)

    def soft(v, t):
        r = np.abs(v)
        return np.where(r <= t * 0.3, 0, v * (1 - t * 0.3 / np.maximum(r, 1e-300)))
    ref, u_ref = tv64.condat_vu(lambda z: Md.conj().T @ (Md @ z - b), soft if with_prox else None, tau, sigma, mu, dims,
                                x0.astype(np.complex128), 12)
    on_ball = tv64.radius(u_ref, dims) >= mu * (1 - 1e-9)
    assert 0.1 < on_ball.mean() < 0.9, on_ball.mean()      # the projection acts on some voxels and not on others
    assert len(seen) == 12
    for k in range(12):
        assert _rel(seen[k], ref[k]) < 1e-5, k
    assert _rel(x, ref[-1]) < 1e-5
    assert _rel(u.to_host(), u_ref) < 1e-5


def test_pics_parses_the_tv_options():
    a = pics.parse(["--tv", "0.01", "--tv-sigma", "2.5", "--l1", "0.02", "--step", "0.5", "x.npz"])
    assert (a.tv, a.tv_sigma, a.l1, a.step, a.data) == (0.01, 2.5, 0.02, 0.5, "x.npz")
    a = pics.parse(["x.npz"])
    assert (a.tv, a.tv_sigma, a.l1) == (0, None, 0)
    with pytest.raises(SystemExit):
        pics.parse(["--tv", "much", "x.npz"])


@pytest.fixture(scope="module")
def scan16(tmp_path_factory, oracle_backend):
    """a 16^3 two-coil radial scan, its k-space data and the dense matrix of its SENSE operator (built as test_wavelet_cpu's is)"""
    N, C, nro, nsp, osf = (16, 16, 16), 2, 16, 30, 1.5
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    img = (np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + g[2] ** 2)) * (1 + 0.3j)).astype(C64)
    img[(np.abs(g[0]) < 0.4) & (np.abs(g[1]) < 0.3)] += 0.5
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph)
                    for cx, cy, ph in [(-1, 0, 0.3), (1, 0.5, -0.4)]], axis=3).astype(C64)
    coord = radial_trajectory(nsp, nro, seed=2)
    traj = coord * np.array(N, dtype=np.float64)[:, None, None]
    B = oracle_backend
    B._scratch = None
    F1 = B.NUFFT((1, nro, nsp), N, coord, width=3, oversamp=(osf,) * 3, dtype=C64)
    A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
    ksp = (A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F')
    # the operator's dense matrix, through its adjoint (fewer rows than columns), a block of rows at a time
    m = A.shape[0]
    AdH = np.concatenate([A.H * np.asfortranarray(np.eye(m, dtype=C64)[:, j:j + 480]) for j in range(0, m, 480)], axis=1)
    Ad = AdH.conj().T
    B._scratch = None
    path = os.path.join(str(tmp_path_factory.mktemp("scan16tv")), "scan.npz")
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path, N, ksp, Ad.astype(np.complex128)


def _pics(B, argv):
    B._scratch = None
    out = pics.main(argv, backend=B)
    B._scratch = None
    return out


def test_pics_tv_zero_is_the_cg_and_the_fista_driver(scan16, oracle_backend):
    path = scan16[0]
    args = ["-i", "4", "--osf", "1.5", "--lamda", "1e-3", "--debug", "40", path]
    for extra in ([], ["--l1", "0.2"]):
        a = _pics(oracle_backend, extra + args)
        b = _pics(oracle_backend, extra + ["--tv", "0"] + args)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), extra
    tv = _pics(oracle_backend, ["--tv", "0.02"] + args)
    assert not np.array_equal(a.view(np.uint64), tv.view(np.uint64))


TV_MU = 0.02        # chosen on the float64 reference below: after 10 iterations about three quarters of the dual vectors sit on the ball


@pytest.mark.parametrize("l1", [0.0, 0.05])
def test_pics_tv_matches_a_float64_condat_vu(scan16, oracle_backend, caplog, l1):
    path, N, ksp, Ad = scan16
    lamda, mu, iters = 1e-3, TV_MU, 10
    y = ksp.reshape(-1, order='F').astype(np.complex128)
    AHy = Ad.conj().T @ y
    b = AHy / np.abs(AHy).max()
    AHA = Ad.conj().T @ Ad + lamda * np.eye(Ad.shape[1])
    L = np.linalg.eigvalsh(AHA)[-1]
    tau, sigma = 0.9 / L, L / 24
    keep = dwt64.coarse_box(N, 'db2', 3)

    def prox(v, t):
        return dwt64.dwt(dwt64.soft(dwt64.dwt(v, N, 'db2', 3), t * l1, N, keep), N, 'db2', 3, inverse=True)
    seen, u = tv64.condat_vu(lambda z: AHA @ z - b, prox if l1 else None, tau, sigma, mu, N, np.zeros_like(b), iters)
    x = seen[-1]
    on_ball = (tv64.radius(u, N) >= mu * (1 - 1e-9)).mean()
    print("share of dual vectors on the ball after %d iterations: %.3f" % (iters, on_ball))
    assert 0.1 < on_ball < 0.9, on_ball                    # the projection acts, and not everywhere
    argv = ["-i", str(iters), "--osf", "1.5", "--lamda", str(lamda), "--tv", str(mu), "--step", "%.12e" % tau, "--debug", "40", path]
    if l1:
        argv = ["--l1", str(l1)] + argv
    with caplog.at_level(logging.INFO, logger="pics"):
        out = _pics(oracle_backend, argv)
    assert out.shape == N + (1, 1)
    assert _rel(out.reshape(-1, order='F'), x) < 1e-4, _rel(out.reshape(-1, order='F'), x)
    # the steps that were logged are those of the rule, and the logged objective is the float64 one of the same iterate
    steps = [r.getMessage() for r in caplog.records if r.getMessage().startswith("tv: tau")]
    assert len(steps) == 1
    got = dict(zip(("tau", "sigma", "mu"), (float(w.rstrip(",")) for w in steps[0].split()[2:7:2])))
    assert abs(got["tau"] - tau) < 1e-6 * tau and abs(got["sigma"] - sigma) < 1e-6 * sigma and got["mu"] == mu, (steps, tau, sigma)
    logged = [r.getMessage() for r in caplog.records if "objective" in r.getMessage()]
    assert logged and logged[-1].startswith("tv iter %d, objective" % iters)
    obj = 0.5 * np.linalg.norm(Ad @ x - y / np.abs(AHy).max()) ** 2 + 0.5 * lamda * np.linalg.norm(x) ** 2 + mu * tv64.tv(x, N)
    if l1:
        W = dwt64.dwt(x, N, 'db2', 3).reshape(N, order='F')
        inside = np.zeros(N, dtype=bool)
        inside[tuple(slice(0, c) for c in keep)] = True
        obj += l1 * np.abs(W[~inside]).sum()
    assert abs(float(logged[-1].split()[-1]) - obj) < 1e-4 * abs(obj), (logged[-1], obj)
