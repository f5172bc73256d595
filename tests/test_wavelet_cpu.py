"""pics --l1 on the CPU: the float64 wavelet restatement (tests/dwt64.py) against its definition, the coarse-box rule, the host
forms of Backend.dwt3 / soft_threshold, operators.Wavelet, Backend.fista against a plain numpy FISTA, and the driver against a
float64 FISTA on the dense matrix of the same operator -- all on the numpy oracle backend."""
import logging
import os

import numpy as np
import pytest

import dwt64
from conftest import check_misc_leaves
from indigo_amd import pics
from indigo_amd.backends.backend import WAVELETS, dwt_coarse_box
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
SHAPES = [(16, 8, 1), (12, 10, 3), (16, 6, 5), (9, 16, 4)]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


@pytest.mark.parametrize("wavelet", ["haar", "db2", "db4"])
def test_filters_from_the_spectral_factorisation(wavelet):
    h = dwt64.daubechies(dwt64.TAPS[wavelet])
    assert np.abs(h - np.array(WAVELETS[wavelet])).max() < 1e-12
    # orthogonality of the filter to its even shifts and vanishing moments of the high-pass filter
    g = dwt64.highpass(h)
    for s in range(0, h.size, 2):
        assert abs(np.dot(h[s:], h[:h.size - s]) - (s == 0)) < 1e-12
    for p in range(h.size // 2):
        assert abs(np.dot(g, np.arange(h.size) ** p)) < 1e-9


@pytest.mark.parametrize("wavelet", ["haar", "db2", "db4"])
@pytest.mark.parametrize("dims", SHAPES)
def test_float64_transform_is_orthogonal(wavelet, dims):
    W = dwt64.dense(dims, wavelet, 3)
    assert np.abs(W @ W.T - np.eye(W.shape[0])).max() < 1e-12
    x = np.random.default_rng(1).standard_normal(W.shape[0])
    np.testing.assert_allclose(dwt64.dwt(x, dims, wavelet, 3, inverse=True), W.T @ x, atol=1e-12)


def test_coarse_box_rule():
    assert dwt_coarse_box((480, 208, 308), 'db4', 3) == (60, 26, 77)
    assert dwt_coarse_box((480, 208, 308), 'db4', 5) == (15, 13, 77)
    assert dwt_coarse_box((64, 48, 1), 'db2', 3) == (8, 6, 1)              # 2-D: the third axis never splits
    assert dwt_coarse_box((8, 8, 8), 'haar', 9) == (2, 2, 2)                # stops after two levels, no error
    for dims in SHAPES + [(480, 208, 308), (8, 8, 8)]:
        for w in WAVELETS:
            for levels in (1, 3, 5, 9):
                assert dwt_coarse_box(dims, w, levels) == dwt64.coarse_box(dims, w, levels)


@pytest.mark.parametrize("wavelet", ["haar", "db2", "db4"])
def test_host_forms_match_the_float64_transform(oracle_backend, wavelet):
    B = oracle_backend
    for dims in SHAPES + [(32, 24, 40)]:
        for levels in (1, 3, 5):
            n = int(np.prod(dims))
            x = rand64c(n, 2, seed=levels) - (0.5 + 0.5j)
            y0 = rand64c(n, 2, seed=9)
            for inverse in (False, True):
                ref = dwt64.dwt(x, dims, wavelet, levels, inverse=inverse)
                y = B.copy_array(np.full((n, 2), np.nan, dtype=C64, order='F'))
                B.dwt3(y, B.copy_array(x), dims, wavelet, levels, inverse=inverse)
                assert _rel(y.to_host(), ref) < 1e-6
                y = B.copy_array(y0)
                B.dwt3(y, B.copy_array(x), dims, wavelet, levels, inverse=inverse, alpha=0.5j, beta=2 - 1j)
                assert _rel(y.to_host(), 0.5j * ref + (2 - 1j) * y0) < 1e-6


def test_host_soft_threshold(oracle_backend):
    dims, tau = (16, 20, 7), np.float32(0.25)
    keep = dwt64.coarse_box(dims, 'db2', 2)                # (4, 5, 7): the rows below lie outside it
    n = int(np.prod(dims))
    u = (rand64c(n, 2, seed=3) - (0.5 + 0.5j)).astype(C64)
    u[-80:-50, 0] = 0
    u[-40:-20, 0] = tau
    u[-20:, 1] = 1j * tau
    u_d = oracle_backend.copy_array(u)
    oracle_backend.soft_threshold(u_d, tau, dims, keep)
    out = u_d.to_host().reshape(dims + (2,), order='F')
    ref = dwt64.soft(u, tau, dims, keep).reshape(dims + (2,), order='F')
    vol = u.reshape(dims + (2,), order='F')
    box = tuple(slice(0, c) for c in keep)
    assert np.array_equal(out[box], vol[box])
    zero = np.abs(ref) == 0
    assert zero.sum() > 100 and np.all(out[zero] == 0)
    assert out.reshape((n, 2), order='F')[-40:-20, 0].tolist() == [0] * 20
    assert np.abs(out - ref).max() < 1e-6


def test_wavelet_operator(oracle_backend):
    B = oracle_backend
    dims = (16, 20, 7)
    W = B.Wavelet(dims, wavelet='db4', levels=3)
    assert W.shape == (16 * 20 * 7,) * 2 and W.coarse == dwt64.coarse_box(dims, 'db4', 3)
    x = rand64c(W.shape[1], 2, seed=4)
    np.testing.assert_allclose(W.H * (W * x), x, atol=1e-6)
    np.testing.assert_allclose(W * x, dwt64.dwt(x, dims, 'db4', 3), atol=1e-6)
    with pytest.raises(ValueError):
        B.Wavelet((1025, 4, 4))
    with pytest.raises(ValueError):
        B.Wavelet((16, 16, 16), wavelet='db8')


def test_fista_reproduces_a_numpy_loop(oracle_backend):
    B = oracle_backend
    rng = np.random.default_rng(2)
    M = (rng.standard_normal((40, 24)) + 1j * rng.standard_normal((40, 24))).astype(C64)
    b = (rng.standard_normal((40, 1)) + 1j * rng.standard_normal((40, 1))).astype(C64)
    A = B.DenseMatrix(M)
    AH_b = B.copy_array(np.asfortranarray(M.conj().T @ b))
    tmp = B.zero_array((40, 1), C64)

    def gradf(g, z):                                  # grad of 1/2 ||M z - b||^2
        A.eval(tmp, z)
        A.H.eval(g, tmp)
        B.axpby(1, g, -1, AH_b)

    def proxg(v, alpha):                              # prox of 0.3 ||v||_1 (complex soft threshold, no box kept)
        B.soft_threshold(v, alpha * 0.3, (24, 1, 1), (0, 0, 0))

    step = 0.9 / np.linalg.norm(M.astype(np.complex128), 2) ** 2
    seen = []
    x0 = rand64c(24, 1, seed=1)
    x = x0.copy(order='F')
    B.fista(gradf, proxg, step, x, maxiter=12, callback=lambda k, xk: seen.append(xk.to_host().copy()))
    # the same iteration in numpy, complex128
    Md = M.astype(np.complex128)

    def soft(v, t):
        r = np.abs(v)
        return np.where(r <= t, 0, v * (1 - t / np.maximum(r, 1e-300)))
    xk = zk = x0.astype(np.complex128)
    t = 1.0
    for k in range(12):
        xn = soft(zk - step * (Md.conj().T @ (Md @ zk - b)), step * 0.3)
        tn = (1 + np.sqrt(1 + 4 * t * t)) / 2
        zk = xn + (t - 1) / tn * (xn - xk)
        xk, t = xn, tn
        assert _rel(seen[k], xk) < 1e-5, k
    assert _rel(x, xk) < 1e-5
    # and the proximal-gradient iteration with the reference's constant momentum is still what the golden vectors hold
    check_misc_leaves(B, 1e-5)


def test_pics_parses_the_l1_options():
    a = pics.parse(["--l1", "0.01", "--wavelet", "db4", "--levels", "4", "--power-iters", "7", "--step", "0.5", "x.npz"])
    assert (a.l1, a.wavelet, a.levels, a.power_iters, a.step, a.data) == (0.01, "db4", 4, 7, 0.5, "x.npz")
    a = pics.parse(["x.npz"])
    assert (a.l1, a.wavelet, a.levels, a.power_iters, a.step) == (0, "db2", 3, 15, None)
    with pytest.raises(SystemExit):
        pics.parse(["--wavelet", "sym4", "x.npz"])


@pytest.fixture(scope="module")
def scan16(tmp_path_factory, oracle_backend):
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
    path = os.path.join(str(tmp_path_factory.mktemp("scan16")), "scan.npz")
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path, N, ksp, Ad.astype(np.complex128)


def test_pics_l1_zero_is_the_cg_driver(scan16, oracle_backend):
    path, N, _, _ = scan16
    args = ["-i", "4", "--osf", "1.5", "--lamda", "1e-3", "--debug", "40", path]
    oracle_backend._scratch = None
    a = pics.main(args, backend=oracle_backend)
    oracle_backend._scratch = None
    b = pics.main(["--l1", "0"] + args, backend=oracle_backend)
    oracle_backend._scratch = None
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_pics_l1_matches_a_float64_fista(scan16, oracle_backend, caplog):
    path, N, ksp, Ad = scan16
    lamda, l1, iters = 1e-3, 0.2, 10
    y = ksp.reshape(-1, order='F').astype(np.complex128)
    AHy = Ad.conj().T @ y
    b = AHy / np.abs(AHy).max()
    AHA = Ad.conj().T @ Ad + lamda * np.eye(Ad.shape[1])
    lam = np.linalg.eigvalsh(AHA)[-1]
    step = 0.9 / lam
    keep = dwt64.coarse_box(N, 'db2', 3)
    x = z = np.zeros_like(b)
    t = 1.0
    for _ in range(iters):
        v = z - step * (AHA @ z - b)
        xn = dwt64.dwt(dwt64.soft(dwt64.dwt(v, N, 'db2', 3), step * l1, N, keep), N, 'db2', 3, inverse=True)
        tn = (1 + np.sqrt(1 + 4 * t * t)) / 2
        z = xn + (t - 1) / tn * (xn - x)
        x, t = xn, tn
    W = dwt64.dwt(x, N, 'db2', 3).reshape(N, order='F')
    inside = np.zeros(N, dtype=bool)
    inside[tuple(slice(0, c) for c in keep)] = True
    assert (abs(W[~inside]) < 1e-12).mean() > 0.3        # the threshold is doing something
    oracle_backend._scratch = None
    with caplog.at_level(logging.INFO, logger="pics"):
        out = pics.main(["-i", str(iters), "--osf", "1.5", "--lamda", str(lamda), "--l1", str(l1), "--step", "%.12e" % step,
                         "--debug", "40", path], backend=oracle_backend)
    oracle_backend._scratch = None
    assert out.shape == N + (1, 1)
    assert _rel(out.reshape(-1, order='F'), x) < 1e-4, _rel(out.reshape(-1, order='F'), x)
    # the logged objective is the float64 one of the same iterate
    logged = [r.getMessage() for r in caplog.records if "objective" in r.getMessage()]
    assert logged and logged[-1].startswith("fista iter %d" % iters)
    obj = 0.5 * np.linalg.norm(Ad @ x - y / np.abs(AHy).max()) ** 2 + 0.5 * lamda * np.linalg.norm(x) ** 2 + l1 * np.abs(W[~inside]).sum()
    assert abs(float(logged[-1].split()[-1]) - obj) < 1e-4 * abs(obj)
    # the power iteration finds the largest eigenvalue of A^H A + lamda I
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="pics"):
        pics.main(["-i", "0", "--osf", "1.5", "--lamda", str(lamda), "--l1", str(l1), "--power-iters", "40", "--debug", "40",
                   path], backend=oracle_backend)
    oracle_backend._scratch = None
    est = [r.getMessage() for r in caplog.records if "largest eigenvalue" in r.getMessage()]
    assert est and abs(float(est[0].split("lamda I ")[1].split()[0]) - lam) < 1e-2 * lam
