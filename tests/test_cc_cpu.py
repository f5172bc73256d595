"""Coil compression and noise prewhitening on the CPU with the numpy oracle backend: the host form of Backend.coil_gram against the
float64 restatement in tests/cc64.py, cc.matrix, the cc driver on a rank-deficient scan, the invariance of the reconstruction under
compression (pics --cc), the refusals, and ecalib on a compressed scan."""
import os

import numpy as np
import pytest

import cc64
import espirit64 as e64
from indigo_amd import cc, ecalib, pics
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')


def _rel(a, b):
    return np.linalg.norm((np.asarray(a) - np.asarray(b)).ravel()) / np.linalg.norm(np.asarray(b).ravel())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the host form of coil_gram ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1, 105, 5049))
@pytest.mark.parametrize("C", (1, 3, 12, 33, 64))
def test_host_coil_gram_matches_the_float64_restatement(oracle_backend, n, C):
    B = oracle_backend
    y = rand64c(n, C, seed=100 * C + n)
    panel = np.full((n + 5, C), np.nan, dtype=C64, order='F')            # 5 NaN rows under every column
    panel[:n] = y
    d = B.copy_array(panel)
    G = B.coil_gram(d[:n], n, C)
    assert G.shape == (C, C) and G.dtype == np.complex128 and np.isfinite(G).all()
    assert np.array_equal(G, G.conj().T) and np.array_equal(G.imag.diagonal(), np.zeros(C))
    err = _rel(G, cc64.gram(y))
    print("coil_gram host form n %d C %d: relative error %.3e (bound %.3e)" % (n, C, err, n * 2.0 ** -52))
    assert err <= n * 2.0 ** -52
    assert np.array_equal(_bits(d.to_host()), _bits(panel))
    # the stacked-vector form
    v = B.copy_array(np.asfortranarray(y.reshape((-1, 1), order='F')))
    assert np.array_equal(B.coil_gram(v, n, C), G)


def test_host_coil_mix_is_frame_basis(oracle_backend):
    B = oracle_backend
    n, C, V = 105, 12, 5
    y, A = rand64c(n, C, seed=1), rand64c(V, C, seed=2).astype(np.complex128)
    out = B.copy_array(np.full((n, V), np.nan, dtype=C64, order='F'))
    B.coil_mix(out, B.copy_array(y), A, n)
    assert _rel(out.to_host(), cc64.mix(A, y, coil_axis=1)) < 1e-6


def test_gram_of_pools_frames_and_apply_keeps_the_other_axes(oracle_backend):
    """a scan with three time frames and maps with two sets: every frame and set is one coil panel, chunks smaller than a panel"""
    B = oracle_backend
    ksp = rand64c(6 * 5 * 7 * 3, 1, seed=20).reshape((1, 6, 5, 7) + (1,) * 6 + (3,), order='F')
    mps = rand64c(4 * 3 * 2 * 7 * 2, 1, seed=21).reshape((4, 3, 2, 7, 2), order='F')
    samples = ksp.reshape((30, 7, 3), order='F').transpose(0, 2, 1).reshape((90, 7))
    G = cc.gram_of(B, ksp, chunk=11)
    assert _rel(G, cc64.gram(samples)) <= 90 * 2.0 ** -52
    assert _rel(cc.gram_of(B, ksp, mps), cc64.gram(samples) + cc64.gram(mps.transpose(0, 1, 2, 4, 3).reshape((-1, 7)))) <= 1e-13
    A, lam = cc.matrix(G, V=3)
    out = cc.apply(B, A, ksp, chunk=11)
    assert out.shape == (1, 6, 5, 3) + (1,) * 6 + (3,) and out.dtype == C64 and _rel(out, cc64.mix(A, ksp)) <= 1e-6
    out = cc.apply(B, A, mps, chunk=11)
    assert out.shape == (4, 3, 2, 3, 2) and _rel(out, cc64.mix(A, mps)) <= 1e-6
    k2, m2, A2, lam2 = cc.compress(B, ksp, mps, V=3, chunk=11)
    assert np.array_equal(A2, A) and np.array_equal(lam2, lam) and k2.shape[3] == m2.shape[3] == 3


# ---- 2. cc.matrix --------------------------------------------------------------------------------------------------------------------

def _spd(C, seed, cond=20.0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C)))
    return (q * np.linspace(1.0, cond, C)) @ q.conj().T


def test_matrix_orthonormality_whitening_phase_and_energy():
    C, V = 12, 5
    G = cc64.gram(rand64c(300, C, seed=3))
    A, lam = cc.matrix(G, V=V)
    assert A.shape == (V, C) and lam.shape == (C,) and np.all(np.diff(lam) <= 0)
    assert np.linalg.norm(A @ A.conj().T - np.eye(V)) <= 1e-12
    A64, lam64 = cc64.matrix(G, V)
    assert np.allclose(lam, lam64, rtol=1e-12, atol=0) and np.linalg.norm(A - A64) <= 1e-10
    # the phase convention: the largest-magnitude component of every eigenvector (row of A, conjugated) is real and positive
    for v in range(V):
        u = np.conj(A[v])
        k = int(np.argmax(np.abs(u)))
        assert abs(u[k].imag) <= 1e-15 and u[k].real > 0
    # with a well-conditioned noise covariance A whitens: A Psi A^H = I
    Psi = _spd(C, seed=4)
    Aw, lamw = cc.matrix(G, V=V, noise_cov=Psi)
    assert np.linalg.norm(Aw @ Psi @ Aw.conj().T - np.eye(V)) <= 1e-10
    A64w, lam64w = cc64.matrix(G, V, noise_cov=Psi)
    assert np.allclose(lamw, lam64w, rtol=1e-10, atol=0) and np.linalg.norm(Aw - A64w) <= 1e-8 * np.linalg.norm(A64w)
    # -e on a rank-deficient G returns its rank
    for rank in (1, 3, 7):
        Y = rand64c(200, rank, seed=5 + rank).astype(np.complex128) @ rand64c(rank, C, seed=9).astype(np.complex128)
        Gr = cc64.gram(Y)
        Ar, lamr = cc.matrix(Gr, energy=1 - 1e-9)
        assert Ar.shape == (rank, C) and cc64.energy_rank(lamr, 1 - 1e-9) == rank
    assert cc.matrix(G, energy=1.0)[0].shape[0] == C


# ---- 3. the driver on a rank-deficient scan ----------------------------------------------------------------------------------------

N16, NRO, NSP, OSF, WIDTH = (16, 16, 16), 32, 60, 2.0, 2
COMMON = ["--osf", str(OSF), "--width", str(WIDTH)]


@pytest.fixture(scope="module")
def scan12(tmp_path_factory, oracle_backend):
    """16^3, 4 true coils seen through 12 channels; -> (path, the restatement's G, A and eigenvalues at V = 4)"""
    path = cc64.rank_deficient_scan(tmp_path_factory.mktemp("cc"), oracle_backend, N16, NRO, NSP, OSF, WIDTH)
    G = cc64.gram(cc64.samples_of(path))
    A, lam = cc64.matrix(G, 4)
    return path, G, A, lam


def _cc(B, argv):
    return cc.main(argv + ["--debug", "40"], backend=B)


def test_driver_on_a_rank_deficient_scan(scan12, oracle_backend):
    path, G, A64, lam64 = scan12
    print("rank-deficient scan: lambda_4 / lambda_5 = %.3e" % (lam64[3] / lam64[4]))
    assert lam64[3] / lam64[4] >= 1e6
    stem = os.path.splitext(path)[0]
    z = np.load(path)
    for how in (["-p", "4"], ["-e", "0.999999"]):
        A, lam = _cc(oracle_backend, how + [path])
        assert A.shape == (4, 12) and lam.shape == (12,)
        out, fa, fv = np.load(stem + ".cc.npz"), np.load(stem + ".ccmat.npy"), np.load(stem + ".ccvals.npy")
        assert sorted(out.files) == sorted(z.files)
        assert out['data'].shape == z['data'].shape[:-4] + (4,) + z['data'].shape[-3:] and out['data'].dtype == C64
        assert out['maps'].shape == z['maps'].shape[:-4] + (4,) + z['maps'].shape[-3:] and out['maps'].dtype == C64
        assert np.array_equal(out['traj'], z['traj'])
        assert fa.shape == (4, 12) and fa.dtype == np.complex128 and np.array_equal(fa, A)
        assert fv.shape == (12,) and fv.dtype == np.float64 and np.array_equal(fv, lam)
        err_d = _rel(out['data'].T, cc64.mix(fa, z['data'].T))
        err_m = _rel(out['maps'].T, cc64.mix(fa, z['maps'].T))
        bound = cc64.davis_kahan(G, lam64, 4)
        err_p = np.linalg.norm(cc64.projector(fa) - cc64.projector(A64))
        print("cc %s: data %.3e maps %.3e, projector %.3e (Davis-Kahan bound %.3e)" % (how, err_d, err_m, err_p, bound))
        assert err_d <= 1e-5 and err_m <= 1e-5
        assert err_p <= bound


def test_driver_calibration_region_noise_and_calib(scan12, oracle_backend, tmp_path):
    path, G, A64, lam64 = scan12
    z = np.load(path)
    d = z['data'].T
    # a scan with a Cartesian `calib` block besides: cut with the same matrix; -r keeps the central samples only
    calib = rand64c(6 * 6 * 6 * 4, 1, seed=11).reshape((6, 6, 6, 4), order='F')
    withc = os.path.join(str(tmp_path), "withcalib.npz")
    np.savez(withc, data=z['data'], maps=z['maps'], traj=z['traj'], calib=cc64.mix(cc64.channel_matrix(), calib).astype(C64).T)
    noise = rand64c(500, 12, seed=12)
    nf = os.path.join(str(tmp_path), "noise.npy")
    np.save(nf, noise.T)
    A, lam = _cc(oracle_backend, ["-p", "4", "-r", "8", "--noise", nf, "--chunk", "700", withc])
    out = np.load(os.path.splitext(withc)[0] + ".cc.npz")
    assert out['calib'].shape == (4, 6, 6, 6) and _rel(out['calib'].T, cc64.mix(A, np.load(withc)['calib'].T)) <= 1e-5
    k = z['traj'].T.reshape((3, -1), order='F')
    inside = np.abs(k).max(axis=0) <= 4.0
    assert 0 < inside.sum() < inside.size
    Psi = cc64.covariance(noise)
    A64r, lam64r = cc64.matrix(cc64.gram(d.reshape((-1, 12), order='F')[inside]), 4, noise_cov=Psi)
    assert np.allclose(lam[:4], lam64r[:4], rtol=1e-5, atol=0)
    assert np.linalg.norm(A @ Psi @ A.conj().T - np.eye(4)) <= 1e-5


# ---- 4. invariance of the reconstruction --------------------------------------------------------------------------------------------

def _pics(B, argv):
    B._scratch = None
    try:
        return pics.main(argv + ["--debug", "40"], backend=B)
    finally:
        B._scratch = None


def test_reconstruction_is_invariant_under_compression(scan12, oracle_backend):
    """Unitary coil mixing leaves sum_c S_c^H F^H F S_c and A^H y unchanged, and the scan's coil vectors span 4 dimensions: pics
    --cc 12, pics --cc 4 and pics on the compressed file are realisations of the operator pics builds without the flag.  lamda = a
    tenth of the largest eigenvalue of A^H A, as tests/test_hip_softsense.py compares two realisations and for its reason."""
    path = scan12[0]
    B = oracle_backend
    L = cc64.largest_eigenvalue(B, COMMON + ["--lamda", "0", path])
    args = COMMON + ["--lamda", "%.8e" % (L / 10)]
    _cc(B, ["-p", "4", path])
    written = os.path.splitext(path)[0] + ".cc.npz"
    for iters, tol in (("1", 1e-5), ("10", 1e-4)):
        ref = _pics(B, ["-i", iters] + args + [path])
        cc12 = _pics(B, ["-i", iters, "--cc", "12"] + args + [path])
        cc4 = _pics(B, ["-i", iters, "--cc", "4"] + args + [path])
        onfile = _pics(B, ["-i", iters] + args + [written])
        errs = (_rel(cc12, ref), _rel(cc4, ref), _rel(onfile, cc4))
        print("pics --cc, %s iterations: --cc 12 %.3e, --cc 4 %.3e against no flag; the written file against --cc 4 %.3e" % ((iters,) + errs))
        assert ref.shape == cc4.shape == N16 + (1,) and max(errs) < tol, (iters, errs)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals(scan12, oracle_backend, tmp_path):
    path = scan12[0]
    B = oracle_backend
    with pytest.raises(ValueError, match=r"13 virtual coils from 12 coils.*min\(coils, 32\) = 12"):
        _cc(B, ["-p", "13", path])
    with pytest.raises(ValueError, match=r"13 virtual coils from 12"):
        _pics(B, ["-i", "1", "--cc", "13"] + COMMON + [path])
    with pytest.raises(ValueError, match=r"33 virtual coils from 40 coils.*= 32"):
        cc.matrix(np.eye(40), V=33)
    assert cc.matrix(np.eye(40), V=32)[0].shape == (32, 40)
    with pytest.raises(ValueError, match=r"65 coils, between 1 and 64"):
        cc.matrix(np.eye(65), V=8)
    with pytest.raises(RuntimeError, match=r"65 coils, between 1 and 64"):
        B.coil_gram(B.copy_array(rand64c(4, 65, seed=1)), 4, 65)
    big = os.path.join(str(tmp_path), "big.npz")
    np.savez(big, data=rand64c(8 * 65, 1, seed=2).reshape((1, 8, 1, 65), order='F').T)
    with pytest.raises(ValueError, match=r"65 coils, between 1 and 64"):
        _cc(B, ["-p", "8", big])
    # a noise file with another coil count, and a singular covariance (fewer noise samples than coils)
    nf = os.path.join(str(tmp_path), "noise11.npy")
    np.save(nf, rand64c(50, 11, seed=3).T)
    with pytest.raises(ValueError, match=r"noise file holds .*12 coils"):
        _cc(B, ["-p", "4", "--noise", nf, path])
    np.save(nf, rand64c(5, 12, seed=4).T)
    with pytest.raises(ValueError, match="not positive definite"):
        _cc(B, ["-p", "4", "--noise", nf, path])
    with pytest.raises(ValueError, match="not positive definite"):
        cc.matrix(np.eye(3), V=2, noise_cov=np.diag([1.0, 1.0, 0.0]))
    with pytest.raises(SystemExit):
        _cc(B, ["-p", "4", "-e", "0.9", path])
    with pytest.raises(SystemExit):
        _cc(B, [path])
    # data and maps with different coil counts
    z = np.load(path)
    odd = os.path.join(str(tmp_path), "odd.npz")
    np.savez(odd, data=z['data'], maps=z['maps'].T[..., :11, :].T, traj=z['traj'])
    with pytest.raises(ValueError, match=r"maps has 11 coils, data has 12"):
        _cc(B, ["-p", "4", odd])
    with pytest.raises(ValueError, match=r"data has 12 coils, maps have 11"):
        _pics(B, ["-i", "1", "--cc", "4"] + COMMON + [odd])


# ---- 6. ecalib on a compressed scan ------------------------------------------------------------------------------------------------------

def test_ecalib_accepts_the_compressed_scan(oracle_backend, tmp_path):
    path, S, sup = e64.noncart_scan(tmp_path, oracle_backend)
    A, lam = _cc(oracle_backend, ["-p", "3", path])
    assert A.shape == (3, 3) and np.linalg.norm(A @ A.conj().T - np.eye(3)) <= 1e-12
    written = os.path.splitext(path)[0] + ".cc.npz"
    oracle_backend._scratch = None
    maps, evals = ecalib.main(["-m", "1", "-c", "0", "--debug", "40"] + e64.NC_ARGS + [written], backend=oracle_backend)
    oracle_backend._scratch = None
    assert maps.shape == e64.NC_DIMS + (3, 1) and np.isfinite(maps).all()
    assert np.load(os.path.splitext(written)[0] + ".maps.npy").shape == (1, 3) + e64.NC_DIMS[::-1]
    # the maps of the compressed scan span what A makes of the true ones
    err = e64.span_residual(cc64.mix(A, S), maps.astype(np.complex128), sup)
    print("ecalib on the compressed scan: residual of A S outside the estimated maps %.3e" % err)
    assert err <= 0.2
