"""A float64 restatement of coil compression and noise prewhitening (indigo_amd.cc, Backend.coil_gram, Backend.coil_mix,
ig_coil_gram_c64), for the tests, and a rank-deficient synthetic scan: 4 true coils seen through 12 channels."""
import logging
import os
import re

import numpy as np

C64 = np.dtype('complex64')


def gram(y):
    """G[p, q] = sum_i y[i, p] conj(y[i, q]) of the (n, C) samples, complex128"""
    y = np.asarray(y, dtype=np.complex128)
    return y.T @ np.conj(y)


def slab_grams(y, slab):
    """the Gram matrices of the slabs [j slab, (j + 1) slab) of the (n, C) samples, (rows, C, C)"""
    return np.stack([gram(y[i:i + slab]) for i in range(0, y.shape[0], slab)])


def unpack(parts, C):
    """rows of packed upper triangles (column p C - p (p - 1) / 2 + (q - p) is [p, q], p <= q) -> (rows, C, C) Hermitian,
    the diagonal's imaginary part KEPT so that a test can see it"""
    parts = np.asarray(parts)
    G = np.zeros((parts.shape[0], C, C), dtype=np.complex128)
    col = 0
    for p in range(C):
        for q in range(p, C):
            G[:, p, q] = parts[:, col]
            if q > p:
                G[:, q, p] = np.conj(parts[:, col])
            col += 1
    return G


def covariance(noise):
    """Psi = (1 / m) sum_j nu_j nu_j^H of the (m, C) noise samples"""
    return gram(noise) / np.asarray(noise).shape[0]


def matrix(G, V, noise_cov=None):
    """-> (A, all eigenvalues descending): A = U[:, :V]^H L^-1 with L L^H = Psi (L = I without noise), U Lambda U^H = L^-1 G L^-H,
    every eigenvector rotated so that its largest-magnitude component is real and positive"""
    G = np.asarray(G, dtype=np.complex128)
    C = G.shape[0]
    Linv = np.eye(C, dtype=np.complex128)
    if noise_cov is not None:
        Linv = np.linalg.inv(np.linalg.cholesky(np.asarray(noise_cov, dtype=np.complex128)))
    lam, U = np.linalg.eigh(Linv @ G @ Linv.conj().T)
    order = np.argsort(-lam, kind='stable')
    lam, U = lam[order], U[:, order]
    for v in range(C):
        k = int(np.argmax(np.abs(U[:, v])))
        U[:, v] = U[:, v] * (np.conj(U[k, v]) / abs(U[k, v]))
    return U[:, :V].conj().T @ Linv, lam


def energy_rank(lam, energy):
    """the smallest V with sum_{v < V} lam_v >= energy * sum lam"""
    total = float(np.sum(lam))
    for V in range(1, len(lam) + 1):
        if float(np.sum(lam[:V])) >= energy * total:
            return V
    return len(lam)


def mix(A, array, coil_axis=3):
    """A applied along the coil axis of the array, complex128"""
    a = np.moveaxis(np.asarray(array, dtype=np.complex128), coil_axis, -1)
    return np.moveaxis(a @ np.asarray(A, dtype=np.complex128).T, -1, coil_axis)


def projector(A):
    return np.asarray(A).conj().T @ np.asarray(A)


def davis_kahan(G, lam, V, bar=1e-5):
    """sqrt(2) ||dG||_F / (lam_V - lam_{V+1}) with ||dG||_F = bar ||G||_F: how far (Frobenius) the projector onto the V leading
    eigenvectors can move when G moves by the project's bar"""
    gap = lam[V - 1] - (lam[V] if V < len(lam) else 0.0)
    return np.sqrt(2.0) * bar * np.linalg.norm(G) / gap


TRUE_COILS, CHANNELS = 4, 12


def channel_matrix(seed=7):
    """12 x 4 with orthonormal columns"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((CHANNELS, TRUE_COILS)) + 1j * rng.standard_normal((CHANNELS, TRUE_COILS)))
    return q


def rank_deficient_scan(tmpdir, B, N, nro, nsp, osf, width, name="scan12.npz"):
    """maps64.softsense_scan with 4 coils and one set of maps, its data and maps multiplied in complex128 by `channel_matrix()` and
    rounded to complex64: a 12-channel scan whose coil vectors span 4 dimensions.  -> its path"""
    import maps64
    B._scratch = None
    four = maps64.softsense_scan(tmpdir, B, N, TRUE_COILS, 1, nro, nsp, osf, width, name="four_" + name)
    B._scratch = None
    z = np.load(four)
    Q = channel_matrix()
    path = os.path.join(str(tmpdir), name)
    np.savez(path, data=mix(Q, z['data'].T).astype(C64).T, maps=mix(Q, z['maps'].T).astype(C64).T, traj=z['traj'])
    return path


def samples_of(path):
    """the (samples, C) complex128 coil vectors of every frame of the scan's data"""
    d = np.load(path)['data'].T
    return d.reshape((-1, d.shape[3], int(np.prod(d.shape[4:]))), order='F').transpose(0, 2, 1).reshape((-1, d.shape[3])).astype(np.complex128)


def largest_eigenvalue(backend, argv):
    """the power-iteration estimate of the largest eigenvalue of A^H A + lamda I that a FISTA run of the pics driver logs (no
    iterations of the solver itself)"""
    from indigo_amd import pics
    records = []

    class Keep(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())
    keep = Keep(level=logging.INFO)
    plog = logging.getLogger("pics")
    old = plog.level
    plog.addHandler(keep)
    plog.setLevel(logging.INFO)
    try:
        backend._scratch = None
        pics.main(["-i", "0", "--power-iters", "6", "--llr", "0.01", "--debug", "40"] + argv, backend=backend)
    finally:
        plog.removeHandler(keep)
        plog.setLevel(old)
        backend._scratch = None
    return [float(m.group(1)) for s in records for m in [re.search(r"largest eigenvalue of A\^H A \+ lamda I (\S+)", s)] if m][0]
