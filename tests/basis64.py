"""A float64 restatement of the temporal-subspace operator Phi (x) I_n (Backend.frame_basis, ig_basis_c64), for the tests, and a
synthetic scan whose frames lie in the span of a given basis."""
import os

import numpy as np

C64 = np.dtype('complex64')


def forward(phi, x):
    """frames[i, t] = sum_k phi[t, k] x[i, k], in complex128"""
    return np.einsum('tk,ik->it', np.asarray(phi, dtype=np.complex128), np.asarray(x, dtype=np.complex128))


def adjoint(phi, x):
    """images[i, k] = sum_t conj(phi[t, k]) x[i, t], in complex128"""
    return np.einsum('tk,it->ik', np.conj(np.asarray(phi, dtype=np.complex128)), np.asarray(x, dtype=np.complex128))


def apply(phi, x, y=None, adjoint_=False, alpha=1, beta=0):
    """beta*y + alpha * (forward or adjoint)(x), in complex128; y is not read when beta == 0"""
    out = complex(alpha) * (adjoint(phi, x) if adjoint_ else forward(phi, x))
    if beta != 0:
        out = out + complex(beta) * np.asarray(y, dtype=np.complex128)
    return out


def exponential_basis(T, rates=(0.15, 0.6)):
    """a QR-orthonormalised T x len(rates) basis of decaying exponentials"""
    t = np.arange(T, dtype=np.float64)
    q, _ = np.linalg.qr(np.stack([np.exp(-r * t) for r in rates], axis=1))
    return q


def subspace_scan(tmpdir, B, N, C, phi, nro, nsp, osf, width=2):
    """a synthetic radial scan of T frames x_t = sum_k phi[t, k] alpha_k (alpha_0 a blob, alpha_1 a box, ...) with a trajectory per
    frame, written as scan.npz; -> its path"""
    from indigo_amd.sense import radial_trajectory
    phi = np.asarray(phi)
    T, K = phi.shape
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    centres = [(-1, 0, 0.3), (1, 0.5, -0.4)][:C]
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph) for cx, cy, ph in centres],
                   axis=3).astype(C64)
    alphas = []
    for k in range(K):
        img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j) / (1 + k)).astype(np.complex128)
        img[(np.abs(g[0] - 0.2 * k) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5 * (-1) ** k
        alphas.append(img)
    ksps, trajs = [], []
    for t in range(T):
        img = sum(phi[t, k] * alphas[k] for k in range(K)).astype(C64)
        coord = radial_trajectory(nsp, nro, seed=2 + t)
        F1 = B.NUFFT((1, nro, nsp), N, coord, width=width, oversamp=(osf, osf, osf), dtype=C64)
        A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
        ksps.append((A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F'))
        trajs.append(coord * np.array(N, dtype=np.float64)[:, None, None])
        B._scratch = None
    ksp = np.stack(ksps, axis=-1).reshape(ksps[0].shape + (1,) * 6 + (T,))
    traj = np.stack(trajs, axis=-1).reshape(trajs[0].shape + (1,) * 7 + (T,))
    path = os.path.join(str(tmpdir), "scan.npz")
    np.savez(path, data=ksp.T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path
