"""A float64 restatement of the Toeplitz normal operator (Backend.psf_mix, operators.ToeplitzNormal, indigo_amd.toeplitz), for
the tests: the K x K mixing pass, the exact point-spread functions by direct summation, and the exact NUDFT normal operator."""
import numpy as np


def unpack(kern, n, K):
    """(n, K, K) complex128 Hermitian matrices of a kernel array: K^2 planes of n floats, the K real diagonals, then re and im of
    every pair (k < k'), the pairs in row-major order of the upper triangle"""
    planes = np.asarray(kern, dtype=np.float64).reshape((K * K, n))
    P = np.zeros((n, K, K), dtype=np.complex128)
    P[:, np.arange(K), np.arange(K)] = planes[:K].T
    pair = 0
    for a in range(K):
        for b in range(a + 1, K):
            P[:, a, b] = planes[K + 2 * pair] + 1j * planes[K + 2 * pair + 1]
            P[:, b, a] = np.conj(P[:, a, b])
            pair += 1
    return P


def mix(kern, x):
    """y[g, c, k] = sum_k' P[g][k, k'] x[g, c, k'] in complex128; x: (n, C, K), kern: (K^2, n)"""
    x = np.asarray(x, dtype=np.complex128)
    n, _, K = x.shape
    return np.einsum('gab,gcb->gca', unpack(kern, n, K), x)


def _phases(traj, dims):
    """E[m, j] = exp(-2 pi i k_m . (j - dims // 2)) over the F-ordered voxels j: the NUDFT of one trajectory (3, M) in cycles per
    pixel, unscaled"""
    idx = np.stack(np.meshgrid(*[np.arange(n) - n // 2 for n in dims], indexing='ij'), axis=0).reshape(3, -1, order='F')
    return np.exp(-2j * np.pi * (np.asarray(traj, dtype=np.float64).reshape(3, -1).T @ idx))


def psf_exact(trajs, phi, dims, scale=1.0):
    """psf[k, k'][d] = scale * sum_t conj(phi[t, k]) phi[t, k'] sum_m exp(2 pi i k_{t,m} . d) for the lags d in [-n_a, n_a) per axis,
    by direct summation: (K, K, 2 n_0, 2 n_1, 2 n_2), lag d at index d + n_a"""
    phi = np.asarray(phi, dtype=np.complex128)
    T, K = phi.shape
    lags = np.stack(np.meshgrid(*[np.arange(-n, n) for n in dims], indexing='ij'), axis=0).reshape(3, -1)
    out = np.zeros((K, K, lags.shape[1]), dtype=np.complex128)
    for t in range(T):
        q = np.exp(2j * np.pi * (lags.T @ np.asarray(trajs[t], dtype=np.float64).reshape(3, -1))).sum(axis=1)
        out += scale * np.einsum('a,b->ab', np.conj(phi[t]), phi[t])[:, :, None] * q
    return out.reshape((K, K) + tuple(2 * n for n in dims))


def normal_exact(trajs, phi, maps, alpha, scale=1.0):
    """Phi^H E^H E Phi alpha with E_t = NUDFT_t * maps, exactly: alpha (N, K) -> (N, K) in complex128; maps: dims + (C,);
    trajs[t]: (3, M) in cycles per pixel; scale multiplies E^H E"""
    phi = np.asarray(phi, dtype=np.complex128)
    maps = np.asarray(maps, dtype=np.complex128)
    dims, C = maps.shape[:3], maps.shape[3]
    S = maps.reshape((-1, C), order='F')
    alpha = np.asarray(alpha, dtype=np.complex128)
    out = np.zeros_like(alpha)
    cache = {}
    for t in range(phi.shape[0]):
        key = np.asarray(trajs[t]).tobytes()
        if key not in cache:
            E = _phases(trajs[t], dims)
            cache[key] = E.conj().T @ E
        x_t = alpha @ phi[t]
        y_t = sum(np.conj(S[:, c]) * (cache[key] @ (S[:, c] * x_t)) for c in range(C))
        out += scale * np.outer(y_t, np.conj(phi[t]))
    return out
