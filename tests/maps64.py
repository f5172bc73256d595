"""A float64 restatement of the per-voxel coil-map product of soft-SENSE (Backend.coil_maps, ig_coil_maps_c64), for the tests, and a
synthetic scan with several sets of coil maps whose k-space comes from the single-map operators."""
import os

import numpy as np

C64 = np.dtype('complex64')


def forward(S, x):
    """coil images[i, c] = sum_m S[i, c, m] x[i, m], in complex128"""
    return np.einsum('icm,im->ic', np.asarray(S, dtype=np.complex128), np.asarray(x, dtype=np.complex128))


def adjoint(S, x):
    """images[i, m] = sum_c conj(S[i, c, m]) x[i, c], in complex128"""
    return np.einsum('icm,ic->im', np.conj(np.asarray(S, dtype=np.complex128)), np.asarray(x, dtype=np.complex128))


def apply(S, x, y=None, adjoint_=False, alpha=1, beta=0):
    """beta*y + alpha * (forward or adjoint)(x), in complex128; S is (n, C, M); y is not read when beta == 0"""
    out = complex(alpha) * (adjoint(S, x) if adjoint_ else forward(S, x))
    if beta != 0:
        out = out + complex(beta) * np.asarray(y, dtype=np.complex128)
    return out


def planes(S, width=None, pad=0):
    """the (n, C, M) maps as the flat array Backend.coil_maps takes: M planes, coil-major (element (i, c) at i + n c) or, with
    `width`, coil-interleaved rows of `width` slots (element (i, c) at i width + c) whose padding slots hold `pad`"""
    S = np.asarray(S, dtype=C64)
    n, C, M = S.shape
    if width is None:
        return np.concatenate([S[:, :, m].reshape(-1, order='F') for m in range(M)])
    out = np.full((M, n, width), pad, dtype=C64)
    out[:, :, :C] = S.transpose(2, 0, 1)
    return out.reshape(-1)


def interleave(a, width, pad=0):
    """the (n, C) coil images as the flat coil-interleaved array of rows of `width` slots, padding slots `pad`"""
    a = np.asarray(a, dtype=C64)
    out = np.full((a.shape[0], width), pad, dtype=C64)
    out[:, :a.shape[1]] = a
    return out.reshape(-1)


def smooth_maps(N, C, M):
    """Gaussian coil maps N + (C, M): set m is shifted and phase-rotated against set 0"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    centres = [(-1, 0, 0.3), (1, 0.5, -0.4), (0, -1, 1.1), (0.3, 1, -0.9), (-0.6, -0.8, 2.0), (0.8, -0.7, 0.6), (0, 0, 1.7), (-1, 1, -1.3)]
    mps = np.zeros(tuple(N) + (C, M), dtype=C64)
    for m in range(M):
        for c in range(C):
            cx, cy, ph = centres[c % len(centres)]
            mps[..., c, m] = (np.exp(-((g[0] - cx - 0.35 * m) ** 2 + (g[1] - cy + 0.25 * m) ** 2 + 0.5 * (g[2] - 0.2 * m) ** 2))
                              * np.exp(1j * (ph + 0.9 * m + 0.7 * m * g[2])) / (1 + 0.5 * m))
    return mps


def objects(N, M):
    """one object image per set: a blob and a box that moves with the set"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    imgs = []
    for m in range(M):
        img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j) / (1 + m)).astype(np.complex128)
        img[(np.abs(g[0] - 0.2 * m) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5 * (-1) ** m
        imgs.append(img.astype(C64))
    return imgs


def single_map_operator(B, N, C, maps_m, coord, nro, nsp, osf, width):
    """today's single-map operator KronI(C, NUFFT) * VStack(Diag(map_c)) for one set of maps N + (C,)"""
    F1 = B.NUFFT((1, nro, nsp), N, coord, width=width, oversamp=(osf, osf, osf), dtype=C64)
    return B.KronI(C, F1) * B.VStack([B.Diag(np.ascontiguousarray(maps_m[..., c]).reshape(tuple(N) + (1,))) for c in range(C)])


def softsense_scan(tmpdir, B, N, C, M, nro, nsp, osf, width=2, T=1, name="scan.npz"):
    """a synthetic radial scan with M sets of C smooth coil maps, one object image per set and a trajectory per frame (frame t holds
    the objects scaled by 1 / (1 + t / 2)), written as an .npz; the k-space is sum_m of the single-map operators' products, so
    the data never pass through the soft-SENSE code.  -> its path"""
    from indigo_amd.sense import radial_trajectory
    mps = smooth_maps(N, C, M)
    imgs = objects(N, M)
    ksps, trajs = [], []
    for t in range(T):
        coord = radial_trajectory(nsp, nro, seed=2 + t)
        ksp = 0
        for m in range(M):
            A = single_map_operator(B, N, C, mps[..., m], coord, nro, nsp, osf, width)
            ksp = ksp + A * np.asfortranarray((imgs[m] / (1 + 0.5 * t)).astype(C64).reshape(-1, 1, order='F'))
            B._scratch = None
        ksps.append(ksp.astype(C64).reshape((1, nro, nsp, C), order='F'))
        trajs.append(coord * np.array(N, dtype=np.float64)[:, None, None])
    if T == 1:
        ksp, traj = ksps[0], trajs[0]
    else:
        ksp = np.stack(ksps, axis=-1).reshape(ksps[0].shape + (1,) * 6 + (T,))
        traj = np.stack(trajs, axis=-1).reshape(trajs[0].shape + (1,) * 7 + (T,))
    path = os.path.join(str(tmpdir), name)
    np.savez(path, data=ksp.T, maps=mps.T, traj=traj.T)
    return path


def first_set_scan(path, name="first.npz"):
    """the scan at `path` with only the first set of maps kept (MAPS axis of length 1), written next to it; -> its path"""
    z = np.load(path)
    maps = z['maps'].T[..., :1]
    out = os.path.join(os.path.dirname(path), name)
    np.savez(out, data=z['data'], maps=maps.T, traj=z['traj'])
    return out
