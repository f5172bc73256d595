"""Float64 restatement of the locally low-rank pieces of pics --llr, written from their definition with
numpy.linalg.svd per block and not from the product's code: the partition into shifted blocks, block-wise singular-value
thresholding and the blocks' nuclear norms.  Test infrastructure, no GPU.

x holds T frames of an F-ordered `dims` volume of N voxels (axis 0 fastest): the panel (N, T), or stacked (N T,) / (N T, 1), frame
t in rows [tN, (t+1)N).  Block sides are clamped to `dims`; voxel i has the shifted coordinates j_a = (i_a + s_a) mod n_a and
belongs to block (j_0 // b_0, j_1 // b_1, j_2 // b_2); blocks are numbered F-order over their block coordinates."""
import itertools

import numpy as np


def clamp(dims, block):
    return tuple(min(int(b), int(n)) for b, n in zip(block, dims))


def blocks(dims, block, shift=(0, 0, 0)):
    """the list, in block order, of the flat F-order voxel indices of every block (each sorted by the shifted coordinates, axis 0
    fastest)"""
    dims = tuple(int(n) for n in dims)
    block = clamp(dims, block)
    assert all(b >= 1 for b in block) and all(0 <= s < b for s, b in zip(shift, block)), (dims, block, shift)
    counts = [(n + b - 1) // b for n, b in zip(dims, block)]
    out = []
    for k2, k1, k0 in itertools.product(*(range(c) for c in reversed(counts))):
        k = (k0, k1, k2)
        # the shifted coordinates j of the block along every axis, and the voxel coordinates i with (i + s) mod n = j
        axes = [[(j - s) % n for j in range(ka * b, min((ka + 1) * b, n))] for ka, b, s, n in zip(k, block, shift, dims)]
        out.append(np.array([i0 + dims[0] * (i1 + dims[1] * i2) for i2 in axes[2] for i1 in axes[1] for i0 in axes[0]], dtype=np.int64))
    return out


def _panel(x, dims, T):
    return np.asarray(x).astype(np.complex128).reshape((int(np.prod(dims)), T), order='F')


def singular_values(x, dims, T, block, shift=(0, 0, 0)):
    """[the singular values of M_b, descending] for every block b"""
    v = _panel(x, dims, T)
    return [np.linalg.svd(v[rows], compute_uv=False) for rows in blocks(dims, block, shift)]


def svt(x, tau, dims, T, block, shift=(0, 0, 0)):
    """M_b <- U max(S - tau, 0) V^H for every block; complex128, shaped like x"""
    v = _panel(x, dims, T)
    for rows in blocks(dims, block, shift):
        U, S, Vh = np.linalg.svd(v[rows], full_matrices=False)
        v[rows] = (U * np.maximum(S - tau, 0.0)) @ Vh
    return v.reshape(np.shape(x), order='F')


def nuc(x, dims, T, block, shift=(0, 0, 0)):
    """the nuclear norm of every block's matrix, (nb,) float64"""
    return np.array([s.sum() for s in singular_values(x, dims, T, block, shift)])
