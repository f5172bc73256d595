"""The shapes and inputs that the locally low-rank kernels are tested on (tests/test_hip_llr.py), kept apart from the GPU tests so
that the CPU suite can check what they assume: that the threshold of every case cuts through the middle of the spectrum."""
import numpy as np

import llr64
from indigo_amd.util import rand64c

# (dims, block, T, shift)
CASES = [
    ((17, 5, 3), (4, 4, 2), 3, (0, 0, 0)),        # partial blocks on every axis
    ((17, 5, 3), (4, 4, 2), 3, (1, 3, 1)),        # the same with wrap-around
    ((16, 16, 8), (8, 8, 8), 16, (3, 5, 1)),      # full blocks, the largest register image in common use
    ((16, 8, 8), (16, 8, 8), 32, (0, 0, 0)),      # the upper limits: 1024 voxels, 32 frames
    ((8, 1, 6), (8, 8, 8), 4, (0, 0, 0)),         # clamped sides and a unit axis
    ((2, 2, 2), (1, 1, 1), 2, (0, 0, 0)),         # one-voxel blocks
    ((9, 7, 5), (4, 4, 4), 1, (2, 0, 3)),         # one frame
    ((64, 64, 40), (2, 2, 2), 2, (1, 1, 0)),      # 20 480 blocks, more than a launch's grid holds at once
]
INPUTS = ("uniform", "lowrank")


def case_id(c):
    return "x".join(map(str, c[0])) + "_b" + "x".join(map(str, c[1])) + "_T%d_s" % c[2] + "".join(map(str, c[3]))


def make_input(kind, dims, block, T, shift):
    """the (N, T) complex64 panel: `uniform` is rand64c - (0.5 + 0.5j); `lowrank` has in every block three dominant components
    (weights 1, 1/2, 1/4; as many as the block's matrix has room for) plus 5 % noise"""
    n = int(np.prod(dims))
    if kind == "uniform":
        return rand64c(n, T, seed=1) - (0.5 + 0.5j)
    rng = np.random.default_rng(7)
    x = np.zeros((n, T), dtype=np.complex128)

    def gauss(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    for rows in llr64.blocks(dims, block, shift):
        r = min(3, rows.size, T)
        low = (gauss(rows.size, r) * (0.5 ** np.arange(r))) @ gauss(r, T)
        x[rows] = low + 0.05 * np.sqrt((np.abs(low) ** 2).mean()) * gauss(rows.size, T)
    return np.asfortranarray(x.astype(np.complex64))


def threshold(sv):
    """the median of all the blocks' singular values, rounded to float32"""
    return float(np.float32(np.median(np.concatenate(sv))))


def share_above(sv, tau):
    return float((np.concatenate(sv) > tau).mean())
