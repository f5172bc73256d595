"""The volumes that the wavelet kernels are tested on (tests/test_hip_wavelet.py), kept apart from the GPU tests so that the CPU
suite can check what the comments claim (tests/test_wavelet_cpu.py): which plans are empty, which begin on another axis than 0,
which strips need more than 64 KB of LDS and how many lines the last strip of a pass holds."""
import numpy as np

import dwt64
from indigo_amd.util import rand64c

# (dims, wavelet, levels)
CASES = [
    ((9, 16, 4), "db2", 3),        # axis 0 never splits: the first pass is an axis-1 strip pass of 9 lines; axis 2 < 2 taps; 2 passes
    ((12, 10, 3), "haar", 3),      # a strip of 6 lines (axis 0 is halved before axis 1 splits); axis 1 stops at 5; odd axis 2; axis 0
                                   # split twice
    ((16, 8, 1), "db2", 3),        # a 2-D volume
    ((1, 1, 64), "db4", 5),        # a single line on axis 2; stops at 8 after three splits although levels = 5
    ((40, 6, 34), "haar", 2),      # strips over 20 lines = 16 + 4, on axis 1 and on axis 2; 34 -> 17
    ((12, 16, 3), "db4", 2),       # a strip of 12 lines: axis 0 is shorter than 2 taps
    ((41, 4, 6), "haar", 2),       # strips over 41 lines = 16 + 16 + 9, on axis 1 and on axis 2
    ((48, 20, 24), "db4", 3),      # axis-0 groups of 16 lines over 20 (16 + 4); 8 taps
    ((20, 640, 3), "db4", 2),      # axis-1 strips of 640 samples = 80 KB of LDS, above the 64 KB opt-in, 10 of 16 lines present
    ((5, 4, 1024), "db4", 9),      # axis 2 at the limit: 128 KB of LDS; 7 passes; 5 lines per strip
    ((1024, 4, 2), "db2", 9),      # axis 0 at the limit: 4 lines per group; 8 passes on one axis
    ((7, 9, 5), "db2", 3),         # no pass: every axis odd
    ((16, 16, 16), "db2", 0),      # no pass: no level
    ((2, 2, 2), "haar", 1),        # no pass: every axis shorter than 2 taps
]
NCOLS = 3
# more columns than a grid's z extent holds (65 535), so the kernels stride over columns
MANY_COLUMNS = ((4, 4, 4), "haar", 3, 70000)

# the launch geometry of ig_wavelet.hip: strips of 16 x-consecutive lines for axes 1 and 2, groups of 4096 / d (at most 16)
# contiguous lines for axis 0, 8 bytes a sample, and 64 KB of LDS without asking for more
STRIP, AX0_ELEMS, LDS_DEFAULT = 16, 4096, 65536


def case_id(c):
    return "x".join(map(str, c[0])) + "_%s_%d" % (c[1], c[2])


def launches(dims, wavelet, levels):
    """for every pass of the plan: (axis, d, P, Q, W, LDS bytes, lines in the last group) -- the lines (p, q) of a pass over
    `box` along `axis` are the box's other two axes, p the faster one; a workgroup takes W consecutive p"""
    out = []
    for box, a in dwt64.passes(dims, wavelet, levels)[0]:
        d, P, Q = box[a], box[1 if a == 0 else 0], box[1 if a == 2 else 2]
        W = max(1, min(AX0_ELEMS // d, STRIP)) if a == 0 else STRIP
        out.append((a, d, P, Q, W, W * d * 8, P % W or W))
    return out


def make_input(dims, ncols, seed):
    """the (N, ncols) complex64 panel rand64c - (0.5 + 0.5j), read-only"""
    x = rand64c(int(np.prod(dims)), ncols, seed=seed) - (0.5 + 0.5j)
    x.setflags(write=False)
    return x
