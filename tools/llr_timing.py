#!/usr/bin/env python3
"""Device-event times of the pieces of pics --llr on the MI355X, steady state after warm-up, as one JSON document:

  * block-wise singular-value thresholding and the blocks' nuclear norms (Backend.llr_threshold / llr_norm's kernel,
    ig_llr_svt_c64 / ig_llr_nuc_c64) at 256^3 x 4, 8 and 16 frames, blocks of 8 voxels a side, at the shifts (0, 0, 0) and
    (3, 5, 1), next to `axpby` on the same panel.  Byte model per voxel and frame: thresholding 16 B (x once in, once out), the
    norms 8 B (+ 4 B per block), axpby 16 B read + 8 B written = 24 B; the rates are the byte model over the time;
  * one FISTA iteration of pics --llr on 4 frames that share one trajectory against 4 evaluations of A^H A, on the headline
    problem (bench.py config 4: 256^3 image, 8 coils, 512^3 grid).

    python tools/llr_timing.py [--warmup 2] [--steps 10] [--frames 4,8,16] [--out profiles/r13_llr_timing.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd.backends import get_backend  # noqa: E402
from indigo_amd.util import rand64c  # noqa: E402
from tools.tv_timing import event_ms  # noqa: E402

C64 = np.dtype('complex64')
DIMS, BLOCK, SHIFTS = (256, 256, 256), (8, 8, 8), [(0, 0, 0), (3, 5, 1)]


def kernels(B, a, T):
    n = int(np.prod(DIMS))
    rng = np.random.default_rng(1)
    x = B.zero_array((n, T), C64)
    for t in range(T):                               # independent frames: full-rank blocks, the spectrum that takes the most sweeps
        x[:, t:t + 1]._copy_from(np.asfortranarray(rng.standard_normal((n, 2), dtype=np.float32).view(C64)))
    y = B.zero_array((n, T), C64)
    row = dict(dims=DIMS, block=BLOCK, frames=T)
    ms = event_ms(B, lambda: B.axpby(0.5, y.reshape((n * T, 1)), 0.5, x.reshape((n * T, 1))), a.warmup, a.steps)
    row.update(axpby_ms=ms, axpby_TBps=24.0 * n * T / ms / 1e9)
    for shift in SHIFTS:
        head, xp, ldx, nb = B._llr_args(y, DIMS, T, BLOCK, shift)
        nuc = B.zero_array((nb, 1), np.dtype('float32'))
        tag = "shift%d%d%d" % shift

        def svt():
            y.copy(x)                                # a fresh panel every time: thresholding its own result would see rank-deficient blocks
            B.llr_threshold(y, 0.5, DIMS, T, BLOCK, shift)

        copy_ms = event_ms(B, lambda: y.copy(x), a.warmup, a.steps)
        svt_ms = event_ms(B, svt, a.warmup, a.steps) - copy_ms
        nuc_ms = event_ms(B, lambda: B._check(B._L.ig_llr_nuc_c64(B._ctx, *head, xp, ldx, ctypes.c_void_p(nuc._arr)), "ig_llr_nuc_c64"),
                          a.warmup, a.steps)
        row.update({"svt_%s_ms" % tag: svt_ms, "svt_%s_TBps" % tag: 16.0 * n * T / svt_ms / 1e9,
                    "svt_%s_rate_of_axpby" % tag: (16.0 / svt_ms) / (24.0 / ms),
                    "nuc_%s_ms" % tag: nuc_ms, "nuc_%s_TBps" % tag: (8.0 * n * T + 4.0 * nb) / nuc_ms / 1e9,
                    "copy_ms": copy_ms})
    print(json.dumps(row), flush=True)
    return row


def iteration(B, a, T=4):
    """one FISTA iteration of pics --llr on T frames of bench.py's config 4 problem against T evaluations of A^H A"""
    import bench
    from indigo_amd.solvers import llr_term
    from indigo_amd.sense import normal_operator
    p = bench.sense_problem(4, 256, 8)
    A = p.build_zpadfft(B)
    AHA1 = normal_operator(A, lamda=1e-3)
    AHA = B.BlockDiag([AHA1] * T)                   # the frames share one trajectory: one tree, evaluated on each frame's rows
    n = AHA.shape[1]
    dims = tuple(p.N)
    x = B.copy_array(rand64c(n, 1, seed=2))
    y = B.zero_array((n, 1), C64)
    aha_ms = event_ms(B, lambda: AHA.eval(y, x), a.warmup, a.steps)
    b = B.copy_array(rand64c(n, 1, seed=3))
    term = llr_term(B, dims, T, 0.01, block=8)

    def gradf(g, z):
        AHA.eval(g, z)
        B.axpby(1, g, -1, b)

    B.fista(gradf, term.proxg, 0.1, x, maxiter=a.warmup)
    it_ms = event_ms(B, lambda: B.fista(gradf, term.proxg, 0.1, x, maxiter=a.steps), 0, 1) / a.steps
    row = dict(problem="bench config 4: image %s, 8 coils, oversampling 2 (grid 512^3), %d frames on one trajectory" % (dims, T),
               device=B.device_name(), frames=T, aha_all_frames_ms=aha_ms, llr_iteration_ms=it_ms, ratio=it_ms / aha_ms)
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", default="4,8,16", help="frame counts of the kernel table")
    ap.add_argument("--no-iteration", action="store_true", help="only the kernel table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_llr_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), kernels=[kernels(B, a, int(T)) for T in a.frames.split(",")])
    if not a.no_iteration:
        doc["llr_fista"] = iteration(B, a)
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
