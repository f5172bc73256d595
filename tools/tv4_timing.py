#!/usr/bin/env python3
"""Device-event times of the pieces of pics --tv-time on the MI355X, steady state after warm-up, as one JSON document:

  * the gradient with the temporal difference, its adjoint (added onto the output, alpha = beta = 1, as the solver calls it) and
    the fused spatio-temporal dual step (Backend.grad4 / tv4_dual_step) at 256^3 x 4 frames, next to the 3-D kernels
    (Backend.grad3 / tv_dual_step) on the same number of voxels, a 256^3 panel of 4 columns.  One frame is 134 MB, so the
    neighbouring frame comes from memory again.  Byte model per voxel and frame with f = (T - 1) / T = 3/4:
    gradient 40 + 8 f = 46 B (3-D: 32), adjoint 32 + 16 f + 8 (the output read) = 52 B (3-D: 40), dual step 80 + 16 f = 92 B
    (3-D: 64);
  * one primal-dual iteration of pics --tv-time on 4 frames that share one trajectory against 4 evaluations of A^H A, on the
    headline problem (bench.py config 4: 256^3 image, 8 coils, 512^3 grid).

    python tools/tv4_timing.py [--warmup 3] [--steps 20] [--frames 4] [--out profiles/r12_tv4_timing.json]
"""
import argparse
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


def kernels(B, a):
    dims, T = (256, 256, 256), a.frames
    n = int(np.prod(dims))
    f = (T - 1) / T
    x = B.copy_array(rand64c(n, T, seed=1))
    xo = B.copy_array(rand64c(n, T, seed=2))
    u4 = B.zero_array((4 * n, T), C64)
    u3 = B.zero_array((3 * n, T), C64)
    row = dict(dims=dims, frames=T)
    for name, nbytes, fn in (("grad4", 40.0 + 8.0 * f, lambda: B.grad4(u4, x, dims, T)),
                             ("grad4h", 40.0 + 16.0 * f, lambda: B.grad4(xo, u4, dims, T, adjoint=True, alpha=1, beta=1)),
                             ("dual4", 80.0 + 16.0 * f, lambda: B.tv4_dual_step(u4, x, xo, 0.5, 0.1, 0.1, dims, T)),
                             ("grad3", 32.0, lambda: B.grad3(u3, x, dims)),
                             ("grad3h", 40.0, lambda: B.grad3(xo, u3, dims, adjoint=True, alpha=1, beta=1)),
                             ("dual3", 64.0, lambda: B.tv_dual_step(u3, x, xo, 0.5, 0.1, dims))):
        ms = event_ms(B, fn, a.warmup, a.steps)
        row[name + "_ms"] = ms
        row[name + "_bytes_per_voxel"] = nbytes
        row[name + "_TBps"] = nbytes * n * T / ms / 1e9
    for k4, k3 in (("grad4", "grad3"), ("grad4h", "grad3h"), ("dual4", "dual3")):
        row[k4 + "_rate_of_" + k3] = row[k4 + "_TBps"] / row[k3 + "_TBps"]
    print(json.dumps(row), flush=True)
    return row


def iteration(B, a):
    """one primal-dual iteration of pics --tv-time on T frames of bench.py's config 4 problem against T evaluations of A^H A"""
    import bench
    from indigo_amd.sense import normal_operator
    T = a.frames
    p = bench.sense_problem(4, 256, 8)
    A = p.build_zpadfft(B)
    AHA1 = normal_operator(A, lamda=1e-3)
    AHA = B.BlockDiag([AHA1] * T)                   # the frames share one trajectory: one tree, evaluated on each frame's rows
    n = AHA.shape[1]
    dims = tuple(p.N)
    x = B.copy_array(rand64c(n, 1, seed=2))
    y = B.zero_array((n, 1), C64)
    aha_ms = event_ms(B, lambda: AHA.eval(y, x), a.warmup, a.steps)
    G = B.GradientT(dims, T)
    b = B.copy_array(rand64c(n, 1, seed=3))
    u = B.zero_array((4 * n, 1), C64)
    tau, sigma, mu, mu_t = 0.1, 0.3, 0.01, 0.01

    def gradf(g, z):
        AHA.eval(g, z)
        B.axpby(1, g, -1, b)

    def KH(g, v):
        G.eval(g, v, alpha=1, beta=1, forward=False)

    def dual_step(v, xn, xo):
        B.tv4_dual_step(v, xn, xo, sigma, mu, mu_t, dims, T)

    B.primal_dual(gradf, None, KH, dual_step, tau, x, u, maxiter=a.warmup)     # (the solver's buffers and the leaf's formats: warm)
    tv_ms = event_ms(B, lambda: B.primal_dual(gradf, None, KH, dual_step, tau, x, u, maxiter=a.steps), 0, 1) / a.steps
    row = dict(problem="bench config 4: image %s, 8 coils, oversampling 2 (grid 512^3), %d frames on one trajectory" % (dims, T),
               device=B.device_name(), frames=T, aha_all_frames_ms=aha_ms, tv_time_iteration_ms=tv_ms, ratio=tv_ms / aha_ms)
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_tv4_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), kernels=kernels(B, a), tv_time=iteration(B, a))
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
