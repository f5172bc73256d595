#!/usr/bin/env python3
"""Device-event times of the pieces of pics --basis on the MI355X, steady state after warm-up, as one JSON document:

  * the temporal-subspace operator and its adjoint (Backend.frame_basis, ig_basis_c64) at 256^3 voxels with K = 4 coefficient
    images and T = 8, 16 and 32 frames, next to `axpby` on vectors of the same byte count.  Byte model: frame_basis moves every
    coefficient image and every frame once, 8 n (K + T) bytes; axpby reads two vectors and writes one, 24 bytes per element,
    so it runs on n (K + T) / 3 elements.  The rates are the byte models over the times;
  * one CG iteration of pics --basis with K = 4 and T = 8 frames that share one trajectory, against 8 evaluations of one
    frame's A^H A, on the headline problem (bench.py config 4: 256^3 image, 8 coils, 512^3 grid).

    python tools/subspace_timing.py [--warmup 2] [--steps 10] [--frames 8,16,32] [--out profiles/r14_subspace_timing.json]
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
N, K = 256 ** 3, 4


def fill(B, rows, cols, seed):
    rng = np.random.default_rng(seed)
    a = B.zero_array((rows, cols), C64)
    for j in range(cols):
        a[:, j:j + 1]._copy_from(np.asfortranarray(rng.standard_normal((rows, 2), dtype=np.float32).view(C64)))
    return a


def kernels(B, a, T):
    phi = B.copy_array(rand64c(T, K, seed=1))
    coef, frames = fill(B, N, K, 2), fill(B, N, T, 3)
    nbytes = 8.0 * N * (K + T)
    m = N * (K + T) // 3
    u, v = fill(B, m, 1, 4), fill(B, m, 1, 5)
    row = dict(voxels=N, coefficients=K, frames=T, bytes=nbytes)
    ms = event_ms(B, lambda: B.axpby(0.5, v, 0.5, u), a.warmup, a.steps)
    row.update(axpby_elements=m, axpby_ms=ms, axpby_TBps=24.0 * m / ms / 1e9)
    for name, adjoint, y, x in (("forward", False, frames, coef), ("adjoint", True, coef, frames)):
        t = event_ms(B, lambda: B.frame_basis(y, x, phi, N, adjoint=adjoint), a.warmup, a.steps)
        row.update({name + "_ms": t, name + "_TBps": nbytes / t / 1e9, name + "_rate_of_axpby": (nbytes / t) / (24.0 * m / ms)})
    print(json.dumps(row), flush=True)
    return row


def iteration(B, a, T=8):
    """one CG iteration of pics --basis (K coefficient images, T frames of bench.py's config 4 problem on one trajectory)
    against T evaluations of one frame's A^H A"""
    import bench
    from indigo_amd.sense import normal_operator
    from indigo_amd.transforms import reserve_for
    p = bench.sense_problem(4, 256, 8)
    A = p.build_zpadfft(B)
    AHA1 = normal_operator(A, lamda=0.0)
    n = AHA1.shape[1]
    reserve_for(AHA1, 1, slack_products=6, extra=2 * n * T)            # the two frame panels of the three-factor product
    x1, y1 = B.copy_array(rand64c(n, 1, seed=2)), B.zero_array((n, 1), C64)
    aha_ms = event_ms(B, lambda: AHA1.eval(y1, x1), a.warmup, a.steps)
    Phi = B.FrameBasis(np.linalg.qr(rand64c(T, K, seed=6))[0], n)
    AHA = Phi.H * B.BlockDiag([AHA1] * T) * Phi + 1e-3 * B.Eye(n * K)
    x, y = B.copy_array(rand64c(n * K, 1, seed=3)), B.zero_array((n * K, 1), C64)
    sub_ms = event_ms(B, lambda: AHA.eval(y, x), a.warmup, a.steps)
    frames = B.zero_array((n * T, 1), C64)
    fwd_ms = event_ms(B, lambda: Phi.eval(frames, x), a.warmup, a.steps)
    adj_ms = event_ms(B, lambda: Phi.H.eval(y, frames), a.warmup, a.steps)
    del frames
    b = B.copy_array(rand64c(n * K, 1, seed=4))
    x._zero()
    B.cg(AHA, b, x, maxiter=a.warmup)
    it_ms = event_ms(B, lambda: B.cg(AHA, b, x, maxiter=a.steps), 0, 1) / (a.steps + 1)   # (one evaluation for the start)
    row = dict(problem="bench config 4: image %s, 8 coils, oversampling 2 (grid 512^3), %d frames on one trajectory, %d coefficients"
               % (tuple(p.N), T, K), device=B.device_name(), frames=T, coefficients=K, aha_one_frame_ms=aha_ms,
               aha_all_frames_ms=T * aha_ms, subspace_aha_ms=sub_ms, basis_forward_ms=fwd_ms, basis_adjoint_ms=adj_ms,
               cg_iteration_ms=it_ms, ratio=it_ms / (T * aha_ms))
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", default="8,16,32", help="frame counts of the kernel table")
    ap.add_argument("--no-iteration", action="store_true", help="only the kernel table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_subspace_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), kernels=[kernels(B, a, int(T)) for T in a.frames.split(",")])
    if not a.no_iteration:
        doc["subspace_cg"] = iteration(B, a)
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
