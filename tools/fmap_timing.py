#!/usr/bin/env python3
"""Device-event times of the pieces of pics --fmap on the MI355X, steady state after warm-up, as one JSON document:

  * the two streaming passes of the time-segmented model, both directions, with L = 4 and 8 segments: the phase pass
    (Backend.segment_phase, ig_fmap_phase_c64) at 256^3 voxels and the combine pass (Backend.segment_combine, ig_fmap_combine_c64)
    at 2^24 samples x 8 coils, with the table of one readout of 512 samples and with one row per sample, each next to `axpby` on
    vectors of the same byte count.  Byte models: phase 8 n (L + 1) + 4 n, combine 8 n (L + 1) + 8 P L; axpby reads two vectors and
    writes one, 24 bytes per element.  The rates are the byte models over the times;
  * one A^H A of pics --fmap in gridding form with L = 4, SegmentPhase^H BlockDiag(A0^H)^L Combine^H Combine BlockDiag(A0)^L
    SegmentPhase, against L evaluations of the plain A0^H A0 (bench.py config 4 at the image edge --img, 8 coils, oversampling 2);
  * one A^H A in Toeplitz form, SegmentPhase^H ToeplitzNormal(K = L) SegmentPhase, against ToeplitzNormal(K = L) alone;
  * the set-up of the L (L + 1) / 2 point-spread functions (indigo_amd.toeplitz.psf_kernel with sample weights).

    python tools/fmap_timing.py [--warmup 2] [--steps 10] [--segments 4,8] [--img 128] [--out profiles/fmap_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd.backends import get_backend  # noqa: E402
from indigo_amd.util import rand64c  # noqa: E402
from tools.tv_timing import event_ms  # noqa: E402

C64 = np.dtype('complex64')
TAU0, DTAU = 1e-3, 2e-3


def fill(B, rows, cols, seed):
    """a rows x cols device panel of random values: one block of 2^20 drawn on the host and repeated"""
    block = np.random.default_rng(seed).standard_normal((1 << 20, 2), dtype=np.float32).view(C64).reshape(-1)
    col = np.asfortranarray(np.resize(block, rows).reshape((rows, 1)))
    a = B.zero_array((rows, cols), C64)
    for j in range(cols):
        a[:, j:j + 1]._copy_from(col)
    return a


def median_ms(B, fn, warmup, steps, reps=5):
    """the median of `reps` means over `steps` back-to-back calls, after `warmup` calls"""
    event_ms(B, fn, warmup, 1)
    return float(np.median([event_ms(B, fn, 0, steps) for _ in range(reps)]))


def axpby_row(B, a, nbytes):
    m = int(nbytes // 24)
    u, v = fill(B, m, 1, 4), fill(B, m, 1, 5)
    ms = median_ms(B, lambda: B.axpby(0.5, v, 0.5, u), a.warmup, a.steps)
    return dict(bytes=nbytes, axpby_elements=m, axpby_ms=ms, axpby_TBps=24.0 * m / ms / 1e9)


def passes(B, a, row, nbytes, fwd, adj):
    row.update(axpby_row(B, a, nbytes))
    for name, fn in (("forward", fwd), ("adjoint", adj)):
        t = median_ms(B, fn, a.warmup, a.steps)
        row.update({name + "_ms": t, name + "_TBps": nbytes / t / 1e9, name + "_rate_of_axpby": (nbytes / t) / row["axpby_TBps"] / 1e9})
    print(json.dumps(row), flush=True)
    return row


def phase_pass(B, a, L, n=256 ** 3):
    f = B.copy_array(np.random.default_rng(1).uniform(-250, 250, n).astype(np.float32))
    img, seg = fill(B, n, 1, 2), fill(B, n, L, 3)
    return passes(B, a, dict(kernel="segment_phase", voxels=n, segments=L), 8.0 * n * (L + 1) + 4.0 * n,
                  lambda: B.segment_phase(seg, img, f, TAU0, DTAU, L, n),
                  lambda: B.segment_phase(img, seg, f, TAU0, DTAU, L, n, adjoint=True))


def combine_pass(B, a, L, P, n=(1 << 24) * 8):
    table = B.copy_array(rand64c(P, L, seed=1))
    smp, seg = fill(B, n, 1, 2), fill(B, n, L, 3)
    return passes(B, a, dict(kernel="segment_combine", rows=n, segments=L, period=P), 8.0 * n * (L + 1) + 8.0 * P * L,
                  lambda: B.segment_combine(smp, seg, table, P, n),
                  lambda: B.segment_combine(seg, smp, table, P, n, adjoint=True))


def normal_operators(B, a, L):
    """A^H A of pics --fmap with L segments in both forms on bench.py's config 4 problem at the image edge a.img"""
    import bench
    from indigo_amd import fmap as fmap_mod
    from indigo_amd.operators import ToeplitzNormal
    from indigo_amd.sense import normal_operator
    from indigo_amd.toeplitz import psf_kernel
    from indigo_amd.transforms import FuseZpadFFT, reserve_for, sense_recipe
    p = bench.sense_problem(4, a.img, 8)
    dims, C = tuple(p.N), p.C
    N = int(np.prod(dims))
    nro = p.coord.shape[1]
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in dims)]
    field = (150.0 * (0.6 * g[0] + 0.3 * g[1] * g[2] + 0.1 * np.cos(3 * g[2]))).astype(np.float32)
    times = 1e-3 + np.arange(nro) * (8e-3 / (nro - 1))
    taus, table, period, err = fmap_mod.segments(field, times, L=L)
    doc = dict(problem="bench config 4: image %s, %d coils, oversampling %g, half-width %g; field map of %.1f cycles span, %d segments (model error %.1e)"
               % (dims, C, p.oversamp, p.width, float(np.abs(field).max() * (times[-1] - times[0])), L, err), segments=L)
    A0 = p.build_zpadfft(B)
    AHA0 = normal_operator(A0, lamda=0.0)
    rows = A0.shape[0]
    B._scratch = None
    reserve_for(AHA0, 1, slack_products=6, extra=2 * ((N * L + 31) // 32 * 32) + 2 * ((rows * L + 31) // 32 * 32))
    x, y = B.copy_array(rand64c(N, 1, seed=2)), B.zero_array((N, 1), C64)
    plain_ms = median_ms(B, lambda: AHA0.eval(y, x), a.warmup, a.steps)
    Phase = B.SegmentPhase(field.reshape(-1, order='F'), taus, N)
    Comb = B.SegmentCombine(table, period, rows)
    A = Comb * B.BlockDiag([A0] * L) * Phase
    AHA = A.H * A
    grid_ms = median_ms(B, lambda: AHA.eval(y, x), a.warmup, a.steps)
    ref = y.to_host()
    seg_img, seg_smp, smp = B.zero_array((N * L, 1), C64), B.zero_array((rows * L, 1), C64), B.zero_array((rows, 1), C64)
    part = dict(phase_forward_ms=median_ms(B, lambda: Phase.eval(seg_img, x), a.warmup, a.steps),
                phase_adjoint_ms=median_ms(B, lambda: Phase.H.eval(y, seg_img), a.warmup, a.steps),
                combine_forward_ms=median_ms(B, lambda: Comb.eval(smp, seg_smp), a.warmup, a.steps),
                combine_adjoint_ms=median_ms(B, lambda: Comb.H.eval(seg_smp, smp), a.warmup, a.steps))
    del seg_img, seg_smp, smp
    doc["gridding"] = dict(plain_aha_ms=plain_ms, plain_aha_times_segments_ms=L * plain_ms, fmap_aha_ms=grid_ms,
                           ratio=grid_ms / (L * plain_ms), **part)
    print(json.dumps(doc["gridding"]), flush=True)
    del A, AHA, AHA0, A0, Comb
    B._scratch = None
    # the Toeplitz form
    order = ToeplitzNormal.memory_order(B, dims)
    weights = np.tile(table, (rows // C // period, 1))
    B.barrier()
    t0 = time.perf_counter()
    kern = psf_kernel(B, dims, [p.coord], [0], None, int(p.width), float(p.oversamp), order=order, recipe=sense_recipe(3) + [FuseZpadFFT],
                      sample_weights=weights)
    B.barrier()
    setup_s = time.perf_counter() - t0
    B._scratch = None
    maps = np.asarray(p.maps, dtype=C64).reshape(dims + (C,))
    TK = B.ToeplitzNormal(dims, maps, kern, L, order=order)
    T = Phase.H * TK * Phase
    reserve_for(T, 1, slack_products=6)
    xl, yl = B.copy_array(rand64c(N * L, 1, seed=3)), B.zero_array((N * L, 1), C64)
    alone_ms = median_ms(B, lambda: TK.eval(yl, xl), a.warmup, a.steps)
    toep_ms = median_ms(B, lambda: T.eval(y, x), a.warmup, a.steps)
    diff = float(np.linalg.norm(ref - y.to_host()) / np.linalg.norm(ref))
    doc["toeplitz"] = dict(toeplitz_normal_alone_ms=alone_ms, fmap_toeplitz_aha_ms=toep_ms, ratio=toep_ms / alone_ms,
                           relative_difference_from_gridding=diff, point_spread_functions=L * (L + 1) // 2, setup_s=setup_s,
                           kernel_bytes=int(kern.nbytes))
    print(json.dumps(doc["toeplitz"]), flush=True)
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--segments", default="4,8", help="segment counts of the kernel table")
    ap.add_argument("--img", type=int, default=128, help="image edge of the A^H A comparison (256: the headline problem)")
    ap.add_argument("--no-operators", action="store_true", help="only the kernel table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmap_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), method="device events; the median of 5 means over %d back-to-back calls after %d warm-up calls" % (a.steps, a.warmup),
               kernels=[])
    for L in (int(v) for v in a.segments.split(",")):
        doc["kernels"].append(phase_pass(B, a, L))
        doc["kernels"].append(combine_pass(B, a, L, 512))
        doc["kernels"].append(combine_pass(B, a, L, 1 << 24))
    if not a.no_operators:
        doc["normal_operator"] = normal_operators(B, a, 4)
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
