#!/usr/bin/env python3
"""Device-event times of the two coil-axis primitives of coil compression and prewhitening (indigo_amd.cc) on the
MI355X, steady state after warm-up, medians over repeated calls, as one JSON document:

  * the Gram pass ig_coil_gram_c64 over n = 2^24 samples of C = 8, 16, 32 and 64 coils (the kernel alone, its partial sums left on the
    device, at the backend's default slab and at the slabs of --slabs), and `Backend.coil_gram` as a whole (wall clock: kernel,
    download of the partial sums, float64 sum on the host).  Byte model: every sample once, 8 n C bytes; flop model: 4 C^2 n real
    flops against the 157 Tflop/s float32 peak;
  * the mix y' = A y (`Backend.coil_mix` = `Backend.frame_basis`, ig_basis_c64) at 32 -> 8 and 64 -> 16 coils with the matrix already
    on the device.  Byte model: 8 n (C + V);
  * `axpby` on vectors of the same byte count (it reads two vectors and writes one, 24 bytes per element) next to each.

    python tools/cc_timing.py [--warmup 2] [--reps 9] [--log2n 24] [--slabs 4096,65536] [--out profiles/cc_timing.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd.backends import get_backend  # noqa: E402
from indigo_amd.util import rand64c  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from softsense_timing import fill, medians  # noqa: E402

C64 = np.dtype('complex64')
PEAK_FP32 = 157e12


def axpby_pair(B, nbytes):
    m = int(nbytes // 24)
    u, v = fill(B, m, 4), fill(B, m, 5)
    return m, (lambda: B.axpby(0.5, v, 0.5, u))


def gram_row(B, a, n, C, slabs):
    nbytes, flops, ntri = 8.0 * n * C, 4.0 * C * C * n, C * (C + 1) // 2
    x = fill(B, n * C, 1)
    m, axpby = axpby_pair(B, nbytes)
    fns = {"axpby": axpby}
    keep = []
    for slab in slabs:
        rows = -(-n // slab)
        parts = B.empty_array((rows, ntri), C64)
        keep.append(parts)
        fns["slab_%d" % slab] = lambda slab=slab, parts=parts, rows=rows: B._check(
            B._L.ig_coil_gram_c64(B._ctx, n, C, ctypes.c_void_p(x._arr), n, slab, ctypes.c_void_p(parts._arr), rows), "ig_coil_gram_c64")
    ms = medians(B, fns, a.warmup, a.reps)
    axpby_rate = 24.0 * m / ms["axpby"]
    B.barrier()
    t0 = time.perf_counter()
    G = B.coil_gram(x, n, C)
    whole = (time.perf_counter() - t0) * 1e3
    row = dict(samples=n, coils=C, bytes=nbytes, flops=flops, axpby_ms=ms["axpby"], axpby_TBps=axpby_rate / 1e9, default_slab=B.tuning['gram_slab'],
               coil_gram_whole_ms=whole, trace_over_samples=float(np.trace(G).real / n))
    for slab in slabs:
        t = ms["slab_%d" % slab]
        row["slab_%d" % slab] = dict(ms=t, TBps=nbytes / t / 1e9, rate_of_axpby=(nbytes / t) / axpby_rate, Tflops=flops / t / 1e9,
                                     fraction_of_fp32_peak=flops / t / 1e-3 / PEAK_FP32, partial_rows=-(-n // slab))
    print(json.dumps(row), flush=True)
    return row


def mix_row(B, a, n, C, V):
    nbytes = 8.0 * n * (C + V)
    x, y = fill(B, n * C, 2), B.zero_array((n * V, 1), C64)
    phi = B.copy_array(np.asfortranarray(rand64c(C, V, seed=3)))
    m, axpby = axpby_pair(B, nbytes)
    ms = medians(B, {"axpby": axpby, "mix": lambda: B.frame_basis(y, x, phi, n, adjoint=True)}, a.warmup, a.reps)
    axpby_rate = 24.0 * m / ms["axpby"]
    row = dict(samples=n, coils=C, virtual=V, bytes=nbytes, axpby_ms=ms["axpby"], axpby_TBps=axpby_rate / 1e9, mix_ms=ms["mix"],
               mix_TBps=nbytes / ms["mix"] / 1e9, mix_rate_of_axpby=(nbytes / ms["mix"]) / axpby_rate)
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--log2n", type=int, default=24, help="samples = 2^this")
    ap.add_argument("--coils", default="8,16,32,64")
    ap.add_argument("--slabs", default="4096,65536", help="slabs timed besides the backend's default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cc_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    n = 1 << a.log2n
    slabs = sorted(set([B.tuning['gram_slab']] + [int(s) for s in a.slabs.split(",") if s]))
    doc = dict(device=B.device_name(), warmup=a.warmup, reps=a.reps,
               gram=[gram_row(B, a, n, int(C), slabs) for C in a.coils.split(",")],
               mix=[mix_row(B, a, n, C, V) for C, V in ((32, 8), (64, 16))])
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
