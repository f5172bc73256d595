#!/usr/bin/env python3
"""Device-event times of the pieces of pics --l1 on the MI355X, steady state after warm-up, as one JSON document:

  * the wavelet transform in place (forward, inverse; Backend.dwt3) and the soft threshold (Backend.soft_threshold) for each
    filter at 256^3, 480 x 208 x 308 and 512^3, 3 levels.  A 256^3 complex64 volume (134 MB) fits in the 256 MiB Infinity
    Cache; the other two do not.  Byte model: every split pass reads and writes its box once (16 B per complex element); the
    threshold reads and writes the volume once.  Rates are given against 8 TB/s;
  * one FISTA iteration of pics --l1 (db2, 3 levels) against one A^H A evaluation on the headline problem (bench.py config 4:
    256^3 image, 8 coils, 512^3 grid).

    python tools/fista_timing.py [--warmup 3] [--steps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd.backends import get_backend  # noqa: E402
from indigo_amd.backends.backend import dwt_plan  # noqa: E402
from indigo_amd.util import rand64c  # noqa: E402

C64 = np.dtype('complex64')
PEAK = 8e12


def event_ms(B, fn, warmup, steps):
    """mean device time of fn() over `steps` back-to-back calls, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    B.barrier()
    e0, e1 = B.event(), B.event()
    B.record(e0)
    for _ in range(steps):
        fn()
    B.record(e1)
    ms = B.elapsed_ms(e0, e1) / steps
    B.event_destroy(e0)
    B.event_destroy(e1)
    return ms


def transforms(B, a):
    out = []
    for dims in [(256, 256, 256), (480, 208, 308), (512, 512, 512)]:
        n = int(np.prod(dims))
        x = B.copy_array(rand64c(n, 1, seed=1))
        for wavelet in ("haar", "db2", "db4"):
            passes, coarse = dwt_plan(dims, wavelet, 3)
            nbytes = 16.0 * sum(int(np.prod(box)) for box, _ in passes)
            row = dict(dims=dims, wavelet=wavelet, levels=3, coarse=coarse, passes=len(passes), model_bytes=nbytes)
            for name, inverse in (("forward", False), ("inverse", True)):
                ms = event_ms(B, lambda: B.dwt3(x, x, dims, wavelet, 3, inverse=inverse), a.warmup, a.steps)
                row[name + "_ms"] = ms
                row[name + "_TBps"] = nbytes / ms / 1e9
                row[name + "_of_8TBps"] = nbytes / ms / 1e-3 / PEAK
            ms = event_ms(B, lambda: B.soft_threshold(x, 0.0, dims, coarse), a.warmup, a.steps)
            row.update(soft_ms=ms, soft_TBps=16.0 * n / ms / 1e9, soft_of_8TBps=16.0 * n / ms / 1e-3 / PEAK)
            print(json.dumps(row), flush=True)
            out.append(row)
        del x
    return out


def iteration(B, a):
    """one FISTA iteration of pics --l1 against one A^H A on bench.py's config 4 problem"""
    sys.path.insert(0, ROOT)
    import bench
    from indigo_amd.sense import normal_operator
    p = bench.sense_problem(4, 256, 8)
    A = p.build_zpadfft(B)
    AHA = normal_operator(A, lamda=1e-3)
    n = AHA.shape[1]
    dims = tuple(p.N)
    x = B.copy_array(rand64c(n, 1, seed=2))
    y = B.zero_array((n, 1), C64)
    aha_ms = event_ms(B, lambda: AHA.eval(y, x), a.warmup, a.steps)
    W = B.Wavelet(dims, wavelet='db2', levels=3)
    b = B.copy_array(rand64c(n, 1, seed=3))

    def gradf(g, z):
        AHA.eval(g, z)
        B.axpby(1, g, -1, b)

    def proxg(v, alpha):
        W.eval(v, v)
        B.soft_threshold(v, alpha * 0.01, dims, W.coarse)
        W.H.eval(v, v)

    z, g = x.copy(), x.copy()
    prox_ms = event_ms(B, lambda: proxg(z, 0.1), a.warmup, a.steps)
    axpby_ms = event_ms(B, lambda: B.axpby(-0.5, z, 1.5, g), a.warmup, a.steps)
    B.fista(gradf, proxg, 0.1, x, maxiter=a.warmup)            # (the solver's buffers and the leaf's formats: warm)
    fista_ms = event_ms(B, lambda: B.fista(gradf, proxg, 0.1, x, maxiter=a.steps), 0, 1) / a.steps
    row = dict(problem="bench config 4: image %s, 8 coils, oversampling 2 (grid 512^3)" % (dims,),
               device=B.device_name(), aha_ms=aha_ms, fista_iteration_ms=fista_ms, ratio=fista_ms / aha_ms,
               prox_ms=prox_ms, axpby_ms=axpby_ms, coarse=W.coarse)
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), transforms=transforms(B, a), fista=iteration(B, a))
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
