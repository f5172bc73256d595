#!/usr/bin/env python3
"""Device-event times of the field-map estimator's hot path on the MI355X, steady state after warm-up, as one JSON document:

  * Backend.fieldmap_step at 256^3, 480 x 208 x 308 and 512^3 with E = 2, 3, 4 echoes: the plain step, the step with the fused cost
    (launch only: the partial sums are not fetched, so that the kernels are compared and not the read-back), the cost alone, and
    the composition step + cost alone that the fusion replaces.  Byte model per voxel: 8 E + 8 for a step with or
    without the cost, 8 E + 4 for the cost alone;
  * next to each, the backend's own axpby on a vector of as many bytes as the step moves (24 bytes per element), the streaming
    yardstick;
  * 200 iterations of indigo_amd.fmapest.estimate end to end (upload, initial field, steps, the cost every 10 iterations with its
    read-back, download), wall clock.

Every figure is the median over `--reps` blocks of `--steps` back-to-back launches.  Run in a fresh process.

    python tools/fmapest_timing.py [--warmup 3] [--steps 20] [--reps 5] [--out profiles/fmapest_timing.json]
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

from indigo_amd import fmapest  # noqa: E402
from indigo_amd.backends import get_backend  # noqa: E402

C64 = np.dtype('complex64')
F32 = np.dtype('float32')
TE = [0.002, 0.004, 0.0065, 0.0095]


def event_ms(B, fn, warmup, steps, reps):
    """median over `reps` blocks of the mean device time of fn() over `steps` back-to-back calls, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    B.barrier()
    e0, e1 = B.event(), B.event()
    blocks = []
    for _ in range(reps):
        B.record(e0)
        for _ in range(steps):
            fn()
        B.record(e1)
        blocks.append(B.elapsed_ms(e0, e1) / steps)
    B.event_destroy(e0)
    B.event_destroy(e1)
    return float(np.median(blocks))


def echoes(dims, E, seed=0):
    """E echo images of a smooth object under a smooth field with noise, (n, E) complex64, made plane by plane"""
    rng = np.random.default_rng(seed)
    g = [np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in dims]
    out = np.empty((int(np.prod(dims)), E), dtype=C64, order='F')
    vol = out.reshape(dims + (E,), order='F')
    for k in range(dims[2]):
        x, y = g[0][:, None], g[1][None, :]
        field = 120.0 * (0.6 * x + 0.5 * y ** 2 - 0.4 * g[2][k] * x + 0.3 * np.sin(2.0 * g[2][k]))
        mag = np.where(x ** 2 + y ** 2 + g[2][k] ** 2 < 0.7, 1.0, 0.02).astype(np.float32)
        for l in range(E):
            noise = (rng.standard_normal(dims[:2], dtype=np.float32) + 1j * rng.standard_normal(dims[:2], dtype=np.float32)) * np.float32(0.035)
            vol[:, :, k, l] = mag * np.exp(-2j * np.pi * TE[l] * field).astype(C64) + noise
    return out


def launch_only(B, f_new, f_old, y, te, beta, dims, n, E, cost_buf):
    """the step with the fused cost (f_new given) or the cost alone (f_new None) without the read-back of the partial sums"""
    yp, ldy = B._frame_panel(y, n, E)
    B._check(B._L.ig_fmapest_step_r32(B._ctx, *dims, E, yp, ldy, ctypes.c_void_p(te.ctypes.data), ctypes.c_float(beta),
                                      ctypes.c_void_p(f_old._arr), ctypes.c_void_p(f_new._arr) if f_new is not None else None,
                                      ctypes.c_void_p(cost_buf._arr), cost_buf.size), "ig_fmapest_step_r32")


def kernels(B, a):
    out = []
    for dims in [(256, 256, 256), (480, 208, 308), (512, 512, 512)]:
        n = int(np.prod(dims))
        host = echoes(dims, 4)
        host /= np.abs(host[:, 0]).max()
        panel = B.copy_array(host)
        parts = B.zero_array((int(B._L.ig_fmapest_cost_parts(*dims)),), np.dtype('float64'))
        f, g = B.zero_array((n,), F32), B.zero_array((n,), F32)
        for E in (2, 3, 4):
            te = np.ascontiguousarray(TE[:E], dtype=np.float64)
            y = panel[:, :E]
            beta = float(np.float32(0.1 * fmapest.relative_beta_scale(host[::97, :E], te)))
            B.fieldmap_init(f, y, dims, te)
            for _ in range(5):                              # a few steps in: the iterate the loop spends its time on
                B.fieldmap_step(g, f, y, te, beta, dims)
                f, g = g, f
            nbytes = (8.0 * E + 8.0) * n
            m = int(nbytes // 24)
            ax, ay = B.zero_array((m, 1), C64), B.zero_array((m, 1), C64)
            row = dict(dims=dims, E=E, beta=beta, bytes_per_voxel=8 * E + 8)
            timed = (("step", lambda: B.fieldmap_step(g, f, y, te, beta, dims)),
                     ("step_cost", lambda: launch_only(B, g, f, y, te, beta, dims, n, E, parts)),
                     ("cost", lambda: launch_only(B, None, f, y, te, beta, dims, n, E, parts)),
                     ("composed", lambda: (B.fieldmap_step(g, f, y, te, beta, dims), launch_only(B, None, f, y, te, beta, dims, n, E, parts))),
                     ("axpby", lambda: B.axpby(0.5, ay, 0.25, ax)))
            for name, fn in timed:
                row[name + "_ms"] = event_ms(B, fn, a.warmup, a.steps, a.reps)
            for name in ("step", "step_cost", "axpby"):
                row[name + "_TBps"] = nbytes / row[name + "_ms"] / 1e9
            row["step_of_axpby"] = row["axpby_ms"] / row["step_ms"]
            row["step_cost_of_axpby"] = row["axpby_ms"] / row["step_cost_ms"]
            row["composed_over_fused"] = row["composed_ms"] / row["step_cost_ms"]
            row["ns_per_voxel_pair"] = 1e6 * row["step_ms"] / (n * (E * (E - 1) // 2))
            del ax, ay
            t0 = time.perf_counter()
            fmapest.estimate(B, host[:, :E].reshape(dims + (E,), order='F'), te, iters=200, beta=0.1, cost_every=10)
            row["estimate_200_s"] = time.perf_counter() - t0
            print(json.dumps(row), flush=True)
            out.append(row)
        del panel, parts, f, g, host
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), warmup=a.warmup, steps=a.steps, reps=a.reps, kernels=kernels(B, a))
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
