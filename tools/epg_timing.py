#!/usr/bin/env python3
"""Device-event times of the extended-phase-graph simulation kernel (ig_epg_sim_c64, Backend.epg_signal) on the
MI355X, steady state after warm-up, medians over repeated calls, as one JSON document:

  * a fingerprinting train (`dictmatch.program_fisp`: an inversion and S = 1000 pulses of varying flip angle and repetition time) on
    N = 2^16 and 2^18 atoms with 32 and 64 states, and an 80-echo `program_fse` train with 81 states on 2^18 atoms, the parameters
    already on the device; the time includes the validation and the upload of the program, which every call repeats;
  * flop model: 74 real flops per step and live state -- 30 fused multiply-adds of the RF pulse, and 5 products and one fused
    multiply-add for each of the two delays -- with min(nstates, 1 + the shifts executed before the step) live states: the states
    above that are zero by definition and a kernel may skip them.  `lane_flops` counts what the kernel's layout issues instead: whole
    groups of W lanes, W = 16, 32 or 64 (two or four atoms share a wavefront up to 32 and 16 states);
  * comparator: the 157.3 Tflop/s float32 vector peak of the device, the fraction of it.

    python tools/epg_timing.py [--warmup 2] [--reps 5] [--log2n 16,18] [--pulses 1000] [--out profiles/epg_timing.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd import dictmatch  # noqa: E402
from indigo_amd.backends import get_backend  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from softsense_timing import medians  # noqa: E402

C64 = np.dtype('complex64')
PEAK_FP32_VECTOR = 157.3e12
FLOPS_PER_STATE_STEP = 74.0


def fisp_program(pulses):
    t = np.arange(pulses)
    flips = np.deg2rad(10 + 50 * np.sin(np.pi * t / 250.0) ** 2)
    tr = 0.012 + 0.002 * np.cos(2 * np.pi * t / 97.0)
    return dictmatch.program_fisp(flips, tr, 0.003, ti=0.02)


def live_states(flags, nstates, lanes=1):
    """sum over the steps of the live states, min(nstates, 1 + shifts so far), rounded up to a multiple of `lanes`"""
    shifts = np.concatenate([[0], np.cumsum([bin(int(f) & 3).count("1") for f in flags])[:-1]])
    live = np.minimum(nstates, 1 + shifts)
    return float((-(-live // lanes) * lanes).sum())


def row(B, a, name, steps, flags, nstates, N):
    rng = np.random.default_rng(N + nstates)
    t1 = rng.uniform(0.1, 3.0, N)
    cols = [B.copy_array(np.asfortranarray(c.astype(np.float32).reshape(-1, 1))) for c in (t1, rng.uniform(0.01, t1), rng.uniform(0.6, 1.3, N))]
    nrec = int(np.count_nonzero(flags & 4))
    sig = B.empty_array((nrec, N), C64)
    call = lambda: B._check(B._L.ig_epg_sim_c64(B._ctx, N, steps.shape[0], nstates, *(ctypes.c_void_p(c._arr) for c in cols),
                                                 ctypes.c_void_p(steps.ctypes.data), ctypes.c_void_p(flags.ctypes.data),
                                                 ctypes.c_void_p(sig._arr), sig._leading_dim), "ig_epg_sim_c64")
    ms = medians(B, {"kernel": call}, a.warmup, a.reps)["kernel"]
    flops = FLOPS_PER_STATE_STEP * live_states(flags, nstates) * N
    lane_flops = FLOPS_PER_STATE_STEP * live_states(flags, nstates, 16 if nstates <= 16 else 32 if nstates <= 32 else 64) * N
    out = dict(program=name, atoms=N, steps=int(steps.shape[0]), states=nstates, records=nrec, flops=flops, lane_flops=lane_flops, kernel_ms=ms,
               Tflops=flops / ms / 1e9, fraction_of_fp32_vector_peak=flops / ms / 1e-3 / PEAK_FP32_VECTOR, lane_Tflops=lane_flops / ms / 1e9,
               atoms_per_second=N / ms * 1e3)
    del cols, sig
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2n", default="16,18", help="atoms = 2^these")
    ap.add_argument("--pulses", type=int, default=1000, help="pulses of the fingerprinting train")
    ap.add_argument("--states", default="32,64", help="states of the fingerprinting train")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epg_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    fisp = fisp_program(a.pulses)
    fse = dictmatch.program_fse(0.006, np.full(80, np.deg2rad(150.0)))
    ns = [1 << int(v) for v in a.log2n.split(",")]
    rows = [row(B, a, "fisp", fisp[0], fisp[1], int(K), N) for N in ns for K in a.states.split(",")]
    rows.append(row(B, a, "fse", fse[0], fse[1], 81, ns[-1]))
    doc = dict(device=B.device_name(), warmup=a.warmup, reps=a.reps, fp32_vector_peak_Tflops=PEAK_FP32_VECTOR / 1e12,
               flops_per_state_and_step=FLOPS_PER_STATE_STEP, rows=rows)
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
