#!/usr/bin/env python3
"""Device-event times of the density-compensation kernels (ig_dcf.hip) on the MI355X, steady state after warm-up,
medians over repeated calls, as one JSON document:

  * spread (ig_dcf_spread_r32) and gather-and-divide (ig_dcf_gather_div_r32) for 2^24 radial samples on a 512^3 grid at half-widths
    2 and 3, with tuning['dcf_lds_min'] at 0 (every tile through LDS), at the default and at 2^31 (every add straight to the grid).
    The route without LDS issues one 8-byte global atomic per tap: its atomic bytes per second stand next to the 1.3 TB/s of added
    bytes that float atomics reach on this device;
  * thirty iterations of `dcf.pipe_menon` on the same trajectory: wall time with the host set-up (records, tiles), and the device
    part alone;
  * the route the library offered before: `B.Interp(...)`, its adjoint and forward on ONE complex64 column, on 2^(--interp-log2m)
    samples of the same kind (its CSR matrix holds 12 bytes per tap: 43 GB at 2^24 samples and half-width 3), with the new kernels
    timed on those samples as well;
  * `row_scale` on 2^24 samples x 8 coils against `axpby` on as many bytes.

    python tools/dcf_timing.py [--warmup 2] [--reps 5] [--log2m 24] [--interp-log2m 20] [--out profiles/dcf_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from scipy.signal.windows import kaiser  # noqa: E402

from indigo_amd import dcf  # noqa: E402
from indigo_amd.backends import get_backend  # noqa: E402
from indigo_amd.interp import interp_sep_records  # noqa: E402
from indigo_amd.sense import radial_trajectory  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from softsense_timing import fill, medians  # noqa: E402

C64 = np.dtype('complex64')
FLOAT_ATOMIC_TBPS = 1.3
DIMS, OSF, NRO = (384, 384, 384), 640 / 480, 512           # int(384 * 640 / 480) = 512


def setup(B, coord, width):
    grid = tuple(int(n * OSF) for n in DIMS)
    beta = B.nufft_params(width, (OSF,) * 3)[1]
    kb = kaiser(2 * 128 + 1, beta)[128:]
    t0 = time.perf_counter()
    sep = interp_sep_records(coord.shape[1], grid, width, kb, coord)
    rec, desc, tiles = dcf.upload(B, sep)
    host_s = time.perf_counter() - t0
    counts = np.diff(tiles['ptr'].to_host().ravel())
    return grid, kb, sep, rec, desc, tiles, host_s, counts


def kernel_rows(B, a, coord, width, thresholds):
    """spread and gather times for every threshold; the taps are counted from the records"""
    M = coord.shape[1]
    grid, kb, sep, rec, desc, tiles, host_s, counts = setup(B, coord, width)
    tw, r = sep['tw'], sep['records']
    h1 = r[:, 3 * tw + 1]
    taps = float((((h1 >> 16) & 15).astype(np.int64) * ((h1 >> 20) & 15) * ((h1 >> 24) & 15)).sum())
    w = B.copy_array(np.ones(M, dtype=np.float32))
    out = B.copy_array(np.ones(M, dtype=np.float32))
    acc = B.zero_array((int(np.prod(grid)),), np.dtype('int64'))
    scale = dcf.scale_for(M, 1.0)
    rows = []
    old = B.tuning['dcf_lds_min']
    try:
        for lds_min in thresholds:
            B.tuning['dcf_lds_min'] = lds_min
            ms = medians(B, {"spread": lambda: B.dcf_spread(acc, w, rec, desc, scale, tiles),
                             "gather": lambda: B.dcf_gather_div(out, acc, w, rec, desc, scale, tiles)}, a.warmup, a.reps)
            row = dict(samples=M, half_width=width, tw=tw, grid=grid, taps=taps, tiles=int(counts.size), largest_tile=int(counts.max()),
                       tiles_through_lds=int((counts >= lds_min).sum()), dcf_lds_min=lds_min, spread_ms=ms["spread"], gather_ms=ms["gather"],
                       spread_Gtaps_per_s=taps / ms["spread"] / 1e6, gather_Gtaps_per_s=taps / ms["gather"] / 1e6, host_setup_s=host_s)
            if lds_min >= M:
                row["atomic_TBps"] = 8.0 * taps / ms["spread"] / 1e9
                row["float_atomic_TBps_of_the_guide"] = FLOAT_ATOMIC_TBPS
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        B.tuning['dcf_lds_min'] = old
    return rows, (grid, kb)


def interp_row(B, a, coord, width, grid, kb):
    """B.Interp's adjoint and forward on one complex64 column"""
    try:
        M = coord.shape[1]
        t0 = time.perf_counter()
        G = B.Interp(grid, coord.reshape((3, M, 1)), width, kb, dtype=np.float32, name='interp')
        x, y = fill(B, int(np.prod(grid)), 1), fill(B, M, 2)
        G.eval(y, x)                                            # (builds and uploads the matrix)
        G.H.eval(x, y)
        build_s = time.perf_counter() - t0
        ms = medians(B, {"forward": lambda: G.eval(y, x), "adjoint": lambda: G.H.eval(x, y)}, a.warmup, a.reps)
        return dict(samples=M, half_width=width, interp_forward_ms=ms["forward"], interp_adjoint_ms=ms["adjoint"], interp_setup_s=build_s)
    except Exception as e:  # the comparator is not the product: record why it did not run
        return dict(samples=coord.shape[1], half_width=width, interp_error="%s: %s" % (type(e).__name__, e))


def rowscale_row(B, a, n, C):
    nbytes = 16.0 * n * C + 4.0 * n
    m = int(nbytes // 24)
    x, w = fill(B, n * C, 1), B.copy_array(np.random.default_rng(0).random(n, dtype=np.float32))
    u, v = fill(B, m, 2), fill(B, m, 3)
    ms = medians(B, {"row_scale": lambda: B.row_scale(x, x, w, n, C), "axpby": lambda: B.axpby(0.5, v, 0.5, u)}, a.warmup, a.reps)
    return dict(samples=n, coils=C, bytes=nbytes, row_scale_ms=ms["row_scale"], row_scale_TBps=nbytes / ms["row_scale"] / 1e9,
                axpby_elements=m, axpby_ms=ms["axpby"], axpby_TBps=24.0 * m / ms["axpby"] / 1e9)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2m", type=int, default=24, help="samples = 2^this")
    ap.add_argument("--interp-log2m", type=int, default=20, help="samples of the B.Interp comparison = 2^this (0: leave it out)")
    ap.add_argument("--widths", default="2,3")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcf_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    default = int(B.tuning['dcf_lds_min'])
    thresholds = sorted({0, default, 1 << 31})
    M = 1 << a.log2m
    coord = np.ascontiguousarray(radial_trajectory(M // NRO, NRO).reshape((3, -1), order='F'))
    doc = dict(device=B.device_name(), warmup=a.warmup, reps=a.reps, default_dcf_lds_min=default, kernels=[], comparison=[])
    for width in (int(v) for v in a.widths.split(",")):
        rows, _ = kernel_rows(B, a, coord, width, thresholds)
        doc["kernels"] += rows
    # thirty iterations: wall time with the host set-up, and the device part from the kernel times above
    t0 = time.perf_counter()
    dcf.pipe_menon(B, coord.reshape((3, NRO, -1), order='F'), DIMS, width=3, osf=OSF, iters=a.iters)
    B.barrier()
    at_default = [r for r in doc["kernels"] if r["half_width"] == 3 and r["dcf_lds_min"] == default]
    doc["pipe_menon"] = dict(samples=M, half_width=3, iterations=a.iters, wall_s=time.perf_counter() - t0,
                             device_s=a.iters * (at_default[0]["spread_ms"] + at_default[0]["gather_ms"]) / 1e3 if at_default else None)
    print(json.dumps(doc["pipe_menon"]), flush=True)
    if a.interp_log2m > 0:
        m = 1 << a.interp_log2m
        small = np.ascontiguousarray(radial_trajectory(m // NRO, NRO).reshape((3, -1), order='F'))
        for width in (int(v) for v in a.widths.split(",")):
            rows, (grid, kb) = kernel_rows(B, a, small, width, [default])
            row = dict(rows[0], **interp_row(B, a, small, width, grid, kb))
            if "interp_adjoint_ms" in row:
                row["interp_adjoint_over_spread"] = row["interp_adjoint_ms"] / row["spread_ms"]
                row["interp_forward_over_gather"] = row["interp_forward_ms"] / row["gather_ms"]
            print(json.dumps(row), flush=True)
            doc["comparison"].append(row)
    doc["row_scale"] = rowscale_row(B, a, M, 8)
    print(json.dumps(doc["row_scale"]), flush=True)
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
