#!/usr/bin/env python3
"""Device-event times of the pieces of soft-SENSE (pics on a scan with several sets of coil maps) on the MI355X, steady state after
warm-up, medians over repeated calls, as one JSON document.  The headline problem (bench.py config 4: 256^3 image, 8 coils,
512^3 grid, half-width 2) with M = 2 sets of maps:

  * the per-voxel coil-map product and its adjoint (Backend.coil_maps, ig_coil_maps_c64) in the coil-major and in the
    coil-interleaved form, next to `axpby` on vectors of the same byte count.  Byte model: coil_maps moves every map, every coil
    image and every image once, 8 n (C M + C + M) bytes; axpby reads two vectors and writes one, 24 bytes per element.  The rates
    are the byte models over the times;
  * A^H A through the fused leaf operators.ZpadFFTMaps against (a) the single-map A^H A of the fused leaf and (b) the HStack of
    two single-map fused trees that share one gridding matrix on the host, all in one process, the three alternating.

    python tools/softsense_timing.py [--warmup 2] [--reps 9] [--img 256] [--out profiles/softsense_timing.json]
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

C64 = np.dtype('complex64')
M = 2


def call_ms(B, fn):
    """device time of one fn()"""
    e0, e1 = B.event(), B.event()
    B.record(e0)
    fn()
    B.record(e1)
    ms = B.elapsed_ms(e0, e1)
    B.event_destroy(e0)
    B.event_destroy(e1)
    return ms


def medians(B, fns, warmup, reps):
    """{name: median device time of fn()} over `reps` rounds that run the functions one after the other, after `warmup` rounds"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    B.barrier()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(call_ms(B, fn))
    return {name: float(np.median(t)) for name, t in times.items()}


def fill(B, rows, seed):
    rng = np.random.default_rng(seed)
    a = B.zero_array((rows, 1), C64)
    step = 1 << 24
    for lo in range(0, rows, step):
        hi = min(lo + step, rows)
        a.dense_rows(lo, hi)._copy_from(np.asfortranarray(rng.standard_normal((hi - lo, 2), dtype=np.float32).view(C64)))
    return a


def kernels(B, a, n, C):
    nbytes = 8.0 * n * (C * M + C + M)
    m = int(nbytes // 24)
    u, v = fill(B, m, 4), fill(B, m, 5)
    S, img, coil = fill(B, n * C * M, 1), fill(B, n * M, 2), fill(B, n * C, 3)
    fns = {"axpby": lambda: B.axpby(0.5, v, 0.5, u)}
    for form, il in (("coil_major", False), ("interleaved", True)):
        kw = dict(interleaved=il, width=C if il else None)
        fns[form + "_forward"] = lambda kw=kw: B.coil_maps(coil, img, S, n, C, M, **kw)
        fns[form + "_adjoint"] = lambda kw=kw: B.coil_maps(img, coil, S, n, C, M, adjoint=True, **kw)
    ms = medians(B, fns, a.warmup, a.reps)
    axpby_rate = 24.0 * m / ms["axpby"]
    row = dict(voxels=n, coils=C, sets=M, bytes=nbytes, axpby_elements=m, axpby_ms=ms["axpby"], axpby_TBps=axpby_rate / 1e9)
    for name, t in ms.items():
        if name != "axpby":
            row.update({name + "_ms": t, name + "_TBps": nbytes / t / 1e9, name + "_rate_of_axpby": (nbytes / t) / axpby_rate})
    print(json.dumps(row), flush=True)
    return row


def normal_operators(B, a, p):
    from indigo_amd.analyses import ScratchUsage
    from indigo_amd.sense import SenseProblem, normal_operator
    from indigo_amd.transforms import reserve_for
    N, C = int(np.prod(p.N)), p.C
    maps = np.empty(tuple(p.N) + (C, M), dtype=C64, order='F')
    for m in range(M):
        for c in range(C):
            maps[..., c, m] = rand64c(*p.N, seed=[40 + m, c])
    singles = []
    for m in range(M):
        q = SenseProblem(p.N, p.coord, maps[..., m], width=p.width, ntable=p.ntable, oversamp=p.oversamp)
        q._interp_cache = p._interp_cache
        singles.append(q.build_zpadfft(B))
    AHA1 = normal_operator(singles[0], lamda=0.0)
    H = B.HStack(singles, name='HStack of single-map trees')
    AHAh = H.H * H
    A = p.build_zpadfft_maps(B, maps)
    AHAm = A.H * A
    B._scratch = None
    reserve_for(max((AHA1, AHAh, AHAm), key=lambda node: ScratchUsage().measure(node, 1)), 1, slack_products=6)
    x1, y1 = fill(B, N, 6), B.zero_array((N, 1), C64)
    x, yh, ym = fill(B, N * M, 7), B.zero_array((N * M, 1), C64), B.zero_array((N * M, 1), C64)
    fns = {"single_map_aha": lambda: AHA1.eval(y1, x1), "hstack_aha": lambda: AHAh.eval(yh, x), "zpadfftmaps_aha": lambda: AHAm.eval(ym, x)}
    ms = medians(B, fns, a.warmup, a.reps)
    ref = yh.to_host()
    diff = float(np.linalg.norm(ref - ym.to_host()) / np.linalg.norm(ref))
    row = dict(problem="bench config 4: image %s, %d coils, oversampling %g (grid %s), half-width %g, %d sets of maps"
               % (tuple(p.N), C, p.oversamp, tuple(p.oN), p.width, M),
               single_map_aha_ms=ms["single_map_aha"], hstack_aha_ms=ms["hstack_aha"], zpadfftmaps_aha_ms=ms["zpadfftmaps_aha"],
               zpadfftmaps_over_hstack=ms["zpadfftmaps_aha"] / ms["hstack_aha"], zpadfftmaps_over_single_map=ms["zpadfftmaps_aha"] / ms["single_map_aha"],
               relative_difference_to_hstack=diff)
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--img", type=int, default=256, help="image edge (256: the headline problem)")
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--no-operators", action="store_true", help="only the kernel table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softsense_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), warmup=a.warmup, reps=a.reps, kernels=kernels(B, a, a.img ** 3, a.coils))
    if not a.no_operators:
        import bench
        doc["normal_operator"] = normal_operators(B, a, bench.sense_problem(4, a.img, a.coils))
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
