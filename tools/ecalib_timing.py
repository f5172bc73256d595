#!/usr/bin/env python3
"""Device-event times of the image-resolution part of ESPIRiT calibration (indigo_amd.ecalib) on the MI355X, steady
state after warm-up, medians over repeated calls, as one JSON document.  The headline size: 256^3 voxels, 8 coils, 2 sets of maps,
kernel 6, calibration block 24^3 cut from the transform of a synthetic object seen through 8 smooth coils (the projector and the
correlation boxes are built once on the host and not timed):

  * the evaluation of G(x): `Backend.place_wrapped` of the C (C + 1) / 2 = 36 boxes and 36 unnormalised inverse transforms in place;
  * `Backend.espirit_eig` on that panel (ig_espirit_eig_c64), next to `axpby` on vectors of the same byte count.  Byte model:
    8 (C (C + 1) / 2 + C M) + 4 M bytes per voxel; the rate is the byte model over the time.  The sweep count of the Jacobi kernel
    depends on the matrices, so the panel is the pipeline's own, not random numbers.

    python tools/ecalib_timing.py [--warmup 1] [--reps 5] [--img 256] [--coils 8] [--out profiles/ecalib_timing.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd import ecalib  # noqa: E402
from indigo_amd.backends import get_backend  # noqa: E402

C64 = np.dtype('complex64')


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
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    B.barrier()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(call_ms(B, fn))
    return {name: float(np.median(t)) for name, t in times.items()}


def calibration_block(C, side=24, small=48):
    """the central block of the transform of a Gaussian-edged object seen through C smooth coils, on a small grid"""
    g = np.mgrid[tuple(slice(-1, 1, small * 1j) for _ in range(3))]
    obj = (np.sqrt(g[0] ** 2 + 1.3 * g[1] ** 2 + 0.8 * g[2] ** 2) < 0.7) * (1 + 0.4 * np.cos(5 * g[0]) * np.sin(4 * g[1] + g[2]))
    coils = []
    for c in range(C):
        a = 2 * np.pi * c / C
        d2 = (g[0] - 1.2 * np.cos(a)) ** 2 + (g[1] - 1.2 * np.sin(a)) ** 2 + (g[2] - 0.5 * (-1) ** c) ** 2
        coils.append(np.exp(-0.6 * d2) * np.exp(1j * (a + 0.5 * g[c % 3])))
    img = np.stack(coils, axis=-1) * obj[..., None]
    ax = (0, 1, 2)
    ksp = np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(img, axes=ax), axes=ax), axes=ax)
    lo = small // 2 - side // 2
    return ksp[lo:lo + side, lo:lo + side, lo:lo + side]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("-k", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecalib_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    C, M, dims = a.coils, a.sets, (a.img,) * 3
    N = a.img ** 3
    P, kdims = ecalib.projector(calibration_block(C), a.k, 0.001)
    R = ecalib.correlation_boxes(P, kdims, C)
    bdims = R.shape[:3]
    pairs = [(p, q) for p in range(C) for q in range(p, C)]
    phase = 1
    for ax in range(3):
        delta = np.arange(bdims[ax]) - (bdims[ax] // 2)
        phase = phase * np.exp(-2j * np.pi * delta * (dims[ax] // 2) / dims[ax]).reshape([-1 if j == ax else 1 for j in range(3)])
    boxes = np.stack([(R[..., p, q] * phase / np.prod(kdims)).reshape(-1, order='F') for p, q in pairs], axis=1)

    B = get_backend("hip")
    box_d = B.copy_array(np.asfortranarray(boxes.astype(C64)))
    G = B.empty_array((N, len(pairs)), C64, name='G')
    maps = B.empty_array((N, C * M), C64, name='maps')
    evals = B.empty_array((N, M), np.dtype('float32'), name='evals')
    cols = [G[:, j:j + 1].reshape(dims + (1,)) for j in range(len(pairs))]

    def evaluate():
        B.place_wrapped(G, box_d, dims, bdims)
        for col in cols:
            B.ifftn(col, col)

    nbytes = N * (8.0 * (len(pairs) + C * M) + 4.0 * M)
    m = int(nbytes // 24)
    u, v = B.zero_array((m, 1), C64), B.zero_array((m, 1), C64)
    fns = {"place_wrapped": lambda: B.place_wrapped(G, box_d, dims, bdims),
           "g_evaluation": evaluate,
           "espirit_eig": lambda: B.espirit_eig(maps, evals, G, N, C, M, iters=a.iters, crop=0.8),
           "axpby": lambda: B.axpby(0.5, v, 0.5, u)}
    ms = medians(B, fns, a.warmup, a.reps)
    ev = evals.to_host()
    doc = dict(device=B.device_name(), warmup=a.warmup, reps=a.reps, image=list(dims), coils=C, sets=M, kernel=list(kdims), iters=a.iters,
               g_bytes=8.0 * N * len(pairs), place_wrapped_ms=ms["place_wrapped"], g_evaluation_ms=ms["g_evaluation"],
               g_evaluation_transforms=len(pairs), espirit_eig_ms=ms["espirit_eig"], espirit_eig_bytes=nbytes,
               espirit_eig_TBps=nbytes / ms["espirit_eig"] / 1e9, espirit_eig_ns_per_voxel=1e6 * ms["espirit_eig"] / N,
               axpby_ms=ms["axpby"], axpby_TBps=24.0 * m / ms["axpby"] / 1e9,
               espirit_eig_rate_of_axpby=(nbytes / ms["espirit_eig"]) / (24.0 * m / ms["axpby"]),
               lambda_1_mean=float(ev[:, 0].mean()), lambda_1_max=float(ev[:, 0].max()), share_above_crop=float((ev[:, 0] >= 0.8).mean()))
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
