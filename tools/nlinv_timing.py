#!/usr/bin/env python3
"""Device-event times of the pieces of NLINV (indigo_amd.nlinv) on the MI355X, steady state after warm-up, medians over repeated
calls, as one JSON document.  A 256^3 image and 8 coils:

  * the linearised coil product and its adjoint (Backend.nlinv_product, ig_nlinv_product_c64) and the weight pass on the 8 coil
    volumes (Backend.sobolev_weight, ig_sobolev_weight_c64), each next to `axpby` on vectors of the same byte count.  Byte models:
    the product moves rho, the coils, x and y once, 8 n (3 C + 2) bytes either way; the weight pass reads and writes every element,
    16 n C bytes; axpby reads two vectors and writes one, 24 bytes per element.  The rates are the byte models over the times;
  * ten CG iterations of DF^H DF = (A NlinvProduct SobolevCoils)^H (A NlinvProduct SobolevCoils) against ten of A^H A alone,
    A = KronI(8, NUFFT) on a radial trajectory, through `Backend.cg`, per iteration.

    python tools/nlinv_timing.py [--warmup 2] [--reps 9] [--img 256] [--out profiles/nlinv_timing.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd.backends import get_backend  # noqa: E402
from tools.softsense_timing import fill, medians  # noqa: E402

C64 = np.dtype('complex64')
CG_ITERS = 10


def kernels(B, a, dims, C):
    n = int(np.prod(dims))
    pbytes, wbytes = 8.0 * n * (3 * C + 2), 16.0 * n * C
    mp, mw = int(pbytes // 24), int(wbytes // 24)
    u, v = fill(B, mp, 4), fill(B, mp, 5)
    rho, coils, wide, narrow = fill(B, n, 1), fill(B, n * C, 2), fill(B, n * (1 + C), 3), fill(B, n * C, 6)
    fns = {"axpby_product_bytes": lambda: B.axpby(0.5, v, 0.5, u),
           "axpby_weight_bytes": lambda: B.axpby(0.5, v.dense_rows(0, mw), 0.5, u.dense_rows(0, mw)),
           "product_forward": lambda: B.nlinv_product(narrow, wide, rho, coils, n, C),
           "product_adjoint": lambda: B.nlinv_product(wide, narrow, rho, coils, n, C, adjoint=True),
           "sobolev_weight": lambda: B.sobolev_weight(narrow, coils, dims, C, 220.0, 32.0, scale=1.0 / np.sqrt(n)),
           "sobolev_weight_in_place": lambda: B.sobolev_weight(narrow, narrow, dims, C, 0.0, 32.0, scale=1.0)}
    ms = medians(B, fns, a.warmup, a.reps)
    rate_p, rate_w = 24.0 * mp / ms["axpby_product_bytes"], 24.0 * mw / ms["axpby_weight_bytes"]
    row = dict(dims=list(dims), coils=C, product_bytes=pbytes, weight_bytes=wbytes, axpby_product_bytes_ms=ms["axpby_product_bytes"],
               axpby_weight_bytes_ms=ms["axpby_weight_bytes"], axpby_TBps=rate_p / 1e9)
    for name, nbytes, rate in (("product_forward", pbytes, rate_p), ("product_adjoint", pbytes, rate_p), ("sobolev_weight", wbytes, rate_w),
                               ("sobolev_weight_in_place", wbytes, rate_w)):
        row.update({name + "_ms": ms[name], name + "_TBps": nbytes / ms[name] / 1e9, name + "_rate_of_axpby": (nbytes / ms[name]) / rate})
    print(json.dumps(row), flush=True)
    return row


def cg_iterations(B, a, dims, C):
    from indigo_amd.sense import radial_trajectory
    from indigo_amd.transforms import reserve_for
    n = int(np.prod(dims))
    coord = radial_trajectory(a.spokes, a.readout, seed=2)
    A = B.KronI(C, B.NUFFT((1, a.readout, a.spokes), dims, coord, width=2, oversamp=(a.osf,) * 3, dtype=C64))
    P, S = B.NlinvProduct(n, C), B.SobolevCoils(dims, C, 220.0, 32.0)
    DF = A * P * S
    DFHDF, AHA = DF.H * DF, A.H * A
    B._scratch = None
    reserve_for(DFHDF, 1, slack_products=6)
    point = fill(B, n * (1 + C), 7)
    P.set_point(point.dense_rows(0, n), point.dense_rows(n, n * (1 + C)))
    rhs_u, rhs_x = fill(B, n * (1 + C), 8), fill(B, n * C, 9)
    du, dx = B.zero_array((n * (1 + C), 1), C64), B.zero_array((n * C, 1), C64)

    def run(op, rhs, x):
        x._zero()
        B.cg(op, rhs, x, lamda=1.0, maxiter=CG_ITERS, tol=0.0)
    fns = {"nlinv_cg": lambda: run(DFHDF, rhs_u, du), "nufft_cg": lambda: run(AHA, rhs_x, dx)}
    ms = medians(B, fns, max(1, a.warmup // 2), max(3, a.reps // 3))
    row = dict(problem="image %s, %d coils, radial %d x %d, oversampling %g, half-width 2" % (tuple(dims), C, a.readout, a.spokes, a.osf),
               cg_iterations=CG_ITERS, nlinv_cg_iteration_ms=ms["nlinv_cg"] / CG_ITERS, nufft_cg_iteration_ms=ms["nufft_cg"] / CG_ITERS,
               nlinv_over_nufft=ms["nlinv_cg"] / ms["nufft_cg"])
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--img", type=int, default=256, help="image edge")
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--readout", type=int, default=256)
    ap.add_argument("--spokes", type=int, default=2000)
    ap.add_argument("--osf", type=float, default=1.25)
    ap.add_argument("--no-operators", action="store_true", help="only the kernel table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlinv_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    dims = (a.img,) * 3
    doc = dict(device=B.device_name(), warmup=a.warmup, reps=a.reps, kernels=kernels(B, a, dims, a.coils))
    if not a.no_operators:
        doc["cg"] = cg_iterations(B, a, dims, a.coils)
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
