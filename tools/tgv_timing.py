#!/usr/bin/env python3
"""Device-event times of the pieces of pics --tgv on the MI355X, steady state after warm-up, as one JSON document:

  * the symmetrised gradient, its adjoint and the two fused passes (Backend.symgrad3 / tgv_adjoint / tgv_dual_step) at 256^3,
    480 x 208 x 308 and 512^3, next to the backend's own axpby on one volume of the same size as the streaming yardstick.  Byte
    model per voxel: symgrad 72 B, symgradh 72 B, K^H 112 B, dual step 208 B, axpby 24 B;
  * the two fused passes against the same step composed from the stand-alone entries, in the same run: K^H as grad3 (adjoint,
    beta = 1), symgrad3 (adjoint) and one axpby; the dual step as two grad3, two axpby and two symgrad3 with beta = 1, which is the
    step without its projections (the composition is spared them);
  * one primal-dual iteration of pics --tgv against one A^H A evaluation on the headline problem (bench.py config 4: 256^3 image,
    8 coils, 512^3 grid).

    python tools/tgv_timing.py [--warmup 3] [--steps 20] [--out profiles/tgv_timing.json]
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


def field(B, src, comps, scale):
    """a device vector of `comps` copies of the volume src, scaled: the random content of v, p and q without a host array of their size"""
    n = src.shape[0]
    out = B.zero_array((comps * n, 1), C64)
    for c in range(comps):
        out.dense_rows(c * n, (c + 1) * n).copy(src)
    B.scale(out, scale)
    return out


def kernels(B, a):
    out = []
    for dims in [(256, 256, 256), (480, 208, 308), (512, 512, 512)]:
        n = int(np.prod(dims))
        x = B.copy_array(rand64c(n, 1, seed=1))
        xo = B.copy_array(rand64c(n, 1, seed=2))
        v, vo, p, q = field(B, x, 3, 0.5), field(B, xo, 3, 0.25), field(B, xo, 3, 0.125), field(B, x, 6, 0.125)
        gv, e = B.zero_array((3 * n, 1), C64), B.zero_array((6 * n, 1), C64)
        sigma, a1, a0 = 0.5, 0.2, 0.4

        def kh_composed():
            B.grad3(xo, p, dims, adjoint=True, alpha=1, beta=1)
            B.symgrad3(gv, q, dims, adjoint=True)
            B.axpby(1, gv, -1, p)

        def dual_composed():                               # p += sigma (D w_x - w_v), q += sigma E w_v, w = 2 new - old; no projection
            B.grad3(p, x, dims, alpha=2 * sigma, beta=1)
            B.grad3(p, xo, dims, alpha=-sigma, beta=1)
            B.axpby(1, p, -2 * sigma, v)
            B.axpby(1, p, sigma, vo)
            B.symgrad3(q, v, dims, alpha=2 * sigma, beta=1)
            B.symgrad3(q, vo, dims, alpha=-sigma, beta=1)

        row = dict(dims=dims)
        for name, nbytes, fn in (("symgrad", 72.0, lambda: B.symgrad3(e, v, dims)),
                                 ("symgradh", 72.0, lambda: B.symgrad3(gv, q, dims, adjoint=True)),
                                 ("kh", 112.0, lambda: B.tgv_adjoint(xo, gv, p, q, dims)),
                                 ("dual", 208.0, lambda: B.tgv_dual_step(p, q, x, xo, v, vo, sigma, a1, a0, dims)),
                                 ("axpby", 24.0, lambda: B.axpby(0.5, xo, 0.25, x))):
            ms = event_ms(B, fn, a.warmup, a.steps)
            row[name + "_ms"] = ms
            row[name + "_TBps"] = nbytes * n / ms / 1e9
        for name in ("symgrad", "symgradh", "kh", "dual"):
            row[name + "_of_axpby"] = row[name + "_TBps"] / row["axpby_TBps"]
        # the compositions last: dual_composed grows p and q without bound, which the fused step above would then project
        row["kh_composed_ms"] = event_ms(B, kh_composed, a.warmup, a.steps)
        row["dual_composed_ms"] = event_ms(B, dual_composed, a.warmup, a.steps)
        for name in ("kh", "dual"):
            row[name + "_composed_over_fused"] = row[name + "_composed_ms"] / row[name + "_ms"]
        print(json.dumps(row), flush=True)
        out.append(row)
        del x, xo, v, vo, p, q, gv, e
    return out


def iteration(B, a):
    """one primal-dual iteration of pics --tgv against one A^H A on bench.py's config 4 problem"""
    import bench
    from indigo_amd.sense import normal_operator
    prob = bench.sense_problem(4, 256, 8)
    A = prob.build_zpadfft(B)
    AHA = normal_operator(A, lamda=1e-3)
    n = AHA.shape[1]
    dims = tuple(prob.N)
    x = B.copy_array(rand64c(n, 1, seed=2))
    y = B.zero_array((n, 1), C64)
    aha_ms = event_ms(B, lambda: AHA.eval(y, x), a.warmup, a.steps)
    b = B.copy_array(rand64c(n, 1, seed=3))
    z = B.zero_array((4 * n, 1), C64)
    z.dense_rows(0, n).copy(x)
    u = B.zero_array((9 * n, 1), C64)
    tau, sigma, a1, a0 = 0.1, 0.3, 0.01, 0.02

    def gradf(g, w):
        gx = g.dense_rows(0, n)
        AHA.eval(gx, w.dense_rows(0, n))
        B.axpby(1, gx, -1, b)

    def KH(g, w):
        B.tgv_adjoint(g.dense_rows(0, n), g.dense_rows(n, 4 * n), w.dense_rows(0, 3 * n), w.dense_rows(3 * n, 9 * n), dims)

    def dual_step(w, zn, zo):
        B.tgv_dual_step(w.dense_rows(0, 3 * n), w.dense_rows(3 * n, 9 * n), zn.dense_rows(0, n), zo.dense_rows(0, n),
                        zn.dense_rows(n, 4 * n), zo.dense_rows(n, 4 * n), sigma, a1, a0, dims)

    B.primal_dual(gradf, None, KH, dual_step, tau, z, u, maxiter=a.warmup)     # (the solver's buffers and the leaf's formats: warm)
    tgv_ms = event_ms(B, lambda: B.primal_dual(gradf, None, KH, dual_step, tau, z, u, maxiter=a.steps), 0, 1) / a.steps
    row = dict(problem="bench config 4: image %s, 8 coils, oversampling 2 (grid 512^3)" % (dims,),
               device=B.device_name(), aha_ms=aha_ms, tgv_iteration_ms=tgv_ms, ratio=tgv_ms / aha_ms)
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), kernels=kernels(B, a), tgv=iteration(B, a))
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
