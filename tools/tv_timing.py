#!/usr/bin/env python3
"""Device-event times of the pieces of pics --tv on the MI355X, steady state after warm-up, as one JSON document:

  * the gradient, its adjoint (added onto the output, alpha = beta = 1, as the solver calls it) and the fused dual step
    (Backend.grad3 / tv_dual_step) at 256^3, 480 x 208 x 308 and 512^3, next to the backend's own axpby on one volume of the
    same size as the streaming yardstick.  A 256^3 complex64 volume is 134 MB: the gradient's four volumes do not fit in the
    256 MiB Infinity Cache either.  Byte model per voxel: gradient 32 B (one volume read, three written), adjoint 32 B (three
    read, one written; + 8 B for the output read when beta != 0, not counted), dual step 64 B (two volumes and three components
    read, three written), axpby 24 B;
  * one primal-dual iteration of pics --tv against one A^H A evaluation on the headline problem (bench.py config 4: 256^3 image,
    8 coils, 512^3 grid).

    python tools/tv_timing.py [--warmup 3] [--steps 20] [--out FILE]
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


def kernels(B, a):
    out = []
    for dims in [(256, 256, 256), (480, 208, 308), (512, 512, 512)]:
        n = int(np.prod(dims))
        x = B.copy_array(rand64c(n, 1, seed=1))
        xo = B.copy_array(rand64c(n, 1, seed=2))
        u = B.zero_array((3 * n, 1), C64)
        row = dict(dims=dims)
        for name, nbytes, fn in (("grad", 32.0, lambda: B.grad3(u, x, dims)),
                                 ("gradh", 32.0, lambda: B.grad3(xo, u, dims, adjoint=True, alpha=1, beta=1)),
                                 ("dual", 64.0, lambda: B.tv_dual_step(u, x, xo, 0.5, 0.1, dims)),
                                 ("axpby", 24.0, lambda: B.axpby(0.5, xo, 0.25, x))):
            ms = event_ms(B, fn, a.warmup, a.steps)
            row[name + "_ms"] = ms
            row[name + "_TBps"] = nbytes * n / ms / 1e9
        for name in ("grad", "gradh", "dual"):
            row[name + "_of_axpby"] = row[name + "_TBps"] / row["axpby_TBps"]
        print(json.dumps(row), flush=True)
        out.append(row)
        del x, xo, u
    return out


def iteration(B, a):
    """one primal-dual iteration of pics --tv against one A^H A on bench.py's config 4 problem"""
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
    G = B.Gradient(dims)
    b = B.copy_array(rand64c(n, 1, seed=3))
    u = B.zero_array((3 * n, 1), C64)
    tau, sigma, mu = 0.1, 0.3, 0.01

    def gradf(g, z):
        AHA.eval(g, z)
        B.axpby(1, g, -1, b)

    def KH(g, v):
        G.eval(g, v, alpha=1, beta=1, forward=False)

    def dual_step(v, xn, xo):
        B.tv_dual_step(v, xn, xo, sigma, mu, dims)

    B.primal_dual(gradf, None, KH, dual_step, tau, x, u, maxiter=a.warmup)     # (the solver's buffers and the leaf's formats: warm)
    tv_ms = event_ms(B, lambda: B.primal_dual(gradf, None, KH, dual_step, tau, x, u, maxiter=a.steps), 0, 1) / a.steps
    row = dict(problem="bench config 4: image %s, 8 coils, oversampling 2 (grid 512^3)" % (dims,),
               device=B.device_name(), aha_ms=aha_ms, tv_iteration_ms=tv_ms, ratio=tv_ms / aha_ms, fista_ratio_r08=1.065)
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    doc = dict(device=B.device_name(), kernels=kernels(B, a), tv=iteration(B, a))
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
