#!/usr/bin/env python3
"""A^H A on a grid whose x axis is chirp-z: the fused leaf after a permutation of the image (SenseProblem.build_zpadfft on
a grid the leaf refuses as it is) against the unfused -O3 leaves (build_fused), device-synchronised wall time of each.

    python tools/permuted_leaf_timing.py [--image 208 240 240] [--coils 8] [--width 2] [--warmup 3] [--steps 10] [--parity]
                                         [--out FILE]

Default: image 208 x 240 x 240 at the reference driver's oversampling 640/480 -- grid 277 x 320 x 320, run as 320 x 277 x 320 --,
8 coils, half-width 2, a radial trajectory at the headline problem's density (3617 spokes per 256^2 of cross-section, one
oversampled grid edge of samples per spoke).  --parity: the fused A^H A against the float64 operator of oracle/sense64.py on
the unpermuted problem.  Run it under `rocprofv3 --kernel-trace --stats -- python ...` for the per-kernel split.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from indigo_amd import fused  # noqa: E402
from indigo_amd import operators as op  # noqa: E402
from indigo_amd.backends import get_backend  # noqa: E402
from indigo_amd.sense import SenseProblem, normal_operator  # noqa: E402
from indigo_amd.util import rand64c  # noqa: E402


def timed(B, AHA, x_d, y_d, warmup, steps):
    for _ in range(warmup):
        AHA.eval(y_d, x_d)
    B.barrier()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        AHA.eval(y_d, x_d)
        B.barrier()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def kernel(B, dims, a):
    """the permutation kernel alone: wall time per launch over `steps` back-to-back launches, and the compulsory bytes per second
    (read + write; three streams with beta != 0)"""
    import itertools
    n = int(np.prod(dims))
    x_d = B.copy_array(rand64c(n, 1, seed=1))
    y_d = B.zero_array((n, 1), np.dtype('complex64'))
    out = dict(dims=dims, device=B.device_name(), runs=[])
    for perm in itertools.permutations(range(3)):
        for beta in (0, 0.5):
            for _ in range(a.warmup):
                B.permute3(y_d, x_d, dims, perm, beta=beta)
            B.barrier()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                B.permute3(y_d, x_d, dims, perm, beta=beta)
            B.barrier()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            nbytes = n * 8 * (2 if beta == 0 else 3)
            out['runs'].append(dict(perm=perm, beta=beta, ms=round(ms, 4), tb_per_s=round(nbytes / ms / 1e9, 3)))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--image', type=int, nargs=3, default=[208, 240, 240])
    ap.add_argument('--coils', type=int, default=8)
    ap.add_argument('--width', type=int, default=2)
    ap.add_argument('--osf', type=float, default=640 / 480)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--parity', action='store_true')
    ap.add_argument('--skip-o3', action='store_true')
    ap.add_argument('--kernel-dims', type=int, nargs=3, default=None,
                    help='instead: ig_permute3_c64 alone on one volume of these dims, every perm, beta = 0 and beta = 0.5')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    B = get_backend('hip')
    if a.kernel_dims:
        return kernel(B, tuple(a.kernel_dims), a)
    N = tuple(a.image)
    nspokes = int(round(3617 * (N[1] * N[2]) / 256.0 ** 2))
    p = SenseProblem.synthetic(N, a.coils, nspokes=nspokes, nreadout=int(N[0] * a.osf), width=a.width, ntable=128, oversamp=a.osf, seed=4)
    perm = fused.image_permutation(B, p.oN, a.coils)
    res = dict(image=N, grid=p.oN, coils=a.coils, width=a.width, samples=p.T, permutation=perm,
               permuted_grid=tuple(p.oN[i] for i in perm) if perm else None, device=B.device_name())
    x = rand64c(int(np.prod(N)), 1, seed=1)
    x_d = B.copy_array(x)
    y_d = B.zero_array((x.shape[0], 1), np.dtype('complex64'))

    A = p.build_zpadfft(B)
    assert A.has(op.ZpadFFT) and (perm is None or A.has(op.AxisPermute))
    AHA = normal_operator(A)
    t = timed(B, AHA, x_d, y_d, a.warmup, a.steps)
    res['fused_ms'] = dict(median=float(np.median(t)), min=float(np.min(t)), all=[round(v, 3) for v in t])
    # the two permutations alone: the same launches the tree makes, timed on their own
    if perm is not None:
        P = A.right
        t_d = B.zero_array((x.shape[0], 1), np.dtype('complex64'))
        for _ in range(a.warmup):
            P.eval(t_d, x_d)
            P.eval(y_d, t_d, forward=False)
        B.barrier()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            P.eval(t_d, x_d)
            P.eval(y_d, t_d, forward=False)
        B.barrier()
        res['permute_pair_ms'] = (time.perf_counter() - t0) * 1e3 / a.steps
        res['permute_bytes_per_pair'] = 4 * x.shape[0] * 8
        del t_d
    if a.parity:
        AHA.eval(y_d, x_d)
        got = y_d.to_host()
        from oracle.sense64 import SenseF64
        exact = SenseF64(p).normal(x)
        res['parity_vs_float64'] = float(np.linalg.norm(got - exact) / np.linalg.norm(exact))
    del AHA, A
    B._scratch = None
    p.drop_cache()

    if not a.skip_o3:
        A3 = p.build_fused(B)
        AHA3 = normal_operator(A3)
        t = timed(B, AHA3, x_d, y_d, a.warmup, a.steps)
        res['o3_ms'] = dict(median=float(np.median(t)), min=float(np.min(t)), all=[round(v, 3) for v in t])
        res['fused_over_o3'] = res['fused_ms']['median'] / res['o3_ms']['median']
        del AHA3, A3
        B._scratch = None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
