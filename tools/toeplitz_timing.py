#!/usr/bin/env python3
"""Device-event times of the pieces of pics --toeplitz on the MI355X, steady state after warm-up, as one JSON document.  The
headline problem (bench.py config 4: 256^3 image, 8 coils, 512^3 grid), K = 4 coefficient images, T = 8 and 32 frames that share
one trajectory:

  * the K x K mixing pass (Backend.psf_mix, ig_psf_mix_c64) in place on the 512^3 x 8-coil x 4-column panel of one coil chunk,
    next to `axpby` on the same byte count (16 n nc nk + 4 nk^2 n bytes; axpby moves 24 bytes per element);
  * one evaluation and one CG iteration of the `--basis` normal operator, FrameBasis^H * BlockDiag(A_t^H A_t) * FrameBasis, and
    of `ToeplitzNormal` with K = 4;
  * one evaluation of `ToeplitzNormal` with K = 1 next to the fused leaf's A^H A of one frame;
  * the set-up: `psf_kernel` for one trajectory (one adjoint NUFFT onto the 512^3 image and one transform; a scan with D distinct
    trajectories and K coefficients pays D of the former and K (K + 1) / 2 of the latter).  With one trajectory shared by all
    frames P = (Phi^H Phi) (x) FFT(q), which is how the K = 4 kernels are made here from the K = 1 one.

    python tools/toeplitz_timing.py [--warmup 1] [--steps 5] [--frames 8,32] [--out profiles/r15_toeplitz_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd.backends import get_backend  # noqa: E402
from indigo_amd.util import rand64c  # noqa: E402
from tools.tv_timing import event_ms  # noqa: E402

C64 = np.dtype('complex64')
K = 4


def gram_kernel(p1, phi):
    """the kernel planes of a basis phi on ONE shared trajectory from the K = 1 plane p1: (Phi^H Phi) (x) P_1"""
    G = phi.astype(np.complex128).conj().T @ phi.astype(np.complex128)
    k = G.shape[0]
    out = np.empty((k * k, p1.size), dtype=np.float32)
    for a in range(k):
        np.multiply(p1, np.float32(G[a, a].real), out=out[a])
    pair = 0
    for a in range(k):
        for b in range(a + 1, k):
            np.multiply(p1, np.float32(G[a, b].real), out=out[k + 2 * pair])
            np.multiply(p1, np.float32(G[a, b].imag), out=out[k + 2 * pair + 1])
            pair += 1
    return out


def mix_pass(B, a, kern_d, P, C):
    panel = B.zero_array((P * C, K), C64, name='panel')
    nbytes = 16.0 * P * C * K + 4.0 * K * K * P
    ms = event_ms(B, lambda: B.psf_mix(panel, panel, kern_d, P, C, interleaved=True), a.warmup, a.steps)
    del panel
    m = int(nbytes // 24)
    u, v = B.zero_array((m, 1), C64), B.zero_array((m, 1), C64)
    ax = event_ms(B, lambda: B.axpby(0.5, v, 0.5, u), a.warmup, a.steps)
    row = dict(grid_points=P, coils=C, coefficients=K, bytes=nbytes, psf_mix_ms=ms, psf_mix_TBps=nbytes / ms / 1e9,
               axpby_elements=m, axpby_ms=ax, axpby_TBps=24.0 * m / ax / 1e9, rate_of_axpby=(nbytes / ms) / (24.0 * m / ax))
    print(json.dumps(row), flush=True)
    return row


def cg_ms(B, AHA, n, a):
    x, b = B.zero_array((n, 1), C64), B.copy_array(rand64c(n, 1, seed=4))
    B.cg(AHA, b, x, maxiter=a.warmup)
    return event_ms(B, lambda: B.cg(AHA, b, x, maxiter=a.steps), 0, 1) / (a.steps + 1)      # (one evaluation for the start)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--frames", default="8,32")
    ap.add_argument("--img", type=int, default=256, help="image edge (256: the headline problem)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_toeplitz_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    import bench
    from indigo_amd.operators import ToeplitzNormal
    from indigo_amd.sense import normal_operator
    from indigo_amd.toeplitz import psf_kernel
    from indigo_amd.transforms import FuseZpadFFT, reserve_for, sense_recipe
    B = get_backend("hip")
    p = bench.sense_problem(4, a.img, 8)
    dims, C = tuple(p.N), p.C
    N, P = int(np.prod(dims)), 8 * int(np.prod(dims))
    doc = dict(device=B.device_name(), problem="bench config 4: image %s, %d coils, oversampling %g, half-width %g; frames on one trajectory, %d coefficients"
               % (dims, C, p.oversamp, p.width, K))

    # set-up: the K = 1 kernel of the one trajectory
    order = ToeplitzNormal.memory_order(B, dims)
    t0 = time.perf_counter()
    p1 = psf_kernel(B, dims, [p.coord], [0], None, int(p.width), float(p.oversamp), order=order, recipe=sense_recipe(3) + [FuseZpadFFT])
    B.barrier()
    doc["setup"] = dict(psf_kernel_one_trajectory_s=time.perf_counter() - t0, kernel_bytes_k1=p1.nbytes, kernel_bytes_k4=K * K * p1.nbytes, order=order)
    print(json.dumps(doc["setup"]), flush=True)
    B._scratch = None
    maps = np.asarray(p.maps, dtype=C64).reshape(dims + (C,))

    # K = 1 next to the fused leaf's A^H A
    A = p.build_zpadfft(B)
    AHA1 = normal_operator(A, lamda=0.0)
    x1, y1 = B.copy_array(rand64c(N, 1, seed=2)), B.zero_array((N, 1), C64)
    leaf_ms = event_ms(B, lambda: AHA1.eval(y1, x1), a.warmup, a.steps)
    T1 = B.ToeplitzNormal(dims, maps, p1, 1, order=order)
    B._scratch = None
    reserve_for(T1, 1, slack_products=2)
    t1_ms = event_ms(B, lambda: T1.eval(y1, x1), a.warmup, a.steps)
    ref = y1.to_host()
    AHA1.eval(y1, x1)
    diff = float(np.linalg.norm(ref - y1.to_host()) / np.linalg.norm(ref))
    doc["one_frame"] = dict(fused_leaf_aha_ms=leaf_ms, toeplitz_k1_ms=t1_ms, ratio=t1_ms / leaf_ms, relative_difference=diff)
    print(json.dumps(doc["one_frame"]), flush=True)
    del T1

    rows = []
    for T in (int(t) for t in a.frames.split(",")):
        phi = np.linalg.qr(rand64c(T, K, seed=6))[0].astype(C64)
        # the parent's path
        B._scratch = None
        reserve_for(AHA1, 1, slack_products=6, extra=2 * N * T)
        Phi = B.FrameBasis(phi, N)
        G = Phi.H * B.BlockDiag([AHA1] * T) * Phi + 1e-3 * B.Eye(N * K)
        x, y = B.copy_array(rand64c(N * K, 1, seed=3)), B.zero_array((N * K, 1), C64)
        g_ms = event_ms(B, lambda: G.eval(y, x), a.warmup, a.steps)
        g_cg = cg_ms(B, G, N * K, a)
        ref = y.to_host()
        del G, Phi
        # the Toeplitz form
        TK = B.ToeplitzNormal(dims, maps, gram_kernel(p1.reshape(-1), phi), K, order=order)
        AHA = 1e-3 * B.Eye(N * K) + TK
        B._scratch = None
        reserve_for(AHA, 1, slack_products=6)
        t_ms = event_ms(B, lambda: AHA.eval(y, x), a.warmup, a.steps)
        diff = float(np.linalg.norm(ref - y.to_host()) / np.linalg.norm(ref))
        t_cg = cg_ms(B, AHA, N * K, a)
        row = dict(frames=T, coefficients=K, gridding_eval_ms=g_ms, gridding_cg_iteration_ms=g_cg, toeplitz_eval_ms=t_ms,
                   toeplitz_cg_iteration_ms=t_cg, speedup_cg_iteration=g_cg / t_cg, relative_difference=diff)
        print(json.dumps(row), flush=True)
        rows.append(row)
        if T == int(a.frames.split(",")[-1]):
            B._scratch = None
            doc["mix_pass"] = mix_pass(B, a, TK._kernel(), P, C)
        del TK, AHA, x, y
    doc["subspace_cg"] = rows
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
