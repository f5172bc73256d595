#!/usr/bin/env python3
"""Device-event times of the fused dictionary-matching kernel (ig_dict_match_c64, Backend.dict_match) on the MI355X,
steady state after warm-up, medians over repeated calls, as one JSON document:

  * the kernel at 256^3 voxels with K = 4 and 8 coefficients against N = 1024, 4096 and 16384 atoms, the dictionary already on the
    device.  Flop model: 8 K N real flops per voxel (a complex multiply-add per coefficient and atom); byte model: 8 K + 12 bytes per
    voxel;
  * comparator 1, the 155 Tflop/s that the float32-input MFMA instructions reach on this device: the fraction of it;
  * comparator 2, the same matching written with torch on the same shapes: `matmul` of a chunk of voxels with the conjugated
    dictionary, `abs`, `argmax`, chunk after chunk (a chunk x N matrix of scores in memory, 2^29 elements of it at a time).  The
    indices of its first chunk are compared with the kernel's.

    python tools/dictmatch_timing.py [--warmup 2] [--reps 5] [--log2n 24] [--torch-reps 2] [--out profiles/dictmatch_timing.json]
"""
import argparse
import ctypes
import json
import os
import sys

os.environ.setdefault("INDIGO_HIP_WITH_TORCH", "1")         # torch first: it and the library then share one HIP runtime
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from indigo_amd.backends import get_backend  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from softsense_timing import fill, medians  # noqa: E402

C64 = np.dtype('complex64')
PEAK_FP32_MFMA = 155e12
TORCH_ELEMENTS = 1 << 29                                    # scores of a torch chunk: 4.3 GB as complex64


def atoms(K, N, seed):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))
    return np.asfortranarray((d / np.linalg.norm(d, axis=0)[None, :]).astype(C64))


def torch_match(torch, x, dh, chunk):
    """idx of every voxel: x (n, K) and dh = conj(d) (K, N) are torch tensors on the device"""
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for i0 in range(0, x.shape[0], chunk):
        out[i0:i0 + chunk] = torch.argmax(torch.abs(torch.matmul(x[i0:i0 + chunk], dh)), dim=1)
    return out


def torch_row(a, x_h_first, d_h, n, K, N, idx_first):
    """median time of the torch form on n voxels, and how many of the first chunk's indices agree with the kernel's"""
    try:
        import torch
        dev = torch.device("cuda")
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        x = torch.view_as_complex(torch.randn((n, K, 2), device=dev, generator=gen))
        dh = torch.from_numpy(np.ascontiguousarray(d_h.conj())).to(dev)
        chunk = max(1, TORCH_ELEMENTS // N)
        first = torch.from_numpy(np.ascontiguousarray(x_h_first)).to(dev)
        agree = float((torch_match(torch, first, dh, chunk).cpu().numpy() == idx_first).mean())
        torch_match(torch, x, dh, chunk)
        times = []
        for _ in range(a.torch_reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch_match(torch, x, dh, chunk)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        del x, dh, first
        torch.cuda.empty_cache()
        return dict(torch_ms=float(np.median(times)), torch_chunk=chunk, torch_first_indices_agree=agree)
    except Exception as e:  # the comparator is not the product: record why it did not run
        return dict(torch_error="%s: %s" % (type(e).__name__, e))


def row(B, a, n, K, N):
    flops, nbytes = 8.0 * K * N * n, (8.0 * K + 12.0) * n
    x = fill(B, n * K, 1)
    d_h = atoms(K, N, 2)
    d = B.copy_array(d_h)
    idx, ip = B.empty_array((n, 1), np.dtype('int32')), B.empty_array((n, 1), C64)
    call = lambda: B._check(B._L.ig_dict_match_c64(B._ctx, n, K, N, ctypes.c_void_p(x._arr), n, ctypes.c_void_p(d._arr), d._leading_dim,
                                                    ctypes.c_void_p(idx._arr), ctypes.c_void_p(ip._arr)), "ig_dict_match_c64")
    ms = medians(B, {"kernel": call}, a.warmup, a.reps)["kernel"]
    out = dict(voxels=n, coefficients=K, atoms=N, flops=flops, bytes=nbytes, kernel_ms=ms, Tflops=flops / ms / 1e9,
               fraction_of_fp32_mfma_peak=flops / ms / 1e-3 / PEAK_FP32_MFMA, GBps=nbytes / ms / 1e6)
    m = min(n, 1 << 14)                                      # the voxels whose indices the torch form is checked on
    x_first = np.stack([x.dense_rows(k * n, k * n + m).to_host().ravel() for k in range(K)], axis=1)
    idx_first = idx.dense_rows(0, m).to_host().ravel()
    del x, idx, ip
    if a.torch_reps > 0:
        out.update(torch_row(a, x_first, d_h, n, K, N, idx_first))
        if "torch_ms" in out:
            out["torch_over_kernel"] = out["torch_ms"] / ms
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2, help="timed runs of the torch comparator after one warm-up (0: leave it out)")
    ap.add_argument("--log2n", type=int, default=24, help="voxels = 2^this (24: 256^3)")
    ap.add_argument("--coefficients", default="4,8")
    ap.add_argument("--atoms", default="1024,4096,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dictmatch_timing.json"), help="where the JSON document goes ('' : only printed)")
    a = ap.parse_args(argv)
    B = get_backend("hip")
    n = 1 << a.log2n
    doc = dict(device=B.device_name(), warmup=a.warmup, reps=a.reps, torch_reps=a.torch_reps, fp32_mfma_peak_Tflops=PEAK_FP32_MFMA / 1e12,
               rows=[row(B, a, n, int(K), int(N)) for K in a.coefficients.split(",") for N in a.atoms.split(",")])
    text = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
