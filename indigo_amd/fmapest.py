#!/usr/bin/env python3
"""Field-map estimation: the off-resonance map of `pics --fmap` from images at two or more echo times.

    python -m indigo_amd.fmapest --te 0.002,0.004[,...] [-i 200] [--beta 0.1] [--cost-every 10] echoes.rec.npy   -> echoes.fmap.npy
    python -m indigo_amd.fmapest --te 0.002,0.004[,...] ... e0.rec.npy e1.rec.npy ...                            -> e0.fmap.npy

The input is either ONE file whose array, transposed, is (X, Y, Z, 1, ..., E) -- what `pics` writes for a multi-echo scan stored
as E time frames -- or E files of (X, Y, Z) images, one per echo; both stored reversed like `rec`.  `--te` are the echo times in
seconds, strictly increasing, 2 to 8 of them.  The images follow the sign convention of `pics --fmap`: y_l ~ m exp(-2 pi i f te_l).

The naive estimate -angle(y_1 conj(y_0)) / (2 pi (te_1 - te_0)) is noise wherever the signal is low (air, bone, outside the
object); the histogram that `indigo_amd.fmap.segments` builds its interpolator from then spans +-1 / (2 dTE) and the segment count
explodes.  This is the penalised-likelihood estimator of Funai, Fessler, Yeo, Olafsson and Noll (IEEE TMI 27:1484, 2008; bart / MIRT
`mri_field_map_reg`; no counterpart in the reference): with p = y_m conj(y_l), w = |p|, k = 2 pi (te_m - te_l) for every pair l < m
and s the principal value of angle(p) + k f,

    Psi(f) = sum_j sum_{l<m} w (1 - cos s)  +  beta/2 sum_{edges (j,j')} (f_j - f_j')^2

over the nearest-neighbour edges of the volume (no wrap-around), minimised by `-i` steps of separable quadratic surrogates from the
naive estimate (`Backend.fieldmap_init`, `Backend.fieldmap_step`).  Every step is one pass over the volume and
decreases Psi; low-signal voxels are filled in smoothly from their neighbours.  NO phase unwrapping is done: the true field has to
satisfy |f| < 1 / (2 (te_1 - te_0)).

Normalisation: the images are scaled by 1 / max|y_0|, and `--beta` is relative, beta_abs = beta * max_j sum_pairs w k^2, the largest
data curvature of the scan, so that one value serves scans of any scale and echo spacing.  The default 0.1 is a first choice, not a
measured optimum.  The number of iterations is fixed; Psi is logged every `--cost-every` iterations (computed by the same pass as
the step) and at the end.

The result is float32 (X, Y, Z) in Hz, stored reversed, so that `pics --fmap` reads it as it is.

The backend is the MI355X one (`hip`); there is no CPU fallback in the product.  `main(argv, backend=...)` lets the CPU test-suite
drive the same code with the numpy oracle backend.
"""
import argparse
import logging
import sys
import time

import numpy as np

log = logging.getLogger("fmapest")
_C64 = np.dtype('complex64')


def relative_beta_scale(y, te, chunk=1 << 20):
    """max_j sum_pairs w k^2 of the N x E panel y, the largest data curvature: what `--beta` is relative to (float64, `chunk` rows
    at a time)"""
    te = np.asarray(te, dtype=np.float64)
    top = 0.0
    for lo in range(0, y.shape[0], chunk):
        rows = y[lo:lo + chunk].astype(np.complex128)
        curv = np.zeros(rows.shape[0])
        for l in range(te.size):
            for m in range(l + 1, te.size):
                curv += np.abs(rows[:, m] * rows[:, l].conj()) * (2.0 * np.pi * (te[m] - te[l])) ** 2
        top = max(top, float(curv.max(initial=0.0)))
    return top


def normalised_panel(images):
    """the (X, Y, Z, E) images as the F-ordered N x E complex64 panel the backend takes, scaled by 1 / max|y_0|"""
    n, E = int(np.prod(images.shape[:3])), int(images.shape[3])
    panel = np.asfortranarray(images.reshape((n, E), order='F').astype(_C64))
    peak = float(np.abs(panel[:, 0]).max())
    if not peak > 0:
        raise ValueError("fmapest: the first echo image vanishes")
    panel *= np.float32(1.0 / peak)
    return panel


def estimate(B, images, te, iters=200, beta=0.1, cost_every=10):
    """The regularised field map in Hz, float32 (X, Y, Z), of the complex echo images (X, Y, Z, E) at the echo times te (seconds,
    strictly increasing, 2 <= E <= 8) on backend B: `iters` SQS steps from the two-echo estimate, beta relative to the largest data
    curvature (module docstring).  No unwrapping: the true field has to satisfy |f| < 1 / (2 (te[1] - te[0])).  Raises ValueError on
    real-valued images, a count of echo times that differs from the echoes, non-finite values, images that vanish."""
    images = np.asarray(images)
    te = np.asarray(te, dtype=np.float64).reshape(-1)
    if not np.iscomplexobj(images):
        raise ValueError("fmapest: the images are real-valued: the field map is in their phase")
    if images.ndim != 4:
        raise ValueError("fmapest: the images have shape %s, (X, Y, Z, E) is expected" % (images.shape,))
    dims, E = tuple(int(n) for n in images.shape[:3]), int(images.shape[3])
    if te.size != E:
        raise ValueError("fmapest: %d echo times for %d echo images" % (te.size, E))
    if not (np.isfinite(images).all() and np.isfinite(te).all()):
        raise ValueError("fmapest: the images or the echo times hold non-finite values")
    if iters < 0 or beta < 0 or not np.isfinite(beta):
        raise ValueError("fmapest: negative iteration count or beta")
    n = int(np.prod(dims))
    panel = normalised_panel(images)
    beta_abs = float(beta) * relative_beta_scale(panel, te)
    t0 = time.perf_counter()
    y = B.copy_array(panel, name='fmapest.y')
    f = B.zero_array((n,), np.dtype('float32'), name='fmapest.f')
    g = B.zero_array((n,), np.dtype('float32'), name='fmapest.g')
    B.fieldmap_init(f, y, dims, te)                      # (refuses E outside 2..8 and echo times that do not increase)
    every = max(int(cost_every), 0)
    for it in range(int(iters)):
        psi = B.fieldmap_step(g, f, y, te, beta_abs, dims, cost=bool(every) and it % every == 0)
        if psi is not None:
            log.info("fmapest iter %d: cost %.9e", it, psi)
        f, g = g, f
    psi = B.fieldmap_cost(f, y, te, beta_abs, dims)
    log.info("fmapest iter %d: cost %.9e", int(iters), psi)
    out = f.to_host().reshape(dims, order='F')
    log.info("fmapest: %s voxels, %d echoes, beta %g (absolute %.6e), %d iterations in %.2f s, field %.2f .. %.2f Hz", dims, E, beta,
             beta_abs, int(iters), time.perf_counter() - t0, float(out.min()), float(out.max()))
    return out


def load_images(paths):
    """(X, Y, Z, E) from one file of E frames or E files of one image, each stored reversed"""
    arrays = [np.load(p).T for p in paths]
    for p, a in zip(paths, arrays):
        if a.ndim < 3:
            raise ValueError("fmapest: %s holds an array of shape %s, at least (X, Y, Z) is expected" % (p, a.shape))
    if len(arrays) == 1:
        a = arrays[0]
        return a.reshape(a.shape[:3] + (-1,))
    for p, a in zip(paths, arrays):
        if int(np.prod(a.shape[3:])) != 1 or a.shape[:3] != arrays[0].shape[:3]:
            raise ValueError("fmapest: %s holds an array of shape %s: with several files each is one (X, Y, Z) image of the same size" % (p, a.shape))
    return np.stack([a.reshape(a.shape[:3]) for a in arrays], axis=3)


def output_path(first):
    """<name>.fmap.npy beside the first input, <name> without its .npy and .rec endings"""
    stem = first[:-4] if first.endswith(".npy") else first
    stem = stem[:-4] if stem.endswith(".rec") else stem
    return stem + ".fmap.npy"


def parse(argv):
    ap = argparse.ArgumentParser(prog="indigo_amd.fmapest", description="Regularised field map in Hz from images at 2 to 8 echo times, for pics --fmap: "
                                 "a fixed number of separable-quadratic-surrogate steps on the penalised-likelihood cost of Funai et al. (2008).")
    ap.add_argument('-i', type=int, default=200, help='SQS iterations (a fixed count)')
    ap.add_argument('--te', required=True, help='the echo times in seconds, comma-separated and strictly increasing: one per echo image')
    ap.add_argument('--beta', type=float, default=0.1, help='roughness penalty relative to the largest data curvature max_j sum_pairs w k^2 (a first choice, not a measured optimum)')
    ap.add_argument('--cost-every', type=int, default=10, help='log the cost every so many iterations (0: only at the end)')
    ap.add_argument('--backend', type=str, default='hip', choices=['hip'])
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--debug', type=int, default=logging.INFO, help='logging level')
    ap.add_argument('images', nargs='+', help='one .npy file of E frames, (X, Y, Z, .., E) stored reversed (a pics result), or E files of one (X, Y, Z) image each')
    args = ap.parse_args(argv)
    try:
        args.te = [float(v) for v in args.te.split(',')]
    except ValueError:
        ap.error("--te must be comma-separated numbers")
    if args.i < 0:
        ap.error("-i must not be negative")
    if args.beta < 0:
        ap.error("--beta must not be negative")
    if args.cost_every < 0:
        ap.error("--cost-every must not be negative")
    return args


def main(argv=None, backend=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=args.debug)
    images = load_images(args.images)
    if images.shape[3] != len(args.te):
        raise ValueError("fmapest: %d values of --te for %d echo images" % (len(args.te), images.shape[3]))
    if backend is None:
        from indigo_amd.backends import get_backend
        backend = get_backend(args.backend, device_id=args.device)
    f = estimate(backend, images, args.te, iters=args.i, beta=args.beta, cost_every=args.cost_every)
    out = output_path(args.images[0])
    np.save(out, f.T)
    log.info("fmapest: field map %s written to %s", f.T.shape, out)
    return f


if __name__ == "__main__":
    main()
