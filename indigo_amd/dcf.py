#!/usr/bin/env python3
"""Density compensation: iterative Pipe-Menon sample weights for a non-Cartesian trajectory.

    python -m indigo_amd.dcf [-i 30] [--width 3] [--osf 640/480] [--dims X:Y:Z] scan.npz        -> scan.dcf.npy

The sample density of a 3-D radial scan falls like 1 / r^2, and the first iterations of an unweighted least-squares solver are
spent undoing it.  The remedy every non-Cartesian toolbox ships (`bart nufft` / `pics -p`, sigpy's `pipe_menon_dcf`; no
counterpart in the reference) is a weighted data term with the weights of Pipe and Menon (MRM 41:179, 1999),

    w <- w / (G G^H w),        from w = 1,

G the gridding matrix of the reconstruction's own NUFFT: the same Kaiser-Bessel kernel (`Backend.nufft_params`) on the same
oversampled grid int(n * osf).  `python -m indigo_amd.pics --dcf scan.dcf.npy` (or `--dcf auto`, which calls `pipe_menon` in
passing) then solves min 1/2 ||W^(1/2) (A x - y)||^2 + ...

What it is for: FEW iterations, or a starting image.  On a 16^3 image with 300 x 32 radial samples and 1 % noise the weighted CG
reaches after two iterations the error the plain one reaches after three to four; from about the sixth iteration on the weighted
run is WORSE: the weights amplify the noise of the sparsely sampled periphery, the known price of a weighted data term.  Hence
opt-in.

The iteration runs on the backend (`Backend.dcf_spread`, `Backend.dcf_gather_div`): G^H w in 64-bit fixed point -- a sum that does
not depend on the order of its adds, bitwise repeatable, exact to half a quantum per contribution however many thousand samples
share a cell at the k-space centre -- then the gather and divide in float64 with one rounding to float32 per sample and
iteration.  The scale of the fixed point is 2^floor(62 - log2(M wmax)) with wmax the largest weight of the iteration before.

The number of iterations is FIXED (default 30), not a tolerance: on the case above rms(s - 1), s = G G^H w, falls from 0.17 to
0.026 in 30 iterations while max |s - 1| stalls near 0.18 and wmax / wmin keeps growing -- the iteration semi-converges, and
stopping on max |s - 1| would never stop.  Every iteration logs max |s - 1| and wmax.

The result is float32, scaled to mean 1, with the axes of `traj` without the coordinate axis, stored reversed like `traj`:
(views, readout) on file for a (3, readout, views) trajectory, (T, ..., views, readout) with time frames.  Frames with equal
trajectories share their weights, computed once.

The backend is the MI355X one (`hip`); there is no CPU fallback in the product.  `main(argv, backend=...)` lets the CPU
test-suite drive the same code with the numpy oracle backend.
"""
import argparse
import logging
import os
import sys
import time

import numpy as np

log = logging.getLogger("dcf")


def scale_for(M, wmax):
    """the fixed-point scale of `Backend.dcf_spread` for M samples of weights up to wmax: the power of two 2^floor(62 - log2(M wmax)),
    so that M * wmax * scale <= 2^62 and no sum of M contributions (taps are <= 1) leaves the int64 range"""
    return float(2.0 ** int(np.floor(62.0 - np.log2(float(max(M, 1)) * float(wmax)))))


def upload(B, sep, stride=None):
    """The device side of a separable-records description for the Pipe-Menon kernels: (records, sep, tiles) as `Backend.dcf_spread`
    takes them.  stride: 32-bit words from one record to the next (None: the records as they are)."""
    from indigo_amd.grid_formats import dcf_tiles
    rec = np.ascontiguousarray(sep['records'])
    words = rec.shape[1]
    if stride is not None and int(stride) != words:
        assert int(stride) > words, (stride, words)
        wide = np.zeros((rec.shape[0], int(stride)), dtype=np.uint32)
        wide[:, :words] = rec
        rec = wide
    t = dcf_tiles(sep['records'], sep['tw'], sep['dims'], piece=getattr(B, 'tuning', {}).get('dcf_piece'))
    tiles = {k: B.copy_array(v, name='dcf.' + k) for k, v in t.items()}
    records = B.copy_array(rec.reshape(-1) if rec.size else np.zeros(1, np.uint32), name='dcf.records')
    return records, dict(tw=int(sep['tw']), dims=tuple(int(n) for n in sep['dims']), stride=int(rec.shape[1])), tiles


def pipe_menon(B, traj, dims, width=3, osf=640 / 480, iters=30):
    """Pipe-Menon weights of one trajectory on backend B: `traj` (3, ...) in cycles per pixel of the `dims` image (what
    `Backend.NUFFT` takes), `width` and `osf` the half-width and oversampling of the reconstruction's NUFFT.  Runs `iters` times
    spread -> gather-and-divide from w = 1 -- a fixed count, the iteration semi-converges (module docstring) -- and returns the
    float32 weights scaled to mean 1, shaped like traj without its first axis.  Raises ValueError where the separable records do not
    exist (a half-width above 4, an axis of the oversampled grid shorter than the taps): there is no other route."""
    from scipy.signal.windows import kaiser
    from indigo_amd.interp import interp_sep_records
    traj = np.asarray(traj, dtype=np.float64)
    assert traj.shape[0] == 3, "only 3-D trajectories are supported"
    out_shape = traj.shape[1:]
    M = int(np.prod(out_shape))
    if M < 1:
        raise ValueError("dcf: the trajectory holds no samples")
    omin, beta = B.nufft_params(width, (osf,) * 3)
    oN = tuple(int(int(n) * osf) for n in dims)
    kb = kaiser(2 * 128 + 1, beta)[128:]
    sep = interp_sep_records(M, oN, width, kb, traj.reshape((3, -1), order='F'))
    if sep is None:
        raise ValueError("dcf: no separable gridding records for half-width %s on the grid %s (the Pipe-Menon kernels serve half-widths "
                         "of 1 to 4 and axes of at least the 4, 6 or 8 taps); there is no other route" % (width, oN))
    t0 = time.perf_counter()
    records, desc, tiles = upload(B, sep)
    f32 = np.dtype('float32')
    w = B.copy_array(np.ones(M, dtype=np.float32), name='dcf.w')
    acc = B.zero_array((int(np.prod(oN)),), np.dtype('int64'), name='dcf.acc')
    wmax = 1.0
    for it in range(int(iters)):
        scale = scale_for(M, wmax)
        B.dcf_spread(acc, w, records, desc, scale, tiles)
        wmax, dev = B.dcf_gather_div(w, acc, w, records, desc, scale, tiles)
        log.info("dcf iter %d: max|s - 1| %.4e, wmax %.6e", it + 1, dev, wmax)
        if not (wmax > 0 and np.isfinite(wmax)):
            raise ValueError("dcf: the weights degenerated at iteration %d (wmax %r)" % (it + 1, wmax))
    wh = np.empty(M, dtype=f32)
    w.copy_to(wh)
    wh = (wh.astype(np.float64) / wh.astype(np.float64).mean()).astype(f32)
    log.info("dcf: %d samples on the %s grid, half-width %s, %d iterations in %.2f s, w max / min %.3e", M, oN, width, int(iters),
             time.perf_counter() - t0, float(wh.max()) / max(float(wh.min()), 1e-300))
    return wh.reshape(out_shape, order='F')


def frame_weights(B, traj, dims, width=3, osf=640 / 480, iters=30):
    """Weights for every frame of `traj` = (3, readout, views[, 1, ..., T]) in cycles per pixel: the same axes without the first;
    frames with equal trajectories share one computation"""
    traj = np.asarray(traj, dtype=np.float64)
    if traj.ndim <= 3:
        return pipe_menon(B, traj, dims, width, osf, iters)
    T = int(np.prod(traj.shape[3:]))
    trjs = traj.reshape(traj.shape[:3] + (T,))
    out = np.empty(traj.shape[1:3] + (T,), dtype=np.float32)
    distinct = []
    for t in range(T):
        k = next((k for k, (seen, _) in enumerate(distinct) if np.array_equal(seen, trjs[..., t])), None)
        if k is None:
            k = len(distinct)
            distinct.append((trjs[..., t], pipe_menon(B, trjs[..., t], dims, width, osf, iters)))
        out[..., t] = distinct[k][1]
    log.info("dcf: frames %d, distinct trajectories %d", T, len(distinct))
    return out.reshape(traj.shape[1:])


def parse(argv):
    ap = argparse.ArgumentParser(prog="indigo_amd.dcf", description="Pipe-Menon density-compensation weights of a scan's trajectory, for pics --dcf: "
                                 "a fixed number of iterations w <- w / (G G^H w) with the gridding kernel and grid of the reconstruction.")
    ap.add_argument('-i', type=int, default=30, help='Pipe-Menon iterations (a fixed count: the iteration semi-converges)')
    ap.add_argument('--backend', type=str, default='hip', choices=['hip'])
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--debug', type=int, default=logging.INFO, help='logging level')
    ap.add_argument('--width', type=int, default=3, help='Kaiser-Bessel kernel half-width of the reconstruction (pics --width)')
    ap.add_argument('--osf', type=float, default=640 / 480, help='gridding oversampling factor of the reconstruction (pics --osf)')
    ap.add_argument('--dims', default=None, help='image size X:Y:Z (default: that of the scan\'s maps)')
    ap.add_argument('data', help='the scan: .npz (or HDF5) with `traj` in pixels, stored reversed, and `maps` unless --dims is given')
    args = ap.parse_args(argv)
    if args.i < 0:
        ap.error("-i must not be negative")
    if args.dims is not None:
        try:
            args.dims = tuple(int(v) for v in args.dims.split(':'))
            assert len(args.dims) == 3 and min(args.dims) >= 1
        except (ValueError, AssertionError):
            ap.error("--dims must be three positive lengths X:Y:Z")
    return args


def main(argv=None, backend=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=args.debug)
    if backend is None:
        from indigo_amd.backends import get_backend
        backend = get_backend(args.backend, device_id=args.device)
    from indigo_amd.pics import load_extras
    arrays = load_extras(args.data, names=('traj', 'maps'))
    if 'traj' not in arrays:
        raise ValueError("dcf: %s holds no `traj`" % args.data)
    traj = np.array(arrays['traj'].T, dtype=np.float64)
    dims = args.dims
    if dims is None:
        if 'maps' not in arrays:
            raise ValueError("dcf: %s holds no `maps` to take the image size from: give --dims X:Y:Z" % args.data)
        dims = tuple(int(n) for n in arrays['maps'].T.shape[:3])
    for a in range(3):                                   # pixels -> units of the field of view, as pics does
        traj[a] /= dims[a]
    w = frame_weights(backend, traj, dims, args.width, args.osf, args.i)
    out = os.path.splitext(args.data)[0] + ".dcf.npy"
    np.save(out, w.T)
    log.info("dcf: weights %s written to %s", w.T.shape, out)
    return w


if __name__ == "__main__":
    main()
