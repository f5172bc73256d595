#!/usr/bin/env python3
"""ESPIRiT calibration: coil sensitivity maps from the scan's own k-space centre (Uecker et al., MRM 71:990, 2014; `bart ecalib`).

    python -m indigo_amd.ecalib [-r 24] [-k 6] [-t 0.001] [-c 0.8] [-m 2] [--iters 30] [--osf O] [--width W] [--dims X:Y:Z] scan.npz

writes `<name>.maps.npy`, (X, Y, Z, C, M) stored reversed like every array of the scan -- what `pics --maps` reads, M sets of maps
selecting SENSE (M = 1) or soft-SENSE --, and `<name>.evals.npy`, the eigenvalue maps (X, Y, Z, 1, M).

The definition (tests/espirit64.py restates it in float64).  s[p, c] is a fully sampled Cartesian block of k-space,
(cx, cy, cz, C), centred as `Backend.FFTc` centres k-space (the origin at index c_a // 2).  The kernel has side k per axis, clamped to
the block, K3 = k0 k1 k2 elements.  For every window origin q at which the window fits, h_q is the vector of s[q + kappa, c] over
(kappa, c), of length K3 C.  Gamma = sum_q h_q h_q^H has the eigenpairs (sigma_j^2, w_j); P = sum w_j w_j^H over those with
sigma_j > t sigma_1 projects onto the space the windows span.  With

    R_cc'[delta] = sum_{kappa - kappa' = delta} P[(kappa, c), (kappa', c')],         delta in [-(k - 1), k - 1]^3
    G(x)_cc'     = (1 / K3) sum_delta R_cc'[delta] exp(+2 pi i delta . xi / N)

(xi: the voxel's coordinate from the voxel FFTc treats as the origin, index n_a // 2; N: the image dims; the sign is that of
k-space = the forward exp(-i ...) transform of the image) G(x) is Hermitian with eigenvalues in [0, 1], and the true sensitivities at
x are an eigenvector with eigenvalue 1 wherever the data are consistent.  The maps are the M <= 4 leading eigenpairs
(lambda_m(x), v_m(x)) in descending order, every v_m of unit 2-norm over the coils and rotated so that its coil-0 component is real and
>= 0 (left as it is where that component's magnitude is below 1e-6); a map is zero where lambda_m(x) < the crop value -c.

The steps:

 1. The calibration block.  The file's `calib` array, (cx, cy, cz, C) stored reversed, if it has one.  Otherwise from `data` and
    `traj` (in pixels, as pics reads them): the samples with max_a |k_a| <= r / 2, pooled over all time frames (maps carry no TIME
    axis), are one readout of a `Backend.NUFFT` onto an r^3 image of the same field of view; (F^H F + lamda I) x = F^H y is solved for all
    coils at once with KronI(C, NUFFT) and 15 iterations of `Backend.cg`, lamda = 1e-3 of the largest eigenvalue of F^H F (ten power
    iterations); the block is the centred transform of the r^3 coil images.  Fewer than K3 C samples inside is an error.
 2. Gamma, its eigen-decomposition, P and R on the host in complex128: set-up work like the host format builders (K3 C <= 4096).
 3. G on the device: the C (C + 1) / 2 boxes of R / K3 (the upper triangle of G), multiplied by the centring phase
    exp(-2 pi i delta . (N // 2) / N), go through `Backend.place_wrapped` into as many zeroed volumes, and every volume through an
    unnormalised inverse transform in place (`Backend.ifftn`): 8 N C (C + 1) / 2 bytes of device memory, 4.8 GB at 256^3 x 8 coils.
 4. `Backend.espirit_eig`: a Hermitian C x C eigenproblem per voxel.
 5. The two files.

Image size: `--dims X:Y:Z`, else the dims of the file's `maps` if it has some, else from the trajectory's extent (2 max |k_a|, rounded
up to an even number: exact only for trajectories that reach the edge of k-space along every axis).

Left out: bart's soft weighting of the maps (`-W`), the automatic threshold (`-a`) and intensity normalisation (`-I`).

The backend is the MI355X one (`hip`); `main(argv, backend=...)` lets the CPU test-suite drive the same code with the numpy oracle.
"""
import argparse
import logging
import os
import sys

import numpy as np

log = logging.getLogger("ecalib")
_C64 = np.dtype('complex64')

MAX_KC = 4096          # K3 C: Gamma is (K3 C)^2 complex128 on the host, 268 MB and a minute of eigh at the limit
CG_ITERS = 15
POWER_ITERS = 10
LAMDA_FRACTION = 1e-3


def parse(argv):
    ap = argparse.ArgumentParser(prog="indigo_amd.ecalib", description="ESPIRiT calibration: M sets of coil sensitivity maps from the scan's k-space centre, "
                                 "written as <name>.maps.npy for pics --maps (and <name>.evals.npy).")
    ap.add_argument('-r', type=int, default=24, help='side of the calibration region cut from non-Cartesian data (not used when the file has `calib`)')
    ap.add_argument('-k', type=int, default=6, help='kernel side (clamped to the calibration block)')
    ap.add_argument('-t', type=float, default=0.001, help='keep the singular vectors of the calibration matrix above t times the largest singular value')
    ap.add_argument('-c', type=float, default=0.8, help='crop: a map is zero where its eigenvalue is below this')
    ap.add_argument('-m', type=int, default=2, help='number of sets of maps (1 ... 4)')
    ap.add_argument('--iters', type=int, default=30, help='iterations of the per-voxel eigen-solver')
    ap.add_argument('--osf', type=float, default=640 / 480, help='gridding oversampling factor, as in pics')
    ap.add_argument('--width', type=int, default=3, help='Kaiser-Bessel kernel half-width, as in pics')
    ap.add_argument('--dims', default=None, help='image size X:Y:Z (default: that of the file\'s maps, else from the trajectory\'s extent)')
    ap.add_argument('--backend', type=str, default='hip', choices=['hip'])
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--debug', type=int, default=logging.INFO, help='logging level')
    ap.add_argument('data', help='.npz scan: `calib` (Cartesian calibration block) or `data` and `traj` as pics reads them')
    args = ap.parse_args(argv)
    if not 1 <= args.m <= 4:
        ap.error("-m must be between 1 and 4")
    if args.k < 1 or args.r < 1 or args.iters < 0:
        ap.error("-k and -r must be at least 1, --iters at least 0")
    return args


def kernel_dims(calib_dims, k):
    return tuple(min(int(k), int(c)) for c in calib_dims)


def check_size(kdims, C):
    K3 = int(np.prod(kdims))
    if K3 * C > MAX_KC:
        raise ValueError("ecalib: kernel %s x %d coils = %d columns of the calibration matrix, at most %d are supported: "
                         "choose a smaller kernel (-k) or compress the coils first" % (kdims, C, K3 * C, MAX_KC))
    return K3


def calib_from_noncart(B, ksp, traj, r, K3C, osf=640 / 480, width=3):
    """ksp: (1, readout, views, C[, 1, ..., T]), traj: (3, readout, views[, 1, ..., T]) in pixels -> the (r, r, r, C) complex128
    calibration block from the samples with max_a |k_a| <= r / 2 of all frames (step 1 of the module docstring)"""
    from indigo_amd.solvers import power_iteration
    from indigo_amd.transforms import reserve_for
    ksp = np.asarray(ksp)
    traj = np.asarray(traj, dtype=np.float64)
    C = ksp.shape[3]
    T = int(np.prod(ksp.shape[4:]))
    T_traj = int(np.prod(traj.shape[3:]))
    assert T_traj in (1, T), "traj has %d time frames, data has %d" % (T_traj, T)
    k = traj.reshape((3, -1, T_traj), order='F')
    y = ksp.reshape((-1, C, T), order='F')
    pts, vals = [], []
    for t in range(T):
        kt = k[:, :, t if T_traj > 1 else 0]
        inside = np.abs(kt).max(axis=0) <= r / 2.0
        pts.append(kt[:, inside])
        vals.append(y[inside, :, t])
    pts, vals = np.concatenate(pts, axis=1), np.concatenate(vals, axis=0)
    npts = pts.shape[1]
    log.info("calibration region %d^3: %d of %d samples (%d frames pooled)", r, npts, k.shape[1] * T, T)
    if npts < K3C:
        raise ValueError("ecalib: %d samples inside the calibration region |k| <= %g, fewer than the %d columns of the calibration "
                         "matrix: enlarge -r or choose a smaller kernel (-k)" % (npts, r / 2.0, K3C))
    coord = (pts / float(r)).reshape((3, npts, 1))
    F1 = B.NUFFT((1, npts, 1), (r, r, r), coord, width=width, oversamp=(osf, osf, osf), dtype=_C64)
    A = B.KronI(C, F1)
    AHA = A.H * A
    AHA._name = 'calibration'
    reserve_for(AHA, 1, slack_products=6)
    b = A.H * np.asfortranarray(vals.astype(_C64).reshape((-1, 1), order='F'))
    scale = abs(b).max()
    if not scale > 0:
        raise ValueError("ecalib: the samples inside the calibration region are all zero")
    b /= scale
    L = power_iteration(B, AHA, POWER_ITERS)
    lamda = LAMDA_FRACTION * L
    log.info("calibration images: largest eigenvalue of F^H F %.6e, lamda %.6e, %d CG iterations", L, lamda, CG_ITERS)
    x = np.zeros((r ** 3 * C, 1), dtype=_C64, order='F')
    B.cg(AHA, b, x, lamda=lamda, maxiter=CG_ITERS)
    B.release_scratch()
    img = x.reshape((r, r, r, C), order='F').astype(np.complex128)
    ax = (0, 1, 2)
    return np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(img, axes=ax), axes=ax), axes=ax) / np.sqrt(float(r) ** 3)


def projector(calib, k, t):
    """-> (P, kdims): the projector onto the space of the calibration windows, (K3 C)^2 complex128, rows and columns ordered
    (kappa_0, kappa_1, kappa_2, c) with kappa_0 fastest and c slowest"""
    s = np.asarray(calib, dtype=np.complex128)
    C = s.shape[3]
    kdims = kernel_dims(s.shape[:3], k)
    K3 = check_size(kdims, C)
    win = np.lib.stride_tricks.sliding_window_view(s, kdims, axis=(0, 1, 2))              # (w0, w1, w2, C, k0, k1, k2)
    H = win.transpose(0, 1, 2, 3, 6, 5, 4).reshape((-1, K3 * C))                          # row q: h_q, kappa_0 fastest, c slowest
    gamma = H.T @ H.conj()
    ev, w = np.linalg.eigh(gamma)
    sigma = np.sqrt(np.maximum(ev, 0))
    keep = sigma > t * sigma[-1]
    log.info("calibration matrix %d windows x %d, kept %d singular vectors above %g x %.4e", H.shape[0], K3 * C, int(keep.sum()), t, sigma[-1])
    wk = w[:, keep]
    return wk @ wk.conj().T, kdims


def correlation_boxes(P, kdims, C):
    """R[delta + k - 1, c, c'] = sum_{kappa - kappa' = delta} P[(kappa, c), (kappa', c')], shape (2 k_a - 1) + (C, C)"""
    k0, k1, k2 = kdims
    P8 = P.reshape((C, k2, k1, k0, C, k2, k1, k0))                                         # (c, kappa reversed, c', kappa' reversed)
    R = np.zeros((2 * k0 - 1, 2 * k1 - 1, 2 * k2 - 1, C, C), dtype=np.complex128)
    for a0 in range(k0):
        for a1 in range(k1):
            for a2 in range(k2):
                blk = P8[:, a2, a1, a0].transpose(4, 3, 2, 0, 1)                           # (kappa'_0, kappa'_1, kappa'_2, c, c')
                # delta + k - 1 = kappa + (k - 1 - kappa'): ascending kappa' is descending delta
                R[a0:a0 + k0, a1:a1 + k1, a2:a2 + k2] += blk[::-1, ::-1, ::-1]
    return R


def eigenmaps(B, R, kdims, dims, M, iters=30, crop=0.8):
    """steps 3 and 4 of the module docstring: -> maps dims + (C, M) complex64, evals dims + (M,) float32"""
    dims = tuple(int(n) for n in dims)
    C = R.shape[3]
    bdims = R.shape[:3]
    if any(b > n for b, n in zip(bdims, dims)):
        raise ValueError("ecalib: kernel %s needs an image of at least %s, this one is %s" % (tuple(kdims), bdims, dims))
    N, K3 = int(np.prod(dims)), int(np.prod(kdims))
    phase = 1
    for a in range(3):
        delta = np.arange(bdims[a]) - (bdims[a] // 2)
        ph = np.exp(-2j * np.pi * delta * (dims[a] // 2) / dims[a])
        phase = phase * ph.reshape([-1 if j == a else 1 for j in range(3)])
    pairs = [(p, q) for p in range(C) for q in range(p, C)]
    boxes = np.stack([(R[..., p, q] * phase / K3).reshape(-1, order='F') for p, q in pairs], axis=1)
    log.info("G: %d volumes of %s, %.1f MB of device memory", len(pairs), dims, 8e-6 * N * len(pairs))
    box_d = B.copy_array(np.asfortranarray(boxes.astype(_C64)), name='ecalib.boxes')
    G = B.empty_array((N, len(pairs)), _C64, name='ecalib.G')
    B.place_wrapped(G, box_d, dims, bdims)
    for j in range(len(pairs)):
        col = G[:, j:j + 1].reshape(dims + (1,))
        B.ifftn(col, col)
    maps = B.empty_array((N, C * M), _C64, name='ecalib.maps')
    evals = B.empty_array((N, M), np.dtype('float32'), name='ecalib.evals')
    B.espirit_eig(maps, evals, G, N, C, M, iters=iters, crop=crop)
    return maps.to_host().reshape(dims + (C, M), order='F'), evals.to_host().reshape(dims + (M,), order='F')


def ecalib(B, calib, dims, k=6, t=0.001, crop=0.8, M=2, iters=30):
    """calib: the (cx, cy, cz, C) calibration block -> (maps dims + (C, M), evals dims + (M,))"""
    calib = np.asarray(calib)
    assert calib.ndim == 4, calib.shape
    C = calib.shape[3]
    if not 1 <= M <= min(4, C):
        raise ValueError("ecalib: %d sets of maps from %d coils, between 1 and min(4, coils) are supported" % (M, C))
    if C > 32:
        raise ValueError("ecalib: %d coils, at most 32 are supported (Backend.espirit_eig): compress the coils first" % C)
    P, kdims = projector(calib, k, t)
    R = correlation_boxes(P, kdims, C)
    return eigenmaps(B, R, kdims, dims, M, iters=iters, crop=crop)


def image_dims(spec, z, traj):
    if spec:
        dims = tuple(int(v) for v in spec.split(":"))
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError("--dims: expected X:Y:Z, got %r" % spec)
        return dims
    if 'maps' in z:
        return tuple(int(n) for n in z['maps'].T.shape[:3])
    if traj is None:
        raise ValueError("ecalib: the image size is unknown: the file has neither `maps` nor `traj`; give --dims X:Y:Z")
    ext = np.abs(np.asarray(traj).reshape((3, -1), order='F')).max(axis=1)
    dims = tuple(int(2 * np.ceil(e - 1e-9)) for e in ext)
    log.warning("image size %s taken from the trajectory's extent; give --dims X:Y:Z if the trajectory does not reach the edge of k-space", dims)
    return dims


def main(argv=None, backend=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=args.debug)
    if not args.data.endswith(".npz"):
        raise SystemExit("ecalib: %s: only .npz scans are read" % args.data)
    z = np.load(args.data)
    traj = z['traj'].T if 'traj' in z else None
    dims = image_dims(args.dims, z, traj)
    if 'calib' in z:
        calib = z['calib'].T
        if calib.ndim != 4:
            raise ValueError("ecalib: calib must be (cx, cy, cz, C) stored reversed, got %s" % (calib.shape,))
        check_size(kernel_dims(calib.shape[:3], args.k), calib.shape[3])
    elif 'data' not in z or traj is None:
        raise ValueError("ecalib: %s has neither `calib` nor `data` and `traj`" % args.data)
    if backend is None:
        from indigo_amd.backends import get_backend
        backend = get_backend(args.backend, device_id=args.device)
    log.info("using backend: %s", type(backend).__name__)
    if 'calib' not in z:
        ksp = z['data'].T
        C = ksp.shape[3]
        K3 = check_size(kernel_dims((args.r,) * 3, args.k), C)
        calib = calib_from_noncart(backend, ksp, traj, args.r, K3 * C, osf=args.osf, width=args.width)
    log.info("calib %s, image %s, kernel %d, sets of maps %d, crop %g", calib.shape, dims, args.k, args.m, args.c)
    maps, evals = ecalib(backend, calib, dims, k=args.k, t=args.t, crop=args.c, M=args.m, iters=args.iters)
    stem = os.path.splitext(args.data)[0]
    np.save(stem + ".maps.npy", maps.T)
    np.save(stem + ".evals.npy", evals.reshape(dims + (1, args.m)).T)
    log.info("calibration complete: %s.maps.npy %s, %s.evals.npy", stem, maps.shape, stem)
    return maps, evals


if __name__ == "__main__":
    main()
