#!/usr/bin/env python3
"""Coil compression and noise prewhitening: a scan of C physical coils cut to V virtual ones (`bart cc`, `bart whiten`).

    python -m indigo_amd.cc (-p V | -e E) [-r R] [--noise FILE.npy] [--chunk N] scan.npz

writes `<name>.cc.npz`, the scan with the COIL axis of `data`, `maps` and `calib` (those it holds) cut to V and every other array as
it was -- `python -m indigo_amd.ecalib` and `python -m indigo_amd.pics` run on it unchanged --, `<name>.ccmat.npy`, the compression
matrix A as a plain (V, C) complex128 array, and `<name>.ccvals.npy`, all C eigenvalues in descending order (float64).

The definition (tests/cc64.py restates it in float64).  A sample i carries the coil vector y_i in C^C.

    Gram          G[p, q] = sum_i y_i[p] conj(y_i[q])                          Hermitian, positive semi-definite
    noise         Psi = (1 / m) sum_j nu_j nu_j^H = L L^H                      m noise samples nu_j; Cholesky; without noise L = I
    whitening     y -> L^-1 y                                                  (a Psi that is not positive definite is an error)
    compression   G_w = L^-1 G L^-H = U Lambda U^H,   A = U[:, :V]^H L^-1      eigenvalues descending, V x C

Every eigenvector is rotated so that its largest-magnitude component is real and positive.  Compressed data are y'_i = A y_i and
compressed maps S'(x) = A S(x): the same A for every frame, every set of maps and `calib`.  One Gram pass over the unwhitened data
serves both steps.  `-p V` sets V; `-e E` takes the smallest V whose leading eigenvalues hold the fraction E of their sum.
1 <= V <= min(C, 32) and C <= 64.

Where the work runs.  G is a tall-skinny Hermitian rank-n update over every sample of the scan, `Backend.coil_gram`
(ig_coil_gram_c64 on the device: float32-input MFMA, one partial sum per slab, the slabs added on the host in float64).  L, the
eigen-decomposition and A are C x C host work in float64.  The mix y' = A y is `Backend.coil_mix`, which is `Backend.frame_basis`
with phi = A^H and adjoint=True (ig_basis_c64 with nt = C, nk = V: the bound of 32 on V is that kernel's bound on nk).  Host arrays go
through the device in chunks of at most `--chunk` samples.

Calibration samples: every sample of every frame (`bart cc -A`), or with `-r R` the samples with max_a |k_a| <= R / 2, the selection
rule of ecalib's step 1 (a host mask; the subset is uploaded).  `--noise FILE.npy` holds (samples, C) stored reversed, like every
array of a scan.

Left out: geometric and ESPIRiT-based compression (`bart cc -G / -E`), more than 32 virtual or 64 physical coils,
compression inside the operator tree.

The backend is the MI355X one (`hip`); `main(argv, backend=...)` lets the CPU test-suite drive the same code with the numpy oracle.
"""
import argparse
import logging
import os
import sys

import numpy as np

log = logging.getLogger("cc")
_C64 = np.dtype('complex64')

MAX_COILS = 64          # Backend.coil_gram
MAX_VIRTUAL = 32        # Backend.coil_mix = Backend.frame_basis: ig_basis_c64 keeps nk <= 32 accumulators per voxel
CHUNK = 1 << 21         # samples of a host array on the device at a time: 1 GB at 64 coils
COIL = 3                # the COIL axis of data, maps and calib


def _panels(array, coil_axis):
    """the array as (samples, C, panels), F-order: everything before the coil axis is a sample, everything after it a panel"""
    a = np.asarray(array)
    assert a.ndim > coil_axis, (a.shape, coil_axis)
    inner, outer = int(np.prod(a.shape[:coil_axis], dtype=np.int64)), int(np.prod(a.shape[coil_axis + 1:], dtype=np.int64))
    return a.reshape((inner, a.shape[coil_axis], outer), order='F')


def check_coils(C):
    if not 1 <= C <= MAX_COILS:
        raise ValueError("cc: %d coils, between 1 and %d are supported (Backend.coil_gram)" % (C, MAX_COILS))


def check_virtual(V, C):
    if not 1 <= V <= min(C, MAX_VIRTUAL):
        raise ValueError("cc: %d virtual coils from %d coils, between 1 and min(coils, %d) = %d are supported "
                         "(Backend.coil_mix keeps at most %d)" % (V, C, MAX_VIRTUAL, min(C, MAX_VIRTUAL), MAX_VIRTUAL))


def gram_of(B, *arrays, coil_axis=COIL, chunk=CHUNK):
    """G = sum over every sample of every array of y y^H, (C, C) complex128: the arrays' samples pooled (all frames of `data`, all
    sets of `maps`), each (samples, C) panel through `Backend.coil_gram` in chunks of at most `chunk` samples"""
    G = None
    for array in arrays:
        v = _panels(array, coil_axis)
        n, C, outer = v.shape
        check_coils(C)
        if G is None:
            G = np.zeros((C, C), dtype=np.complex128)
        if G.shape[0] != C:
            raise ValueError("cc: arrays of %d and of %d coils cannot share a Gram matrix" % (G.shape[0], C))
        for o in range(outer):
            for i0 in range(0, n, chunk):
                rows = min(chunk, n - i0)
                x_d = B.copy_array(np.asfortranarray(v[i0:i0 + rows, :, o].astype(_C64, copy=False)), name='cc.panel')
                G += B.coil_gram(x_d, rows, C)
                del x_d
    if G is None:
        raise ValueError("cc: no array to take the Gram matrix of")
    return G


def choose(lam, V=None, energy=None):
    """the number of virtual coils: V itself, or the smallest V whose leading eigenvalues sum to at least energy * their total"""
    if (V is None) == (energy is None):
        raise ValueError("cc: give either the number of virtual coils (-p) or the energy fraction (-e), not both")
    C = lam.size
    if V is None:
        if not 0 < energy <= 1:
            raise ValueError("cc: energy fraction %g, must be in (0, 1]" % energy)
        pos = np.maximum(lam, 0)
        V = int(np.searchsorted(np.cumsum(pos), energy * pos.sum(), side='left')) + 1
        V = min(V, C)
        log.info("energy %g: %d virtual coils", energy, V)
    check_virtual(int(V), C)
    return int(V)


def matrix(G, V=None, energy=None, noise_cov=None):
    """-> (A, eigenvalues): the V x C compression (and whitening) matrix A = U[:, :V]^H L^-1 of the module docstring, complex128, and
    all C eigenvalues of L^-1 G L^-H in descending order, float64"""
    G = np.asarray(G, dtype=np.complex128)
    assert G.ndim == 2 and G.shape[0] == G.shape[1], G.shape
    C = G.shape[0]
    check_coils(C)
    Linv = np.eye(C, dtype=np.complex128)
    if noise_cov is not None:
        Psi = np.asarray(noise_cov, dtype=np.complex128)
        if Psi.shape != (C, C):
            raise ValueError("cc: a noise covariance of %s for %d coils" % (Psi.shape, C))
        # (a singular Psi can pass the factorisation with a pivot of rounding size: the samples are float32, and a pivot 1e-6 of
        # the largest says that Psi has no more than rounding in that direction)
        try:
            L = np.linalg.cholesky((Psi + Psi.conj().T) / 2)
            pivots = np.abs(np.diag(L))
            if not pivots.min() > 1e-6 * pivots.max():
                raise np.linalg.LinAlgError("pivot")
        except np.linalg.LinAlgError:
            raise ValueError("cc: the noise covariance is not positive definite (fewer independent noise samples than coils?)")
        import scipy.linalg
        Linv = scipy.linalg.solve_triangular(L, np.eye(C, dtype=np.complex128), lower=True)
    Gw = Linv @ G @ Linv.conj().T
    lam, U = np.linalg.eigh((Gw + Gw.conj().T) / 2)
    lam, U = lam[::-1].copy(), U[:, ::-1].copy()
    V = choose(lam, V, energy)
    big = np.argmax(np.abs(U), axis=0)
    pivot = U[big, np.arange(C)]
    U = U * (np.conj(pivot) / np.abs(pivot))[None, :]
    U[big, np.arange(C)] = np.abs(pivot)
    return U[:, :V].conj().T @ Linv, lam


def apply(B, A, array, coil_axis=COIL, chunk=CHUNK):
    """the array with A applied along its coil axis (C -> V), complex64: every (samples, C) panel -- a time frame of `data`, a set
    of `maps`, `calib` -- goes through `Backend.coil_mix` in chunks of at most `chunk` samples"""
    A = np.asarray(A)
    a = np.asarray(array)
    V, C = A.shape
    if a.shape[coil_axis] != C:
        raise ValueError("cc: an array of %d coils and a matrix for %d" % (a.shape[coil_axis], C))
    v = _panels(a, coil_axis)
    n, _, outer = v.shape
    out = np.empty((n, V, outer), dtype=_C64, order='F')
    for o in range(outer):
        for i0 in range(0, n, chunk):
            rows = min(chunk, n - i0)
            x_d = B.copy_array(np.asfortranarray(v[i0:i0 + rows, :, o].astype(_C64, copy=False)), name='cc.panel')
            y_d = B.empty_array((rows, V), _C64, name='cc.mixed')
            B.coil_mix(y_d, x_d, A, rows)
            out[i0:i0 + rows, :, o] = y_d.to_host()
            del x_d, y_d
    return out.reshape(a.shape[:coil_axis] + (V,) + a.shape[coil_axis + 1:], order='F')


def compress(B, ksp, mps, V=None, energy=None, noise_cov=None, chunk=CHUNK):
    """ksp (1, readout, views, C, 1, ..., T) and mps (X, Y, Z, C[, M]) cut to V virtual coils with the matrix of all samples of
    all frames -> (ksp', mps', A, eigenvalues)"""
    ksp, mps = np.asarray(ksp), np.asarray(mps)
    if ksp.shape[COIL] != mps.shape[COIL]:
        raise ValueError("cc: data has %d coils, maps have %d" % (ksp.shape[COIL], mps.shape[COIL]))
    A, lam = matrix(gram_of(B, ksp, chunk=chunk), V=V, energy=energy, noise_cov=noise_cov)
    log.info("coil compression %d -> %d, leading eigenvalues hold %.6f of the sum", A.shape[1], A.shape[0],
             lam[:A.shape[0]].sum() / max(lam.sum(), 1e-300))
    return apply(B, A, ksp, chunk=chunk), apply(B, A, mps, chunk=chunk), A, lam


def central_samples(ksp, traj, r):
    """the (samples, C) panels, one per frame, of the samples with max_a |k_a| <= r / 2 (ecalib's rule, step 1 of its docstring)"""
    ksp = np.asarray(ksp)
    traj = np.asarray(traj, dtype=np.float64)
    C = ksp.shape[COIL]
    T, T_traj = int(np.prod(ksp.shape[4:])), int(np.prod(traj.shape[3:]))
    assert T_traj in (1, T), "traj has %d time frames, data has %d" % (T_traj, T)
    k = traj.reshape((3, -1, T_traj), order='F')
    y = ksp.reshape((-1, C, T), order='F')
    picked = [y[np.abs(k[:, :, t if T_traj > 1 else 0]).max(axis=0) <= r / 2.0, :, t] for t in range(T)]
    picked = [p for p in picked if p.shape[0]]
    log.info("calibration region |k| <= %g: %d of %d samples", r / 2.0, sum(p.shape[0] for p in picked), y.shape[0] * T)
    if not picked:
        raise ValueError("cc: no sample inside the calibration region |k| <= %g: enlarge -r" % (r / 2.0))
    return picked


def parse(argv):
    ap = argparse.ArgumentParser(prog="indigo_amd.cc", description="Coil compression and noise prewhitening: writes <name>.cc.npz (the scan with V "
                                 "virtual coils), <name>.ccmat.npy (the V x C matrix) and <name>.ccvals.npy (all eigenvalues).")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument('-p', type=int, default=None, help='number of virtual coils V (1 ... min(C, 32))')
    how.add_argument('-e', type=float, default=None, help='energy fraction: the smallest V whose leading eigenvalues hold it')
    ap.add_argument('-r', type=int, default=None, help='calibrate on the samples with max |k_a| <= r / 2 only (default: every sample of every frame)')
    ap.add_argument('--noise', default=None, help='noise samples, a .npy file with (samples, C) stored reversed: prewhiten with their covariance')
    ap.add_argument('--chunk', type=int, default=CHUNK, help='samples of a host array on the device at a time')
    ap.add_argument('--backend', type=str, default='hip', choices=['hip'])
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--debug', type=int, default=logging.INFO, help='logging level')
    ap.add_argument('data', help='.npz scan: `data` (and `traj` for -r), `maps` and `calib` if it has them')
    args = ap.parse_args(argv)
    if args.chunk < 1 or (args.r is not None and args.r < 1):
        ap.error("--chunk and -r must be at least 1")
    return args


def main(argv=None, backend=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=args.debug)
    if not args.data.endswith(".npz"):
        raise SystemExit("cc: %s: only .npz scans are read" % args.data)
    z = np.load(args.data)
    source = 'data' if 'data' in z else 'calib' if 'calib' in z else None
    if source is None:
        raise ValueError("cc: %s has neither `data` nor `calib`" % args.data)
    src = z[source].T
    if src.ndim <= COIL:
        raise ValueError("cc: %s must have a COIL axis (dimension %d), got %s" % (source, COIL, src.shape))
    C = src.shape[COIL]
    check_coils(C)
    cut = [name for name in ('data', 'maps', 'calib') if name in z]
    for name in cut:
        shape = z[name].T.shape
        if len(shape) <= COIL or shape[COIL] != C:
            raise ValueError("cc: %s has %s coils, %s has %d" % (name, shape[COIL] if len(shape) > COIL else 'no', source, C))
    if args.p is not None:
        check_virtual(args.p, C)                                        # before any device work
    noise = None
    if args.noise is not None:
        noise = np.load(args.noise).T
        if noise.ndim != 2 or noise.shape[1] != C:
            raise ValueError("cc: the noise file holds %s, expected (samples, %d coils) stored reversed" % (noise.shape, C))
    if backend is None:
        from indigo_amd.backends import get_backend
        backend = get_backend(args.backend, device_id=args.device)
    log.info("using backend: %s", type(backend).__name__)
    if args.r is not None:
        if source != 'data' or 'traj' not in z:
            raise ValueError("cc: -r selects samples by their trajectory: the scan needs `data` and `traj`")
        G = gram_of(backend, *central_samples(src, z['traj'].T, args.r), coil_axis=1, chunk=args.chunk)
    else:
        G = gram_of(backend, src, chunk=args.chunk)
    Psi = None
    if noise is not None:
        Psi = gram_of(backend, noise, coil_axis=1, chunk=args.chunk) / noise.shape[0]
    A, lam = matrix(G, V=args.p, energy=args.e, noise_cov=Psi)
    V = A.shape[0]
    log.info("%d coils -> %d virtual coils%s; leading eigenvalues hold %.6f of the sum", C, V, ", prewhitened" if Psi is not None else "",
             lam[:V].sum() / max(lam.sum(), 1e-300))
    out = {name: z[name] for name in z.files}
    for name in cut:
        out[name] = apply(backend, A, z[name].T, chunk=args.chunk).T
    stem = os.path.splitext(args.data)[0]
    np.savez(stem + ".cc.npz", **out)
    np.save(stem + ".ccmat.npy", A)
    np.save(stem + ".ccvals.npy", lam)
    log.info("compression complete: %s.cc.npz, %s.ccmat.npy %s, %s.ccvals.npy", stem, stem, A.shape, stem)
    return A, lam


if __name__ == "__main__":
    main()
