#!/usr/bin/env python3
"""NLINV: the image and the coil sensitivities as joint unknowns of one bilinear model, by regularised nonlinear inversion
(Uecker et al., MRM 60:674, 2008; `bart nlinv`).  No calibration region is needed: what a scan with a thin k-space centre (few
spokes, real-time radial) gets its coil maps from when `ecalib` cannot.

    python -m indigo_amd.nlinv [-i 8] [--cg-iters 10] [--alpha 1] [--redu 2] [--sobolev-a 220] [--sobolev-b 32] [--osf O] [--width W]
                               [--dims X:Y:Z] [--cc V] scan.npz

writes `<name>.nlinv.npy`, the image (X, Y, Z), and `<name>.maps.npy`, the maps (X, Y, Z, C, 1), both stored reversed like every array
of the scan; the maps file is what `pics --maps` reads.

The definition (tests/nlinv64.py restates it in float64).  The volume has dims = (n0, n1, n2), N voxels, F-ordered,
and there are C coils.  The unknown is u = (rho, c^_1 ... c^_C), one column of N (1 + C) complex64 values, rho in rows [0, N) and c^_c
in rows [N (1 + c), N (2 + c)).

  Coil weighting.  c_c = W c^_c = (1 / sqrt N) ifftn(w * c^_c),  W^H z = w * fftn(z) / sqrt N, with the backend's plain, uncentred,
      unnormalised transforms and w(k) = (1 + a |kappa|^2)^(-b/2), kappa_a = k'_a / n_a, k'_a = k_a if 2 k_a <= n_a else k_a - n_a
      (operators.SobolevCoils).  w is real and even: W commutes with shifts, no centring modulation is needed.
  Model.  F(u) = A vec_c(rho * c_c),  A = L^(-1/2) KronI(C, NUFFT): trajectory (in pixels), width and osf as pics and ecalib take
      them; L is the largest eigenvalue of F_1^H F_1 for one coil (ten power iterations, as ecalib's).  The data are scaled to
      ||y|| = 100, s = 100 / ||y_file||.
  Derivative.  DF(u)[d rho, d c^] = A vec_c(d rho * c_c + rho * W d c^_c) = A * NlinvProduct * SobolevCoils, an ordinary tree;
      its adjoint with z = A^H r:  d rho = sum_c conj(c_c) z_c,  d c^_c = W^H(conj(rho) z_c).
  IRGNM.  u_0 = (1, 0).  alpha_n = alpha_0 q^(-n).  For n = 0 ... iters - 1:
      (DF^H DF + alpha_n I) du = DF^H (y - F(u_n)) + alpha_n (u_0 - u_n)      by `Backend.cg` from du = 0, cg_iters iterations,
      u_{n+1} = u_n + du.
  Results.  c = W c^, rss = sqrt(sum_c |c_c|^2); image = rho rss / (s sqrt L), in the units of the file's data; maps = c_c / rss, zero
      where rss = 0, the phase kept: image * maps = rho c / (s sqrt L).

One time frame only.  `--cc V` compresses the coils first, as `pics --cc` does (all samples, no whitening).

Left out: the fused SENSE leaf's transforms in place of KronI(C, NUFFT), the coil transform as a padded FFT of the
few k-space points where w is not negligible, time frames with temporal regularisation, ENLIVE, Cartesian data, a Toeplitz normal
operator.

The backend is the MI355X one (`hip`); `main(argv, backend=...)` lets the CPU test-suite drive the same code with the numpy oracle.
"""
import argparse
import logging
import os
import sys

import numpy as np

log = logging.getLogger("nlinv")
_C64 = np.dtype('complex64')

POWER_ITERS = 10
DATA_NORM = 100.0


def parse(argv):
    ap = argparse.ArgumentParser(prog="indigo_amd.nlinv", description="NLINV: image and coil maps jointly from a non-Cartesian scan without calibration "
                                 "data, written as <name>.nlinv.npy and <name>.maps.npy (for pics --maps).")
    ap.add_argument('-i', type=int, default=8, help='Newton steps')
    ap.add_argument('--cg-iters', type=int, default=10, help='CG iterations per Newton step')
    ap.add_argument('--alpha', type=float, default=1.0, help='regularisation weight of the first Newton step')
    ap.add_argument('--redu', type=float, default=2.0, help='the weight is divided by this after every step')
    ap.add_argument('--sobolev-a', type=float, default=220.0, help='a of the coil weight (1 + a |k|^2)^(-b/2)')
    ap.add_argument('--sobolev-b', type=float, default=32.0, help='b of the coil weight (1 + a |k|^2)^(-b/2)')
    ap.add_argument('--osf', type=float, default=640 / 480, help='gridding oversampling factor, as in pics')
    ap.add_argument('--width', type=int, default=3, help='Kaiser-Bessel kernel half-width, as in pics')
    ap.add_argument('--dims', default=None, help='image size X:Y:Z (default: that of the file\'s maps, else from the trajectory\'s extent)')
    ap.add_argument('--cc', type=int, default=None, help='compress the coils of data to this many virtual coils first (indigo_amd.cc: all samples, no whitening)')
    ap.add_argument('--backend', type=str, default='hip', choices=['hip'])
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--debug', type=int, default=logging.INFO, help='logging level')
    ap.add_argument('data', help='.npz scan: `data` and `traj` as pics reads them')
    args = ap.parse_args(argv)
    if args.i < 0 or args.cg_iters < 1:
        ap.error("-i must not be negative, --cg-iters at least 1")
    if not (args.alpha > 0 and args.redu >= 1 and args.sobolev_a >= 0):
        ap.error("--alpha must be positive, --redu at least 1, --sobolev-a not negative")
    return args


def nlinv(B, ksp, traj, dims, iters=8, cg_iters=10, alpha=1.0, redu=2.0, a=220.0, b=32.0, osf=640 / 480, width=3, state=None):
    """ksp: (1, readout, views, C), traj: (3, readout, views) in pixels -> (image dims complex64, maps dims + (C,) complex64, history):
    the steps of the module docstring; history holds one {'alpha', 'cg_iters', 'residual'} per Newton step, residual being
    ||y - F(u_{n+1})|| / ||y|| after the step.  state: a dict that receives the iterate the results are made of: 'rho' (N,) and 'coils'
    (N, C) complex64 as the device holds them, 'L' and 's'."""
    from indigo_amd.solvers import power_iteration
    from indigo_amd.transforms import reserve_for
    ksp = np.asarray(ksp)
    traj = np.array(traj, dtype=np.float64)
    if ksp.ndim < 4 or int(np.prod(ksp.shape[4:])) != 1 or int(np.prod(traj.shape[3:])) != 1:
        raise ValueError("nlinv: data %s and traj %s: one time frame only, (1, readout, views, C) and (3, readout, views) "
                         "(time frames are a follow-up)" % (ksp.shape, traj.shape))
    dims = tuple(int(n) for n in dims)
    ksp = ksp.reshape(ksp.shape[:4])
    traj = traj.reshape(traj.shape[:3])
    nro, nsp, C = ksp.shape[1:4]
    assert traj.shape == (3, nro, nsp), (traj.shape, ksp.shape)
    N = int(np.prod(dims))
    ynorm = float(np.linalg.norm(ksp.astype(np.complex128).ravel()))
    if not ynorm > 0:
        raise ValueError("nlinv: the data are all zero")
    s = DATA_NORM / ynorm
    coord = traj / np.array(dims, dtype=np.float64)[:, None, None]       # in units of the field of view, as pics does
    F1 = B.NUFFT((1, nro, nsp), dims, coord, width=width, oversamp=(osf, osf, osf), dtype=_C64)
    F1HF1 = F1.H * F1
    reserve_for(F1HF1, 1, slack_products=6)
    L = power_iteration(B, F1HF1, POWER_ITERS)
    if not L > 0:
        raise ValueError("nlinv: the largest eigenvalue of F^H F came out as %g" % L)
    A = (1.0 / np.sqrt(L)) * B.KronI(C, F1)
    P = B.NlinvProduct(N, C)
    S = B.SobolevCoils(dims, C, a, b)
    DF = A * P * S
    DFHDF = DF.H * DF
    DFHDF._name = 'NLINV'
    reserve_for(DFHDF, 1, slack_products=6)
    log.info("tree:\n%s", DFHDF.dump())
    log.info("image %s, coils %d, samples %d x %d, largest eigenvalue of F^H F %.6e, data scale %.6e, sobolev (%g, %g)", dims, C, nro, nsp, L, s, a, b)

    y = B.copy_array(np.asfortranarray((ksp.astype(np.complex128) * s).astype(_C64).reshape((-1, 1), order='F')), name='nlinv.y')
    u0_h = np.zeros((N * (1 + C), 1), dtype=_C64, order='F')
    u0_h[:N] = 1
    u0 = B.copy_array(u0_h, name='nlinv.u0')
    u = B.copy_array(u0_h, name='nlinv.u')
    cu = B.zero_array((N * (1 + C), 1), _C64, name='nlinv.point')        # (rho, c) = SobolevCoils u: the linearisation point
    du = B.zero_array((N * (1 + C), 1), _C64, name='nlinv.du')
    rhs = B.zero_array((N * (1 + C), 1), _C64, name='nlinv.rhs')
    pc = B.zero_array((N * C, 1), _C64, name='nlinv.coil images')
    r = B.zero_array((nro * nsp * C, 1), _C64, name='nlinv.residual')
    rho_d, coils_d = cu.dense_rows(0, N), cu.dense_rows(N, N * (1 + C))

    def residual():
        """the point of u, r = y - F(u) -> ||r|| / ||y||"""
        S.eval(cu, u)
        P.set_point(rho_d, coils_d)
        B.coil_maps(pc, rho_d, coils_d, N, C, 1)                         # rho * c_c: the map product with one set of maps
        A.eval(r, pc)
        B.axpby(-1, r, 1, y)
        return float(np.sqrt(B.norm2(r))) / DATA_NORM

    history = []
    res = residual()
    log.info("start: residual %.6e", res)
    for n in range(int(iters)):
        alpha_n = float(alpha) * float(redu) ** (-n)
        DF.eval(rhs, r, forward=False)
        B.axpby(1, rhs, alpha_n, u0)
        B.axpby(1, rhs, -alpha_n, u)
        du._zero()
        trail = B.cg(DFHDF, rhs, du, lamda=alpha_n, maxiter=int(cg_iters))
        B.axpby(1, u, 1, du)
        res = residual()
        history.append({'alpha': alpha_n, 'cg_iters': len(trail or []), 'residual': res})
        log.info("newton step %d: alpha %.6e, %d CG iterations, residual %.6e", n, alpha_n, history[-1]['cg_iters'], res)

    point = cu.to_host().reshape((N, 1 + C), order='F')
    del DFHDF, DF, A, F1HF1
    B.release_scratch()
    if state is not None:
        state.update(rho=point[:, 0].copy(), coils=point[:, 1:].copy(), L=L, s=s)
    rho, c = point[:, 0].astype(np.complex128), point[:, 1:].astype(np.complex128)
    rss = np.sqrt((np.abs(c) ** 2).sum(axis=1))
    image = (rho * rss / (s * np.sqrt(L))).astype(_C64).reshape(dims, order='F')
    with np.errstate(divide='ignore', invalid='ignore'):
        maps = np.where(rss[:, None] > 0, c / rss[:, None], 0).astype(_C64).reshape(dims + (C,), order='F')
    return image, maps, history


def main(argv=None, backend=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=args.debug)
    if not args.data.endswith(".npz"):
        raise SystemExit("nlinv: %s: only .npz scans are read" % args.data)
    z = np.load(args.data)
    if 'data' not in z or 'traj' not in z:
        raise ValueError("nlinv: %s has no `%s`: NLINV here takes non-Cartesian data, `data` and `traj` as pics reads them "
                         "(Cartesian data are a follow-up)" % (args.data, 'data' if 'data' not in z else 'traj'))
    ksp, traj = z['data'].T, z['traj'].T
    if ksp.ndim < 4 or int(np.prod(ksp.shape[4:])) != 1 or int(np.prod(traj.shape[3:])) != 1:
        raise ValueError("nlinv: %s holds %d time frames (data %s, traj %s): one time frame only (time frames are a follow-up)"
                         % (args.data, int(np.prod(ksp.shape[4:])), ksp.shape, traj.shape))
    from indigo_amd.ecalib import image_dims
    dims = image_dims(args.dims, z, traj)
    if backend is None:
        from indigo_amd.backends import get_backend
        backend = get_backend(args.backend, device_id=args.device)
    log.info("using backend: %s", type(backend).__name__)
    if args.cc is not None:
        from indigo_amd import cc
        mix, lam = cc.matrix(cc.gram_of(backend, ksp), V=args.cc)
        log.info("coil compression %d -> %d, leading eigenvalues hold %.6f of the sum", mix.shape[1], mix.shape[0],
                 lam[:mix.shape[0]].sum() / max(lam.sum(), 1e-300))
        ksp = cc.apply(backend, mix, ksp)
    image, maps, history = nlinv(backend, ksp, traj, dims, iters=args.i, cg_iters=args.cg_iters, alpha=args.alpha, redu=args.redu,
                                 a=args.sobolev_a, b=args.sobolev_b, osf=args.osf, width=args.width)
    stem = os.path.splitext(args.data)[0]
    np.save(stem + ".nlinv.npy", image.T)
    np.save(stem + ".maps.npy", maps.reshape(maps.shape + (1,)).T)
    log.info("nlinv complete: %s.nlinv.npy %s, %s.maps.npy %s", stem, image.shape, stem, maps.shape + (1,))
    return image, maps, history


if __name__ == "__main__":
    main()
