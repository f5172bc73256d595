#!/usr/bin/env python3
"""Parallel-imaging reconstruction driver: non-Cartesian SENSE by conjugate gradients, L1-wavelet or locally low-rank FISTA, or
total-variation or total-generalized-variation primal-dual; time frames one by one or in a temporal subspace; soft-SENSE on scans with several sets of coil maps.

    python -m indigo_amd.pics [-i ITER] [--lamda L] [-O LEVEL] [--crop "COIL:2,TIME:1"] [--no-fuse] scan.h5 | scan.npz
    python -m indigo_amd.pics --l1 LAMBDA [--wavelet db2] [--levels 3] [--step S | --power-iters 15] ... scan.npz
    python -m indigo_amd.pics --tv MU [--tv-sigma S] [--l1 LAMBDA ...] [--step S | --power-iters 15] ... scan.npz
    python -m indigo_amd.pics --tgv A1 [--tgv-ratio 2.0] [--tgv-sigma S] [--l1 LAMBDA | --llr LAMBDA] [--step S] ... scan.npz
    python -m indigo_amd.pics --tv-time MU_T [--tv MU] [--l1 LAMBDA ...] ... frames.npz         (a scan with several time frames)
    python -m indigo_amd.pics --llr LAMBDA [--llr-block 8] [--llr-shifts [--llr-seed 0]] [--tv MU] [--tv-time MU_T] ... frames.npz
    python -m indigo_amd.pics --basis PHI.npy [--basis-rank K] [--l1 LAMBDA | --llr LAMBDA] [--tv MU] ... frames.npz
    python -m indigo_amd.pics --toeplitz [--basis PHI.npy ...] ... scan.npz | frames.npz        (A^H A as one Toeplitz operator)
    python -m indigo_amd.pics [--l1 | --tv | --llr ...] [--crop "MAPS:1"] espirit.npz           (maps with a MAPS axis of length M: soft-SENSE)
    python -m indigo_amd.pics --maps scan.maps.npy ... scan.npz                                  (maps from python -m indigo_amd.ecalib scan.npz)
    python -m indigo_amd.pics --cc V ... scan.npz                                                (V virtual coils: python -m indigo_amd.cc in passing)
    python -m indigo_amd.pics --fmap B0.npy --dwell 4e-6 [--te 1e-3] [--fmap-segments L] ... scan.npz   (off-resonance correction)
    python -m indigo_amd.pics --fmap B0.npy --times T.npy [--fmap-tol 1e-3] [--toeplitz] ... scan.npz
    python -m indigo_amd.pics --dcf scan.dcf.npy | auto [--dcf-iters 30] ... scan.npz          (density-compensated data term)

The counterpart of the reference's driver script (examples/pics.py:20-95 arguments, data layout and tree
construction, :179-233 recipe, normal equations, CG, output): reads `data` (k-space), `maps` (coil sensitivities)
and `traj` (trajectory, in units of 1/FOV pixels) with the reference's BART-style dimension order

    READ, PHS1, PHS2, COIL, MAPS, ..., TIME (dimension 10)            (stored reversed, hence the `.T`)

builds  A = KronI(C, NUFFT) * VStack(Diag(maps_c)),  rewrites it with `sense_recipe(level)` (= pics.py -O<level>),
and -- where the backend has zero-pad-aware transforms for the grid -- `FuseZpadFFT`, solves
(A^H A + lamda I) x = A^H y with `Backend.cg`, and writes the image back as `rec`.

With `--l1 LAMBDA > 0` (compressed sensing, no counterpart in the reference's driver; `bart pics -R W`) it solves instead

    min_x  1/2 ||A x - y||^2 + lamda/2 ||x||^2 + LAMBDA ||W x||_1        (W: operators.Wavelet, coarse band not penalised)

by `Backend.fista` on the same A and the same normalised A^H y, with the fixed step 0.9 / (largest eigenvalue of
A^H A + lamda I, from `--power-iters` power iterations) unless `--step` gives one.

With `--tv MU > 0` (total variation, `bart pics -R T`; no counterpart in the reference's driver either) it solves

    min_x  1/2 ||A x - y||^2 + lamda/2 ||x||^2 + MU sum_i ||(D x)_i||_2   [ + LAMBDA ||W x||_1  when --l1 is also given ]

(D: operators.Gradient, forward differences; isotropic: the 2-norm of the three complex differences at a voxel) by
`Backend.primal_dual` (Condat-Vu) on the same A and normalised A^H y, with the steps of `tv_solve`.

With `--tgv A1 > 0` (second-order total generalized variation, Bredies, Kunisch, Pock 2010, Knoll et al. 2011; `bart pics -R G`) it
solves

    min_{x, v}  1/2 ||A x - y||^2 + lamda/2 ||x||^2 + A1 sum_i ||(D x - v)_i||_2 + A0 sum_i ||(E v)_i||_F,     A0 = --tgv-ratio * A1

(E: operators.SymGradient, the symmetrised backward difference of the 3-component field v, six components per voxel with the
off-diagonal ones scaled by 1/sqrt(2)), the piecewise-smooth prior: v takes up the smooth part of the differences, so
that an intensity ramp costs nothing where `--tv` turns it into stairs.  `tgv_solve` runs the same `Backend.primal_dual` on the unknown
(x; v) of 4N rows and the dual (p; q) of 9N rows, with `Backend.tgv_adjoint` and `Backend.tgv_dual_step`, one fused kernel each.
`--tgv-ratio` defaults to 2, the choice of Knoll et al.; `--tgv-sigma` is the dual step (default L / 32, ||K||^2 <= 16).  `--tgv` with
`--tv` or `--tv-time` is rejected: one analysis operator per run.  It takes `--l1` or `--llr` in its prox slot, and with several
frames, sets of maps or `--basis` every image gets its own v; `--toeplitz`, `--fmap`, `--dcf` and `--cc` change only A^H A and run
unchanged.

Time frames.  With T = the length of TIME > 1 the image is frame-major (frame t in rows [tN, (t+1)N) of the unknown),
A = BlockDiag(A_t) with A_t built as above from frame t's trajectory (`traj` with a TIME axis of length T) or from the one
trajectory that all frames share (no TIME axis, or length 1; frames with equal trajectories share one operator tree, built
and uploaded once), the maps are those of every frame, and all three solvers run on the stacked vectors: CG solves the block
system jointly, `--l1` and `--tv` act on every frame, and `--tv-time MU_T > 0` adds

    MU_T sum_{t < T-1} sum_i |x_{t+1}[i] - x_t[i]|                       (`bart pics -R T:1024:0:MU_T`)

the term that couples the frames: `tv_solve` then uses operators.GradientT, a dual variable of 4NT rows and
`Backend.tv4_dual_step`, whose temporal component has its own constraint |u_3| <= MU_T.  The result keeps
the TIME axis: (X, Y, Z, 1, ..., T).

Locally low rank.  `--llr LAMBDA > 0` (`bart pics -R L:7:7:LAMBDA -b 8`) adds

    LAMBDA sum_b ||M_b(x)||_*                                              (the nuclear norm: the sum of the singular values)

where the blocks b of `--llr-block B` voxels a side (clamped to the volume; the last block of an axis is shorter) tile the
volume and M_b is the (voxels of block b) x T matrix of the frames' values there.  Its proximal map is block-wise
singular-value thresholding, `Backend.llr_threshold`, which takes the prox slot of the solver: `--llr` alone runs
`Backend.fista` exactly as `--l1` does, with `--tv` and / or `--tv-time` it is the prox of `tv_solve` where the wavelet prox
goes otherwise.  `--llr` with `--l1` is rejected: two non-smooth terms in one slot are not a prox.  Without `--llr-shifts` the
partition is the one at shift (0, 0, 0) and the iteration is a true proximal method on the objective above.  With it a fresh
shift is drawn before every prox call, uniformly in [0, side) per axis from numpy.random.default_rng(--llr-seed) on the host
(every backend sees the same sequence; this is what bart does); the logged objective is that of shift 0 in both cases.  On
one frame every block has rank one and the term shrinks the blocks' 2-norms.

Temporal subspace.  `--basis PHI.npy` (`bart pics -B`; PHI a real or complex T x K array, T the length of TIME, `--basis-rank K`
keeps its first K columns, K <= 32) reconstructs the K coefficient images alpha_k of  x_t = sum_k PHI[t, k] alpha_k  in place of
the T frames: scans of tens to hundreds of frames (multi-echo, T2 shuffling, fingerprinting) whose frames lie in a known
low-dimensional subspace.  With A_t and their trees built as above, lamda left out of the frames,

    A = BlockDiag(A_t) * FrameBasis(PHI, N),    A^H A + lamda I = FrameBasis^H * BlockDiag(A_t^H A_t) * FrameBasis + lamda I_{NK}

(operators.FrameBasis = PHI (x) I_N, `Backend.frame_basis`).  PHI need not be orthonormal (||PHI^H PHI - I|| is
logged; the step comes from the power iteration on this A^H A).  The unknown, the momentum, the TV dual and the LLR panel have K
columns in place of T, and every regulariser acts on the coefficient images: CG solves the NK system, `--l1` thresholds every
coefficient image, `--tv` is the spatial term on every coefficient image, `--llr` penalises the (block voxels) x K matrices, the
T2-shuffling penalty.  `--tv-time` is rejected: differences between coefficient images are not differences in time.  The result
is the coefficient images on the COEFF axis (dimension 6), (X, Y, Z, 1, 1, 1, K), with no TIME axis.

Toeplitz normal operator.  `--toeplitz` (bart's Toeplitz mode) replaces A^H A in every solver by `operators.ToeplitzNormal`:
sum_c S_c^H crop F^-1 P F zpad S_c on the grid of twice the image size, S_c the maps alone, F a plain FFT, P the transformed
point-spread functions (indigo_amd.toeplitz.psf_kernel: one adjoint NUFFT of ones onto the doubled image per distinct trajectory,
with the run's `--width` and `--osf`).  With `--basis`, P is a K x K Hermitian matrix at every grid point,
P_kk' = FFT(sum_t conj(PHI[t, k]) PHI[t, k'] q_t), and A^H A + lamda I = lamda I + ToeplitzNormal(K): the cost of an iteration
depends on K, not on T, and no frame panel is held (K <= 8: the kernel array is 4 K^2 bytes per point of the doubled grid).
Without a basis every distinct trajectory gets its own ToeplitzNormal(K = 1) under the frames' `BlockDiag`, or alone for one frame.
A and A^H y stay the gridding operator, which is used once; CG, `--l1`, `--tv`, `--tv-time` and `--llr` and the power iteration
run unchanged on the new A^H A.  The two forms of A^H A differ by the NUFFT's own approximation error (the gridding form carries
it twice, the Toeplitz form once).  Without `--toeplitz` the driver runs the code it ran before.

Soft-SENSE.  A scan whose `maps` carry a MAPS axis of length M > 1 (`bart ecalib` writes two sets by default; `data` keeps MAPS = 1)
is reconstructed as `bart pics` does: the unknown of a frame is M images, one per set,

    y_c = NUFFT( sum_m S_{c,m} . x_m ),        (A^H y)_m = sum_c conj(S_{c,m}) . NUFFT^H y_c        (M <= 4)

the remedy for a field of view smaller than the object, for phase singularities and for motion-corrupted calibration.  The
transforms and the gridding do not depend on M, only the per-voxel C x M map product does (`Backend.coil_maps`):
where `FuseZpadFFT` fuses the tree, its `ZpadFFT` leaves become `operators.ZpadFFTMaps` (`transforms.soft_sense_tree`); at -O0..2,
with --no-fuse, on grids the fused leaf refuses and on grids it takes only behind an image permutation A is
Optimize(recipe)(KronI(C, NUFFT)) * operators.CoilMaps(maps).  The M images of a frame are stacked map-major, the frames stay
frame-major around them, and the result is (X, Y, Z, 1, M[, 1, ..., T]).  The solvers run on the N M T unknown as they are: CG
jointly, `--l1` on every image, `--tv` the spatial term on every image (M T columns, no coupling between them), `--llr` on the (block
voxels) x (M T) matrices (M T <= 32), which is what bart penalises.  `--tv-time`, `--basis` and `--toeplitz` with M > 1 are refused
(maps inside frames is not the column order GradientT and FrameBasis act on; ToeplitzNormal takes one set).  No flag: the file
carries M, and `--crop "MAPS:1"` reproduces the run on a file that holds only the first set, bit for bit.  With M = 1 (with or
without a MAPS axis) the driver builds the trees it built before.

Maps from a file.  `--maps FILE.npy` takes the coil maps from that file, (X, Y, Z, C, M) stored reversed -- what
`python -m indigo_amd.ecalib` estimates from the scan's own k-space centre --, in place of the scan's `maps`; the scan
then need not hold any.  The M of the file selects SENSE or soft-SENSE as above.  Without the flag nothing changes.

Coil compression.  `--cc V` cuts `data` and the maps (the scan's or those of `--maps`), after `--crop`, to V virtual coils before the
reconstruction sees them: `indigo_amd.cc.compress` with the Gram matrix of all samples of all frames and no whitening (DESIGN.md §3.14;
`python -m indigo_amd.cc` writes the compressed scan, takes noise samples and a calibration region).  An iteration then costs V / C
of what it did.  Data and maps with different coil counts are refused.  Without the flag the driver runs the code it ran before.

Off-resonance.  `--fmap FILE.npy` (a real (X, Y, Z) field map in Hz, stored reversed like the maps; a scan that holds an array
`fmap` uses it without the flag) corrects the phase exp(-2 pi i f(r) t) that the field inhomogeneity f(r) builds up along a long
spiral, cone or radial-EPI readout and that no regulariser removes (`bart pics` with a field map, MIRT, sigpy; no counterpart in the
reference's driver).  The sample times come from `--times FILE.npy` (seconds, (readout,) or (readout, views), stored reversed; a scan
array `times` counts as the flag) or from `--dwell SECONDS [--te SECONDS]`, t = te + dwell * readout index.  The model is time
segmentation, exp(-2 pi i f t_j) ~ sum_{l<L} b_l(t_j) exp(-2 pi i f tau_l) with L equispaced tau_l and the histogram-weighted
least-squares interpolator b of `indigo_amd.fmap.segments` (`--fmap-segments L`, or the smallest L <= 16 whose model error is below
`--fmap-tol`; the histogram is taken where any coil map is non-zero).  With A0 the tree built as above,

    A = SegmentCombine(b) * BlockDiag([A0] * L) * SegmentPhase(f, tau),        A^H A + lamda I = A^H * A + lamda I_N

(operators.SegmentPhase, operators.SegmentCombine, `Backend.segment_phase`, `Backend.segment_combine`): the L
segments are L frames that share one trajectory, so they share one tree.  The unknown is the one image of N voxels: CG, `--l1`,
`--tv` and `--llr` run on it unchanged and the result has the shape of the plain run.  With `--toeplitz`,
A^H A + lamda I = lamda I + SegmentPhase^H * ToeplitzNormal(K = L) * SegmentPhase, whose L x L point-spread functions are the adjoint
NUFFTs of conj(b_l) b_l' (L <= 8).  A field map with several time frames, with `--basis` or with M > 1 sets of maps is refused, as
is a complex one (R2* decay).  Without a field map the driver runs the code it ran before.

Density compensation.  `--dcf FILE.npy` (what `python -m indigo_amd.dcf scan.npz` writes: real weights with the axes of `traj` without
the coordinate axis, stored reversed like `traj`; a scan that holds an array `dcf` uses it without the flag) or `--dcf auto` (Pipe-Menon
weights computed in passing, `--dcf-iters` iterations with the run's `--width` and `--osf`, once per distinct trajectory) solves

    min_x  1/2 ||W^(1/2) (A x - y)||^2 + ...            A <- SampleWeights(sqrt w) * A,   y <- sqrt(w) . y

(`bart pics -p`, sigpy's `dcf`; operators.SampleWeights, `Backend.row_scale`): one real weight per sample, shared by the
coils.  The 1 / r^2 density of a 3-D radial scan is what the first CG iterations are spent undoing; with the weights the second iteration is
where the plain run is after three or four.  It is for FEW iterations or a starting image: from about the sixth iteration on the weighted
run is worse (noise amplification at the sparsely sampled periphery), hence opt-in.  Every solver, `--basis`, `--fmap` and M > 1 sets of
maps run unchanged on the weighted A and y; with `--toeplitz` the point-spread functions are the adjoint NUFFTs of w in place of ones.
Weights of another shape than the trajectory's, negative or non-finite weights and all-zero weights are refused.  Without the flag the
driver runs the code it ran before.

Containers: HDF5 (`.h5`, the reference's format; needs h5py, which this image does not ship) or NumPy `.npz` with
the same three arrays in the same orientation; the result goes back into the HDF5 file as dataset `rec`, or next to
an `.npz` input as `<name>.rec.npy`.

The backend is the MI355X one (`hip`); there is no CPU fallback in the product.  `main(argv, backend=...)` lets the
CPU test-suite drive the same code with the numpy oracle backend.
"""
import argparse
import collections
import inspect
import logging
import os
import sys

import numpy as np

from indigo_amd.solvers import fista_solve, llr_term, power_iteration, tgv_solve, tv_solve      # noqa: F401  (power_iteration: for those who took it from here)

log = logging.getLogger("pics")


class dim:
    READ, PHS1, PHS2, COIL, MAPS, COEFF, TIME, NDIM = 0, 1, 2, 3, 4, 6, 10, 20


def parse(argv):
    ap = argparse.ArgumentParser(prog="indigo_amd.pics", description="Parallel Imaging and Compressed Sensing (non-Cartesian SENSE: CG, L1-wavelet or locally-low-rank FISTA, or total-variation primal-dual). "
                                 "Maps with a MAPS axis of length M > 1 (two sets from an ESPIRiT calibration) are reconstructed as soft-SENSE: M images per frame, "
                                 "result (X, Y, Z, 1, M[, ..., T]); not with --tv-time, --basis or --toeplitz.")
    ap.add_argument('-i', type=int, default=20, help='number of CG iterations')
    ap.add_argument('--backend', type=str, default='hip', choices=['hip'])
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--debug', type=int, default=logging.INFO, help='logging level')
    ap.add_argument('--crop', help='crop data before recon: --crop "COIL:2,TIME:4" (MAPS:1 keeps the first of several sets of maps)')
    ap.add_argument('--lamda', type=float, default=0, help='Tikhonov regularisation parameter')
    ap.add_argument('-O', '--recipe', type=int, default=3, choices=range(5), help='optimization level (pics.py -O)')
    ap.add_argument('--osf', type=float, default=640 / 480, help='gridding oversampling factor (pics.py: 640/480)')
    ap.add_argument('--width', type=int, default=3, help='Kaiser-Bessel kernel half-width (Backend.NUFFT default)')
    ap.add_argument('--no-fuse', action='store_true', help='keep the -O tree as it is (no FuseZpadFFT)')
    ap.add_argument('--l1', type=float, default=0, help='L1-wavelet weight; > 0 solves by FISTA instead of CG (0: CG)')
    ap.add_argument('--wavelet', default='db2', choices=['haar', 'db2', 'db4'], help='wavelet of --l1')
    ap.add_argument('--levels', type=int, default=3, help='wavelet levels of --l1')
    ap.add_argument('--power-iters', type=int, default=15, help='power iterations that estimate the FISTA step')
    ap.add_argument('--step', type=float, default=None, help='FISTA step (default 0.9 / the power-iteration estimate)')
    ap.add_argument('--tv', type=float, default=0, help='total-variation weight; > 0 solves by the primal-dual iteration (0: off)')
    ap.add_argument('--tv-sigma', type=float, default=None, help='dual step of --tv (default L / 24, with several time frames L / 32; L = 0.9 / the primal step)')
    ap.add_argument('--tv-time', type=float, default=0, help='weight of the total variation between neighbouring time frames (0: off; no effect on one frame)')
    ap.add_argument('--tgv', type=float, default=0, help='weight a1 of second-order total generalized variation; > 0 solves by the primal-dual iteration on (x; v) (0: off; not with --tv or --tv-time)')
    ap.add_argument('--tgv-ratio', type=float, default=2.0, help='a0 / a1 of --tgv: the weight of the symmetrised gradient of v (default 2, Knoll et al. 2011)')
    ap.add_argument('--tgv-sigma', type=float, default=None, help='dual step of --tgv (default L / 32; L = 0.9 / the primal step)')
    ap.add_argument('--llr', type=float, default=0, help='locally-low-rank weight; > 0 adds the blocks\' nuclear norms, by FISTA or as the prox of --tv / --tv-time (0: off)')
    ap.add_argument('--llr-block', type=int, default=8, help='block side of --llr along all three axes (clamped to the volume)')
    ap.add_argument('--llr-shifts', action='store_true', help='draw a fresh block shift before every prox call of --llr')
    ap.add_argument('--llr-seed', type=int, default=0, help='seed of --llr-shifts')
    ap.add_argument('--basis', default=None, help='temporal basis, a .npy file with a T x K array: reconstruct the K coefficient images of the subspace')
    ap.add_argument('--basis-rank', type=int, default=None, help='keep the first K columns of --basis')
    ap.add_argument('--toeplitz', action='store_true', help='evaluate A^H A as one Toeplitz operator on the grid of twice the image size (with --basis: K x K point-spread functions, the cost no longer grows with the frames)')
    ap.add_argument('--maps', default=None, help='coil maps from this .npy file, (X, Y, Z, C, M) stored reversed (what python -m indigo_amd.ecalib writes), in place of the scan\'s `maps`')
    ap.add_argument('--cc', type=int, default=None, help='compress the coils of data and maps to this many virtual coils first (indigo_amd.cc: all samples, no whitening)')
    ap.add_argument('--fmap', default=None, help='off-resonance correction: a real (X, Y, Z) field map in Hz from this .npy file, stored reversed like the maps (a scan array `fmap` is used without the flag)')
    ap.add_argument('--times', default=None, help='sample times of --fmap in seconds, a .npy file with a (readout,) or (readout, views) array stored reversed (a scan array `times` counts as this flag)')
    ap.add_argument('--dwell', type=float, default=None, help='sample times of --fmap as te + dwell * readout index, in seconds (instead of --times)')
    ap.add_argument('--te', type=float, default=None, help='time of the first sample of --dwell in seconds (default 0)')
    ap.add_argument('--fmap-segments', type=int, default=None, help='time segments of --fmap, 1..16 (default: the smallest count that reaches --fmap-tol)')
    ap.add_argument('--fmap-tol', type=float, default=1e-3, help='model error (weighted RMS over the field-map histogram) that the automatic choice of --fmap-segments must reach')
    ap.add_argument('--dcf', default=None, help='density compensation: sample weights from this .npy file (python -m indigo_amd.dcf writes one; a scan array `dcf` is used without the flag), or `auto`: Pipe-Menon weights computed in passing')
    ap.add_argument('--dcf-iters', type=int, default=30, help='Pipe-Menon iterations of --dcf auto')
    ap.add_argument('data', nargs='?', default="scan.h5", help='k-space data: HDF5 (data/maps/traj) or .npz; maps may hold M <= 4 sets on the MAPS axis (soft-SENSE)')
    args = ap.parse_args(argv)
    if args.llr > 0 and args.l1 > 0:
        ap.error("--llr and --l1 cannot be combined: two non-smooth terms in one prox slot are not a prox")
    if args.llr_block < 1:
        ap.error("--llr-block must be at least 1")
    if args.tgv > 0 and (args.tv > 0 or args.tv_time > 0):
        ap.error(TGV_WITH_TV)
    if not args.tgv_ratio > 0:
        ap.error("--tgv-ratio must be positive")
    if args.basis is not None and args.tv_time > 0:
        ap.error("--tv-time cannot be combined with --basis: the unknowns are coefficient images, and differences between "
                 "coefficients are not differences in time")
    if args.basis_rank is not None and args.basis is None:
        ap.error("--basis-rank needs --basis")
    if args.basis_rank is not None and args.basis_rank < 1:
        ap.error("--basis-rank must be at least 1")
    if args.toeplitz and args.basis_rank is not None and args.basis_rank > 8:
        ap.error("--toeplitz serves at most 8 coefficient images (--basis-rank %d): its kernel array holds 4 K^2 bytes per point "
                 "of the doubled grid, 137 GB at K = 16 on a 512^3 grid" % args.basis_rank)
    if args.times is not None and args.dwell is not None:
        ap.error("--times and --dwell cannot be combined: the sample times come from one of them")
    if args.te is not None and args.dwell is None:
        ap.error("--te needs --dwell")
    if args.dwell is not None and not args.dwell > 0:
        ap.error("--dwell must be positive")
    if args.fmap is not None and args.basis is not None:
        ap.error("--fmap cannot be combined with --basis: the time segments take the place of the frames (a follow-up)")
    if args.fmap_segments is not None and not 1 <= args.fmap_segments <= 16:
        ap.error("--fmap-segments must lie between 1 and 16")
    if args.toeplitz and args.fmap_segments is not None and args.fmap_segments > 8:
        ap.error("--toeplitz serves at most 8 time segments (--fmap-segments %d): its kernel array holds 4 K^2 bytes per point "
                 "of the doubled grid, 137 GB at K = 16 on a 512^3 grid" % args.fmap_segments)
    if not args.fmap_tol > 0:
        ap.error("--fmap-tol must be positive")
    if args.dcf_iters < 0:
        ap.error("--dcf-iters must not be negative")
    return args


def load_extras(path, names=('fmap', 'times', 'dcf')):
    """the optional arrays of a scan as stored, {name: array} for those of `names` that the file holds"""
    if path.endswith(".npz"):
        z = np.load(path)
        return {k: z[k] for k in names if k in z}
    try:
        import h5py
    except ImportError:
        return {}
    with h5py.File(path, 'r') as hdf:
        return {k: hdf[k][:] for k in names if k in hdf}


def load(path, maps_file=None):
    """-> (data, maps, traj, writer): arrays as stored (reversed dimension order), writer(img_T) stores `rec`.  maps_file: a .npy
    file whose array takes the place of the scan's `maps`, which the scan then need not hold (`--maps`)"""
    if path.endswith(".npz"):
        z = np.load(path)
        out = os.path.splitext(path)[0] + ".rec.npy"
        if maps_file is not None:
            maps = np.load(maps_file)
        elif 'maps' in z:
            maps = z['maps']
        else:
            raise ValueError("pics: %s holds no `maps`: give --maps FILE.npy (python -m indigo_amd.ecalib writes one from the scan itself)" % path)
        return z['data'], maps, z['traj'], lambda rec: np.save(out, rec)
    try:
        import h5py
    except ImportError:
        raise SystemExit("pics: reading %s needs h5py; convert the scan to .npz (arrays data, maps, traj) or install h5py" % path)
    hdf = h5py.File(path, 'r+')

    def write(rec):
        if 'rec' in hdf:
            del hdf['rec']
        hdf.create_dataset('rec', data=rec)
        hdf.close()
    if maps_file is None and 'maps' not in hdf:
        raise ValueError("pics: %s holds no `maps`: give --maps FILE.npy (python -m indigo_amd.ecalib writes one from the scan itself)" % path)
    return hdf['data'][:], (np.load(maps_file) if maps_file is not None else hdf['maps'][:]), hdf['traj'][:], write


def crop_limits(spec):
    crops = [10 ** 6] * dim.NDIM
    if spec:
        names = {k: v for k, v in vars(dim).items() if k.isupper()}
        for item in spec.split(","):
            name, size = item.split(":")
            d = names[name.strip()]
            crops[-(d + 1)] = int(size)
            log.info("cropping dim %d to length %d", d, int(size))
    return crops


def subspace_basis(basis, frames, rank=None):
    """the T x K complex64 basis of a `--basis` run: `basis` (real or complex, T x K') cut to its first `rank` columns, checked
    against the scan's `frames` = T time frames and the 32 coefficient images that `Backend.frame_basis` serves"""
    phi = np.asarray(basis)
    if phi.ndim != 2:
        raise ValueError("--basis: the basis must be a 2-D array (frames x coefficients), got shape %s" % (phi.shape,))
    if frames < 2:
        raise ValueError("--basis needs a scan with several time frames, this one has %d" % frames)
    if phi.shape[0] != frames:
        raise ValueError("--basis: the basis has %d rows, the scan has %d time frames" % (phi.shape[0], frames))
    if rank is not None:
        if rank < 1:
            raise ValueError("--basis-rank must be at least 1, got %d" % rank)
        if rank > phi.shape[1]:
            raise ValueError("--basis-rank %d exceeds the %d columns of the basis" % (rank, phi.shape[1]))
        phi = phi[:, :rank]
    K = phi.shape[1]
    if K < 1:
        raise ValueError("--basis: the basis has no columns")
    if K > 32:
        raise ValueError("--basis: %d coefficients, at most 32 are supported (--basis-rank keeps the first K columns)" % K)
    return np.asfortranarray(phi.astype(np.complex64))


def sample_density(dcf, traj_shape):
    """the weights of a `--dcf` run, checked: `dcf` real, with the axes of the trajectory `traj_shape` = (3, readout, views[, 1, ..., T])
    without the first (trailing axes of length 1 do not count), non-negative, finite and not all zero -> float64 (readout views, T')
    with T' the trajectory's frames, the samples of a frame in the order of the k-space vector"""
    w = np.asarray(dcf)
    if np.iscomplexobj(w) or w.dtype.kind not in 'fiub':
        raise ValueError("--dcf: the weights must be a real array, got dtype %s" % w.dtype)

    def strip(shape):
        shape = tuple(int(n) for n in shape)
        while len(shape) > 2 and shape[-1] == 1:
            shape = shape[:-1]
        return shape
    if strip(w.shape) != strip(traj_shape[1:]):
        raise ValueError("--dcf: the weights have shape %s, the trajectory has %s samples (its axes without the coordinate axis)"
                         % (tuple(w.shape), tuple(traj_shape[1:])))
    w = w.astype(np.float64)
    if not np.isfinite(w).all():
        raise ValueError("--dcf: the weights are not finite (%d of %d are NaN or infinite)" % (int((~np.isfinite(w)).sum()), w.size))
    if (w < 0).any():
        raise ValueError("--dcf: %d of %d weights are negative (their square roots scale the data)" % (int((w < 0).sum()), w.size))
    if not (w > 0).any():
        raise ValueError("--dcf: all weights are zero")
    rows = int(np.prod(traj_shape[1:3]))
    return w.reshape((rows, -1), order='F')


def toeplitz_normal(B, mps, distinct, which, phi, lamda, width, osf, recipe=None, segments=None, density=None):
    """A^H A + lamda I of `reconstruct` in Toeplitz form, with the scratch arena reserved for it.  phi (T x K): one
    `ToeplitzNormal` of K coefficient images; phi None: one `ToeplitzNormal` (K = 1) per distinct trajectory, each + lamda I, under a
    `BlockDiag` over the frames `which`, or alone for one frame.  distinct: the trajectories (3, readout, views) in cycles per pixel;
    recipe: the pass list of the run's own trees, for the set-up transform of `psf_kernel`.
    segments = (Phase, weights), the `SegmentPhase` of a field-map run and the (samples, L) expansion of its interpolator: one
    `ToeplitzNormal` of the L segments between Phase and Phase^H.
    density: one real array of sample weights per distinct trajectory (pics --dcf): A^H W A in place of A^H A."""
    from indigo_amd.operators import ToeplitzNormal
    from indigo_amd.toeplitz import psf_kernel
    from indigo_amd.transforms import reserve_for
    dims = tuple(int(n) for n in mps.shape[:3])
    N = int(np.prod(dims))
    maps = mps.reshape(dims + (-1,))
    order = ToeplitzNormal.memory_order(B, dims)

    def normal(trajs, frames, basis, K, name, tree, dens, wrap=lambda T: T, weights=None):
        """lamda I + wrap(the `ToeplitzNormal` of K images `name` with the point-spread functions of `trajs`), named `tree`"""
        kern = psf_kernel(B, dims, trajs, frames, basis, width, osf, order=order, recipe=recipe, sample_weights=weights, density=dens)
        # (lamda I + T, not T + lamda I: a Sum evaluates its right child first, with the caller's beta, so T runs with beta = 0)
        AHA = lamda * B.Eye(N * (1 if basis is None else K)) + wrap(B.ToeplitzNormal(dims, maps, kern, K, order=order, name=name))
        AHA._name = tree
        return AHA
    if segments is not None:
        Phase, weights = segments
        ops = [normal(distinct, which, None, weights.shape[1], 'toeplitz segments', 'SENSE off-resonance (Toeplitz)', density,
                      lambda T: Phase.H * T * Phase, weights)]
    elif phi is not None:
        ops = [normal(distinct, which, phi, phi.shape[1], 'toeplitz subspace', 'SENSE subspace (Toeplitz)', density)]
    else:
        ops = [normal([trj3], [0], None, 1, 'toeplitz', 'SENSE (Toeplitz)', None if density is None else [density[k]])
               for k, trj3 in enumerate(distinct)]
    frames = segments is None and phi is None and len(which) > 1
    AHA = B.BlockDiag([ops[k] for k in which], name='SENSE frames (Toeplitz)') if frames else ops[0]
    # (the children run one after the other on the same arena, and all have the same size)
    reserve_for(ops[0], 1, slack_products=6)
    return AHA


# ---- the stages of `reconstruct` --------------------------------------------------------------------------------------------------------

# the sizes of a scan: the image `dims` of N voxels, C coils, M sets of maps, T time frames of which the trajectory has T_traj (1 or T),
# `samples` = (1, readout, views) with `rows` = readout views samples per coil and frame, and `img_dims`, the shape of the result
Geometry = collections.namedtuple('Geometry', 'dims N C M T T_traj samples rows img_dims')


def geometry(ksp, mps, traj):
    """the `Geometry` of ksp (1, readout, views, C, 1, ..., T), mps (X, Y, Z, C, M) and traj (3, readout, views[, 1, ..., T])"""
    M = mps.shape[dim.MAPS] if mps.ndim > dim.MAPS else 1          # sets of coil maps: M > 1 is soft-SENSE, M images per frame
    if ksp.ndim > dim.MAPS and ksp.shape[dim.MAPS] != 1:
        raise ValueError("data has a MAPS axis of length %d: only the maps carry several sets, the k-space is one measurement "
                         "(MAPS must be 1 in data)" % ksp.shape[dim.MAPS])
    img_dims = mps.shape[:3] + (1,) + ksp.shape[4:]
    if M > 1:
        img_dims = img_dims + (1,) * (dim.MAPS + 1 - len(img_dims))
        img_dims = img_dims[:dim.MAPS] + (M,) + img_dims[dim.MAPS + 1:]
    log.info('img %s %s', img_dims, ksp.dtype)
    log.info('mps %s, ksp %s, trj %s, sets of maps %d', mps.shape, ksp.shape, traj.shape, M)
    T = ksp.shape[dim.TIME] if ksp.ndim > dim.TIME else 1
    T_traj = traj.shape[dim.TIME] if traj.ndim > dim.TIME else 1
    assert M == 1 or int(np.prod(mps.shape[dim.MAPS + 1:])) == 1, "Of the maps only COIL and MAPS may be longer than 1."
    assert mps.ndim <= dim.TIME or mps.shape[dim.TIME] == 1, "The maps carry no TIME axis: one set for all frames."
    assert T_traj in (1, T), "traj has %d time frames, data has %d" % (T_traj, T)
    assert int(np.prod(ksp.shape[4:])) == T and int(np.prod(traj.shape[3:])) == T_traj, "Only COIL and TIME may be longer than 1."
    return Geometry(tuple(mps.shape[:3]), int(np.prod(mps.shape[:3])), ksp.shape[dim.COIL], M, T, T_traj, tuple(ksp.shape[:3]),
                    int(np.prod(ksp.shape[1:3])), img_dims)


TGV_WITH_TV = ("--tgv cannot be combined with --tv or --tv-time: one analysis operator per run (the primal-dual iteration carries one K "
               "and one dual variable; with v held at zero --tgv is --tv)")


def check_options(g, tv_time=0.0, l1=0.0, llr=0.0, basis=None, basis_rank=None, toeplitz=False, tv=0.0, tgv=0.0):
    """refuses the options that the scan `g` or one another rule out (a field map and density weights are checked where they are read:
    `field_map_segments`, `sample_density`) -> the checked T x K basis of `subspace_basis`, or None"""
    M, T = g.M, g.T
    if tgv > 0 and (tv > 0 or tv_time > 0):
        raise ValueError(TGV_WITH_TV)
    if M > 1:
        # soft-SENSE follow-ups: the unknown is ordered maps inside frames, which is not what these three take
        if tv_time > 0:
            raise ValueError("--tv-time cannot be combined with M = %d sets of maps: GradientT differences neighbouring columns of the "
                             "unknown, which are then the images of one frame's sets, not neighbouring frames" % M)
        if basis is not None:
            raise ValueError("--basis cannot be combined with M = %d sets of maps: FrameBasis mixes the columns of the unknown as "
                             "frames, and they are then the images of the sets inside every frame" % M)
        if toeplitz:
            raise ValueError("--toeplitz cannot be combined with M = %d sets of maps: ToeplitzNormal takes one set" % M)
        if M > 4:
            raise ValueError("%d sets of maps, at most 4 are supported (Backend.coil_maps)" % M)
        if llr > 0 and M * T > 32:
            raise ValueError("--llr: M * T = %d x %d = %d columns, at most 32 are supported (Backend.llr_threshold)" % (M, T, M * T))
    # (the two that `parse` refuses already)
    assert basis is None or not tv_time > 0, "--tv-time cannot be combined with --basis: differences between coefficients are not differences in time"
    assert not (llr > 0 and l1 > 0), "--llr and --l1 cannot be combined: two non-smooth terms in one prox slot are not a prox"
    if basis is None:
        return None
    phi = subspace_basis(basis, T, basis_rank)
    K = phi.shape[1]
    gram = phi.astype(np.complex128)
    log.info("basis: %d frames, %d coefficients, ||Phi^H Phi - I|| %.3e", T, K, np.linalg.norm(gram.conj().T @ gram - np.eye(K)))
    if toeplitz and K > 8:
        raise ValueError("--toeplitz: %d coefficients, at most 8 are supported: the kernel array holds 4 K^2 bytes per point of the "
                         "doubled grid, %.1f GB here (--basis-rank keeps the first K columns)" % (K, 32e-9 * K * K * g.N))
    return phi


def field_map_segments(g, mps, fmap, times, segments=None, tol=1e-3, basis=None, toeplitz=False):
    """fmap: a real (X, Y, Z) field map in Hz, times: the sample times in seconds, (readout,) or (readout, views) -> (the field map flattened,
    (taus, table, period, error) of `indigo_amd.fmap.segments` for `segments` segments or the fewest within `tol`), None without a field map"""
    if fmap is None:
        if times is not None:
            log.info("sample times without a field map have no effect")
        return None
    from indigo_amd import fmap as fmap_mod
    nro, nviews = g.samples[1:]
    fmap = np.asarray(fmap)
    if np.iscomplexobj(fmap):
        raise ValueError("--fmap: the field map is complex: only a real one in Hz is supported (R2* decay in the imaginary part "
                         "is a follow-up)")
    if basis is not None:
        raise ValueError("--fmap cannot be combined with --basis: the time segments take the place of the frames (a follow-up)")
    if g.T > 1:
        raise ValueError("--fmap cannot be combined with %d time frames: the time segments take the place of the frames (a follow-up)" % g.T)
    if g.M > 1:
        raise ValueError("--fmap cannot be combined with M = %d sets of maps: the segments' BlockDiag takes one image per segment "
                         "(a follow-up)" % g.M)
    if times is None:
        raise ValueError("--fmap needs the sample times: give --times FILE.npy or --dwell SECONDS [--te SECONDS]")
    fmap = fmap.reshape(fmap.shape[:3] + (-1,))[..., 0] if fmap.ndim > 3 and int(np.prod(fmap.shape[3:])) == 1 else fmap
    if fmap.shape != g.dims:
        raise ValueError("--fmap: the field map has shape %s, the maps have %s" % (fmap.shape, g.dims))
    times = np.asarray(times, dtype=np.float64)
    times = times.reshape(times.shape[:2]) if times.ndim > 2 and int(np.prod(times.shape[2:])) == 1 else times
    if times.ndim == 2 and times.shape[1] == 1 and nviews != 1:
        times = times[:, 0]
    if times.shape not in ((nro,), (nro, nviews)):
        raise ValueError("--times: the sample times have shape %s, the k-space has %d readout points and %d views: (readout,) or "
                         "(readout, views) is expected" % (times.shape, nro, nviews))
    mask = (np.abs(mps.reshape(g.dims + (-1,))) > 0).any(axis=3)
    seg = fmap_mod.segments(fmap.astype(np.float32), times, L=segments, mask=mask, tol=tol)
    if toeplitz and seg[0].size > 8:
        raise ValueError("--toeplitz: %d time segments, at most 8 are supported: the kernel array holds 4 K^2 bytes per point of the "
                         "doubled grid, %.1f GB here (--fmap-segments fixes their number)" % (seg[0].size, 32e-9 * seg[0].size ** 2 * g.N))
    return fmap.reshape(-1, order='F'), seg


def density_lookup(B, g, traj_shape, dcf, dcf_iters=30, width=3, osf=640 / 480):
    """-> frame_density(trj3, t): the weights of trajectory trj3, frame t of the trajectory's own frames, float64 (rows,): those of the
    array `dcf` (checked by `sample_density`), Pipe-Menon weights for dcf = 'auto', None without dcf"""
    if dcf is None:
        return lambda trj3, t: None
    if isinstance(dcf, str) and dcf == 'auto':
        from indigo_amd.dcf import pipe_menon
        return lambda trj3, t: pipe_menon(B, trj3, g.dims, width=width, osf=osf, iters=dcf_iters).reshape(-1, order='F').astype(np.float64)
    dens = sample_density(dcf, traj_shape)
    if dens.shape[1] not in (1, g.T_traj):
        raise ValueError("--dcf: the weights have %d frames, the trajectory has %d" % (dens.shape[1], g.T_traj))
    return lambda trj3, t: dens[:, t if dens.shape[1] > 1 else 0]


def forward_model(B, g, mps, traj, recipe, lamda=0.0, width=3, osf=640 / 480, phi=None, seg=None, frame_density=lambda trj3, t: None):
    """The forward model of the module docstring, the scratch arena reserved for it -> (A, A^H A + lamda I, the distinct trajectories, the
    index into them of every frame, the density weights of every distinct trajectory or None).  traj: in units of the field of view; recipe:
    the pass list of the trees; phi: the basis of a subspace run; seg: from `field_map_segments`; frame_density: from `density_lookup`"""
    from indigo_amd.analyses import ScratchUsage
    from indigo_amd.transforms import Optimize, reserve_for, soft_sense_tree
    N, C, M, T, rows = g.N, g.C, g.M, g.T, g.rows

    def panel(n):                                        # a product's temporary of n rows in the arena, which carves in steps of 32
        return (n + 31) // 32 * 32

    def weighted(A, wts):
        """W^(1/2) A: the forward model of the density-compensated data term (one weight per sample, shared by the coils)"""
        if wts is None:
            return A
        WA = B.SampleWeights(np.sqrt(wts), rows, A.shape[0] // rows, name='sqrt dcf') * A
        WA._name = A._name
        return WA

    def frame_operators(trj3, wts=None):
        """A_t and A_t^H A_t + lamda I of one trajectory (in a temporal subspace A_t^H A_t alone: lamda acts on the coefficients);
        wts: density-compensation weights of its samples, W^(1/2) A_t in place of A_t"""
        def nufft():
            return B.NUFFT(g.samples, g.dims, trj3, width=width, oversamp=(osf, osf, osf), dtype=np.dtype('complex64'))
        if M > 1:
            A = soft_sense_tree(B, nufft, mps.reshape(g.dims + (C, M)), recipe)
        else:
            A = B.KronI(C, nufft()) * B.VStack([B.Diag(mps[:, :, :, c].reshape(g.dims + (1,))) for c in range(C)], name='maps')
            A._name = 'SENSE1'
            A = Optimize(recipe).visit(A)
        A = weighted(A, wts)
        AHA = (A.H * A) + lamda * B.Eye(A.shape[1]) if phi is None else A.H * A
        AHA._name = 'SENSE'
        return A, AHA

    # frames with equal trajectories share one tree: its matrices are built and uploaded once, and BlockDiag evaluates the
    # same child on each of those frames' rows in turn
    trjs = traj.reshape(traj.shape[:3] + (g.T_traj,))
    distinct, trees, which, density = [], [], [], []
    for t in range(T):
        t_traj = t if g.T_traj > 1 else 0
        trj3 = trjs[..., t_traj]
        k = next((k for k, seen in enumerate(distinct) if np.array_equal(seen, trj3)), None)
        if k is None:
            k = len(distinct)
            distinct.append(trj3)
            density.append(frame_density(trj3, t_traj))
            # (with a field map the weights go around the segments' combination, not into every segment's tree)
            trees.append(frame_operators(trj3, density[-1] if seg is None else None))
        which.append(k)
    A, AHA = trees[0]
    if T > 1:
        log.info("frames %d, distinct trajectories %d", T, len(distinct))
        A = B.BlockDiag([trees[k][0] for k in which], name='SENSE1 frames')
        AHA = B.BlockDiag([trees[k][1] for k in which], name='SENSE frames')
    # the children run one after the other on the same arena: the scratch of the most demanding one, once, and what the products around them hold
    worst = max((tree[1] for tree in trees), key=lambda node: ScratchUsage().measure(node, 1))
    krows = trees[0][0].shape[0]
    extra = 0 if density[0] is None else panel(krows)    # the weighted product's extra k-space panel
    if phi is not None:
        # x_t = sum_k Phi[t, k] alpha_k: the unknowns are the K coefficient images.  Below the frames' trees the three-factor
        # product holds two panels of all T frames: the synthesised frames and what the frames' operators make of them
        Phi = B.FrameBasis(phi, N, name='basis')
        A = A * Phi
        A._name = 'SENSE1 subspace'
        AHA = Phi.H * AHA * Phi + lamda * B.Eye(N * phi.shape[1])
        AHA._name = 'SENSE subspace'
        extra += 2 * panel(N * T)
    if seg is not None:
        # the L segments are L frames on one trajectory: one tree under the BlockDiag.  Around it the product holds two panels
        # of the segments' images and two of their samples
        field, (taus, table, period, _) = seg
        L = taus.size
        extra += 2 * panel(N * L) + 2 * panel(krows * L)
    reserve_for(worst, 1, slack_products=6, extra=extra)
    if seg is not None:
        Phase = B.SegmentPhase(field, taus, N, name='segment phase')
        A = B.SegmentCombine(table, period, krows, name='segment combine') * B.BlockDiag([A] * L, name='SENSE1 segments') * Phase
        A._name = 'SENSE1 off-resonance'
        A = weighted(A, density[0])
        AHA = (A.H * A) + lamda * B.Eye(N)
        AHA._name = 'SENSE off-resonance'
    return A, AHA, distinct, which, None if density[0] is None else density


def right_hand_side(g, A, which, density, ksp):
    """-> (y, AHy, scale, density): the k-space vector (with density weights sqrt(w) . y, frame by frame: the data of the same weighted
    problem), A^H y divided by `scale`, its largest modulus, and the weights as the operators apply them, rounded through float32"""
    y = np.asfortranarray(ksp.reshape((-1, 1), order='F'))
    if density is not None:
        sq = np.sqrt(np.stack([density[k] for k in which], axis=1)).astype(np.float32)
        y = np.asfortranarray((y.reshape((g.rows, g.C, g.T), order='F') * sq[:, None, :]).astype(ksp.dtype).reshape((-1, 1), order='F'))
        density = [np.square(np.sqrt(d).astype(np.float32).astype(np.float64)) for d in density]
    AHy = A.H * y
    scale = abs(AHy).max()
    AHy /= scale
    return y, AHy, scale, density


def solve(B, g, AHA, AHy, cols, iters=20, l1=0.0, tv=0.0, tv_sigma=None, tv_time=0.0, llr=0.0, llr_block=8, llr_shifts=False, llr_seed=0,
          tgv=0.0, tgv_ratio=2.0, tgv_sigma=None, **prox):
    """the solver that the options select (`reconstruct`'s docstring), on AHA x = AHy with `cols` images in the unknown -> x, host (n, 1).
    prox: what `fista_solve`, `tv_solve` and `tgv_solve` all take: wavelet, levels, power_iters, step, ynorm2"""
    if tv_time > 0 and g.T == 1:
        log.info("--tv-time %g has no effect on a scan with one time frame", tv_time)
        tv_time = 0.0
    term = None
    if llr > 0:
        term = llr_term(B, g.dims, cols, llr, block=llr_block, shifts=llr_shifts, seed=llr_seed)
        if cols == 1:
            log.info("--llr on a scan with one time frame: every block has rank one, the term shrinks the blocks' 2-norms")
    if tgv > 0:
        return tgv_solve(B, AHA, AHy, g.dims, iters, tgv, tgv_ratio * tgv, sigma=tgv_sigma, l1=l1, frames=cols, term=term, **prox)[0]
    if tv > 0 or tv_time > 0:
        return tv_solve(B, AHA, AHy, g.dims, iters, tv, sigma=tv_sigma, l1=l1, frames=cols, mu_t=tv_time, term=term, **prox)[0]
    if l1 > 0 or llr > 0:
        return fista_solve(B, AHA, AHy, g.dims, iters, l1, term=term, **prox)[0]
    x = np.zeros((AHA.shape[1], 1), dtype=np.complex64, order='F')
    hist = B.cg(AHA, AHy, x, maxiter=iters)
    log.info("residuals: %s", " ".join("%.3e" % h for h in (hist or [])))
    return x


def reconstruct(B, ksp, mps, traj, iters=20, lamda=0.0, level=3, osf=640 / 480, width=3, fuse=True,
                l1=0.0, wavelet='db2', levels=3, power_iters=15, step=None, tv=0.0, tv_sigma=None, tv_time=0.0,
                llr=0.0, llr_block=8, llr_shifts=False, llr_seed=0, basis=None, basis_rank=None, toeplitz=False,
                fmap=None, times=None, fmap_segments=None, fmap_tol=1e-3, dcf=None, dcf_iters=30, tgv=0.0, tgv_ratio=2.0, tgv_sigma=None):
    """ksp: (1, readout, views, C, 1, ..., T), mps: (X, Y, Z, C, M), traj: (3, readout, views[, 1, ..., T]) in pixels -> image
    (X, Y, Z, 1, M, ..., T).  T > 1 time frames: the block-diagonal problem of the module docstring, one A_t per frame.
    M > 1 sets of maps: soft-SENSE, M images per frame (module docstring); not with tv_time, basis or toeplitz.
    tv > 0 (or, with T > 1, tv_time > 0): total-variation regularised by the primal-dual iteration (`tv_solve`; with l1 > 0 the
    wavelet term as well); tgv > 0: second-order total generalized variation with the weights a1 = tgv and a0 = tgv_ratio * tgv by the
    same iteration on (x; v) (`tgv_solve`; not with tv or tv_time; l1 or llr in its prox slot); l1 > 0: L1-wavelet regularised by FISTA (`fista_solve`); llr > 0: the locally low-rank term
    (`llr_term`) in the prox slot of whichever of the two applies, in place of the wavelet term; else CG on the normal equations.
    basis: a T x K array (its first basis_rank columns): the temporal-subspace problem of the module docstring, whose unknowns and
    result are the K coefficient images (X, Y, Z, 1, 1, 1, K); every regulariser then acts on those.
    toeplitz: A^H A of every solver is `operators.ToeplitzNormal` (module docstring); A^H y still comes from the gridding operator
    fmap: a real (X, Y, Z) field map in Hz, with times: the sample times in seconds, (readout,) or (readout, views): the
    time-segmented off-resonance model of the module docstring with fmap_segments segments (None: the fewest that reach the model
    error fmap_tol); one frame, one set of maps, no basis.  The unknown and the result are those of the plain run.
    dcf: density-compensation weights with the axes of traj without the first, or 'auto' (Pipe-Menon, dcf_iters iterations, once per
    distinct trajectory): the weighted data term of the module docstring; every solver runs unchanged on the weighted A and y."""
    from indigo_amd.transforms import FuseZpadFFT, sense_recipe
    ksp, mps, traj = np.asarray(ksp, dtype=np.complex64), np.asarray(mps, dtype=np.complex64), np.array(traj, dtype=np.float64)
    g = geometry(ksp, mps, traj)
    for i in range(3):                                   # trajectory in units of the field of view (pics.py:69-72)
        traj[i] /= g.dims[i]
    phi = check_options(g, tv_time=tv_time, l1=l1, llr=llr, basis=basis, basis_rank=basis_rank, toeplitz=toeplitz, tv=tv, tgv=tgv)
    seg = field_map_segments(g, mps, fmap, times, fmap_segments, fmap_tol, basis=basis, toeplitz=toeplitz)
    recipe = sense_recipe(level) + ([FuseZpadFFT] if fuse and level >= 3 else [])
    frame_density = density_lookup(B, g, traj.shape, dcf, dcf_iters, width, osf)
    A, AHA, distinct, which, density = forward_model(B, g, mps, traj, recipe, lamda, width, osf, phi, seg, frame_density)
    log.info("tree:\n%s", AHA.dump())
    log.info('using %d MB of device memory', (AHA.memusage() + 4 * AHA.shape[1] * ksp.dtype.itemsize) / 1e6)
    y, AHy, scale, density = right_hand_side(g, A, which, density, ksp)
    if toeplitz:
        # the gridding operator has done its one job, the right-hand side: every solver below runs on the Toeplitz form of A^H A
        del A, AHA
        B.release_scratch()
        segments = None
        if seg is not None:
            field, (taus, table, period, _) = seg
            segments = (B.SegmentPhase(field, taus, g.N, name='segment phase'), np.tile(table, (g.rows // period, 1)))
        AHA = toeplitz_normal(B, mps, distinct, which, phi, lamda, width, osf, recipe=recipe, segments=segments, density=density)
        log.info("tree:\n%s", AHA.dump())
    # the data term of the same normalised problem, for the solvers that log their objective
    ynorm2 = float(np.vdot(y, y).real) / float(scale) ** 2 if tv > 0 or tv_time > 0 or tgv > 0 or l1 > 0 or llr > 0 else 0.0
    cols = g.M * g.T if phi is None else phi.shape[1]    # the images of the unknown: the sets' images of every frame, or the coefficient images
    x = solve(B, g, AHA, AHy, cols, iters, l1, tv, tv_sigma, tv_time, llr, llr_block, llr_shifts, llr_seed, tgv, tgv_ratio, tgv_sigma,
              wavelet=wavelet, levels=levels, power_iters=power_iters, step=step, ynorm2=ynorm2)
    return x.reshape(g.img_dims if phi is None else g.dims + (1,) * (dim.COEFF - 3) + (cols,), order='F')


def cropped(arr, limits):                                # arr cut to the `limits` of its axes, in the order of those axes
    return arr[tuple(slice(0, min(n, c)) for n, c in zip(arr.shape, limits))]


def main(argv=None, backend=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=args.debug)
    if backend is None:
        from indigo_amd.backends import get_backend
        backend = get_backend(args.backend, device_id=args.device)
    log.info("using backend: %s", type(backend).__name__)
    extras = load_extras(args.data)                      # (before `load`, which keeps an HDF5 file open for the result)
    data, maps, traj, write = load(args.data, args.maps)
    crops = crop_limits(args.crop)
    ksp, mps, trj = (cropped(a, crops[-a.ndim:]).T for a in (data, maps, traj))
    # the keywords of `reconstruct` are the command-line options of their names, but for these: other names, or arrays for file names
    opts = dict(vars(args), iters=args.i, level=args.recipe, fuse=not args.no_fuse, times=None,
                basis=np.load(args.basis) if args.basis is not None else None,
                fmap=np.load(args.fmap).T if args.fmap is not None else extras['fmap'].T if 'fmap' in extras else None)
    if args.times is not None or 'times' in extras:
        if args.dwell is not None:
            raise ValueError("--dwell cannot be combined with the scan's own `times`: the sample times come from one of them")
        opts['times'] = (np.load(args.times) if args.times is not None else extras['times']).T
    elif args.dwell is not None:
        opts['times'] = (args.te or 0.0) + args.dwell * np.arange(ksp.shape[1], dtype=np.float64)
    if args.dcf != 'auto' and (args.dcf is not None or 'dcf' in extras):
        dcf = (np.load(args.dcf) if args.dcf is not None else extras['dcf']).T
        opts['dcf'] = cropped(dcf, crops[-2:-dcf.ndim - 2:-1])           # (its axes are the trajectory's from PHS1 on)
    if args.cc is not None:
        from indigo_amd import cc
        ksp, mps = cc.compress(backend, ksp, mps, V=args.cc)[:2]
    img = reconstruct(backend, ksp, mps, trj, **{k: opts[k] for k in list(inspect.signature(reconstruct).parameters)[4:]})
    write(img.T)
    log.info("reconstruction complete")
    return img


if __name__ == "__main__":
    main()
