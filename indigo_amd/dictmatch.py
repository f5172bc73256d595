#!/usr/bin/env python3
"""Dictionary matching: the temporal basis that `pics --basis` needs, and quantitative maps from the coefficient images it returns
(`bart signal`, `bart svd` and the matching step of T2 shuffling and MR fingerprinting).

    python -m indigo_amd.dictmatch basis --model t2 --te S --echoes T --t2 lo:hi:N (--rank K | --energy E) out
    python -m indigo_amd.dictmatch basis --model ir --ti FILE.npy --t1 lo:hi:N (--rank K | --energy E) out
    python -m indigo_amd.dictmatch basis --model fse --te S --echoes T (--flip DEG | --flips FILE.npy) --t2 lo:hi:N [--t1 lo:hi:N]
                                         [--b1 lo:hi:N] [--states K] (--rank K | --energy E) out
    python -m indigo_amd.dictmatch basis --model fisp --flips FILE.npy --tr VALUE|FILE.npy --te S [--phases FILE.npy] [--ti S]
                                         --t1 lo:hi:N --t2 lo:hi:N [--b1 lo:hi:N] [--states K] (--rank K | --energy E) out
    python -m indigo_amd.dictmatch basis --atoms FILE.npy --params FILE.npy (--rank K | --energy E) out
    python -m indigo_amd.dictmatch fit --atoms A.npy --params P.npy --basis phi.npy [--basis-rank K] [--mask-rel 0.02] [--chunk N] rec.npy

`basis` writes `<out>.atoms.npy`, the N simulated signal curves as an (N, T) array, `<out>.params.npy`, their parameters as (N, P), and
`<out>.phi.npy`, the (T, K) temporal basis that `python -m indigo_amd.pics --basis` reads: the K leading right singular vectors of the
atoms, K given by `--rank` or as the smallest K whose singular values hold the fraction `--energy` of their squared sum.  Two models
need no input: multi-echo spin echo, s_t = exp(-t TE / T2) at the echoes t = 1 ... T, and inversion recovery,
s = 1 - 2 exp(-TI / T1) at the inversion times of `--ti`; both on a log-spaced grid lo:hi:N of their parameter (seconds, as TE and
TI).  `--atoms` with `--params` takes any dictionary simulated elsewhere (a Bloch simulation, several parameters per atom).

Two more models run on the extended-phase-graph simulator, `Backend.epg_signal` (ig_epg_sim_c64 on the device, one wavefront per atom;
DESIGN.md §3.19; tests/epg64.py restates it in float64).  An atom is (T1, T2, B1), B1 scaling every flip angle; `params` is (N, 3) in
that order, the atoms ordered with T1 slowest and B1 fastest, T1 and T2 on log-spaced grids and B1 on a linear one (`--t1` and `--b1`
default to the single value 1.0 where they are optional).  `--model fse` is a CPMG echo train with imperfect and variable refocusing:
an excitation (90 degrees, phase 90 degrees) and T refocusing pulses of `--flip` degrees, or of the T angles in `--flips`, `--te`
apart, one record per echo; `--states` defaults to min(T + 1, 256), which truncates nothing up to T = 255.  `--model fisp` is an
unbalanced steady-state train as MR fingerprinting runs it: an optional inversion (180 degrees, `--ti` seconds, spoiled), then per
pulse the flip angle of `--flips` (degrees) and the phase of `--phases` (degrees, default 0), a record `--te` after the pulse and one
dephasing shift per repetition of `--tr` seconds (a value, or a file of T values); atoms with T2 > T1 are dropped; `--states` defaults
to 32.  `program_fse` and `program_fisp` return the `(steps, flags)` that `epg_signal` takes: with them any program can be run from
Python.  The simulation runs on `--backend` / `--device`, `--chunk` atoms at a time.

`fit` reads `rec.npy`, the coefficient images exactly as `pics --basis` saves them (stored reversed, K on the COEFF axis), and writes,
stored reversed like every array of a scan,

    <name>.qmaps.npy    (X, Y, Z, P) float32    the parameters of the matched atom
    <name>.pd.npy       (X, Y, Z) complex64     proton density and phase: d_a^H c divided by the norm of the compressed atom
    <name>.index.npy    (X, Y, Z) int32         the atom index
    <name>.misfit.npy   (X, Y, Z) float32       1 - s / ||c||^2, the part of the voxel's energy that the atom does not explain

The definition (tests/dict64.py restates it in float64).  A voxel of density rho whose signal is atom a has the
frames rho s_a and the coefficients c = rho Phi^H s_a.  The atoms are compressed to Phi^H s_a and normalised to d_a, in float64; the
matched atom is the smallest a that attains max_a |d_a^H c|^2, and rho = d_a^H c / ||Phi^H s_a||.  Voxels with ||c|| below
`--mask-rel` times the largest ||c|| get zeros in all four files.

Where the work runs.  The matching step is a (voxels x K)(K x N) complex product followed by an arg-max over N,
`Backend.dict_match` (ig_dict_match_c64 on the device: float32-input MFMA fused with a running maximum per voxel, the scores are
never stored).  The dictionary is uploaded once; the voxels of a host array go through the device in chunks of at most `--chunk`.
The closed-form models, the SVD and the compression are host work in float64.  `fit_frames` serves a reconstruction of T frames made without
`--basis`: it projects the frames with `Backend.frame_basis(adjoint=True)` and matches the same way.

Left out: interpolation between the atoms of the grid, a search restricted by a per-voxel B1 map, dictionaries
beyond the L2.

The backend is the MI355X one (`hip`); `main(argv, backend=...)` lets the CPU test-suite drive the same code with the numpy oracle.
"""
import argparse
import logging
import os
import sys

import numpy as np

log = logging.getLogger("dictmatch")
_C64 = np.dtype('complex64')

MAX_COEFFS = 32         # Backend.dict_match (and Backend.frame_basis) keep at most 32 coefficients per voxel
CHUNK = 1 << 21         # voxels of a host array on the device at a time
EPG_CHUNK = 1 << 16     # atoms of an EPG simulation on the device at a time
COEFF = 6               # the COEFF axis of a `pics --basis` result


# ---- the dictionary and its basis -------------------------------------------------------------------------------------------------

def grid(spec, log=True):
    """'lo:hi:N' -> N log-spaced (or, log=False, evenly spaced) values from lo to hi (float64)"""
    try:
        lo, hi, N = spec.split(":")
        lo, hi, N = float(lo), float(hi), int(N)
    except ValueError:
        raise ValueError("dictmatch: a parameter grid is lo:hi:N, got %r" % (spec,))
    if not (0 < lo <= hi and N >= 1):
        raise ValueError("dictmatch: a parameter grid lo:hi:N needs 0 < lo <= hi and N >= 1, got %r" % (spec,))
    if N == 1:
        return np.array([lo])
    return np.geomspace(lo, hi, N) if log else np.linspace(lo, hi, N)


def atoms_t2(te, echoes, t2):
    """multi-echo spin echo: atoms[a, t - 1] = exp(-t te / t2[a]), t = 1 ... echoes -> (atoms (N, T), params (N, 1))"""
    if not (te > 0 and echoes >= 1):
        raise ValueError("dictmatch: --model t2 needs --te > 0 and --echoes >= 1")
    t2 = np.asarray(t2, dtype=np.float64).ravel()
    t = te * np.arange(1, int(echoes) + 1, dtype=np.float64)
    return np.exp(-t[None, :] / t2[:, None]), t2[:, None].copy()


def atoms_ir(ti, t1):
    """inversion recovery: atoms[a, t] = 1 - 2 exp(-ti[t] / t1[a]) -> (atoms (N, T), params (N, 1))"""
    ti = np.asarray(ti, dtype=np.float64).ravel()
    if ti.size < 1 or not (ti >= 0).all():
        raise ValueError("dictmatch: --model ir needs at least one inversion time, none of them negative")
    t1 = np.asarray(t1, dtype=np.float64).ravel()
    return 1.0 - 2.0 * np.exp(-ti[None, :] / t1[:, None]), t1[:, None].copy()


# ---- extended-phase-graph programs (Backend.epg_signal) ---------------------------------------------------------------------------

SHIFT_A, SHIFT_B, RECORD, SPOIL = 1, 2, 4, 8        # the flag bits of a step
MAX_STATES = 256


def _program(rows):
    steps = np.array([r[:4] for r in rows], dtype=np.float64).reshape(-1, 4)
    return steps, np.array([r[4] for r in rows], dtype=np.int32)


def program_fse(te, flips):
    """CPMG echo train -> (steps (T + 1, 4) float64, flags (T + 1,) int32) for `Backend.epg_signal`: an excitation (pi/2, phase pi/2)
    followed by te/2 and a shift, then for each of the T refocusing angles `flips` (radians): the pulse (phase 0), te/2, a shift, the
    record of the echo, te/2, a shift.  T records."""
    flips = np.asarray(flips, dtype=np.float64).ravel()
    if not (np.isfinite(te) and te > 0):
        raise ValueError("dictmatch: an fse program needs an echo spacing --te > 0, got %r" % (te,))
    if flips.size < 1 or not np.isfinite(flips).all():
        raise ValueError("dictmatch: an fse program needs at least one refocusing flip angle, all of them finite")
    rows = [(np.pi / 2, np.pi / 2, te / 2, 0.0, SHIFT_A)]
    rows += [(a, 0.0, te / 2, te / 2, SHIFT_A | RECORD | SHIFT_B) for a in flips]
    return _program(rows)


def program_fisp(flips, tr, te, phases=None, ti=None):
    """Unbalanced steady-state (fingerprinting) train -> (steps, flags) for `Backend.epg_signal`: if `ti` is given an inversion
    (pi, phase 0), ti and a spoiler; then for pulse t of the T `flips` (radians; `phases` radians, default 0): the pulse, te, the
    record, tr[t] - te, a shift.  `tr` is one value or T values.  T records."""
    flips = np.asarray(flips, dtype=np.float64).ravel()
    T = flips.size
    if T < 1 or not np.isfinite(flips).all():
        raise ValueError("dictmatch: a fisp program needs at least one flip angle, all of them finite")
    tr = np.asarray(tr, dtype=np.float64).ravel()
    if tr.size == 1:
        tr = np.full(T, tr[0])
    if tr.size != T:
        raise ValueError("dictmatch: %d flip angles and %d repetition times: --tr is one value or one per flip angle" % (T, tr.size))
    phases = np.zeros(T) if phases is None else np.asarray(phases, dtype=np.float64).ravel()
    if phases.size != T or not np.isfinite(phases).all():
        raise ValueError("dictmatch: %d flip angles and %d phases: --phases holds one finite value per flip angle" % (T, phases.size))
    if not (np.isfinite(te) and te >= 0):
        raise ValueError("dictmatch: a fisp program needs an echo time --te >= 0, got %r" % (te,))
    if not np.isfinite(tr).all() or (tr < te).any():
        t = int(np.argmax(~(tr >= te)))
        raise ValueError("dictmatch: repetition time %g of pulse %d is below the echo time %g" % (tr[t], t, te))
    rows = []
    if ti is not None:
        if not (np.isfinite(ti) and ti >= 0):
            raise ValueError("dictmatch: the inversion time --ti must be >= 0, got %r" % (ti,))
        rows.append((np.pi, 0.0, float(ti), 0.0, SPOIL))
    rows += [(flips[t], phases[t], te, tr[t] - te, RECORD | SHIFT_B) for t in range(T)]
    return _program(rows)


def check_states(nstates):
    if not 1 <= nstates <= MAX_STATES:
        raise ValueError("dictmatch: --states %d, between 1 and %d are supported" % (nstates, MAX_STATES))
    return int(nstates)


def atom_grid(t1, t2, b1, drop_t2_above_t1=False):
    """-> (N, 3) float64 rows (T1, T2, B1) of the product grid, T1 slowest and B1 fastest; optionally without the rows with T2 > T1"""
    g = np.stack([a.ravel() for a in np.meshgrid(t1, t2, b1, indexing='ij')], axis=1)
    if drop_t2_above_t1:
        g = g[g[:, 1] <= g[:, 0]]
        if g.shape[0] < 1:
            raise ValueError("dictmatch: every atom of the grid has T2 > T1, nothing is left to simulate")
    return np.ascontiguousarray(g)


def check_dictionary(atoms, params):
    atoms, params = np.asarray(atoms), np.asarray(params)
    if atoms.ndim != 2 or atoms.shape[0] < 1 or atoms.shape[1] < 1:
        raise ValueError("dictmatch: the atoms must be an (N, T) array, got shape %s" % (atoms.shape,))
    if params.ndim == 1:
        params = params[:, None]
    if params.ndim != 2 or params.shape[0] != atoms.shape[0]:
        raise ValueError("dictmatch: the parameters must be an (N, P) array with a row per atom: %d atoms, parameters of shape %s"
                         % (atoms.shape[0], params.shape))
    if not np.isfinite(atoms).all():
        raise ValueError("dictmatch: the atoms hold values that are not finite")
    return atoms, params


def basis_of(atoms, rank=None, energy=None):
    """-> (phi, singular values): the (T, K) matrix of the K leading right singular vectors of the (N, T) atoms, so that
    atoms ~ (atoms phi) phi^H, and all singular values (descending).  K = rank, or the smallest K whose singular values hold the
    fraction `energy` of their squared sum.  Every vector is rotated so that its largest-magnitude component is real and positive."""
    if (rank is None) == (energy is None):
        raise ValueError("dictmatch: give either the number of basis vectors (--rank) or the energy fraction (--energy), not both")
    atoms = np.asarray(atoms)
    atoms = atoms.astype(np.complex128 if np.iscomplexobj(atoms) else np.float64)
    _, sv, vh = np.linalg.svd(atoms, full_matrices=False)
    if rank is None:
        if not 0 < energy <= 1:
            raise ValueError("dictmatch: energy fraction %g, must be in (0, 1]" % energy)
        e = sv ** 2
        rank = min(int(np.searchsorted(np.cumsum(e), energy * e.sum(), side='left')) + 1, sv.size)
        log.info("energy %g: %d basis vectors", energy, rank)
    rank = int(rank)
    if not 1 <= rank <= sv.size:
        raise ValueError("dictmatch: --rank %d, between 1 and min(N, T) = %d are possible" % (rank, sv.size))
    check_coeffs(rank)
    phi = vh[:rank].conj().T.copy()
    big = np.argmax(np.abs(phi), axis=0)
    pivot = phi[big, np.arange(rank)]
    phi = phi * (np.conj(pivot) / np.abs(pivot))[None, :]
    return phi, sv


def check_coeffs(K):
    if not 1 <= K <= MAX_COEFFS:
        raise ValueError("dictmatch: %d coefficients, between 1 and %d are supported (Backend.dict_match; --basis-rank keeps the "
                         "first K columns of the basis)" % (K, MAX_COEFFS))


def check_basis(phi, T, rank=None):
    """the (T, K) basis cut to its first `rank` columns, checked against the atoms' T time points"""
    phi = np.asarray(phi)
    if phi.ndim != 2:
        raise ValueError("dictmatch: the basis must be a 2-D array (frames x coefficients), got shape %s" % (phi.shape,))
    if phi.shape[0] != T:
        raise ValueError("dictmatch: the basis has %d rows, the atoms have %d time points" % (phi.shape[0], T))
    if rank is not None:
        if not 1 <= rank <= phi.shape[1]:
            raise ValueError("dictmatch: --basis-rank %d, the basis has %d columns" % (rank, phi.shape[1]))
        phi = phi[:, :rank]
    check_coeffs(phi.shape[1])
    return phi


def compress(atoms, phi):
    """-> (d, norms): the atoms in the subspace, Phi^H s_a, normalised -- the (K, N) complex128 dictionary `Backend.dict_match`
    takes (once cast to complex64) -- and the N norms ||Phi^H s_a|| (float64)"""
    D = np.asarray(phi, dtype=np.complex128).conj().T @ np.asarray(atoms, dtype=np.complex128).T
    norms = np.sqrt((D.real ** 2 + D.imag ** 2).sum(axis=0))
    if not (norms > 0).all():
        raise ValueError("dictmatch: atom %d has no component in the subspace of the basis" % int(np.argmin(norms)))
    return D / norms[None, :], norms


# ---- matching -------------------------------------------------------------------------------------------------------------------

def fit(B, coeffs, atoms, params, phi, mask_rel=0.02, chunk=CHUNK):
    """Match the (n, K) host panel of coefficients `coeffs` (voxel i in row i) against the (N, T) atoms seen through the (T, K)
    basis phi -> {'qmaps': (n, P) float32, 'pd': (n,) complex64, 'index': (n,) int32, 'misfit': (n,) float32, 'mask': (n,) bool}, the
    arrays of the module docstring with the voxels in one axis; voxels outside the mask hold zeros"""
    atoms, params = check_dictionary(atoms, params)
    phi = check_basis(phi, atoms.shape[1])
    c = np.asarray(coeffs)
    K = phi.shape[1]
    if c.ndim != 2 or c.shape[1] != K:
        raise ValueError("dictmatch: a panel of coefficients of shape %s for a basis of %d columns" % (c.shape, K))
    if not 0 <= mask_rel < 1:
        raise ValueError("dictmatch: --mask-rel %g, must be in [0, 1)" % mask_rel)
    n, chunk = c.shape[0], max(1, int(chunk))
    d, norms = compress(atoms, phi)
    d_d = B.copy_array(np.asfortranarray(d.astype(_C64)), name='dict.atoms')              # uploaded once
    index, ip = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=_C64)
    for i0 in range(0, n, chunk):
        rows = min(chunk, n - i0)
        x_d = B.copy_array(np.asfortranarray(c[i0:i0 + rows].astype(_C64, copy=False)), name='dict.panel')
        index[i0:i0 + rows], ip[i0:i0 + rows] = B.dict_match(x_d, d_d, rows)
        del x_d
    c64 = c.astype(_C64, copy=False)
    norm2 = (c64.real.astype(np.float64) ** 2 + c64.imag.astype(np.float64) ** 2).sum(axis=1)
    mask = (norm2 > 0) & (np.sqrt(norm2) >= mask_rel * np.sqrt(norm2.max(initial=0.0)))
    log.info("matched %d voxels against %d atoms of %d coefficients; %d voxels inside the mask", n, atoms.shape[0], K, int(mask.sum()))
    index = np.where(mask, index, 0).astype(np.int32)
    s = ip.real.astype(np.float64) ** 2 + ip.imag.astype(np.float64) ** 2
    return {'qmaps': np.where(mask[:, None], params[index], 0).astype(np.float32),
            'pd': np.where(mask, ip / norms[index], 0).astype(_C64),
            'index': index,
            'misfit': np.where(mask, 1.0 - s / np.where(mask, norm2, 1.0), 0).astype(np.float32),
            'mask': mask}


def fit_frames(B, frames_panel, phi, atoms, params, mask_rel=0.02, chunk=CHUNK):
    """`fit` for a reconstruction of T time frames made without `--basis`: frames_panel is the (n, T) host panel of the frames
    (voxel i in row i); its coefficients c = Phi^H x come from `Backend.frame_basis(adjoint=True)`, chunk by chunk"""
    atoms, params = check_dictionary(atoms, params)
    phi = check_basis(phi, atoms.shape[1])
    f = np.asarray(frames_panel)
    T, K = phi.shape
    if f.ndim != 2 or f.shape[1] != T:
        raise ValueError("dictmatch: a panel of frames of shape %s for a basis of %d rows" % (f.shape, T))
    n, chunk = f.shape[0], max(1, int(chunk))
    phi_d = B.copy_array(np.asfortranarray(phi.astype(_C64)), name='dict.phi')
    c = np.empty((n, K), dtype=_C64, order='F')
    for i0 in range(0, n, chunk):
        rows = min(chunk, n - i0)
        x_d = B.copy_array(np.asfortranarray(f[i0:i0 + rows].astype(_C64, copy=False)), name='dict.frames')
        y_d = B.empty_array((rows, K), _C64, name='dict.panel')
        B.frame_basis(y_d, x_d, phi_d, rows, adjoint=True)
        c[i0:i0 + rows] = y_d.to_host()
        del x_d, y_d
    return fit(B, c, atoms, params, phi, mask_rel=mask_rel, chunk=chunk)


# ---- the command line -------------------------------------------------------------------------------------------------------------

def parse(argv):
    ap = argparse.ArgumentParser(prog="indigo_amd.dictmatch", description="Dictionary matching: `basis` writes the temporal basis for "
                                 "pics --basis from simulated signal curves, `fit` turns the coefficient images into quantitative maps.")
    sub = ap.add_subparsers(dest='command', required=True)
    b = sub.add_parser('basis', help='simulate a dictionary and write <out>.atoms.npy, <out>.params.npy and <out>.phi.npy')
    b.add_argument('--model', choices=['t2', 'ir', 'fse', 'fisp'], default=None,
                   help='t2: multi-echo spin echo; ir: inversion recovery; fse: CPMG echo train (EPG); fisp: unbalanced steady-state train (EPG)')
    b.add_argument('--te', type=float, default=None, help='echo spacing (--model t2, fse) or echo time (--model fisp) in seconds')
    b.add_argument('--echoes', type=int, default=None, help='number of echoes T (--model t2, fse)')
    b.add_argument('--t2', default=None, help='lo:hi:N, a log-spaced grid of T2 values in seconds (--model t2, fse, fisp)')
    b.add_argument('--ti', default=None, help='a .npy file with the T inversion times in seconds (--model ir); the inversion time in '
                   'seconds (--model fisp, optional)')
    b.add_argument('--t1', default=None, help='lo:hi:N, a log-spaced grid of T1 values in seconds (--model ir, fisp; fse: default 1.0)')
    b.add_argument('--b1', default=None, help='lo:hi:N, an evenly spaced grid of B1 scales of the flip angles (--model fse, fisp; default 1.0)')
    b.add_argument('--flip', type=float, default=None, help='the refocusing flip angle in degrees (--model fse)')
    b.add_argument('--flips', default=None, help='a .npy file with the T flip angles in degrees (--model fse, fisp)')
    b.add_argument('--phases', default=None, help='a .npy file with the T pulse phases in degrees (--model fisp, default 0)')
    b.add_argument('--tr', default=None, help='the repetition time in seconds, or a .npy file with T of them (--model fisp)')
    b.add_argument('--states', type=int, default=None, help='configuration states kept, 1 ... 256 (--model fse: default min(T + 1, 256); '
                   'fisp: default 32)')
    b.add_argument('--chunk', type=int, default=EPG_CHUNK, help='atoms simulated on the device at a time (--model fse, fisp)')
    b.add_argument('--backend', type=str, default='hip', choices=['hip'], help='where --model fse and fisp are simulated')
    b.add_argument('--device', type=int, default=0)
    b.add_argument('--atoms', default=None, help='a .npy file with an (N, T) dictionary simulated elsewhere (with --params)')
    b.add_argument('--params', default=None, help='a .npy file with the (N, P) parameters of --atoms')
    how = b.add_mutually_exclusive_group(required=True)
    how.add_argument('--rank', type=int, default=None, help='number of basis vectors K (1 ... 32)')
    how.add_argument('--energy', type=float, default=None, help='the smallest K whose singular values hold this fraction of their squared sum')
    b.add_argument('out', help='stem of the three files written')
    f = sub.add_parser('fit', help='match the coefficient images of pics --basis and write <name>.qmaps/.pd/.index/.misfit.npy')
    f.add_argument('--atoms', required=True, help='the (N, T) dictionary, a .npy file (`basis` writes one)')
    f.add_argument('--params', required=True, help='the (N, P) parameters of the atoms, a .npy file')
    f.add_argument('--basis', required=True, help='the (T, K) temporal basis the reconstruction used, a .npy file')
    f.add_argument('--basis-rank', type=int, default=None, help='keep the first K columns of --basis, as pics --basis-rank did')
    f.add_argument('--mask-rel', type=float, default=0.02, help='voxels with ||c|| below this fraction of the largest ||c|| get zeros')
    f.add_argument('--chunk', type=int, default=CHUNK, help='voxels on the device at a time')
    f.add_argument('--backend', type=str, default='hip', choices=['hip'])
    f.add_argument('--device', type=int, default=0)
    f.add_argument('rec', help='the .npy result of pics --basis: the coefficient images, stored reversed')
    for p in (b, f):
        p.add_argument('--debug', type=int, default=logging.INFO, help='logging level')
    args = ap.parse_args(argv)
    if args.chunk < 1:
        ap.error("--chunk must be at least 1")
    return args


def _degrees(path, what):
    a = np.asarray(np.load(path), dtype=np.float64).ravel()
    if a.size < 1 or not np.isfinite(a).all():
        raise ValueError("dictmatch basis: %s holds no values, or values that are not finite" % what)
    return np.deg2rad(a)


def epg_program(args):
    """-> (steps, flags, nstates, (N, 3) params) of `basis --model fse | fisp`"""
    b1 = grid(args.b1, log=False) if args.b1 is not None else np.array([1.0])
    if args.model == 'fse':
        if args.te is None or args.echoes is None or args.t2 is None or (args.flip is None) == (args.flips is None):
            raise ValueError("dictmatch basis: --model fse needs --te, --echoes, --t2 and either --flip or --flips")
        if args.echoes < 1:
            raise ValueError("dictmatch basis: --model fse needs --echoes >= 1")
        flips = np.full(args.echoes, np.deg2rad(args.flip)) if args.flip is not None else _degrees(args.flips, "--flips")
        if flips.size != args.echoes:
            raise ValueError("dictmatch basis: --flips holds %d angles for --echoes %d" % (flips.size, args.echoes))
        steps, flags = program_fse(args.te, flips)
        nstates = check_states(args.states if args.states is not None else min(args.echoes + 1, MAX_STATES))
        t1 = grid(args.t1) if args.t1 is not None else np.array([1.0])
        return steps, flags, nstates, atom_grid(t1, grid(args.t2), b1)
    if args.flips is None or args.tr is None or args.te is None or args.t1 is None or args.t2 is None:
        raise ValueError("dictmatch basis: --model fisp needs --flips, --tr, --te, --t1 and --t2")
    try:
        tr = np.array([float(args.tr)])
    except ValueError:
        tr = np.asarray(np.load(args.tr), dtype=np.float64).ravel()
    try:
        ti = None if args.ti is None else float(args.ti)
    except ValueError:
        raise ValueError("dictmatch basis: --model fisp takes the inversion time --ti as a value in seconds, got %r" % (args.ti,))
    steps, flags = program_fisp(_degrees(args.flips, "--flips"), tr, args.te,
                                phases=None if args.phases is None else _degrees(args.phases, "--phases"), ti=ti)
    nstates = check_states(args.states if args.states is not None else 32)
    return steps, flags, nstates, atom_grid(grid(args.t1), grid(args.t2), b1, drop_t2_above_t1=True)


def simulate(args, backend=None):
    """the (atoms, params) of a `basis` run: one of the four models, or the files of --atoms and --params"""
    given = (args.model is not None) + (args.atoms is not None)
    if given != 1:
        raise ValueError("dictmatch basis: give either --model or --atoms with --params")
    if args.atoms is not None:
        if args.params is None:
            raise ValueError("dictmatch basis: --atoms needs --params, the parameters of every atom")
        return check_dictionary(np.load(args.atoms), np.load(args.params))
    if args.model == 't2':
        if args.te is None or args.echoes is None or args.t2 is None:
            raise ValueError("dictmatch basis: --model t2 needs --te, --echoes and --t2")
        return atoms_t2(args.te, args.echoes, grid(args.t2))
    if args.model in ('fse', 'fisp'):
        steps, flags, nstates, params = epg_program(args)
        if backend is None:
            from indigo_amd.backends import get_backend
            backend = get_backend(args.backend, device_id=args.device)
        log.info("simulating %d atoms, %d steps, %d states on %s", params.shape[0], steps.shape[0], nstates, type(backend).__name__)
        return check_dictionary(backend.epg_signal(params, steps, flags, nstates, chunk=args.chunk), params)
    if args.ti is None or args.t1 is None:
        raise ValueError("dictmatch basis: --model ir needs --ti and --t1")
    return atoms_ir(np.load(args.ti), grid(args.t1))


def main(argv=None, backend=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=args.debug)
    if args.command == 'basis':
        atoms, params = simulate(args, backend)
        phi, sv = basis_of(atoms, rank=args.rank, energy=args.energy)
        K = phi.shape[1]
        log.info("%d atoms of %d time points, %d basis vectors hold %.8f of the energy", atoms.shape[0], atoms.shape[1], K,
                 (sv[:K] ** 2).sum() / max((sv ** 2).sum(), 1e-300))
        np.save(args.out + ".atoms.npy", atoms)
        np.save(args.out + ".params.npy", params)
        np.save(args.out + ".phi.npy", phi)
        return atoms, params, phi
    atoms, params = check_dictionary(np.load(args.atoms), np.load(args.params))
    phi = check_basis(np.load(args.basis), atoms.shape[1], args.basis_rank)
    K = phi.shape[1]
    rec = np.load(args.rec).T
    if rec.ndim != COEFF + 1 or rec.shape[COEFF] != K or rec.shape[3:COEFF] != (1,) * (COEFF - 3):
        raise ValueError("dictmatch fit: %s holds %s (stored reversed); expected the coefficient images of pics --basis, "
                         "(X, Y, Z, 1, 1, 1, K) with K = %d, the columns of the basis" % (args.rec, rec.shape, K))
    if backend is None:
        from indigo_amd.backends import get_backend
        backend = get_backend(args.backend, device_id=args.device)
    log.info("using backend: %s", type(backend).__name__)
    dims = rec.shape[:3]
    out = fit(backend, rec.reshape((-1, K), order='F'), atoms, params, phi, mask_rel=args.mask_rel, chunk=args.chunk)
    stem = os.path.splitext(args.rec)[0]
    shaped = {'qmaps': out['qmaps'].reshape(dims + (params.shape[1],), order='F'), 'pd': out['pd'].reshape(dims, order='F'),
              'index': out['index'].reshape(dims, order='F'), 'misfit': out['misfit'].reshape(dims, order='F')}
    for name, a in shaped.items():
        np.save("%s.%s.npy" % (stem, name), a.T)
    log.info("matching complete: %s.qmaps.npy %s, .pd.npy, .index.npy, .misfit.npy", stem, shaped['qmaps'].shape)
    return shaped


if __name__ == "__main__":
    main()
