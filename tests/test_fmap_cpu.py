"""Off-resonance correction on the numpy oracle backend: the host forms of Backend.segment_phase / segment_combine against the
float64 restatement in tests/fmap64.py, the interpolator of indigo_amd.fmap, the time-segmented model against the exact
off-resonant signal, and pics --fmap."""
import logging
import os

import numpy as np
import pytest

import fmap64
from test_toeplitz_cpu import accuracy  # noqa: F401  (the fixture whose e_grid is the bar of the Toeplitz comparison)
from indigo_amd import fmap as fmap_mod
from indigo_amd import pics
from indigo_amd.toeplitz import psf_kernel
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
ALPHA, BETA = 0.7 - 0.3j, 0.5 + 0.25j
WIDTH, OSF = 3, 2.0          # of the accuracy test and of the driver runs: those of tests/test_toeplitz_cpu.py, whose bar they take


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _field(n, cycles, taus, seed):
    """n float32 field values with max|f tau| = cycles"""
    f = np.random.default_rng(seed).uniform(-1, 1, n)
    return (f * (cycles / (np.abs(f).max() * np.abs(taus).max()))).astype(np.float32)


# ---- 1. the host forms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stacked", [False, True], ids=["panel", "vector"])
@pytest.mark.parametrize("L", [1, 3, 16])
def test_host_forms_match_the_float64_restatement(oracle_backend, L, stacked):
    B = oracle_backend
    n, P = 105, 7
    taus = 1e-3 + 2.5e-3 * np.arange(L)
    f = _field(n, 5.0, taus, seed=L)
    table = rand64c(P, L, seed=L + 1)
    f_d, b_d = B.copy_array(f), B.copy_array(table)

    def dev(a):
        return B.copy_array(np.asfortranarray(a.reshape((-1, 1), order='F')) if stacked else a)
    for adjoint in (False, True):
        for which in ("phase", "combine"):
            wide_x = adjoint == (which == "phase")                         # the side with L columns
            x = rand64c(n, L if wide_x else 1, seed=2)
            y = rand64c(n, 1 if wide_x else L, seed=3)
            for beta, y0 in ((0, np.full_like(y, np.nan)), (BETA, y)):
                y_d = dev(y0)
                if which == "phase":
                    B.segment_phase(y_d, dev(x), f_d, taus[0], 2.5e-3, L, n, adjoint=adjoint, alpha=ALPHA, beta=beta)
                    want = fmap64.phase(f, taus, x, y, adjoint, ALPHA, beta)
                else:
                    B.segment_combine(y_d, dev(x), b_d, P, n, adjoint=adjoint, alpha=ALPHA, beta=beta)
                    want = fmap64.combine(table, P, x, y, adjoint, ALPHA, beta)
                got = y_d.to_host().reshape(want.shape, order='F')
                assert got.dtype == C64 and _rel(got, want) < 2e-7, (which, adjoint, beta, _rel(got, want))


def test_operators_shapes_adjointness_and_errors(oracle_backend):
    B = oracle_backend
    n, P, L = 105, 7, 3
    taus = np.linspace(1e-3, 6e-3, L)
    f = _field(n, 5.0, taus, seed=1)
    table = rand64c(P, L, seed=2)
    Ph, Cb = B.SegmentPhase(f, taus, n), B.SegmentCombine(table, P, n)
    assert Ph.shape == (n * L, n) and Ph.H.shape == (n, n * L) and Ph.dtype == C64
    assert Cb.shape == (n, n * L) and Cb.H.shape == (n * L, n) and Cb.dtype == C64
    x, z = rand64c(n, 2, seed=3), rand64c(n * L, 2, seed=4)               # two columns: evaluated column by column
    for op, (u, v) in ((Ph, (x, z)), (Cb, (z, x))):
        fwd, adj = (op * u).astype(np.complex128), (op.H * v).astype(np.complex128)
        for j in range(2):
            lhs, rhs = np.vdot(v[:, j].astype(np.complex128), fwd[:, j]), np.vdot(adj[:, j], u[:, j].astype(np.complex128))
            assert abs(lhs - rhs) < 1e-5 * abs(lhs), (lhs, rhs)
    assert _rel(Ph * x[:, :1], fmap64.phase(f, taus, x[:, 0]).reshape((-1, 1), order='F')) < 2e-7
    assert _rel(Cb.H * x[:, :1], fmap64.combine(table, P, x[:, 0], adjoint=True).reshape((-1, 1), order='F')) < 2e-7
    y_d = B.copy_array(z[:, :1])
    Ph.eval(y_d, B.copy_array(x[:, :1]), alpha=ALPHA, beta=BETA)
    want = fmap64.phase(f, taus, x[:, 0], z[:, 0].reshape((n, L), order='F'), False, ALPHA, BETA)
    assert _rel(y_d.to_host(), want.reshape((-1, 1), order='F')) < 2e-7
    for bad, msg in ((lambda: B.SegmentPhase(f, np.linspace(0, 1, 17), n), "SegmentPhase: 17 segments"),
                     (lambda: B.SegmentPhase(f, [], n), "SegmentPhase: 0 segments"),
                     (lambda: B.SegmentPhase(f[:-1], taus, n), "SegmentPhase: a field map of 104 values"),
                     (lambda: B.SegmentPhase(f + 1j, taus, n), "SegmentPhase: the field map and the segment times must be real"),
                     (lambda: B.SegmentPhase(f, [0.0, 1e-3, 3e-3], n), "SegmentPhase: the segment times must be equispaced"),
                     (lambda: B.SegmentPhase(f, taus, 0), "SegmentPhase: n must be positive"),
                     (lambda: B.SegmentCombine(rand64c(P, 17, seed=1), P, n), "SegmentCombine: 17 segments"),
                     (lambda: B.SegmentCombine(table, P + 1, n), "SegmentCombine: a table of 7 rows for the period 8"),
                     (lambda: B.SegmentCombine(table, P, n + 1), "SegmentCombine: n = 106 rows are no positive multiple"),
                     (lambda: B.SegmentCombine(table[:, 0], P, n), "SegmentCombine: the table must be 2-D")):
        with pytest.raises(ValueError, match=msg):
            bad()
    with pytest.raises(RuntimeError, match="17 segments"):
        B.segment_phase(B.copy_array(rand64c(n, 17, seed=1)), B.copy_array(x[:, :1]), B.copy_array(f), 0.0, 1e-3, 17, n)


# ---- 2-6. the interpolator ---------------------------------------------------------------------------------------------------

DIMS = (16, 16, 16)
TIMES = 1e-3 + np.arange(64) * (10e-3 / 63)                               # a 10 ms readout
FIELD = fmap64.smooth_field(DIMS, 200.0, seed=1).astype(np.float32)       # max|f| (t_max - t_min) = 2 cycles


def test_err_is_the_residual_at_the_histogram_centres():
    t2 = TIMES[:, None] + 1e-4 * np.arange(3)[None, :]                    # (readout, views): every sample its own time
    for times, L in ((TIMES, 4), (t2, 5), (TIMES, 1)):
        taus, b, period, err = fmap_mod.segments(FIELD, times, L=L, bins=64)
        assert taus.shape == (L,) and b.shape == (times.size, L) and period == times.size
        assert taus[0] == (times.min() if L > 1 else 0.5 * (times.min() + times.max())) and (L == 1 or taus[-1] == times.max())
        counts, edges = np.histogram(FIELD.astype(np.float64), bins=64)
        centres = 0.5 * (edges[:-1] + edges[1:])
        t = np.unique(times)
        model = np.zeros((centres.size, t.size), dtype=np.complex128)
        rows = {v: b[j] for j, v in enumerate(times.reshape(-1, order='F'))}
        for j, tj in enumerate(t):
            for l in range(L):
                model[:, j] += rows[tj][l] * np.exp(-2j * np.pi * centres * taus[l])
        res = np.abs(np.exp(-2j * np.pi * np.outer(centres, t)) - model) ** 2
        want = np.sqrt((counts[:, None] * res).sum() / (counts.sum() * t.size))
        assert abs(err - want) <= 1e-9 * want, (L, err, want)
    assert np.array_equal(fmap_mod.segments(FIELD, TIMES, L=1)[1], np.ones((64, 1)))


def test_a_zero_field_map_gives_rows_that_sum_to_one():
    for L in (1, 2, 5, 16):
        taus, b, period, err = fmap_mod.segments(np.zeros(DIMS, np.float32), TIMES, L=L)
        assert np.abs(b.sum(axis=1) - 1).max() < 1e-12 and err < 1e-12
    assert fmap_mod.segments(np.zeros(DIMS, np.float32), TIMES)[0].size == 1       # and the automatic choice is one segment


def test_a_constant_field_map_is_modelled_exactly():
    f0 = np.float32(137.5)
    for L in (2, 3, 8):
        taus, b, period, err = fmap_mod.segments(np.full(DIMS, f0), TIMES, L=L)
        model = (b * np.exp(-2j * np.pi * float(f0) * taus)[None, :]).sum(axis=1)
        assert np.abs(model - np.exp(-2j * np.pi * float(f0) * TIMES)).max() < 1e-10


def test_the_automatic_choice_is_the_first_count_below_the_tolerance(caplog):
    errs = [fmap_mod.segments(FIELD, TIMES, L=L)[3] for L in range(1, 17)]
    # non-increasing: L + 1 equispaced times do not contain the L, but the residual falls by a factor of 2 to 8 per segment
    # until it reaches the rounding of the solve (1e-16 times the condition number); 1e-12 absolute covers that floor
    assert all(b <= a + 1e-12 for a, b in zip(errs, errs[1:])), errs
    for tol in (1e-1, 1e-3, 1e-6):
        with caplog.at_level(logging.INFO, logger="indigo_amd.fmap"):
            taus, b, period, err = fmap_mod.segments(FIELD, TIMES, tol=tol)
        first = next(L for L, e in enumerate(errs, 1) if e < tol)
        assert taus.size == first and err == errs[first - 1]
        assert any("%d segments, field map span 2.00 cycles" % first in r.getMessage() for r in caplog.records)
        caplog.clear()


def test_an_unreachable_tolerance_raises():
    with pytest.raises(ValueError, match=r"4 segments reach a model error of \S+, not the tolerance 1.000e-03: the field map spans 2.0 cycles"):
        fmap_mod.segments(FIELD, TIMES, maxL=4)
    with pytest.raises(ValueError, match="must be real"):
        fmap_mod.segments(FIELD + 1j, TIMES)
    with pytest.raises(ValueError, match="17 segments"):
        fmap_mod.segments(FIELD, TIMES, L=17)


# ---- 7-8. the model against the exact off-resonant signal ---------------------------------------------------------------

def test_the_segmented_model_against_the_exact_signal(oracle_backend):
    """16^3, 2 coils, 64 x 48 radial samples, half-width 3, oversampling 2, a smooth field map of 2 cycles span over a 10 ms readout.
    Measured on the oracle backend: L = 8 (err 4.37e-04), e0 8.10e-03, e_seg 1.20e-02, e_plain 1.05e+00."""
    from oracle.sense64 import SenseF64
    from indigo_amd.sense import SenseProblem, radial_trajectory
    B = oracle_backend
    B._scratch = None
    C, nro, nsp = 2, 64, 48
    img, mps = fmap64.phantom(DIMS)
    coord = radial_trajectory(nsp, nro, seed=2)
    x = np.asfortranarray(img.reshape(-1, 1, order='F'))
    exact0 = fmap64.exact_offres(img, mps, coord, np.zeros(DIMS), TIMES, WIDTH, OSF)
    exactf = fmap64.exact_offres(img, mps, coord, FIELD, TIMES, WIDTH, OSF)
    # the direct sum itself, against the float64 gridding operator at f = 0: they differ by the Kaiser-Bessel NUFFT's own error,
    # per cent at this half-width and oversampling (tests/test_toeplitz_cpu.py measures 2.4e-2 where it enters twice); a wrong
    # sign, centre or constant gives a difference of order one
    p = SenseProblem(DIMS, coord, np.asfortranarray(mps), width=WIDTH, oversamp=OSF)
    assert _rel(SenseF64(p).forward(x).reshape((-1, C), order='F'), exact0) < 3e-2
    F1 = B.NUFFT((1, nro, nsp), DIMS, coord, width=WIDTH, oversamp=(OSF,) * 3, dtype=C64)
    A0 = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
    taus, b, period, err = fmap_mod.segments(FIELD, TIMES)
    n = int(np.prod(DIMS))
    A = B.SegmentCombine(b, period, A0.shape[0]) * B.BlockDiag([A0] * taus.size) * B.SegmentPhase(FIELD.reshape(-1, order='F'), taus, n)
    assert A.shape == A0.shape
    plain, seg = (A0 * x).reshape((-1, C), order='F'), (A * x).reshape((-1, C), order='F')
    e0, e_seg, e_plain = _rel(plain, exact0), _rel(seg, exactf), _rel(plain, exactf)
    print("L %d, err %.3e, e0 %.3e, e_seg %.3e, e_plain %.3e" % (taus.size, err, e0, e_seg, e_plain))
    assert e_seg <= 2 * e0 + 2 * err, (e_seg, e0, err)
    assert e_plain >= 10 * e_seg, (e_plain, e_seg)
    # A^H through adjointness: <z, A x> = <A^H z, x>
    z = rand64c(A.shape[0], 1, seed=3)
    lhs = np.vdot(z.astype(np.complex128), (A * x).astype(np.complex128))
    rhs = np.vdot((A.H * z).astype(np.complex128), x.astype(np.complex128))
    assert abs(lhs - rhs) < 1e-5 * abs(lhs), (lhs, rhs)
    B._scratch = None


# ---- 9-12. the driver --------------------------------------------------------------------------------------------------------

def _pics(B, argv):
    B._scratch = None
    out = pics.main(argv, backend=B)
    B._scratch = None
    return out


SCAN_DIMS, NRO, NSP = (16, 16, 8), 32, 96
SCAN_TIMES = 1e-3 + np.arange(NRO) * (8e-3 / (NRO - 1))
COMMON = ["--osf", str(OSF), "--width", str(WIDTH), "--lamda", "1e-3", "--debug", "40"]


@pytest.fixture(scope="module")
def scans(tmp_path_factory, oracle_backend):
    """a scan without a field map, with fmap.npy of zeros next to it, and one under a field map of 1 cycle span"""
    zero = fmap64.fmap_scan(tmp_path_factory.mktemp("fmap_zero"), oracle_backend, SCAN_DIMS, np.zeros(SCAN_DIMS), SCAN_TIMES,
                            NRO, NSP, OSF, WIDTH)
    field = fmap64.smooth_field(SCAN_DIMS, 125.0, seed=2)
    offres = fmap64.fmap_scan(tmp_path_factory.mktemp("fmap_field"), oracle_backend, SCAN_DIMS, field, SCAN_TIMES, NRO, NSP, OSF, WIDTH)
    return zero, offres


def test_a_zero_field_map_gives_the_plain_run(scans, oracle_backend):
    """The two runs solve the same system with different rounding (b = 1/3 is not a float32 number, and every product is summed
    over three segments): they differ by 7e-7 after one iteration, and CG amplifies that by the condition number of A^H A + lamda I.
    A radial scan without density compensation has eigenvalues from the hundreds (the centre, which every spoke crosses) down to
    zero, so the test takes lamda = 10: a condition number of tens.  Measured: 7.6e-07 after 1 iteration, 5.2e-05 after 10
    (with lamda = 1e-3: 1.6e-04 after 10, and the plain run with and without --no-fuse then differs by 4.3e-05 from itself)."""
    (path, fmap, times), _ = scans
    common = [a if a != "1e-3" else "10" for a in COMMON]
    for iters, tol in (("1", 1e-5), ("10", 1e-4)):
        plain = _pics(oracle_backend, ["-i", iters] + common + [path])
        seg = _pics(oracle_backend, ["-i", iters, "--fmap", fmap, "--fmap-segments", "3", "--times", times] + common + [path])
        assert seg.shape == plain.shape == SCAN_DIMS + (1,)
        print("zero field map, %s iterations: relative difference %.3e" % (iters, _rel(seg, plain)))
        assert _rel(seg, plain) < tol, (iters, _rel(seg, plain))


def test_the_field_map_changes_the_image_and_the_flags_agree(scans, oracle_backend, tmp_path, caplog):
    _, (path, fmap, times) = scans
    args = ["-i", "4", "--fmap", fmap] + COMMON + [path]
    with caplog.at_level(logging.INFO, logger="indigo_amd.fmap"):
        by_times = _pics(oracle_backend, ["--times", times] + args)
    assert any("segments, field map span 1.00 cycles" in r.getMessage() for r in caplog.records)
    dwell, te = SCAN_TIMES[1] - SCAN_TIMES[0], SCAN_TIMES[0]
    by_dwell = _pics(oracle_backend, ["--dwell", repr(float(dwell)), "--te", repr(float(te))] + args)
    assert _rel(by_dwell, by_times) < 1e-5
    plain = _pics(oracle_backend, ["-i", "4"] + COMMON + [path])
    assert by_times.shape == plain.shape and _rel(plain, by_times) > 0.05
    # the arrays inside the scan are used without the flags, and (readout, views) times give the same image
    z = dict(np.load(path))
    both = os.path.join(str(tmp_path), "both.npz")
    np.savez(both, fmap=np.load(fmap), times=np.broadcast_to(SCAN_TIMES[:, None], (NRO, NSP)).T, **z)
    inside = _pics(oracle_backend, ["-i", "4"] + COMMON + [both])
    assert _rel(inside, by_times) < 1e-5
    # every regulariser runs on the N unknowns
    for extra in (["--l1", "0.01", "--levels", "2"], ["--tv", "0.01"], ["--llr", "0.02", "--llr-block", "6"]):
        out = _pics(oracle_backend, extra + ["--power-iters", "4", "--times", times] + args)
        assert out.shape == plain.shape and np.isfinite(out).all() and np.abs(out).max() > 0


def test_the_toeplitz_form_agrees_with_the_gridding_form(scans, oracle_backend, accuracy, monkeypatch, caplog):  # noqa: F811
    """A^H A x of both forms of pics --fmap for a random x.  The two forms differ by the NUFFT's own error: the bar is the one
    tests/test_toeplitz_cpu.py sets between the existing Toeplitz form and the gridding form, 10 e_grid at the same half-width and
    oversampling.  Measured on the oracle backend: 1.1e-2 against a bar of 2.4e-1."""
    _, (path, fmap, times) = scans
    x = rand64c(int(np.prod(SCAN_DIMS)), 1, seed=11)
    got = []

    def capture(AHA, b, x0, maxiter=0, **kwargs):
        got.append(AHA * x)
        return []
    monkeypatch.setattr(oracle_backend, "cg", capture, raising=False)
    args = ["-i", "1", "--fmap", fmap, "--times", times, "--fmap-segments", "4"] + COMMON + [path]
    _pics(oracle_backend, args)
    with caplog.at_level(logging.INFO):
        _pics(oracle_backend, ["--toeplitz", "--debug", "20"] + args)
    msgs = [r.getMessage() for r in caplog.records]
    assert not any("scratch arena too small" in m for m in msgs), msgs
    assert any("kernel of 4 x 4 point-spread functions" in m for m in msgs), msgs
    err = _rel(got[1], got[0])
    print("pics --fmap --toeplitz against --fmap on A^H A x: relative difference %.3e, bar %.3e" % (err, 10 * accuracy[0]))
    assert err < 10 * accuracy[0], (err, accuracy)


def test_psf_kernel_without_sample_weights_is_unchanged(oracle_backend):
    B = oracle_backend
    rng = np.random.default_rng(2)
    trj = rng.random((3, 60, 1)) - 0.5
    phi = rand64c(3, 2, seed=8)
    B._scratch = None
    a = psf_kernel(B, (6, 5, 4), [trj], [0, 0, 0], phi, WIDTH, OSF)
    B._scratch = None
    b = psf_kernel(B, (6, 5, 4), [trj], [0, 0, 0], phi, WIDTH, OSF, sample_weights=None)
    B._scratch = None
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # weights that factor, w[:, l] = c_l, give the kernel of the one-frame basis phi = c
    c = rand64c(1, 2, seed=9)
    w = psf_kernel(B, (6, 5, 4), [trj], [0], None, WIDTH, OSF, sample_weights=np.tile(c, (60, 1)))
    B._scratch = None
    k = psf_kernel(B, (6, 5, 4), [trj], [0], c, WIDTH, OSF)
    B._scratch = None
    assert _rel(w, k) < 1e-5
    with pytest.raises(ValueError, match="sample weights of shape"):
        psf_kernel(B, (6, 5, 4), [trj], [0], None, WIDTH, OSF, sample_weights=np.ones((59, 2)))
    with pytest.raises(ValueError, match="one trajectory, one frame and no basis"):
        psf_kernel(B, (6, 5, 4), [trj], [0, 0], None, WIDTH, OSF, sample_weights=np.ones((60, 2)))


def test_refusals(scans, oracle_backend, tmp_path, capsys):
    (path, fmap, times), _ = scans
    tmp = str(tmp_path)
    base = COMMON + [path]
    z = dict(np.load(path))
    # flags alone
    for argv, msg in ((["--fmap", fmap, "--times", times, "--dwell", "1e-5"], "--times and --dwell cannot be combined"),
                      (["--fmap", fmap, "--te", "1e-3"], "--te needs --dwell"),
                      (["--fmap", fmap, "--dwell", "1e-5", "--basis", "phi.npy"], "--fmap cannot be combined with --basis"),
                      (["--fmap", fmap, "--dwell", "1e-5", "--fmap-segments", "17"], "--fmap-segments must lie between 1 and 16"),
                      (["--fmap", fmap, "--dwell", "1e-5", "--fmap-segments", "9", "--toeplitz"], "at most 8 time segments")):
        with pytest.raises(SystemExit):
            pics.parse(argv + [path])
        assert msg in capsys.readouterr().err
    # a field map without times
    with pytest.raises(ValueError, match="--fmap needs the sample times"):
        _pics(oracle_backend, ["--fmap", fmap] + base)
    # --dwell with a scan that holds its own times
    both = os.path.join(tmp, "both.npz")
    np.savez(both, times=SCAN_TIMES, **z)
    with pytest.raises(ValueError, match="--dwell cannot be combined with the scan's own `times`"):
        _pics(oracle_backend, ["--fmap", fmap, "--dwell", "1e-5"] + COMMON + [both])
    # a shape that differs from the maps', and times that do not fit the k-space
    np.save(os.path.join(tmp, "short.npy"), np.zeros(SCAN_DIMS[:2] + (SCAN_DIMS[2] - 1,), np.float32).T)
    with pytest.raises(ValueError, match=r"the field map has shape \(16, 16, 7\), the maps have \(16, 16, 8\)"):
        _pics(oracle_backend, ["--fmap", os.path.join(tmp, "short.npy"), "--times", times] + base)
    np.save(os.path.join(tmp, "t31.npy"), SCAN_TIMES[:-1])
    with pytest.raises(ValueError, match=r"the sample times have shape \(31,\)"):
        _pics(oracle_backend, ["--fmap", fmap, "--times", os.path.join(tmp, "t31.npy")] + base)
    # a complex field map
    np.save(os.path.join(tmp, "cplx.npy"), np.zeros(SCAN_DIMS, np.complex64).T)
    with pytest.raises(ValueError, match="the field map is complex"):
        _pics(oracle_backend, ["--fmap", os.path.join(tmp, "cplx.npy"), "--times", times] + base)
    # several frames, a basis, several sets of maps
    ksp, mps, trj = z['data'].T, z['maps'].T, z['traj'].T
    kw = dict(fmap=np.zeros(SCAN_DIMS, np.float32), times=SCAN_TIMES, osf=OSF, width=WIDTH)
    frames = np.stack([ksp, ksp], axis=-1).reshape(ksp.shape + (1,) * 6 + (2,))
    with pytest.raises(ValueError, match="--fmap cannot be combined with 2 time frames"):
        pics.reconstruct(oracle_backend, frames, mps, trj, **kw)
    with pytest.raises(ValueError, match="--fmap cannot be combined with --basis"):
        pics.reconstruct(oracle_backend, frames, mps, trj, basis=np.ones((2, 1)), **kw)
    two = np.concatenate([mps, mps], axis=4)
    with pytest.raises(ValueError, match="--fmap cannot be combined with M = 2 sets of maps"):
        pics.reconstruct(oracle_backend, ksp, two, trj, **kw)
    # more than 8 segments with --toeplitz, chosen automatically
    with pytest.raises(ValueError, match=r"--toeplitz: \d+ time segments, at most 8 are supported: the kernel array holds 4 K\^2 bytes"):
        pics.reconstruct(oracle_backend, ksp, mps, trj, toeplitz=True, fmap_tol=1e-6,
                         **dict(kw, fmap=fmap64.smooth_field(SCAN_DIMS, 250.0, seed=2)))
    oracle_backend._scratch = None


def test_a_run_without_a_field_map_builds_no_segment_operator(scans, oracle_backend, monkeypatch):
    (path, fmap, times), _ = scans

    def refuse(*args, **kwargs):
        raise AssertionError("a run without a field map constructs no segment operator")
    monkeypatch.setattr(type(oracle_backend), "SegmentPhase", refuse, raising=False)
    monkeypatch.setattr(type(oracle_backend), "SegmentCombine", refuse, raising=False)
    out = _pics(oracle_backend, ["-i", "1"] + COMMON + [path])
    assert out.shape == SCAN_DIMS + (1,)
    with pytest.raises(AssertionError, match="constructs no segment operator"):
        _pics(oracle_backend, ["-i", "1", "--fmap", fmap, "--times", times] + COMMON + [path])
