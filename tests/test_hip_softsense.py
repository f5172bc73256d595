"""Soft-SENSE (several sets of coil maps) on the MI355X: ig_coil_maps_c64 against the float64 restatement in tests/maps64.py, the
fused leaf operators.ZpadFFTMaps inside the SENSE tree against today's single-map leaves, and the driver against the same driver
on the numpy oracle backend."""
import ctypes
import logging
import re

import numpy as np
import pytest

import maps64
from indigo_amd import pics
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
TOL = 1e-5          # the project's bar on the relative 2-norm; sums of at most 64 float32 products land near 1e-6
ALPHA, BETA = 0.7 - 0.3j, 0.5 + 0.25j
PAD = 37
NAN = np.complex64(complex(np.nan, np.nan))

NS = (1, 105, 2048, 5049)                       # one voxel; 5 * 7 * 3; whole workgroups; 33 * 17 * 9: several workgroups and a tail
# (coils, width of an interleaved row or None for coil-major)
COILS = [(1, None), (2, None), (3, None), (5, None), (8, None), (12, None), (33, None),
         (2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (12, 16)]
MS = (1, 2, 3, 4)

# every (coils, M) once with n rotating through its four values, every n with every layout, and the corners the rotation misses
CASES = [(NS[(i + j) % 4], C, w, M) for i, (C, w) in enumerate(COILS) for j, M in enumerate(MS)]
CASES += [c for c in [(5049, 33, None, 4), (5049, 12, 16, 4), (1, 12, 16, 4), (2048, 8, 8, 2), (5049, 3, 4, 3), (1, 1, None, 1), (2048, 5, 8, 4)]
          if c not in CASES]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _bits(a):
    """the bit patterns of a complex64 array (NaN payloads included), whatever its memory order"""
    return np.ascontiguousarray(a).view(np.uint32)


def _padded(hip, a, pad):
    """the panel a on the device with `pad` extra rows of NaN under every column, and the host copy"""
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _vec(hip, flat):
    return hip.copy_array(np.asfortranarray(np.asarray(flat, dtype=C64).reshape((-1, 1))))


def _run(hip, S, n, C, width, M, x, y, adjoint, alpha, beta, pad):
    """coil_maps on panels with `pad` NaN rows under every column (coil-major coil images and the images) or on a contiguous
    coil-interleaved array whose padding slots hold NaN.  Everything the call must not write -- the padding rows, the input, the
    padding slots of an adjoint's input -- must come back bit-identical; forward padding slots must be zero.  -> y as (n, cols)"""
    il = width is not None
    S_d = _vec(hip, maps64.planes(S, width, pad=NAN if adjoint else 0))
    img, coil = (y, x) if adjoint else (x, y)
    img_d, img_h = _padded(hip, img, pad)
    if il:
        coil_h = maps64.interleave(coil, width, pad=NAN).reshape((-1, 1))
        coil_d = _vec(hip, coil_h)
        coil_v = coil_d
    else:
        coil_d, coil_h = _padded(hip, coil, pad)
        coil_v = coil_d[:n]
    x_v, y_v = (coil_v, img_d[:n]) if adjoint else (img_d[:n], coil_v)
    hip.coil_maps(y_v, x_v, S_d, n, C, M, adjoint=adjoint, alpha=alpha, beta=beta, interleaved=il, width=width)
    if adjoint:
        out = img_d.to_host()
        assert np.array_equal(_bits(coil_d.to_host()), _bits(coil_h))           # x, its padding rows or slots included
        assert np.array_equal(_bits(out[n:]), _bits(img_h[n:]))
        return out[:n]
    assert np.array_equal(_bits(img_d.to_host()), _bits(img_h))
    out = coil_d.to_host()
    if il:
        out = out.reshape((n, width))
        assert np.array_equal(_bits(out[:, C:]), _bits(np.zeros((n, width - C), dtype=C64)))
        return out[:, :C]
    assert np.array_equal(_bits(out[n:]), _bits(coil_h[n:]))
    return out[:n]


WORST = {"err": 0.0}


@pytest.mark.parametrize("n,C,width,M", CASES, ids=lambda v: str(v))
def test_kernel_matches_the_float64_restatement(hip, n, C, width, M):
    S = rand64c(n * C, M, seed=C * 100 + M).reshape((n, C, M), order='F')
    for adjoint in (False, True):
        cols_x, cols_y = (C, M) if adjoint else (M, C)
        x, y = rand64c(n, cols_x, seed=n + 1), rand64c(n, cols_y, seed=n + 2)
        for beta, y0 in ((0, np.full_like(y, np.nan)), (BETA, y)):
            got = _run(hip, S, n, C, width, M, x, y0, adjoint, ALPHA, beta, PAD)
            err = _rel(got, maps64.apply(S, x, y, adjoint, ALPHA, beta))
            WORST["err"] = max(WORST["err"], err)
            assert np.isfinite(got).all() and err < TOL, (adjoint, beta, err)
    print("coil_maps n %d C %d width %s M %d: worst relative error so far %.3e" % (n, C, width, M, WORST["err"]))


@pytest.mark.parametrize("n,C,M", [(2048, 8, 2), (2048, 3, 4), (5049, 5, 3), (2048, 33, 1)], ids=lambda v: str(v))
def test_coil_major_forms_give_the_same_bits(hip, n, C, M):
    """the stacked vectors, the plain panels (both with 16-byte accesses when n is even) and panels with an odd leading
    dimension (8-byte accesses) hold the same bits"""
    S = rand64c(n * C, M, seed=3).reshape((n, C, M), order='F')
    S_d = _vec(hip, maps64.planes(S))
    for adjoint in (False, True):
        cols_x, cols_y = (C, M) if adjoint else (M, C)
        x, y = rand64c(n, cols_x, seed=4), rand64c(n, cols_y, seed=5)
        outs = [_run(hip, S, n, C, None, M, x, y, adjoint, ALPHA, BETA, pad) for pad in (PAD, 0, 2)]
        xs, ys = (hip.copy_array(np.asfortranarray(a.reshape((-1, 1), order='F'))) for a in (x, y))
        hip.coil_maps(ys, xs, S_d, n, C, M, adjoint=adjoint, alpha=ALPHA, beta=BETA)
        outs.append(ys.to_host().reshape((n, cols_y), order='F'))
        for o in outs[1:]:
            assert np.array_equal(_bits(o), _bits(outs[0]))


@pytest.mark.parametrize("n,C,width,M", [(2048, 8, 8, 2), (105, 3, 4, 3), (5049, 5, 8, 4), (2048, 12, 16, 1), (105, 2, 2, 2)], ids=lambda v: str(v))
def test_interleaved_forms_give_the_same_bits(hip, n, C, width, M):
    """16-byte aligned coil images and maps (two slots per lane) and ones that start 8 bytes off (one slot per lane), with the images
    as a stacked vector, a plain panel or a panel with an odd leading dimension, hold the same bits"""
    S = rand64c(n * C, M, seed=6).reshape((n, C, M), order='F')
    planes = maps64.planes(S, width, pad=NAN)
    for adjoint in (False, True):
        cols_x, cols_y = (C, M) if adjoint else (M, C)
        x, y = rand64c(n, cols_x, seed=7), rand64c(n, cols_y, seed=8)
        img, coil = (y, x) if adjoint else (x, y)
        outs = []
        for off, pad in ((0, 0), (1, 0), (0, 3), (1, PAD)):
            S_d = _vec(hip, np.concatenate([np.zeros(off, dtype=C64), planes]))
            coil_d = _vec(hip, np.concatenate([np.zeros(off, dtype=C64), maps64.interleave(coil, width, pad=NAN)]))
            img_d, _ = _padded(hip, img, pad)
            cv, sv, iv = coil_d[off:], S_d[off:], (img_d[:n] if pad else img_d.reshape((n * M, 1)))
            cv, sv = cv.dense_rows(0, n * width), sv.dense_rows(0, n * width * M)
            xv, yv = (cv, iv) if adjoint else (iv, cv)
            hip.coil_maps(yv, xv, sv, n, C, M, adjoint=adjoint, alpha=ALPHA, beta=BETA, interleaved=True, width=width)
            outs.append(img_d.to_host()[:n] if adjoint else coil_d.to_host()[off:].reshape((n, width))[:, :C])
        for o in outs[1:]:
            assert np.array_equal(_bits(o), _bits(outs[0]))


def test_adjointness_on_the_device(hip):
    n, M = 5049, 3
    for C, width in ((5, None), (5, 8), (12, 16)):
        il = width is not None
        S = rand64c(n * C, M, seed=9).reshape((n, C, M), order='F')
        S_d = _vec(hip, maps64.planes(S, width))
        x, y = rand64c(n, M, seed=10), rand64c(n, C, seed=11)
        ax, ahy = hip.zero_array((n * (width or C), 1), C64), hip.zero_array((n * M, 1), C64)
        hip.coil_maps(ax, _vec(hip, x.reshape(-1, order='F')), S_d, n, C, M, interleaved=il, width=width)
        y_flat = maps64.interleave(y, width) if il else y.reshape(-1, order='F')
        hip.coil_maps(ahy, _vec(hip, y_flat), S_d, n, C, M, adjoint=True, interleaved=il, width=width)
        axh = ax.to_host().reshape((n, width))[:, :C] if il else ax.to_host().reshape((n, C), order='F')
        lhs = np.vdot(y.astype(np.complex128), axh.astype(np.complex128))
        rhs = np.vdot(ahy.to_host().reshape((n, M), order='F').astype(np.complex128), x.astype(np.complex128))
        assert abs(lhs - rhs) < 1e-5 * abs(lhs), (C, width, lhs, rhs)


def test_limits(hip):
    n = 64
    x = hip.copy_array(rand64c(n * 5, 1, seed=1))
    y = hip.copy_array(rand64c(n * 16, 1, seed=2))
    S = hip.copy_array(rand64c(n * 16 * 5, 1, seed=3))
    before = y.to_host()
    with pytest.raises(RuntimeError, match="5 sets of maps"):
        hip.coil_maps(y.dense_rows(0, n * 3), x, S.dense_rows(0, n * 3 * 5), n, 3, 5)
    with pytest.raises(RuntimeError, match="strides"):
        hip.coil_maps(y.dense_rows(0, n * 3), x.dense_rows(0, n * 2), S.dense_rows(0, n * 3 * 2), n, 3, 2, interleaved=True, width=3)
    with pytest.raises(RuntimeError, match="5 coils in rows of width 4"):
        hip.coil_maps(y.dense_rows(0, n * 4), x.dense_rows(0, n * 2), S.dense_rows(0, n * 4 * 2), n, 5, 2, interleaved=True, width=4)
    assert np.array_equal(_bits(y.to_host()), _bits(before))
    # the limits themselves are served: four sets, rows of sixteen slots
    Sh = rand64c(n * 12, 4, seed=4).reshape((n, 12, 4), order='F')
    xh = rand64c(n, 4, seed=5)
    hip.coil_maps(y, _vec(hip, xh.reshape(-1, order='F')), _vec(hip, maps64.planes(Sh, 16)), n, 12, 4, interleaved=True, width=16)
    assert _rel(y.to_host().reshape((n, 16))[:, :12], maps64.forward(Sh, xh)) < TOL


def test_overlapping_arrays_raise(hip):
    n, C, M = 64, 2, 2
    # elements: y (the coil images, 128) may start anywhere; x = [192, 320); maps = [400, 656)
    host = rand64c(800, 1, seed=9)
    buf = hip.copy_array(host)

    def at(y_off):
        return hip._L.ig_coil_maps_c64(hip._ctx, n, C, M, ctypes.c_void_p(buf._arr + 8 * 400), 0, ctypes.c_void_p(buf._arr + 8 * 192),
                                       1.0, 0.0, 0.0, 0.0, ctypes.c_void_p(buf._arr + 8 * y_off), n, 1, n)
    for off in (65, 319, 200, 330, 655):         # x's first element, its last, inside it; the maps' first element, their last
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(at(off), "ig_coil_maps_c64")
    assert np.array_equal(buf.to_host(), host)
    hip._check(at(64), "ig_coil_maps_c64")                                # adjacent to x, not overlapping
    after = buf.to_host()
    assert np.array_equal(after[:64], host[:64]) and np.array_equal(after[192:], host[192:])
    S = np.stack([host[400 + 128 * m:528 + 128 * m, 0].reshape((n, C), order='F') for m in range(M)], axis=2)
    want = maps64.forward(S, host[192:320, 0].reshape((n, M), order='F'))
    assert _rel(after[64:192, 0].reshape((n, C), order='F'), want) < TOL


# ---- ZpadFFTMaps inside the SENSE tree ----------------------------------------------------------------------------------------

N64, OSF, WIDTH = (64, 64, 64), 2.0, 2


@pytest.fixture(scope="module")
def problem(hip):
    from indigo_amd.sense import SenseProblem, radial_trajectory
    grid = tuple(int(n * OSF) for n in N64)
    assert hip.supports_padded_fft(grid), "128^3 is the smallest grid the fused leaf takes"
    coord = radial_trajectory(300, 128, seed=5)
    return SenseProblem(N64, coord, np.ones(N64 + (1,), dtype=C64), width=WIDTH, oversamp=OSF)


LEAF_CASES = [(C, M, True) for C in (2, 3, 8) for M in (2, 3)] + [(2, 2, False), (3, 3, False), (8, 2, False)]


@pytest.mark.parametrize("C,M,support", LEAF_CASES, ids=lambda v: str(v))
def test_fused_leaf_matches_the_single_map_leaves(hip, problem, C, M, support):
    """A x = sum_m A_m x_m and A^H y = (A_m^H y)_m, A_m = build_zpadfft on maps[..., m] with the problem's cached gridding matrix:
    an exact chunk (2, 8), a chunk padded with a zero coil (3); compared in k-space and image space only"""
    from indigo_amd.operators import UnscaledFFT, ZpadFFT, ZpadFFTMaps
    from indigo_amd.sense import SenseProblem
    from indigo_amd.transforms import reserve_for
    N = int(np.prod(N64))
    maps = rand64c(N * C, M, seed=60 + C).reshape(N64 + (C, M), order='F')
    A = problem.build_zpadfft_maps(hip, maps, support=support)
    assert A.has(ZpadFFTMaps) and not A.has(UnscaledFFT) and A.shape == (C * problem.T, N * M)
    singles = []
    for m in range(M):
        q = SenseProblem(N64, problem.coord, np.asfortranarray(maps[..., m]), width=WIDTH, oversamp=OSF)
        q._interp_cache = problem._interp_cache
        singles.append(q.build_zpadfft(hip, support=support))
        assert singles[-1].has(ZpadFFT) and not singles[-1].has(ZpadFFTMaps)
    x, y = rand64c(N * M, 1, seed=70), rand64c(C * problem.T, 1, seed=71)
    x_d, y_d = hip.copy_array(x), hip.copy_array(y)
    # forward, alpha != 1 (beta == 0 is ZpadFFT's contract)
    hip._scratch = None
    reserve_for(A, 1)
    out = hip.zero_array((A.shape[0], 1), C64)
    A.eval(out, x_d, alpha=ALPHA)
    got_f = out.to_host()
    out0 = hip.copy_array(y)
    A.eval(out0, x_d.dense_rows(0, N * M), alpha=1, beta=0)
    # adjoint with alpha != 1 and beta != 0 on a prefilled image
    z0 = rand64c(N * M, 1, seed=72)
    img = hip.copy_array(z0)
    A.eval(img, y_d, alpha=ALPHA, beta=BETA, forward=False)
    got_a = img.to_host()
    img1 = hip.copy_array(np.full((N * M, 1), np.nan, dtype=C64))
    A.eval(img1, y_d, forward=False)
    got_a1 = img1.to_host()
    hip._scratch = None
    want_f = np.zeros((C * problem.T, 1), dtype=np.complex128)
    want_a = []
    for m, Am in enumerate(singles):
        reserve_for(Am, 1)
        want_f += (Am * np.asfortranarray(x[m * N:(m + 1) * N])).astype(np.complex128)
        want_a.append((Am.H * y).astype(np.complex128))
        hip._scratch = None
    want_a = np.concatenate(want_a, axis=0)
    errs = (_rel(got_f, ALPHA * want_f), _rel(out0.to_host(), want_f), _rel(got_a, ALPHA * want_a + BETA * z0), _rel(got_a1, want_a))
    print("ZpadFFTMaps C %d M %d support %s: forward %.3e %.3e adjoint %.3e %.3e" % ((C, M, support) + errs))
    assert np.isfinite(got_a1).all() and max(errs) < TOL, errs


# ---- the driver -------------------------------------------------------------------------------------------------------------------

def _largest_eigenvalue(backend, argv):
    """the power-iteration estimate that a FISTA run of the driver logs (no iterations of the solver itself)"""
    records = []

    class Keep(logging.Handler):
        def emit(self, record):
            records.append(record.getMessage())
    keep = Keep(level=logging.INFO)
    plog = logging.getLogger("pics")
    old = plog.level
    plog.addHandler(keep)
    plog.setLevel(logging.INFO)
    try:
        pics.main(["-i", "0", "--power-iters", "6", "--llr", "0.01", "--debug", "40"] + argv, backend=backend)
    finally:
        plog.removeHandler(keep)
        plog.setLevel(old)
    backend._scratch = None
    trees = [s for s in records if s.startswith("tree:")]
    est = [float(m.group(1)) for s in records for m in [re.search(r"largest eigenvalue of A\^H A \+ lamda I (\S+)", s)] if m][0]
    return est, trees


# image, coils, sets, spokes x readout, driver options, whether the oracle gives the eigenvalue (the small case), solvers,
# the leaf the dumped tree must name
DRIVER_CASES = {
    "a-coilmaps-32": ((32, 32, 32), 2, 2, (100, 64), ["--osf", "2.0", "--width", "2"], True,
                      [[], ["--l1", "0.01"], ["--tv", "0.01"], ["--llr", "0.02", "--llr-block", "8"]], "CoilMaps"),
    "b-fused-64": ((64, 64, 64), 3, 2, (150, 128), ["--osf", "2.0", "--width", "2"], False, [[], ["--l1", "0.01"]], "ZpadFFTMaps"),
    "c-chirpz-default-osf": ((120, 52, 77), 2, 2, (150, 120), [], False, [[]], "ZpadFFTMaps"),
    "d-permuted-grid": ((52, 96, 96), 2, 2, (150, 96), ["--width", "2"], False, [[]], "CoilMaps"),
}


@pytest.mark.parametrize("case", sorted(DRIVER_CASES))
def test_pics_softsense_on_the_gpu_matches_the_oracle_backend(case, tmp_path, hip, oracle_backend, caplog):
    """Regularisation: two overlapping sets of maps leave A^H A close to singular, and complex64 iterates of two realisations of the
    same operator drift apart by about (condition number) x (their 1e-6 rounding difference) per iteration; with the project's
    bars of 1e-5 after one iteration and 1e-4 after ten, the comparison runs at lamda = a tenth of the largest eigenvalue of
    A^H A (a power iteration at lamda = 0: on the oracle for the small case, whose proximal solvers take their step from it,
    on the GPU otherwise), i.e. a condition number of eleven."""
    N, C, M, (nsp, nro), opts, oracle_power, solvers, leaf = DRIVER_CASES[case]
    from indigo_amd import fused
    osf = float(opts[opts.index("--osf") + 1]) if "--osf" in opts else 640 / 480
    width = int(opts[opts.index("--width") + 1]) if "--width" in opts else 3
    grid = tuple(int(n * osf) for n in N)
    if case.startswith("d"):
        assert not hip.supports_padded_fft(grid, C) and fused.image_permutation(hip, grid, C) is not None, grid
    oracle_backend._scratch = None
    path = maps64.softsense_scan(tmp_path, oracle_backend, N, C, M, nro, nsp, osf, width)
    L, trees = _largest_eigenvalue(oracle_backend if oracle_power else hip, (["--no-fuse"] if oracle_power else []) + opts + ["--lamda", "0", path])
    args = opts + ["--lamda", "%.8e" % (L / 10), path]
    step = ["--step", "%.8e" % (0.9 / (1.1 * L))]
    with caplog.at_level(logging.INFO, logger="pics"):
        for extra in solvers:
            for iters, tol in (("1", 1e-5), ("10", 1e-4)):
                argv = extra + ["-i", iters] + (step if extra else []) + args
                hip._scratch = None
                out = pics.main(argv, backend=hip)
                hip._scratch = None
                with caplog.at_level(logging.WARNING, logger="pics"):
                    ref = pics.main(["--no-fuse", "--debug", "40"] + argv, backend=oracle_backend)
                oracle_backend._scratch = None
                assert out.shape == N + (1, M)
                print("pics soft-SENSE %s %s, %s iterations: relative difference %.3e" % (case, extra, iters, _rel(out, ref)))
                assert _rel(out, ref) < tol, (case, extra, iters, _rel(out, ref))
    dumps = [r.getMessage() for r in caplog.records if r.getMessage().startswith("tree:")]
    assert dumps and all(leaf in d for d in dumps), dumps[:1]
    if leaf == "ZpadFFTMaps":
        assert all("UnscaledFFT" not in d and "CoilMaps," not in d for d in dumps)
    assert not any("scratch arena too small" in r.getMessage() for r in caplog.records)
