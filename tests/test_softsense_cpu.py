"""Soft-SENSE (several sets of coil maps) on the CPU with the numpy oracle backend: the host form of Backend.coil_maps against the
float64 restatement in tests/maps64.py, operators.CoilMaps against today's single-map stacks, the operator the driver builds for
two sets against the single-map trees, and the command line."""
import logging
import os

import numpy as np
import pytest

import maps64
from indigo_amd import pics
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
ALPHA, BETA = 0.7 - 0.3j, 0.5 + 0.25j
NAN = np.complex64(complex(np.nan, np.nan))


def _rel(a, b):
    return np.linalg.norm((np.asarray(a) - np.asarray(b)).ravel()) / np.linalg.norm(np.asarray(b).ravel())


def _col(a):
    return np.asfortranarray(np.asarray(a, dtype=C64).reshape((-1, 1), order='F'))


LAYOUTS = [(1, None), (3, None), (8, None), (2, 2), (3, 4), (5, 8)]          # (coils, width of an interleaved row or None)


@pytest.mark.parametrize("n", (1, 105, 2048))
@pytest.mark.parametrize("C,width", LAYOUTS, ids=lambda v: str(v))
def test_host_coil_maps_matches_the_float64_restatement(oracle_backend, n, C, width):
    B = oracle_backend
    il = width is not None
    worst = 0.0
    for M in (1, 2, 4):
        S = rand64c(n * C, M, seed=n + 10 * C + M).reshape((n, C, M), order='F')
        xi, yc = rand64c(n, M, seed=n + 1), rand64c(n, C, seed=n + 2)          # images, coil images
        for adjoint in (False, True):
            x, y = (yc, xi) if adjoint else (xi, yc)
            # the padding slots of x and S hold NaN in the adjoint, which must not read them
            S_d = B.copy_array(_col(maps64.planes(S, width, pad=NAN if adjoint else 0)))
            x_d = B.copy_array(_col(maps64.interleave(x, width, pad=NAN)) if (il and adjoint) else _col(x))
            for beta in (0, BETA):
                y0 = np.full_like(y, np.nan) if beta == 0 else y
                y_d = B.copy_array(_col(maps64.interleave(y0, width, pad=NAN)) if (il and not adjoint) else _col(y0))
                B.coil_maps(y_d, x_d, S_d, n, C, M, adjoint=adjoint, alpha=ALPHA, beta=beta, interleaved=il, width=width)
                got = y_d.to_host()
                if il and not adjoint:
                    got = got.reshape((n, width))
                    assert np.array_equal(got[:, C:], np.zeros((n, width - C), dtype=C64))          # forward: padding slots are zero
                    got = got[:, :C]
                else:
                    got = got.reshape(y.shape, order='F')
                err = _rel(got, maps64.apply(S, x, y, adjoint, ALPHA, beta))
                worst = max(worst, err)
                assert np.isfinite(got).all() and err < 1e-6, (M, adjoint, beta, err)
        # <A x, y> = <x, A^H y>
        Sd = B.copy_array(_col(maps64.planes(S, width)))
        ax = B.zero_array((n * (width or C), 1), C64)
        ahy = B.zero_array((n * M, 1), C64)
        B.coil_maps(ax, B.copy_array(_col(xi)), Sd, n, C, M, interleaved=il, width=width)
        B.coil_maps(ahy, B.copy_array(_col(maps64.interleave(yc, width)) if il else _col(yc)), Sd, n, C, M, adjoint=True, interleaved=il, width=width)
        axh = ax.to_host().reshape((n, width))[:, :C] if il else ax.to_host().reshape((n, C), order='F')
        lhs = np.vdot(yc.astype(np.complex128), axh.astype(np.complex128))
        rhs = np.vdot(ahy.to_host().reshape((n, M), order='F').astype(np.complex128), xi.astype(np.complex128))
        assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), np.linalg.norm(yc) * np.linalg.norm(axh)), (M, lhs, rhs)
    print("coil_maps host form n %d C %d width %s: worst relative error %.3e" % (n, C, width, worst))


def test_coil_maps_operator(oracle_backend):
    B = oracle_backend
    dims, C = (5, 7, 3), 3
    n = int(np.prod(dims))
    for M in (1, 2):
        maps = rand64c(n * C, M, seed=30 + M).reshape(dims + (C, M), order='F')
        S = B.CoilMaps(maps)
        assert S.shape == (n * C, n * M) and S.H.shape == (n * M, n * C)
        stacks = [B.VStack([B.Diag(np.ascontiguousarray(maps[..., c, m]).reshape(dims + (1,))) for c in range(C)]) for m in range(M)]
        ref = stacks[0] if M == 1 else B.HStack(stacks)
        x, y = rand64c(n * M, 1, seed=40), rand64c(n * C, 1, seed=41)
        assert _rel(S * x, ref * x) < 1e-6
        assert _rel(S.H * y, ref.H * y) < 1e-6
        # inside a Product, both directions
        d = rand64c(n * C, 1, seed=42)
        P = B.Diag(d) * S
        assert P.shape == (n * C, n * M)
        assert _rel(P * x, d * (ref * x)) < 1e-6
        assert _rel(P.H * y, ref.H * (np.conj(d) * y)) < 1e-6
    with pytest.raises(ValueError, match="5 sets"):
        B.CoilMaps(rand64c(n * C, 5, seed=1).reshape(dims + (C, 5), order='F'))


N16, NRO, NSP, OSF, WIDTH = (16, 16, 16), 32, 60, 2.0, 2


@pytest.fixture(scope="module")
def scan2(tmp_path_factory, oracle_backend):
    """16^3, 2 coils, 2 sets of maps; the arrays as the driver sees them"""
    oracle_backend._scratch = None
    path = maps64.softsense_scan(tmp_path_factory.mktemp("softsense"), oracle_backend, N16, 2, 2, NRO, NSP, OSF, WIDTH)
    z = np.load(path)
    return path, z['data'].T, z['maps'].T, z['traj'].T


def _single_map_trees(B, mps, traj):
    coord = traj / np.array(N16, dtype=np.float64)[:, None, None]
    return [maps64.single_map_operator(B, N16, mps.shape[3], mps[..., m], coord, NRO, NSP, OSF, WIDTH) for m in range(mps.shape[4])]


@pytest.mark.parametrize("level,fuse", [(0, False), (3, False), (3, True)], ids=["O0", "O3-no-fuse", "O3"])
def test_driver_operator_for_two_sets(scan2, oracle_backend, level, fuse):
    from indigo_amd.operators import CoilMaps, ZpadFFTMaps
    from indigo_amd.transforms import FuseZpadFFT, sense_recipe, soft_sense_tree
    B = oracle_backend
    path, ksp, mps, traj = scan2
    grid = tuple(int(n * OSF) for n in N16)
    if fuse and not B.supports_padded_fft(grid, 2):
        pytest.skip("the oracle does not take this grid")
    N = int(np.prod(N16))
    coord = traj / np.array(N16, dtype=np.float64)[:, None, None]
    recipe = sense_recipe(level) + ([FuseZpadFFT] if fuse else [])
    B._scratch = None
    A = soft_sense_tree(B, lambda: B.NUFFT((1, NRO, NSP), N16, coord, width=WIDTH, oversamp=(OSF,) * 3, dtype=C64), mps, recipe)
    assert A.shape == (2 * NRO * NSP, 2 * N)
    assert A.has(ZpadFFTMaps) == fuse and A.has(CoilMaps) == (not fuse)
    x, y = rand64c(2 * N, 1, seed=50), rand64c(2 * NRO * NSP, 1, seed=51)
    got_f, got_a = A * x, A.H * y
    B._scratch = None
    trees = _single_map_trees(B, mps, traj)
    want_f = sum(T * np.asfortranarray(x[m * N:(m + 1) * N]) for m, T in enumerate(trees))
    want_a = np.concatenate([T.H * y for T in trees], axis=0)
    B._scratch = None
    print("soft-SENSE tree -O%d fuse %s: forward %.3e adjoint %.3e" % (level, fuse, _rel(got_f, want_f), _rel(got_a, want_a)))
    assert _rel(got_f, want_f) < 1e-5 and _rel(got_a, want_a) < 1e-5


@pytest.mark.parametrize("extra", [["-O", "0"], ["-O", "3", "--no-fuse"], ["-O", "3"]], ids=["O0", "O3-no-fuse", "O3"])
def test_driver_cg_matches_cg_on_the_hstack_of_single_map_trees(scan2, oracle_backend, extra):
    # lamda: two sets of overlapping maps leave A^H A close to singular (what one set explains the other explains nearly as well), and
    # complex64 CG iterates of two realisations of the same operator then drift apart by about (condition number) x (their 1e-6
    # rounding difference) per iteration.  The bar is 1e-4 after ten iterations, so the comparison runs at a condition number of
    # about ten: lamda = 10 against a largest eigenvalue of A^H A of 87 (power iteration on this scan).  At lamda = 1e-3 the -O0 tree,
    # which shares every kernel with the comparison, already differs from it by 6e-4.
    B = oracle_backend
    path, ksp, mps, traj = scan2
    lamda, N = 10.0, int(np.prod(N16))
    B._scratch = None
    out = pics.main(extra + ["-i", "10", "--osf", str(OSF), "--width", str(WIDTH), "--lamda", str(lamda), "--debug", "40", path], backend=B)
    B._scratch = None
    assert out.shape == N16 + (1, 2)
    H = B.HStack(_single_map_trees(B, mps, traj))
    y = np.asfortranarray(ksp.astype(C64).reshape((-1, 1), order='F'))
    AHy = H.H * y
    AHy /= abs(AHy).max()
    x = np.zeros((2 * N, 1), dtype=C64, order='F')
    B.cg((H.H * H) + lamda * B.Eye(2 * N), AHy, x, maxiter=10)
    B._scratch = None
    err = _rel(out.reshape((-1, 1), order='F'), x)
    print("pics %s, 10 CG iterations against cg on the HStack: %.3e" % (extra, err))
    assert err < 1e-4


def _main(B, argv):
    B._scratch = None
    try:
        return pics.main(argv + ["--debug", "40"], backend=B)
    finally:
        B._scratch = None


COMMON = ["--osf", str(OSF), "--width", str(WIDTH), "--lamda", "1e-3"]


def test_cli_shapes_and_regularisers(scan2, oracle_backend, tmp_path):
    path = scan2[0]
    assert _main(oracle_backend, ["-i", "2"] + COMMON + [path]).shape == N16 + (1, 2)
    for reg in (["--l1", "0.01", "--levels", "2"], ["--tv", "0.01"], ["--llr", "0.02", "--llr-block", "8"]):
        out = _main(oracle_backend, ["-i", "2", "--power-iters", "3"] + reg + COMMON + [path])
        assert out.shape == N16 + (1, 2) and np.isfinite(out).all() and np.abs(out).max() > 0, reg
    path3 = maps64.softsense_scan(tmp_path, oracle_backend, N16, 2, 2, NRO, NSP, OSF, WIDTH, T=3, name="frames.npz")
    out = _main(oracle_backend, ["-i", "2"] + COMMON + [path3])
    assert out.shape == N16 + (1, 2, 1, 1, 1, 1, 1, 3) and np.isfinite(out).all()
    out = _main(oracle_backend, ["-i", "2", "--power-iters", "3", "--llr", "0.02"] + COMMON + [path3])
    assert out.shape == N16 + (1, 2, 1, 1, 1, 1, 1, 3) and np.isfinite(out).all()


def test_cli_crop_to_the_first_set_equals_the_first_set_file(scan2, oracle_backend, caplog):
    path = scan2[0]
    first = maps64.first_set_scan(path)
    a = _main(oracle_backend, ["-i", "3", "--crop", "MAPS:1"] + COMMON + [path])
    with caplog.at_level(logging.INFO, logger="pics"):
        oracle_backend._scratch = None
        b = pics.main(["-i", "3"] + COMMON + [first], backend=oracle_backend)
        oracle_backend._scratch = None
    assert a.shape == b.shape == N16 + (1,) and np.array_equal(a, b)          # (data without a MAPS axis: the image has none either)
    trees = [r.getMessage() for r in caplog.records if r.getMessage().startswith("tree:")]
    assert trees and all("CoilMaps" not in t and "ZpadFFTMaps" not in t for t in trees)


def test_cli_rejected_combinations(scan2, oracle_backend, tmp_path):
    path, ksp, mps, traj = scan2
    phi = os.path.join(str(tmp_path), "phi.npy")
    np.save(phi, np.eye(3, 2))
    path3 = maps64.softsense_scan(tmp_path, oracle_backend, N16, 2, 2, NRO, NSP, OSF, WIDTH, T=3, name="frames.npz")
    for option, argv in (("--tv-time", ["--tv-time", "0.01", path3]), ("--basis", ["--basis", phi, path3]), ("--toeplitz", ["--toeplitz", path])):
        with pytest.raises(ValueError, match=r"%s.*M = 2" % option):
            _main(oracle_backend, ["-i", "1"] + COMMON + argv)
    # the k-space is one measurement: a MAPS axis in data is refused
    bad = os.path.join(str(tmp_path), "bad.npz")
    z = np.load(path)
    d = z['data'].T
    np.savez(bad, data=np.concatenate([d.reshape(d.shape + (1,))] * 2, axis=4).T, maps=z['maps'], traj=z['traj'])
    with pytest.raises(ValueError, match="MAPS"):
        _main(oracle_backend, ["-i", "1"] + COMMON + [bad])
    # M T = 3 x 11 = 33 columns are beyond llr_threshold's 32
    with pytest.raises(ValueError, match=r"--llr.*33"):
        pics.reconstruct(oracle_backend, np.zeros((1, 4, 4, 2) + (1,) * 6 + (11,), dtype=C64), np.ones(N16 + (2, 3), dtype=C64),
                         np.zeros((3, 4, 4)), llr=0.1)
