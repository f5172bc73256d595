"""Density compensation on the numpy oracle backend: the Backend host forms of the Pipe-Menon halves and of
row_scale against the independent restatement tests/dcf64.py, the tile binning, operators.SampleWeights, the dcf driver and
pics --dcf -- including the claim the feature rests on: after two CG iterations the weighted image is closer than the plain one."""
import logging
import os

import numpy as np
import pytest
from scipy.signal.windows import kaiser

import dcf64
from test_toeplitz_cpu import accuracy            # noqa: F401  (the fixture: e_grid, the bar of the --toeplitz comparison)
from indigo_amd import dcf, pics
from indigo_amd.backends.backend import Backend
from indigo_amd.grid_formats import DCF_TILE, dcf_tiles
from indigo_amd.interp import interp_sep_records
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
F32 = np.dtype('float32')


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def ulps(a, b):
    """distance of two non-negative float32 arrays in units in the last place"""
    return np.abs(np.asarray(a, dtype=F32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=F32).view(np.int32).astype(np.int64))


def records(grid, width, coord):
    """separable records of plain positive taps for the samples `coord` (3, M) on `grid`"""
    beta = Backend.nufft_params(width, 1.5)[1]
    sep = interp_sep_records(coord.shape[1], grid, width, kaiser(2 * 128 + 1, beta)[128:], coord)
    assert sep is not None and sep['gconst'] == 1
    return sep


def mixed_coords(M, seed=0):
    """radial samples with a dense centre, uniform ones that wrap on every axis, and 300 copies of one point (fewer for a small M)"""
    rng = np.random.default_rng(seed)
    rad = radial_trajectory(max(M // 32, 1), 16).reshape(3, -1)
    uni = rng.random((3, max(M, 4))) - 0.5
    uni[:, :4] = [[-0.5, 0.499, -0.5, 0.499], [-0.5, -0.5, 0.499, 0.499], [0.499, -0.5, 0.499, -0.5]]
    same = np.repeat(np.array([[0.123], [-0.321], [0.251]]), min(300, M // 3), axis=1)
    return np.ascontiguousarray(np.concatenate([same, rad, uni], axis=1)[:, :M])


def some_weights(M, seed=1):
    w = (np.random.default_rng(seed).random(M) * 2).astype(np.float32)
    w[::7] = 0
    return w


def iterate_weights(sep, seed=1):
    """Weights as the divide meets them in use: three float64 Pipe-Menon iterations, times a factor in [0.5, 1.5), some set to 0.
    Then s = G G^H w stays below 16, where a float32 -- the type of the device's max |s - 1| -- resolves the 1e-6 that the
    comparison of that maximum asks for (300 coincident samples of weight one alone put s near 500, half an ulp at 1.5e-5)."""
    M = sep['records'].shape[0]
    w = (dcf64.pipe_menon(sep, 3, normalise=False) * (0.5 + np.random.default_rng(seed).random(M))).astype(np.float32)
    w[3::7] = 0
    return w


@pytest.mark.parametrize("width,tw", [(2, 4), (3, 6), (4, 8)])
def test_host_forms_match_the_restatement(oracle_backend, width, tw):
    B = oracle_backend
    grid, M = (24, 20, 18), 1000
    sep = records(grid, width, mixed_coords(M))
    assert sep['tw'] == tw
    w = iterate_weights(sep)
    scale = dcf.scale_for(M, float(w.max()))
    rec_d, desc, tiles = dcf.upload(B, sep, stride=sep['records'].shape[1] + 8)
    acc_d = B.copy_array(np.full(int(np.prod(grid)), -7, dtype=np.int64))
    w_d = B.copy_array(w)
    B.dcf_spread(acc_d, w_d, rec_d, desc, scale, tiles)
    want = dcf64.spread(sep, w, scale)
    np.testing.assert_array_equal(acc_d.to_host(), want)                 # bits
    assert want.max() > 2 ** 40                                           # (the fixed point is used, not a few integer steps)
    q, s = dcf64.gather_div(sep, want, w, scale)
    out_d, s_d = B.copy_array(np.full(M, np.nan, dtype=np.float32)), B.copy_array(np.full(M, np.nan, dtype=np.float32))
    wmax, dev = B.dcf_gather_div(out_d, acc_d, w_d, rec_d, desc, scale, tiles, s_out=s_d)
    got = out_d.to_host()
    assert ulps(got, q).max() <= 1 and np.all(got[w == 0] == 0)
    assert ulps(s_d.to_host(), s.astype(np.float32)).max() <= 1
    assert np.abs(s - 1).max() < 16
    assert np.float32(wmax) == q.max() and abs(dev - np.abs(s - 1).max()) < 1e-6
    B.dcf_gather_div(w_d, acc_d, w_d, rec_d, desc, scale, tiles)         # in place
    np.testing.assert_array_equal(w_d.to_host(), got)


def test_spread_of_zero_weights_and_the_scale(oracle_backend):
    B = oracle_backend
    grid, M = (16, 16, 16), 65
    sep = records(grid, 3, mixed_coords(M))
    rec_d, desc, tiles = dcf.upload(B, sep)
    acc_d = B.copy_array(np.ones(16 ** 3, dtype=np.int64))
    w_d = B.copy_array(np.zeros(M, dtype=np.float32))
    B.dcf_spread(acc_d, w_d, rec_d, desc, 2.0 ** 40, tiles)
    assert not acc_d.to_host().any()
    out_d = B.copy_array(np.ones(M, dtype=np.float32))
    assert B.dcf_gather_div(out_d, acc_d, w_d, rec_d, desc, 2.0 ** 40, tiles) == (0.0, 1.0)     # s == 0 everywhere: w_out = 0
    assert not out_d.to_host().any()
    with pytest.raises(RuntimeError, match="power of two"):
        B.dcf_spread(acc_d, w_d, rec_d, desc, 3.0, tiles)
    for M_, wmax in ((1, 1.0), (4097, 3.7), (1 << 24, 1e-3), (1 << 24, 5e4)):
        sc = dcf.scale_for(M_, wmax)
        assert np.frexp(sc)[0] == 0.5 and M_ * wmax * sc <= 2.0 ** 62 < 2 * M_ * wmax * sc


@pytest.mark.parametrize("grid", [(24, 20, 18), (16, 16, 16)])
@pytest.mark.parametrize("width", [2, 3, 4])
def test_tiles_are_a_partition_by_first_tap(grid, width):
    M = 4097
    sep = records(grid, width, mixed_coords(M, seed=3))
    tw, rec = sep['tw'], sep['records']
    t = dcf_tiles(rec, tw, grid)
    order, ptr, ids = t['order'], t['ptr'], t['ids']
    assert order.dtype == np.uint32 and ptr.dtype == np.int64 and ids.dtype == np.int32
    np.testing.assert_array_equal(np.sort(order), np.arange(M))           # a permutation
    assert ptr[0] == 0 and ptr[-1] == M and np.all(np.diff(ptr) > 0) and ptr.size == ids.size + 1      # every sample once, no empty tile
    assert np.all(np.diff(ids) > 0)
    j = np.stack([rec[:, 3 * tw] & 0xffff, rec[:, 3 * tw] >> 16, rec[:, 3 * tw + 1] & 0xffff], axis=1).astype(np.int64)
    assert np.all(j < np.array(grid))                                      # first taps are wrapped
    nt = [-(-n // b) for n, b in zip(grid, DCF_TILE)]
    for k, tile in enumerate(ids):
        o = np.array([tile % nt[0], (tile // nt[0]) % nt[1], tile // (nt[0] * nt[1])]) * np.array(DCF_TILE)
        mine = j[order[ptr[k]:ptr[k + 1]]]
        assert np.all(mine >= o) and np.all(mine < o + np.array(DCF_TILE)), (k, tile)
        assert np.all(np.diff(order[ptr[k]:ptr[k + 1]].astype(np.int64)) > 0)                           # trajectory order inside a tile


@pytest.mark.parametrize("ncols", [1, 3, 8, 12])
def test_row_scale_host_form_is_exact(oracle_backend, ncols):
    B = oracle_backend
    n, ld = 65, 70
    w = some_weights(n, seed=ncols)
    x = rand64c(ld, ncols, seed=2)
    want = (w[:, None] * x[:n].real) + 1j * (w[:, None] * x[:n].imag)
    x_d, y_d = B.copy_array(x), B.copy_array(np.full((ld, ncols), np.nan + 0j, dtype=C64))
    w_d = B.copy_array(w)
    B.row_scale(y_d[:n, :], x_d[:n, :], w_d, n, ncols)                   # padded panels
    got = y_d.to_host()
    np.testing.assert_array_equal(got[:n], want.astype(C64))
    assert np.isnan(got[n:]).all()
    xs_d = B.copy_array(np.asfortranarray(x[:n].reshape((-1, 1), order='F')))         # the stacked form, in place
    B.row_scale(xs_d, xs_d, w_d, n, ncols)
    np.testing.assert_array_equal(xs_d.to_host().reshape((n, ncols), order='F'), want.astype(C64))


def test_sample_weights_operator(oracle_backend):
    B = oracle_backend
    B._scratch = None
    n, C = 40, 3
    w = some_weights(n) + 0.5
    W = B.SampleWeights(w, n, C)
    assert W.shape == (n * C, n * C) and W.dtype == C64
    x = rand64c(n * C, 2, seed=1)
    want = np.tile(w, C)[:, None] * x
    assert _rel(W * x, want) < 1e-7 and _rel(W.H * x, want) < 1e-7         # real and diagonal: self-adjoint
    y = rand64c(n * C, 2, seed=2)
    y_d = B.copy_array(y)
    W.eval(y_d, B.copy_array(x), alpha=0.5 - 1j, beta=2.0)
    assert _rel(y_d.to_host(), (0.5 - 1j) * want + 2.0 * y) < 1e-6
    A = W * B.Eye(n * C)
    assert "sample weights" in A.dump() and A.memusage() >= 4 * n
    from indigo_amd.analyses import ScratchUsage
    assert ScratchUsage().measure(A, 1) >= n * C
    for bad, msg in ((np.ones(n + 1), "weights for n"), (np.ones(n) * 1j, "real array"), (np.full(n, np.inf), "finite")):
        with pytest.raises(ValueError, match=msg):
            B.SampleWeights(bad, n, C)
    B._scratch = None


# ---- the drivers -----------------------------------------------------------------------------------------------------------------

N, C, NRO, NSP = (12, 10, 8), 3, 24, 80
OSF, WIDTH = 1.5, 3


def _pics(B, argv):
    B._scratch = None
    out = pics.main(["--debug", "40"] + argv, backend=B)
    B._scratch = None
    return out


def _sense(B, coord, mps, osf=OSF, width=WIDTH):
    F1 = B.NUFFT((1,) + coord.shape[1:], mps.shape[:3], coord, width=width, oversamp=(osf,) * 3, dtype=C64)
    return B.KronI(mps.shape[3], F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(mps.shape[3])])


@pytest.fixture(scope="module")
def scan(tmp_path_factory, oracle_backend):
    """the scan of test_pics_cli.py, with 1 % noise; (path, directory, coord, maps, k-space vector)"""
    B = oracle_backend
    B._scratch = None
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    img = (np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + g[2] ** 2)) * (1 + 0.3j)).astype(C64)
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph)
                    for cx, cy, ph in [(-1, 0, 0.3), (1, 0.5, -0.4), (0, -1, 1.0)]], axis=3).astype(C64)
    coord = radial_trajectory(NSP, NRO, seed=2)
    y = _sense(B, coord, mps) * np.asfortranarray(img.reshape(-1, 1, order='F'))
    rng = np.random.default_rng(0)
    y = (y + 0.01 * np.abs(y).max() * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))).astype(C64)
    B._scratch = None
    tmp = str(tmp_path_factory.mktemp("dcf"))
    path = os.path.join(tmp, "scan.npz")
    traj = coord * np.array(N, dtype=np.float64)[:, None, None]
    ksp = y.reshape((1, NRO, NSP, C), order='F')
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path, tmp, coord, mps, y


@pytest.fixture(scope="module")
def weights(scan, oracle_backend):
    """python -m indigo_amd.dcf on the scan: the file it writes"""
    path = scan[0]
    w = dcf.main(["--osf", str(OSF), "--width", str(WIDTH), "--debug", "40", path], backend=oracle_backend)
    return os.path.splitext(path)[0] + ".dcf.npy", w


def test_dcf_driver_writes_the_documented_file(scan, weights, oracle_backend):
    path, tmp, coord, mps, y = scan
    file, w = weights
    stored = np.load(file)
    assert stored.dtype == np.float32 and stored.shape == (NSP, NRO) and w.shape == (NRO, NSP)      # traj's axes without the coordinate axis, reversed
    np.testing.assert_array_equal(stored, w.T)
    assert abs(float(stored.astype(np.float64).mean()) - 1) < 1e-6 and stored.min() > 0
    # the weights of the run's own NUFFT: kernel and grid of Backend.NUFFT(width, osf); float32 device rounding against float64
    beta = Backend.nufft_params(WIDTH, (OSF,) * 3)[1]
    sep = interp_sep_records(NRO * NSP, tuple(int(n * OSF) for n in N), WIDTH, kaiser(257, beta)[128:], coord.reshape((3, -1), order='F'))
    want = dcf64.pipe_menon(sep, 30).reshape((NRO, NSP), order='F')
    assert np.abs(w / want - 1).max() < 1e-4
    # dense centre, sparse periphery: the weights grow along the readout away from the centre
    assert w[NRO // 2].mean() < 0.1 * w[0].mean()
    # --dims in place of the maps, and fewer iterations
    bare = os.path.join(tmp, "bare.npz")                                   # (its own name: the driver writes next to its input)
    np.savez(bare, traj=np.load(path)['traj'])
    w5 = dcf.main(["-i", "5", "--dims", "12:10:8", "--osf", str(OSF), "--debug", "40", bare], backend=oracle_backend)
    assert np.load(os.path.join(tmp, "bare.dcf.npy")).shape == (NSP, NRO)
    assert np.abs(w5 / dcf64.pipe_menon(sep, 5).reshape((NRO, NSP), order='F') - 1).max() < 1e-4


def test_frames_with_one_trajectory_share_their_weights(scan, oracle_backend, monkeypatch, tmp_path):
    path, tmp, coord, mps, y = scan
    other = radial_trajectory(NSP, NRO, seed=5)
    frames = np.stack([coord, other, coord], axis=-1).reshape((3, NRO, NSP) + (1,) * 7 + (3,)) * np.array(N, dtype=np.float64).reshape((3,) + (1,) * 10)
    fpath = str(tmp_path / "frames.npz")
    np.savez(fpath, traj=frames.T, maps=mps.reshape(mps.shape + (1,)).T)
    calls = []
    real = dcf.pipe_menon
    monkeypatch.setattr(dcf, "pipe_menon", lambda *a, **k: calls.append(1) or real(*a, **k))
    w = dcf.main(["-i", "4", "--osf", str(OSF), "--debug", "40", fpath], backend=oracle_backend)
    assert len(calls) == 2                                                  # two distinct trajectories among three frames
    assert w.shape == (NRO, NSP) + (1,) * 7 + (3,) and np.load(str(tmp_path / "frames.dcf.npy")).shape == w.T.shape
    np.testing.assert_array_equal(w[..., 0], w[..., 2])
    assert np.abs(w[..., 0] - w[..., 1]).max() > 1e-3


def test_unsupported_kernels_are_refused(oracle_backend):
    coord = radial_trajectory(4, 8)
    with pytest.raises(ValueError, match="no separable gridding records"):
        dcf.pipe_menon(oracle_backend, coord, (16, 16, 16), width=5, osf=1.5, iters=1)       # wider than 8 taps
    with pytest.raises(ValueError, match="no separable gridding records"):
        dcf.pipe_menon(oracle_backend, coord, (3, 16, 16), width=3, osf=1.5, iters=1)        # an axis of 4 cells for 6 taps


def test_pics_dcf_from_a_file_auto_and_the_scan(scan, weights, oracle_backend):
    path, tmp, coord, mps, y = scan
    file, w = weights
    args = ["-i", "4", "--osf", str(OSF), "--lamda", "1e-4"]
    from_file = _pics(oracle_backend, args + ["--dcf", file, path])
    auto = _pics(oracle_backend, args + ["--dcf", "auto", path])
    z = dict(np.load(path))
    inside = os.path.join(tmp, "with_dcf.npz")
    np.savez(inside, dcf=np.load(file), **z)
    from_scan = _pics(oracle_backend, args + [inside])
    assert from_file.shape == N + (1, 1)
    np.testing.assert_array_equal(auto, from_file)
    np.testing.assert_array_equal(from_scan, from_file)
    # ... and it is the weighted problem: float64 CG on A^H W A x = A^H W y
    oracle_backend._scratch = None
    want = dcf64.weighted_cg(_sense(oracle_backend, coord, mps), y, w, 4, lamda=1e-4, ncoils=C).reshape(N + (1, 1), order='F')
    oracle_backend._scratch = None
    err = _rel(from_file, want)
    print("pics --dcf against the float64 weighted CG: %.3e" % err)
    assert err < 2e-3, err                                                  # (the tolerance of test_pics_cli.py for plain CG)
    plain = _pics(oracle_backend, args + [path])
    assert _rel(from_file, plain) > 0.05                                    # not the unweighted problem
    # fewer Pipe-Menon iterations are other weights
    assert _rel(_pics(oracle_backend, args + ["--dcf", "auto", "--dcf-iters", "2", path]), from_file) > 1e-3


def test_pics_with_weights_of_one_is_the_plain_run(scan, oracle_backend):
    path, tmp, coord, mps, y = scan
    ones = os.path.join(tmp, "ones.npy")
    np.save(ones, np.ones((NSP, NRO), dtype=np.float32))
    args = ["-i", "6", "--osf", str(OSF), "--lamda", "1e-4"]
    assert _rel(_pics(oracle_backend, args + ["--dcf", ones, path]), _pics(oracle_backend, args + [path])) < 2e-3


@pytest.mark.parametrize("extra", [["--l1", "0.01", "--levels", "2"], ["--tv", "0.01"]], ids=["l1", "tv"])
def test_regularised_solvers_run_on_the_weighted_problem(scan, weights, oracle_backend, caplog, extra):
    path = scan[0]
    with caplog.at_level(logging.INFO):
        oracle_backend._scratch = None
        out = pics.main(["-i", "12", "--osf", str(OSF), "--power-iters", "6", "--dcf", weights[0], path] + extra, backend=oracle_backend)
        oracle_backend._scratch = None
    msgs = [r.getMessage() for r in caplog.records]
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    assert not any("scratch arena too small" in m for m in msgs), msgs
    assert any("sqrt dcf" in m for m in msgs), msgs                        # the tree that was logged holds the weights


def test_pics_dcf_with_toeplitz(scan, weights, oracle_backend, accuracy):     # noqa: F811
    """the weighted Toeplitz form against the weighted gridding form, at the half-width and oversampling of test_toeplitz_cpu.py
    and with its bar: 10 x the operator-level e_grid; each result divided by its own 2-norm"""
    path = scan[0]
    file = os.path.join(scan[1], "scan_osf2.dcf.npy")
    w = dcf.main(["--osf", "2.0", "--width", "3", "--debug", "40", path], backend=oracle_backend)
    np.save(file, w.T)
    args = ["-i", "3", "--osf", "2.0", "--width", "3", "--lamda", "1e-3", "--dcf", file, path]
    grid = _pics(oracle_backend, args)
    toep = _pics(oracle_backend, ["--toeplitz"] + args)
    err = _rel(toep / np.linalg.norm(toep), grid / np.linalg.norm(grid))
    print("pics --dcf --toeplitz against --dcf: relative difference %.3e, bar %.3e" % (err, 10 * accuracy[0]))
    assert err < 10 * accuracy[0], (err, accuracy)
    unweighted = _pics(oracle_backend, ["--toeplitz"] + args[:-3] + [path])
    assert _rel(unweighted / np.linalg.norm(unweighted), toep / np.linalg.norm(toep)) > 0.05


def test_bad_weights_are_refused(scan, oracle_backend):
    path, tmp = scan[0], scan[1]

    def run(w):
        f = os.path.join(tmp, "bad.npy")
        np.save(f, w)
        return _pics(oracle_backend, ["-i", "1", "--osf", str(OSF), "--dcf", f, path])
    good = np.ones((NSP, NRO), dtype=np.float32)
    with pytest.raises(ValueError, match="the weights have shape"):
        run(good[:, :-1])
    with pytest.raises(ValueError, match="the weights have shape"):
        run(good.T)
    neg = good.copy()
    neg[3, 4] = -1e-3
    with pytest.raises(ValueError, match="1 of 1920 weights are negative"):
        run(neg)
    nan = good.copy()
    nan[0, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        run(nan)
    inf = good.copy()
    inf[5, 5] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        run(inf)
    with pytest.raises(ValueError, match="all weights are zero"):
        run(np.zeros_like(good))
    with pytest.raises(ValueError, match="real array"):
        run(good.astype(np.complex64))
    assert pics.parse([path]).dcf is None and pics.parse(["--dcf", "auto", path]).dcf_iters == 30


def test_two_weighted_iterations_beat_two_plain_ones(oracle_backend, tmp_path):
    """The claim the feature rests on.  16^3 image, radial_trajectory(300, 32) (seed 3), half-width 3, oversampling 640/480, 1 %
    noise, one coil of ones.  The float64 restatement alone gives 0.338 (weighted) against 0.416 (plain) after two iterations;
    here both come from the driver, each image scaled to the phantom by least squares (pics normalises its right-hand side)."""
    B = oracle_backend
    B._scratch = None
    n, nro, nsp = (16, 16, 16), 32, 300
    coord = radial_trajectory(nsp, nro, seed=3)
    g = np.indices(n).astype(float) - 8
    x0 = ((g ** 2).sum(0) < 36).astype(float) + 0.5 * (((g[0] - 2) ** 2 + (g[1] + 1) ** 2 + g[2] ** 2) < 9)
    x0 = (x0 * np.exp(1j * 0.3 * g[0] / 8)).astype(C64)
    mps = np.ones(n + (1,), dtype=C64)
    y = _sense(B, coord, mps, osf=640 / 480) * np.asfortranarray(x0.reshape(-1, 1, order='F'))
    rng = np.random.default_rng(0)
    y = (y + 0.01 * np.abs(y).max() * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))).astype(C64)
    path = str(tmp_path / "claim.npz")
    ksp = y.reshape((1, nro, nsp, 1), order='F')
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T,
             traj=(coord * 16.0).T)

    def error(argv):
        x = _pics(B, ["-i", "2"] + argv + [path]).reshape(-1, order='F').astype(np.complex128)
        t = x0.reshape(-1, order='F').astype(np.complex128)
        return np.linalg.norm(np.vdot(x, t) / np.vdot(x, x) * x - t) / np.linalg.norm(t)
    plain, weighted = error([]), error(["--dcf", "auto"])
    print("image error after two CG iterations: plain %.3f, weighted %.3f" % (plain, weighted))
    assert weighted < plain, (weighted, plain)
