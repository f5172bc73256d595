"""Density compensation on the MI355X (ig_dcf.hip): the fixed-point spread bit for bit against the exact integer
restatement tests/dcf64.py on every route, the gather and divide within one float32 ulp of its float64, row_scale exactly, thirty
device iterations against the float64 iteration with the bound taken from a float32 emulation, and pics --dcf against the oracle
backend."""
import logging
import os
import re

import numpy as np
import pytest
from scipy.signal.windows import kaiser

import dcf64
from test_dcf_cpu import iterate_weights, mixed_coords, records, ulps
from indigo_amd import dcf, pics
from indigo_amd.backends.backend import Backend
from indigo_amd.interp import interp_sep_records
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu

C64 = np.dtype('complex64')
GUARD = 8                       # int64 words around acc
PAD = 5                         # NaN floats behind w, w_out and s_out
SENTINEL = -0x0123456789abcdef


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


@pytest.fixture(scope="module")
def cases():
    """(sep, w, scale, exact acc, float64 divide) per (grid, half-width, M), computed once on the host"""
    memo = {}

    def get(grid, width, M):
        key = (grid, width, M)
        if key not in memo:
            sep = records(grid, width, mixed_coords(M, seed=M))
            w = iterate_weights(sep, seed=width)
            scale = dcf.scale_for(M, float(w.max()))
            acc = dcf64.spread(sep, w, scale)
            memo[key] = (sep, w, scale, acc) + dcf64.gather_div(sep, acc, w, scale)
        return memo[key]
    return get


def padded(B, values, fill=np.nan):
    """a device array of values.size + PAD elements, the tail filled; (whole array, view of the head)"""
    full = np.concatenate([values, np.full(PAD, fill, dtype=values.dtype)])
    d = B.copy_array(full)
    return d, d[:values.size]


@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000, 4097])
@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("grid", [(24, 20, 18), (16, 16, 16)])
def test_spread_and_divide_match_the_restatement(hip, cases, grid, width, M):
    sep, w, scale, want, q, s = cases(grid, width, M)
    n = int(np.prod(grid))
    stride = sep['records'].shape[1] + 12                                  # (a record stride larger than the record)
    piece = hip.tuning['dcf_piece']
    try:
        hip.tuning['dcf_piece'] = 300                                      # (the heavy tiles of the larger cases in several workgroups)
        rec_d, desc, tiles = dcf.upload(hip, sep, stride=stride)
    finally:
        hip.tuning['dcf_piece'] = piece
    assert desc['stride'] == stride and (w == 0).any() == (M > 3)
    assert (tiles['ids'].size > np.unique(tiles['ids'].to_host()).size) == (M >= 1000)
    wfull_d, w_d = padded(hip, w)
    results = []
    old = hip.tuning['dcf_lds_min']
    try:
        for lds_min in (0, 8, 2 ** 31, 8):                                 # every tile through LDS, the dense ones, none; and once more
            hip.tuning['dcf_lds_min'] = lds_min
            full_d = hip.copy_array(np.full(n + 2 * GUARD, SENTINEL, dtype=np.int64))
            acc_d = full_d[GUARD:GUARD + n]
            hip.dcf_spread(acc_d, w_d, rec_d, desc, scale, tiles)
            full = full_d.to_host()
            assert np.all(full[:GUARD] == SENTINEL) and np.all(full[GUARD + n:] == SENTINEL), lds_min
            results.append(full[GUARD:GUARD + n])
    finally:
        hip.tuning['dcf_lds_min'] = old
    for got in results:
        np.testing.assert_array_equal(got, want)                           # bits: of the restatement, across the routes, across two calls
    assert np.isnan(wfull_d.to_host()[M:]).all() and np.array_equal(wfull_d.to_host()[:M], w)
    # the gather and divide
    outfull_d, out_d = padded(hip, np.full(M, np.nan, dtype=np.float32))
    sfull_d, s_d = padded(hip, np.full(M, np.nan, dtype=np.float32))
    wmax, dev = hip.dcf_gather_div(out_d, acc_d, w_d, rec_d, desc, scale, tiles, s_out=s_d)
    got, gots = outfull_d.to_host(), sfull_d.to_host()
    assert np.isnan(got[M:]).all() and np.isnan(gots[M:]).all()
    worst = int(ulps(got[:M], q).max())
    print("grid %s tw %d M %d: w_out within %d ulp, max|s - 1| %.6f (float64 %.6f)" % (grid, sep['tw'], M, worst, dev, np.abs(s - 1).max()))
    assert worst <= 1 and np.all(got[:M][w == 0] == 0)
    assert ulps(gots[:M], s.astype(np.float32)).max() <= 1
    assert np.float32(wmax).view(np.uint32) == q.max().view(np.uint32)
    assert abs(dev - np.abs(s - 1).max()) < 1e-6
    np.testing.assert_array_equal(full_d.to_host(), full)                  # acc and its guards are read only
    wmax2, dev2 = hip.dcf_gather_div(w_d, acc_d, w_d, rec_d, desc, scale, tiles)          # in place, without s_out
    assert (wmax2, dev2) == (wmax, dev)
    again = wfull_d.to_host()
    np.testing.assert_array_equal(again[:M], got[:M])
    assert np.isnan(again[M:]).all()


def test_zero_sums_give_zero_weights(hip):
    grid, M = (16, 16, 16), 65
    sep = records(grid, 3, mixed_coords(M))
    rec_d, desc, tiles = dcf.upload(hip, sep)
    acc_d = hip.copy_array(np.ones(16 ** 3, dtype=np.int64))
    w_d = hip.copy_array(np.zeros(M, dtype=np.float32))
    hip.dcf_spread(acc_d, w_d, rec_d, desc, 2.0 ** 40, tiles)
    assert not acc_d.to_host().any()
    out_d = hip.copy_array(np.ones(M, dtype=np.float32))
    assert hip.dcf_gather_div(out_d, acc_d, w_d, rec_d, desc, 2.0 ** 40, tiles) == (0.0, 1.0)
    assert not out_d.to_host().any()
    with pytest.raises(RuntimeError, match="power of two"):
        hip.dcf_spread(acc_d, w_d, rec_d, desc, 3.0, tiles)


@pytest.mark.parametrize("n", [65, 64, 1000])
@pytest.mark.parametrize("ncols", [1, 3, 8, 12])
def test_row_scale_is_exact(hip, ncols, n):
    ld = n + 6
    w = (np.random.default_rng(ncols).random(n) * 2).astype(np.float32)
    w[::7] = 0
    x = rand64c(ld, ncols, seed=2)
    want = ((w[:, None] * x[:n].real) + 1j * (w[:, None] * x[:n].imag)).astype(C64)
    x_d, y_d = hip.copy_array(x), hip.copy_array(np.full((ld, ncols), np.nan + 0j, dtype=C64))
    wfull_d, w_d = padded(hip, w)
    hip.row_scale(y_d[:n, :], x_d[:n, :], w_d, n, ncols)                  # padded panels
    got = y_d.to_host()
    np.testing.assert_array_equal(got[:n], want)
    assert np.isnan(got[n:]).all() and np.array_equal(x_d.to_host(), x)
    hip.row_scale(x_d[:n, :], x_d[:n, :], w_d, n, ncols)                  # in place
    after = x_d.to_host()
    np.testing.assert_array_equal(after[:n], want)
    np.testing.assert_array_equal(after[n:], x[n:])
    xs_d = hip.copy_array(np.asfortranarray(x[:n].reshape((-1, 1), order='F')))       # the stacked form
    ys_d = hip.zero_array((n * ncols, 1), C64)
    hip.row_scale(ys_d, xs_d, w_d, n, ncols)
    np.testing.assert_array_equal(ys_d.to_host().reshape((n, ncols), order='F'), want)
    hip.row_scale(xs_d, xs_d, w_d, n, ncols)
    np.testing.assert_array_equal(xs_d.to_host().reshape((n, ncols), order='F'), want)
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.row_scale(x_d[1:n + 1, :], x_d[:n, :], w_d, n, ncols)
    np.testing.assert_array_equal(x_d.to_host(), after)


def test_sample_weights_in_a_product(hip):
    hip._scratch = None
    n, C = 1000, 4
    w = np.random.default_rng(0).random(n) + 0.25
    W = hip.SampleWeights(w, n, C)
    x = rand64c(n * C, 1, seed=1)
    want = (np.tile(w.astype(np.float32), C)[:, None] * x).astype(C64)
    np.testing.assert_array_equal(W * x, want)
    np.testing.assert_array_equal(W.H * x, want)
    y = rand64c(n * C, 1, seed=2)
    y_d = hip.copy_array(y)
    W.eval(y_d, hip.copy_array(x), alpha=0.5 - 1j, beta=2.0)
    assert _rel(y_d.to_host(), (0.5 - 1j) * want + 2.0 * y) < 1e-6


@pytest.mark.parametrize("nsp", [300, 120])
def test_thirty_iterations_against_float64(hip, nsp):
    """The device iteration against tests/dcf64.pipe_menon on the 16^3-image radial case (half-width 3, oversampling 640/480).  The
    bound is four times what the SAME iteration emulated in float32 numpy deviates from float64 (computed here on the host: 8.2e-6
    with 300 spokes, 4.6e-6 with 120; the device: 5.4e-7 and 5.2e-7): the emulation rounds every sum, the device once per sample and
    iteration."""
    dims, nro, width, osf = (16, 16, 16), 32, 3, 640 / 480
    coord = radial_trajectory(nsp, nro)
    beta = Backend.nufft_params(width, (osf,) * 3)[1]
    sep = interp_sep_records(nro * nsp, tuple(int(n * osf) for n in dims), width, kaiser(257, beta)[128:], coord.reshape((3, -1), order='F'))
    want = dcf64.pipe_menon(sep, 30)
    emulated = np.abs(dcf64.pipe_menon32(sep, 30) / want - 1).max()
    got = dcf.pipe_menon(hip, coord, dims, width=width, osf=osf, iters=30).reshape(-1, order='F').astype(np.float64)
    err = np.abs(got / want - 1).max()
    print("30 Pipe-Menon iterations, %d spokes: device %.3e, float32 emulation %.3e (maximum relative deviation from float64)" % (nsp, err, emulated))
    assert abs(got.mean() - 1) < 1e-6
    assert err <= 4 * emulated, (err, emulated)


# ---- the driver --------------------------------------------------------------------------------------------------------------------

def _scan(tmpdir, B, N, C, nro, nsp, osf, width):
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j)).astype(C64)
    img[(np.abs(g[0]) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5
    centres = [(-1, 0, 0.3), (1, 0.5, -0.4), (0, -1, 1.0), (0.3, 1, -1.2)][:C]
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph) for cx, cy, ph in centres], axis=3).astype(C64)
    coord = radial_trajectory(nsp, nro, seed=2)
    traj = coord * np.array(N, dtype=np.float64)[:, None, None]
    F1 = B.NUFFT((1, nro, nsp), N, coord, width=width, oversamp=(osf, osf, osf), dtype=C64)
    A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
    ksp = (A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F')
    path = os.path.join(str(tmpdir), "scan.npz")
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path


@pytest.fixture(scope="module")
def scan(tmp_path_factory, hip, oracle_backend):
    """16^3, 4 coils, 300 x 32 radial samples; the weights file from the oracle backend; the proximal step from its power iteration"""
    tmp = tmp_path_factory.mktemp("dcf_scan")
    hip._scratch = None
    path = _scan(tmp, hip, (16, 16, 16), 4, nro=32, nsp=300, osf=2.0, width=3)
    hip._scratch = None
    common = ["--osf", "2.0", "--width", "3", "--lamda", "1e-3"]
    dcf.main(["--osf", "2.0", "--width", "3", "--debug", "40", path], backend=oracle_backend)
    file = os.path.splitext(path)[0] + ".dcf.npy"
    seen = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    keep, plog = Keep(level=logging.INFO), logging.getLogger("pics")
    old = plog.level
    plog.addHandler(keep)
    plog.setLevel(logging.INFO)
    try:
        oracle_backend._scratch = None
        pics.main(["-i", "0", "--power-iters", "6", "--no-fuse", "--l1", "0.01", "--dcf", file, "--debug", "40"] + common + [path], backend=oracle_backend)
    finally:
        plog.removeHandler(keep)
        plog.setLevel(old)
    oracle_backend._scratch = None
    est = [float(m.group(1)) for s in seen for m in [re.search(r"largest eigenvalue of A\^H A \+ lamda I (\S+)", s)] if m][0]
    return path, file, common, ["--step", "%.8e" % (0.9 / est)]


@pytest.mark.parametrize("source", ["auto", "file"])
@pytest.mark.parametrize("solver", ["cg", "l1", "toeplitz"])
def test_pics_dcf_on_the_gpu_matches_the_oracle_backend(scan, hip, oracle_backend, caplog, solver, source):
    """the bars of the same solvers without weights: CG 1e-5 after one iteration and 1e-3 after four (test_hip_pics.py), --l1 with the
    oracle's step 1e-5 / 1e-4 after one / ten (test_hip_wavelet.py), --toeplitz 1e-5 / 1e-4 after one / ten (test_hip_toeplitz.py)"""
    path, file, common, step = scan
    extra, runs = {"cg": ([], (("1", 1e-5), ("4", 1e-3))),
                   "l1": (["--l1", "0.02"] + step, (("1", 1e-5), ("10", 1e-4))),
                   "toeplitz": (["--toeplitz"], (("1", 1e-5), ("10", 1e-4)))}[solver]
    weights = ["--dcf", "auto" if source == "auto" else file]
    with caplog.at_level(logging.WARNING):
        for iters, tol in runs:
            argv = ["-i", iters, "--debug", "40"] + extra + weights + common + [path]
            hip._scratch = None
            out = pics.main(argv, backend=hip)
            hip._scratch = None
            oracle_backend._scratch = None
            ref = pics.main(["--no-fuse"] + argv, backend=oracle_backend)
            oracle_backend._scratch = None
            err = _rel(out, ref)
            print("pics --dcf %s, %s, %s iterations: relative difference %.3e" % (source, solver, iters, err))
            assert out.shape == (16, 16, 16, 1, 1) and err < tol, (solver, source, iters, err)
    assert not any("scratch arena too small" in r.getMessage() for r in caplog.records)
