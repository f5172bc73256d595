"""Field-map estimation without a GPU: the float64 restatement in tests/fmapest64.py against closed forms (its gradient against a
finite difference of its own cost, monotone descent, the fixed point of noiseless data, what the penalty buys on a phantom), the
host forms of Backend.fieldmap_init / fieldmap_step against the restatement, every refusal, the driver indigo_amd.fmapest on the numpy
oracle backend, and one end-to-end case: pics on two echoes, fmapest, pics --fmap with the estimated map."""
import logging
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import fmap64
import fmapest64
from indigo_amd import fmapest, pics

C64 = np.dtype('complex64')
F32 = np.dtype('float32')
DIMS = (12, 10, 9)
TE2, TE3 = [0.002, 0.004], [0.002, 0.004, 0.0065]


def _normalised(dims, te, seed=3, **kwargs):
    """the phantom as the driver sees it: scaled by 1 / max|y_0|; and the largest data curvature, what --beta is relative to"""
    y, field, inside = fmapest64.phantom(dims, te, seed=seed, **kwargs)
    y = y / np.abs(y[:, 0]).max()
    return y, field, inside, fmapest.relative_beta_scale(y, te)


def _rms(f, field, mask):
    return float(np.sqrt(np.mean((np.asarray(f, dtype=np.float64).reshape(-1) - field)[mask] ** 2)))


# ---- 1-4. the restatement against closed forms ---------------------------------------------------------------------------------

def test_the_gradient_is_the_derivative_of_the_cost():
    dims, te = (5, 4, 3), TE3
    rng = np.random.default_rng(1)
    n = int(np.prod(dims))
    y = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    f = rng.uniform(-200.0, 200.0, n)
    scale = fmapest.relative_beta_scale(y, te)
    for beta in (0.0, 0.05 * scale):
        g = fmapest64.gradient(y, f, te, beta, dims)
        h = 1e-4
        fd = np.empty(n)
        for j in range(n):
            e = np.zeros(n)
            e[j] = h
            fd[j] = (fmapest64.cost(y, f + e, te, beta, dims) - fmapest64.cost(y, f - e, te, beta, dims)) / (2 * h)
        # the central difference is off by h^2 / 6 |Psi'''| <= h^2 / 6 sum w k^3 ~ 1e-9 of sum w k, and by the cost's rounding / h
        assert np.abs(fd - g).max() < 1e-6 * np.abs(g).max(), (beta, np.abs(fd - g).max(), np.abs(g).max())


@pytest.mark.parametrize("te", [TE2, TE3], ids=["E2", "E3"])
@pytest.mark.parametrize("rel", [0.01, 0.1, 1.0])
def test_the_cost_decreases_monotonically(te, rel):
    y, _, _, scale = _normalised(DIMS, te)
    beta = rel * scale
    f = fmapest64.init(y, te)
    psi = fmapest64.cost(y, f, te, beta, DIMS)
    first = psi
    for it in range(100):
        f = fmapest64.step(y, f, te, beta, DIMS)
        nxt = fmapest64.cost(y, f, te, beta, DIMS)
        assert nxt <= psi * (1 + 1e-13), (it, psi, nxt)
        psi = nxt
    assert psi < 0.9 * first, (first, psi)


# The penalty's benefit.  beta = 0.01 in --beta units (1.46e-6 absolute on this phantom: dTE = 2 ms, curvature scale 1.46e-4) is where
# the float64 restatement alone meets both bounds after 100 steps: outside 137 -> 29 Hz (a quarter is 34), inside 3.9 -> 3.7 Hz; at
# 0.06 the outside error is 36 Hz, at 0.3 the inside error 5.9 Hz (the smoothing then biases the object's own field).
RMS_BETA = 0.01


def test_the_penalty_fills_the_background_and_keeps_the_object(oracle_backend):
    y, field, inside, scale = _normalised(DIMS, TE2)
    f0 = fmapest64.init(y, TE2)
    in0, out0 = _rms(f0, field, inside), _rms(f0, field, ~inside)
    f = f0
    for _ in range(100):
        f = fmapest64.step(y, f, TE2, RMS_BETA * scale, DIMS)
    print("restatement: inside %.2f -> %.2f Hz, outside %.2f -> %.2f Hz" % (in0, _rms(f, field, inside), out0, _rms(f, field, ~inside)))
    assert _rms(f, field, ~inside) < 0.25 * out0
    assert _rms(f, field, inside) <= in0
    est = fmapest.estimate(oracle_backend, y.reshape(DIMS + (2,), order='F'), TE2, iters=100, beta=RMS_BETA, cost_every=0)
    assert est.dtype == F32 and est.shape == DIMS
    est = est.reshape(-1, order='F')
    assert _rms(est, field, ~inside) < 0.25 * out0
    assert _rms(est, field, inside) <= in0
    assert np.abs(est - f).max() < 1e-2                  # the driver on float32 storage follows the float64 iteration (Hz)


def test_noiseless_data_without_a_penalty_leave_the_initial_field_alone(oracle_backend):
    y, field, _, _ = _normalised(DIMS, TE2, noise=0.0)
    f0 = fmapest64.init(y, TE2)
    assert np.abs(f0 - field).max() < 1e-9
    assert np.abs(fmapest64.step(y, f0, TE2, 0.0, DIMS) - f0).max() < 1e-9
    B = oracle_backend
    n = f0.size
    yd = B.copy_array(np.asfortranarray(y.astype(C64)))
    a, b = B.zero_array((n,), F32), B.zero_array((n,), F32)
    B.fieldmap_init(a, yd, DIMS, TE2)
    B.fieldmap_step(b, a, yd, TE2, 0.0, DIMS)
    fa, fb = a.to_host().astype(np.float64), b.to_host().astype(np.float64)
    # on complex64 data s is 1e-7 rad off zero, a step of 1e-7 / k = 1e-5 Hz, and the result is rounded to float32
    assert np.abs(fb - fa).max() <= 1e-4


# ---- 5. the host forms -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,te", [((7, 5, 3), TE2), ((1, 6, 4), TE3), ((9, 1, 1), [0.001, 0.002, 0.0035, 0.006]), ((4, 3, 1), TE3)],
                         ids=["7x5x3", "1x6x4", "9x1x1", "4x3x1"])
@pytest.mark.parametrize("stacked", [False, True], ids=["panel", "stacked"])
def test_the_host_forms_match_the_restatement(oracle_backend, dims, te, stacked):
    B = oracle_backend
    n, E = int(np.prod(dims)), len(te)
    rng = np.random.default_rng(5)
    y = (rng.standard_normal((n, E)) + 1j * rng.standard_normal((n, E))).astype(C64)
    y[0] = 0                                              # a voxel without signal
    f_old = rng.uniform(-300.0, 300.0, n).astype(F32)
    beta = float(np.float32(0.03 * fmapest.relative_beta_scale(y, te)))
    yd = B.copy_array(np.asfortranarray(y.reshape((-1, 1), order='F') if stacked else y))
    fo, fn = B.copy_array(f_old), B.zero_array((n,), F32)
    B.fieldmap_init(fn, yd, dims, te)
    ref0 = fmapest64.init(y, te)
    assert np.abs(fn.to_host() - ref0).max() <= 2.0 ** -24 * np.abs(ref0).max()
    assert B.fieldmap_step(fn, fo, yd, te, beta, dims) is None
    ref = fmapest64.step(y, f_old, te, beta, dims)
    out = fn.to_host().astype(np.float64)
    assert (np.abs(out - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-9).all(), np.abs(out - ref).max()
    psi = B.fieldmap_step(fn, fo, yd, te, beta, dims, cost=True)
    assert np.array_equal(fn.to_host().astype(np.float64), out)
    ref_psi = fmapest64.cost(y, f_old, te, beta, dims)
    assert abs(psi - ref_psi) <= 1e-11 * ref_psi, (psi, ref_psi)
    assert B.fieldmap_cost(fo, yd, te, beta, dims) == psi
    assert np.array_equal(fo.to_host(), f_old) and np.array_equal(yd.to_host().reshape(y.shape, order='F'), y)
    # beta = 0 and no signal: the voxel is left alone
    B.fieldmap_step(fn, fo, yd, te, 0.0, dims)
    assert fn.to_host()[0] == f_old[0]


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_the_backend_refuses_what_it_cannot_do(oracle_backend):
    B = oracle_backend
    dims, n = (4, 3, 2), 24
    y2, y9 = B.zero_array((n, 2), C64), B.zero_array((n, 9), C64)
    f = B.zero_array((2 * n,), F32)
    a, b = f[:n], f[n:]
    with pytest.raises(ValueError, match="between 2 and 8"):
        B.fieldmap_step(a, b, B.zero_array((n, 1), C64), [0.002], 0.1, dims)
    with pytest.raises(ValueError, match="between 2 and 8"):
        B.fieldmap_step(a, b, y9, np.arange(1, 10) * 1e-3, 0.1, dims)
    with pytest.raises(ValueError, match="between 2 and 8"):
        B.fieldmap_init(a, y9, dims, np.arange(1, 10) * 1e-3)
    for te in ([0.004, 0.002], [0.002, 0.002]):
        with pytest.raises(ValueError, match="strictly increasing"):
            B.fieldmap_step(a, b, y2, te, 0.1, dims)
        with pytest.raises(ValueError, match="strictly increasing"):
            B.fieldmap_init(a, y2, dims, te)
    with pytest.raises(ValueError, match="overlaps"):
        B.fieldmap_step(a, a, y2, TE2, 0.1, dims)
    with pytest.raises(ValueError, match="overlaps"):
        B.fieldmap_step(f[1:n + 1], a, y2, TE2, 0.1, dims)
    with pytest.raises(ValueError, match="N x E"):
        B.fieldmap_step(a, b, y2, TE3, 0.1, dims)        # three echo times, two images
    with pytest.raises(ValueError, match="N x E"):
        B.fieldmap_init(a, y2, (4, 3, 3), TE2)
    with pytest.raises(ValueError, match="beta"):
        B.fieldmap_step(a, b, y2, TE2, -1e-3, dims)
    with pytest.raises(ValueError, match="beta"):
        B.fieldmap_step(a, b, y2, TE2, float('nan'), dims)
    B.fieldmap_step(a, b, y2, TE2, 0.1, dims)             # adjacent halves of one array: fine


def test_the_driver_refuses_what_it_cannot_do(oracle_backend, tmp_path):
    y = fmapest64.phantom((4, 3, 2), TE2)[0].reshape((4, 3, 2, 2), order='F')
    with pytest.raises(ValueError, match="real-valued"):
        fmapest.estimate(oracle_backend, np.abs(y), TE2)
    with pytest.raises(ValueError, match="3 echo times for 2"):
        fmapest.estimate(oracle_backend, y, TE3)
    bad = y.copy()
    bad[1, 1, 1, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        fmapest.estimate(oracle_backend, bad, TE2)
    with pytest.raises(ValueError, match="non-finite"):
        fmapest.estimate(oracle_backend, y, [0.002, np.inf])
    with pytest.raises(ValueError, match="strictly increasing"):
        fmapest.estimate(oracle_backend, y, [0.004, 0.002])
    path = os.path.join(str(tmp_path), "echoes.rec.npy")
    np.save(path, y.T)
    with pytest.raises(ValueError, match="3 values of --te for 2"):
        fmapest.main(["--te", "0.002,0.004,0.006", path], backend=oracle_backend)
    np.save(path, np.abs(y).T)
    with pytest.raises(ValueError, match="real-valued"):
        fmapest.main(["--te", "0.002,0.004", path], backend=oracle_backend)
    with pytest.raises(SystemExit):
        fmapest.main(["--te", "0.002,0.004", "--beta", "-1", path], backend=oracle_backend)


# ---- 7. the driver ---------------------------------------------------------------------------------------------------------------

def test_the_driver_reads_both_forms_and_writes_what_pics_reads(oracle_backend, tmp_path, caplog):
    dims = (8, 6, 5)
    y, field, inside = fmapest64.phantom(dims, TE3, seed=4)
    vol = y.reshape(dims + (3,), order='F')
    frames = os.path.join(str(tmp_path), "echoes.rec.npy")
    np.save(frames, vol.reshape(dims + (1, 1, 3)).astype(C64).T)          # as pics stores T = 3 time frames
    singles = [os.path.join(str(tmp_path), "e%d.rec.npy" % l) for l in range(3)]
    for l, p in enumerate(singles):
        np.save(p, vol[..., l].astype(C64).T)
    args = ["--te", "0.002,0.004,0.0065", "-i", "20", "--cost-every", "5", "--debug", "40"]
    with caplog.at_level(logging.INFO, logger="fmapest"):
        a = fmapest.main(args + [frames], backend=oracle_backend)
    costs = [float(m.group(1)) for r in caplog.records for m in [re.search(r"fmapest iter \d+: cost (\S+)", r.getMessage())] if m]
    assert len(costs) == 5 and all(b < c for c, b in zip(costs, costs[1:])), costs      # iterations 0, 5, 10, 15 and the end
    b = fmapest.main(args + singles, backend=oracle_backend)
    assert a.shape == dims and a.dtype == F32 and np.array_equal(a, b)
    out = os.path.join(str(tmp_path), "echoes.fmap.npy")
    assert os.path.exists(out) and os.path.exists(os.path.join(str(tmp_path), "e0.fmap.npy"))
    stored = np.load(out)
    assert stored.dtype == F32 and stored.T.shape == dims and np.array_equal(stored.T, a)
    assert np.array_equal(a, fmapest.estimate(oracle_backend, vol.astype(C64), TE3, iters=20, beta=0.1))
    # pics takes it as --fmap
    nro, nviews = 16, 4
    g = SimpleNamespace(samples=(1, nro, nviews), dims=dims, T=1, M=1, N=int(np.prod(dims)))
    flat, seg = pics.field_map_segments(g, np.ones(dims + (2,), dtype=C64), stored.T, 1e-3 + 4e-6 * np.arange(nro))
    assert flat.shape == (g.N,) and np.array_equal(flat, a.reshape(-1, order='F')) and 1 <= seg[0].size <= 16


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------

def _pics(B, argv):
    B._scratch = None
    out = pics.main(argv, backend=B)
    B._scratch = None
    return out


def test_two_echoes_to_a_corrected_long_readout(oracle_backend, tmp_path):
    """12 x 12 x 8 voxels, two coils, 24 x 96 radial samples, a smooth field map of +-100 Hz.  Two scans with a 0.24 ms readout at
    TE = 2 and 4 ms, simulated with the project's time-segmented forward model, reconstructed by pics without a map; fmapest on the
    two images; then a scan with a 10 ms readout reconstructed without a map, with the estimated map and with the true one.
    Errors are relative to the same reconstruction of the same long scan simulated without a field; DESIGN.md §3.21 records them."""
    B = oracle_backend
    dims, nro, nsp, osf, width = (12, 12, 8), 24, 96, 2.0, 3
    field = fmap64.smooth_field(dims, 100.0, seed=2)
    common = ["--osf", str(osf), "--width", str(width), "--lamda", "1e-3", "--debug", "40", "-i", "12"]
    recs = []
    for l, te in enumerate(TE2):
        times = te + 1e-5 * np.arange(nro)
        d = tmp_path / ("echo%d" % l)
        d.mkdir()
        path = fmap64.fmap_scan(d, B, dims, field, times, nro, nsp, osf, width)[0]
        _pics(B, common + [path])
        recs.append(os.path.splitext(path)[0] + ".rec.npy")
    est = fmapest.main(["--te", "0.002,0.004", "-i", "100", "--debug", "40"] + recs, backend=B)
    est_path = os.path.join(str(tmp_path), "echo0", "scan.fmap.npy")
    assert os.path.exists(est_path)
    img, mps = fmap64.phantom(dims)
    mask = np.abs(img) > 0.1 * np.abs(img).max()
    print("field map: rms error %.2f Hz where the object is, field rms %.2f Hz" % (
        float(np.sqrt(np.mean((est - field)[mask] ** 2))), float(np.sqrt(np.mean(field[mask] ** 2)))))
    d = tmp_path / "long"
    d.mkdir()
    long_times = 1e-3 + np.arange(nro) * (10e-3 / (nro - 1))
    path, true_path, times_path = fmap64.fmap_scan(d, B, dims, field, long_times, nro, nsp, osf, width)

    d = tmp_path / "ideal"
    d.mkdir()
    ideal = _pics(B, common + [fmap64.fmap_scan(d, B, dims, np.zeros(dims), long_times, nro, nsp, osf, width)[0]]).reshape(dims)

    def err(rec):                                         # against the same reconstruction of the same scan without off-resonance
        return float(np.linalg.norm((rec.reshape(dims) - ideal).ravel()) / np.linalg.norm(ideal.ravel()))
    e_none = err(_pics(B, common + [path]))
    e_est = err(_pics(B, common + ["--fmap", est_path, "--times", times_path, path]))
    e_true = err(_pics(B, common + ["--fmap", true_path, "--times", times_path, path]))
    print("long readout: error without a map %.4f, with the estimated map %.4f, with the true map %.4f" % (e_none, e_est, e_true))
    assert e_est < e_none, (e_est, e_none, e_true)
