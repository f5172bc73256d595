"""Locally low-rank regularisation without a GPU: the base-class host forms Backend.llr_threshold / llr_norm against the float64
restatement in tests/llr64.py, the properties of the proximal map, the options of pics --llr and the driver on the numpy oracle
backend."""
import logging
import os
import re

import numpy as np
import pytest

import llr64
from llr_cases import CASES, INPUTS, case_id, make_input, share_above, threshold
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
DIMS, BLOCK, T = (17, 5, 3), (4, 4, 2), 3
SHIFTS = [(0, 0, 0), (1, 3, 1)]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _x(seed=1):
    return rand64c(int(np.prod(DIMS)), T, seed=seed) - (0.5 + 0.5j)


def _median_sigma(x, shift):
    return float(np.float32(np.median(np.concatenate(llr64.singular_values(x, DIMS, T, BLOCK, shift)))))


def test_blocks_partition_the_volume():
    for dims, block, shift in [(DIMS, BLOCK, (0, 0, 0)), (DIMS, BLOCK, (1, 3, 1)), ((8, 1, 6), (8, 8, 8), (0, 0, 0)), ((9, 7, 5), (4, 4, 4), (2, 0, 3))]:
        parts = llr64.blocks(dims, block, shift)
        sides = llr64.clamp(dims, block)
        assert len(parts) == int(np.prod([-(-n // b) for n, b in zip(dims, sides)]))
        assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(int(np.prod(dims))))
        assert max(p.size for p in parts) <= int(np.prod(sides))
    # with a shift the first block holds the voxels that wrap around: j = 0 is i = n - s
    first = llr64.blocks((17, 5, 3), (4, 4, 2), (1, 3, 1))[0]
    assert first[0] == 16 + 17 * (2 + 5 * 2)


@pytest.mark.parametrize("shift", SHIFTS)
def test_host_forms_match_the_float64_restatement(oracle_backend, shift):
    B = oracle_backend
    x = _x()
    tau = _median_sigma(x, shift)
    ref = llr64.svt(x, tau, DIMS, T, BLOCK, shift)
    for shaped in (x, np.asfortranarray(x.reshape((-1, 1), order='F'))):     # the panel and the stacked column
        x_d = B.copy_array(shaped)
        B.llr_threshold(x_d, tau, DIMS, T, BLOCK, shift)
        assert _rel(x_d.to_host().reshape(x.shape, order='F'), ref) < 2e-7
        val = B.llr_norm(B.copy_array(shaped), DIMS, T, BLOCK, shift)
        assert isinstance(val, float) and abs(val - llr64.nuc(x, DIMS, T, BLOCK, shift).sum()) < 1e-12 * val
    # sides larger than the volume are clamped
    x_d = B.copy_array(x)
    B.llr_threshold(x_d, tau, DIMS, T, (64, 64, 64))
    assert _rel(x_d.to_host(), llr64.svt(x, tau, DIMS, T, DIMS)) < 2e-7


@pytest.mark.parametrize("shift", SHIFTS)
def test_svt_is_the_proximal_map_of_the_nuclear_norm(shift):
    v = _x().astype(np.complex128)
    tau = _median_sigma(v, shift)
    p = llr64.svt(v, tau, DIMS, T, BLOCK, shift)

    def cost(q):
        return 0.5 * np.linalg.norm(q - v) ** 2 + tau * llr64.nuc(q, DIMS, T, BLOCK, shift).sum()
    rng = np.random.default_rng(3)
    for eps in (1e-3, 1e-2, 1e-1, 1.0):
        for _ in range(3):
            q = p + eps * (rng.standard_normal(p.shape) + 1j * rng.standard_normal(p.shape))
            assert cost(p) <= cost(q)
    assert cost(p) <= cost(v) and cost(p) <= cost(np.zeros_like(v))
    # the singular values come down by tau, to zero at the least
    for s_in, s_out in zip(llr64.singular_values(v, DIMS, T, BLOCK, shift), llr64.singular_values(p, DIMS, T, BLOCK, shift)):
        np.testing.assert_allclose(s_out, np.maximum(s_in - tau, 0), atol=1e-12)


def test_rank_one_blocks_are_scaled_not_reshaped(oracle_backend):
    B = oracle_backend
    n = int(np.prod(DIMS))
    rng = np.random.default_rng(5)
    x = np.zeros((n, T), dtype=np.complex128)
    parts = llr64.blocks(DIMS, BLOCK)
    for rows in parts:                                                   # an outer product per block
        x[rows] = np.outer(rng.standard_normal(rows.size) + 1j * rng.standard_normal(rows.size),
                           rng.standard_normal(T) + 1j * rng.standard_normal(T))
    x = np.asfortranarray(x.astype(C64))
    norms = np.array([np.linalg.norm(x[rows].astype(np.complex128)) for rows in parts])
    tau = float(np.float32(np.median(norms)))
    x_d = B.copy_array(x)
    B.llr_threshold(x_d, tau, DIMS, T, BLOCK)
    out = x_d.to_host().astype(np.complex128)
    for rows, nrm in zip(parts, norms):
        np.testing.assert_allclose(out[rows], x[rows] * max(1 - tau / nrm, 0.0), atol=2e-6 * nrm)
    assert 0 < sum(nrm <= tau for nrm in norms) < len(parts)


def test_one_frame_shrinks_the_norm_of_every_block(oracle_backend):
    B = oracle_backend
    dims, block, shift = (9, 7, 5), (4, 4, 4), (2, 0, 3)
    x = rand64c(int(np.prod(dims)), 1, seed=2) - (0.5 + 0.5j)
    parts = llr64.blocks(dims, block, shift)
    norms = np.array([np.linalg.norm(x[rows].astype(np.complex128)) for rows in parts])
    np.testing.assert_allclose(llr64.nuc(x, dims, 1, block, shift), norms, rtol=1e-12)
    tau = float(np.median(norms))
    x_d = B.copy_array(x)
    B.llr_threshold(x_d, tau, dims, 1, block, shift)
    out = x_d.to_host()
    for rows, nrm in zip(parts, norms):
        np.testing.assert_allclose(out[rows], x[rows] * max(1 - tau / nrm, 0.0), atol=2e-7 * nrm)


@pytest.mark.parametrize("case", [c for c in CASES if c[2] > 1], ids=case_id)
def test_the_thresholds_of_the_gpu_cases_bite(case):
    """what tests/test_hip_llr.py relies on: the median singular value leaves between 20 % and 80 % of them above it"""
    dims, block, T, shift = case
    for kind in INPUTS:
        sv = llr64.singular_values(make_input(kind, dims, block, T, shift), dims, T, block, shift)
        assert 0.2 <= share_above(sv, threshold(sv)) <= 0.8, (kind, share_above(sv, threshold(sv)))


def test_options():
    a = pics.parse(["--llr", "0.02", "--llr-block", "6", "--llr-shifts", "--llr-seed", "7", "--tv-time", "0.1", "x.npz"])
    assert (a.llr, a.llr_block, a.llr_shifts, a.llr_seed, a.tv_time, a.data) == (0.02, 6, True, 7, 0.1, "x.npz")
    a = pics.parse(["x.npz"])
    assert (a.llr, a.llr_block, a.llr_shifts, a.llr_seed) == (0, 8, False, 0)
    with pytest.raises(SystemExit):
        pics.parse(["--llr", "0.02", "--l1", "0.01", "x.npz"])
    with pytest.raises(SystemExit):
        pics.parse(["--llr", "0.02", "--llr-block", "0", "x.npz"])
    pics.parse(["--llr", "0", "--l1", "0.01", "x.npz"])                  # --llr 0 is off


def test_llr_and_l1_are_rejected_with_a_clear_message(capsys):
    with pytest.raises(SystemExit):
        pics.parse(["--llr", "0.02", "--l1", "0.01", "x.npz"])
    assert "--llr and --l1 cannot be combined" in capsys.readouterr().err


def _scan(tmpdir, B, N, C, T, nro, nsp, osf, width=2):
    """a synthetic radial scan of T frames (a box that moves) with a trajectory per frame"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    centres = [(-1, 0, 0.3), (1, 0.5, -0.4)][:C]
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph) for cx, cy, ph in centres],
                   axis=3).astype(np.complex64)
    ksps, trajs = [], []
    for t in range(T):
        img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j)).astype(np.complex64)
        img[(np.abs(g[0] - 0.15 * t) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5
        coord = radial_trajectory(nsp, nro, seed=2 + t)
        F1 = B.NUFFT((1, nro, nsp), N, coord, width=width, oversamp=(osf, osf, osf), dtype=C64)
        A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
        ksps.append((A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F'))
        trajs.append(coord * np.array(N, dtype=np.float64)[:, None, None])
        B._scratch = None
    ksp = np.stack(ksps, axis=-1).reshape(ksps[0].shape + (1,) * 6 + (T,))
    traj = np.stack(trajs, axis=-1).reshape(trajs[0].shape + (1,) * 7 + (T,))
    path = os.path.join(str(tmpdir), "scan.npz")
    np.savez(path, data=ksp.T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path


def _pics(B, argv):
    B._scratch = None
    out = pics.main(argv, backend=B)
    B._scratch = None
    return out


@pytest.fixture(scope="module")
def scan(tmp_path_factory, oracle_backend):
    return _scan(tmp_path_factory.mktemp("llr_scan"), oracle_backend, (16, 16, 16), 2, 3, nro=32, nsp=30, osf=1.5)


COMMON = ["--osf", "1.5", "--width", "2", "--lamda", "1e-3", "--power-iters", "8", "--llr", "0.05", "--llr-block", "6"]


def test_pics_llr_objective_does_not_increase(scan, oracle_backend, caplog):
    with caplog.at_level(logging.INFO, logger="pics"):
        out = _pics(oracle_backend, ["-i", "30"] + COMMON + [scan])
    assert out.shape == (16, 16, 16) + (1,) * 7 + (3,)
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith("fista: locally low rank, blocks (6, 6, 6)") and "shift (0, 0, 0)" in m for m in msgs), msgs
    vals = [float(m.group(1)) for m in (re.search(r"fista iter \d+, objective (\S+)", s) for s in msgs) if m]
    assert len(vals) == 3 and all(b <= a for a, b in zip(vals, vals[1:])), vals
    # the penalty does something: not the image of the same iteration without it
    plain = _pics(oracle_backend, ["-i", "30", "--debug", "40"] + [a if a != "0.05" else "1e-9" for a in COMMON] + [scan])
    assert _rel(out, plain) > 1e-3


def test_pics_llr_with_tv_time_objective_does_not_increase(scan, oracle_backend, caplog):
    with caplog.at_level(logging.INFO, logger="pics"):
        _pics(oracle_backend, ["-i", "30", "--tv-time", "0.02"] + COMMON + [scan])
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith("tv: locally low rank") for m in msgs), msgs
    vals = [float(m.group(1)) for m in (re.search(r"tv iter \d+, objective (\S+)", s) for s in msgs) if m]
    assert len(vals) == 3 and all(b <= a for a, b in zip(vals, vals[1:])), vals


def test_pics_llr_shifts_follow_the_seed(scan, oracle_backend):
    argv = ["-i", "6", "--debug", "40", "--llr-shifts"] + COMMON + [scan]
    a = _pics(oracle_backend, argv + ["--llr-seed", "3"])
    b = _pics(oracle_backend, argv + ["--llr-seed", "3"])
    c = _pics(oracle_backend, argv + ["--llr-seed", "4"])
    fixed = _pics(oracle_backend, [v for v in argv if v != "--llr-shifts"])
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c) and not np.array_equal(a, fixed)


def test_pics_llr_on_one_frame_runs_and_says_so(scan, oracle_backend, caplog):
    with caplog.at_level(logging.INFO, logger="pics"):
        out = _pics(oracle_backend, ["-i", "3", "--crop", "TIME:1"] + COMMON + [scan])
    assert out.shape[:3] == (16, 16, 16) and out.size == 16 ** 3 and np.isfinite(out).all()
    assert any("every block has rank one" in r.getMessage() for r in caplog.records)
