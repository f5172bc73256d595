"""ESPIRiT calibration on the CPU with the numpy oracle backend: the host forms of Backend.place_wrapped and Backend.espirit_eig and
the pipeline of indigo_amd.ecalib against the float64 restatement in tests/espirit64.py, the conditions that restatement itself must
meet (recovery of the true maps, separated eigenvalues), and the command lines of ecalib and pics --maps."""
import logging
import os

import numpy as np
import pytest

import espirit64 as e64
from indigo_amd import ecalib, pics
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
F32 = np.dtype('float32')

# Bounds: each is the figure measured with this file on the CPU (in the comment) times the stated margin.
RESTATEMENT_RECOVERY = 2 * 7.5e-4        # the restatement against the true maps on the phantom: measured 7.4e-4, x 2 (the issue's margin)
ORACLE_MAPS = 3 * 6.4e-7                 # oracle pipeline against the restatement, relative 2-norm over the separated voxels: measured 6.36e-7, x 3
NONCART_RECOVERY = 2 * 0.0215            # oracle pipeline from radial data against the true maps: measured 2.15e-2, x 2; must stay below 0.2
PICS_DIFFERENCE = 2 * 0.0462             # pics on estimated maps against pics on the true normalised maps: measured 4.61e-2, x 2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _main(B, argv):
    B._scratch = None
    try:
        return ecalib.main(argv + ["--debug", "40"], backend=B)
    finally:
        B._scratch = None


def _pics(B, argv):
    B._scratch = None
    try:
        return pics.main(argv + ["--debug", "40"], backend=B)
    finally:
        B._scratch = None


# ---- the host forms -------------------------------------------------------------------------------------------------------------

# (a 7^3 box does not fit the 17 x 9 x 5 volume: that pair is the refusal below)
PLACE_CASES = [((16, 12, 10), (7, 7, 7)), ((16, 12, 10), (5, 3, 1)), ((17, 9, 5), (5, 3, 1))]


@pytest.mark.parametrize("dims,box", PLACE_CASES, ids=str)
def test_host_place_wrapped_is_bit_exact(oracle_backend, dims, box):
    B = oracle_backend
    N, nb, ncols, pad = int(np.prod(dims)), int(np.prod(box)), 3, 5
    boxes = rand64c(nb, ncols, seed=N + nb)
    host = np.full((N + pad, ncols), np.nan, dtype=C64, order='F')
    vol = B.copy_array(host)
    B.place_wrapped(vol[:N], B.copy_array(boxes), dims, box)
    out = vol.to_host()
    for j in range(ncols):
        want = e64.place_wrapped(boxes[:, j].reshape(box, order='F'), dims)
        assert np.array_equal(_bits(out[:N, j]), _bits(want.reshape(-1, order='F')))
    assert np.array_equal(_bits(out[N:]), _bits(host[N:]))


def test_host_place_wrapped_refuses_a_box_larger_than_the_volume(oracle_backend):
    B = oracle_backend
    vol = B.zero_array((17 * 9 * 5, 1), C64)
    with pytest.raises(RuntimeError, match="box"):
        B.place_wrapped(vol, B.copy_array(rand64c(343, 1, seed=1)), (17, 9, 5), (7, 7, 7))


@pytest.mark.parametrize("C,M", [(1, 1), (2, 2), (3, 1), (8, 2), (8, 4), (9, 2)], ids=str)
def test_host_espirit_eig_matches_the_restatement(oracle_backend, C, M):
    B = oracle_backend
    n, pad = 105, 3
    G = e64.prescribed(n, C, seed=C * 10 + M)
    tri = e64.pack_triangle(G).astype(C64)
    want, lam = e64.eigenmaps(e64.unpack_triangle(tri, C), M, crop=0.3)
    g = np.full((n + pad, tri.shape[1]), np.nan, dtype=C64, order='F')
    g[:n] = tri
    maps = B.copy_array(np.full((n + pad, C * M), np.nan, dtype=C64, order='F'))
    evals = B.copy_array(np.full((n + pad, M), np.nan, dtype=F32, order='F'))
    B.espirit_eig(maps[:n], evals[:n], B.copy_array(g)[:n], n, C, M, crop=0.3)
    got, ev = maps.to_host(), evals.to_host()
    assert np.isnan(got[n:]).all() and np.isnan(ev[n:]).all()
    got = got[:n].reshape((n, C, M), order='F')
    assert np.abs(ev[:n] - lam).max() < 1e-6 and np.abs(got - want).max() < 1e-6
    assert np.abs(got[:, 0, :].imag).max() <= 1e-6 and (got[:, 0, :].real >= 0).all()
    for m in range(M):
        zero = (got[:, :, m] == 0).all(axis=1)
        assert zero.all() if m >= 2 else not zero.any()
    with pytest.raises(RuntimeError, match="sets of maps"):
        B.espirit_eig(maps[:n], evals[:n], B.copy_array(g)[:n], n, C, 5)


# ---- the restatement itself -----------------------------------------------------------------------------------------------------

def test_restatement_recovers_the_true_maps_and_separates_the_eigenvalues():
    """The conditions of the comparisons below: G(x) has eigenvalues in [0, 1]; the voxels with lambda_1 - lambda_2 >= 0.2 cover at least
    90 % of the phantom's support (measured 96.2 %); the estimated maps are the true ones S_c / sqrt(sum |S|^2), phase of coil 0 removed,
    within 0.1 in the relative 2-norm over the support (measured 7.4e-4) -- a mirrored or conjugated G(x) misses that by O(1)."""
    ref = e64.phantom_reference()
    sup = ref['support']
    assert ref['ev'].min() > -1e-9 and ref['ev'].max() < 1 + 1e-9
    cover = (ref['well'] & sup).sum() / sup.sum()
    err = e64.rel_on(ref['maps'][..., 0], ref['truth'], sup)
    mirrored = e64.rel_on(ref['maps'][::-1, ::-1, ::-1, :, 0], ref['truth'], sup)
    print("restatement on the phantom: support %.1f %% of the volume, separated on %.1f %% of it, recovery error %.3e (mirrored %.2f)"
          % (100 * sup.mean(), 100 * cover, err, mirrored))
    assert cover >= 0.9
    assert err < 0.1 and err <= RESTATEMENT_RECOVERY
    assert mirrored > 0.5


def test_restatement_on_two_sets():
    """calibration data of the soft-SENSE model: where both images are non-zero the second eigenvalue exceeds 0.9 on at least 90 % of the
    voxels (measured 100 %), and span(v_1, v_2) holds both true maps (residuals measured 9.4e-3 and 1.8e-2)"""
    ref = e64.two_set_reference()
    share = (ref['lam'][..., 1][ref['both']] > 0.9).mean()
    print("restatement on two sets: both images on %.1f %% of the volume, lambda_2 > 0.9 on %.1f %% of those, residuals %.3e %.3e"
          % (100 * ref['both'].mean(), 100 * share, ref['residual'][0], ref['residual'][1]))
    assert share >= 0.9
    assert max(ref['residual']) < 0.05


# ---- the pipeline on the oracle backend -----------------------------------------------------------------------------------------

def test_oracle_pipeline_matches_the_restatement(oracle_backend, tmp_path):
    ref = e64.phantom_reference()
    path = e64.write_calib(tmp_path, ref['calib'], "phantom.npz")
    maps, evals = _main(oracle_backend, ["-k", "4", "-m", "1", "-c", "0", "--dims", "32:28:24", path])
    assert maps.shape == e64.PHANTOM_DIMS + (4, 1) and evals.shape == e64.PHANTOM_DIMS + (1,)
    d_lam = np.abs(evals[..., 0] - ref['lam'][..., 0]).max()
    d_map = e64.rel_on(maps[..., 0], ref['maps'][..., 0], ref['well'])
    d_max = np.abs(maps[..., 0] - ref['maps'][..., 0])[ref['well']].max()
    err = e64.rel_on(maps[..., 0].astype(np.complex128), ref['truth'], ref['support'])
    err64 = e64.rel_on(ref['maps'][..., 0], ref['truth'], ref['support'])
    print("oracle pipeline against the restatement: lambda_1 %.3e, maps at separated voxels %.3e (largest element %.3e); recovery %.3e "
          "(restatement %.3e)" % (d_lam, d_map, d_max, err, err64))
    assert d_lam < 1e-4
    assert d_map <= ORACLE_MAPS
    assert err <= 1.1 * err64 + 1e-5


def test_oracle_pipeline_on_two_sets(oracle_backend, tmp_path):
    ref = e64.two_set_reference()
    path = e64.write_calib(tmp_path, ref['calib'], "two.npz")
    maps, evals = _main(oracle_backend, ["-k", "4", "-m", "2", "-c", "0", "--dims", "32:28:24", path])
    assert maps.shape == e64.PHANTOM_DIMS + (4, 2)
    for m in range(2):
        res = e64.span_residual(ref['S'][..., m], maps, ref['both'])
        print("oracle pipeline, two sets: residual of true set %d %.3e (restatement %.3e)" % (m, res, ref['residual'][m]))
        assert res <= 1.1 * ref['residual'][m] + 1e-5
    assert np.abs(evals - ref['lam']).max() < 1e-4


@pytest.fixture(scope="module")
def radial(tmp_path_factory, oracle_backend):
    return e64.noncart_scan(tmp_path_factory.mktemp("ecalib"), oracle_backend)


def test_oracle_pipeline_from_non_cartesian_data(oracle_backend, radial):
    """no `calib` in the file: the block comes from the radial samples inside |k| <= 8.  Gridding and truncation error come on top
    of the Cartesian case, so the bound is looser, but a mirrored or conjugated block would still miss it by O(1)."""
    path, S, sup = radial
    maps, evals = _main(oracle_backend, ["-m", "1", "-c", "0"] + e64.NC_ARGS + [path])
    assert maps.shape == e64.NC_DIMS + (3, 1)
    err = e64.rel_on(maps[..., 0].astype(np.complex128), e64.normalised(S), sup)
    print("oracle pipeline from radial data: recovery error %.3e" % err)
    assert NONCART_RECOVERY < 0.2 and err <= NONCART_RECOVERY


def test_too_few_central_samples_is_an_error(oracle_backend, tmp_path):
    path, _, _ = e64.noncart_scan(tmp_path, oracle_backend, name="few.npz", nsp=10)
    with pytest.raises(ValueError, match=r"samples inside the calibration region.*fewer than the 192"):
        _main(oracle_backend, ["-r", "4", "-k", "4", "-m", "1", "--osf", "2.0", "--width", "2", path])


# ---- the command lines ----------------------------------------------------------------------------------------------------------

PICS = ["-i", "8", "--osf", str(e64.NC_OSF), "--width", str(e64.NC_WIDTH), "--lamda", "1e-3"]


def test_ecalib_writes_both_files(oracle_backend, radial):
    path = radial[0]
    maps, evals = _main(oracle_backend, ["-m", "2"] + e64.NC_ARGS + [path])
    stem = os.path.splitext(path)[0]
    fm, fe = np.load(stem + ".maps.npy"), np.load(stem + ".evals.npy")
    assert fm.shape == (2, 3) + e64.NC_DIMS[::-1] and fm.dtype == C64
    assert fe.shape == (2, 1) + e64.NC_DIMS[::-1] and fe.dtype == F32
    assert np.array_equal(fm.T, maps) and np.array_equal(fe.T[..., 0, :], evals)
    assert (evals[..., 0] >= evals[..., 1]).all()
    cropped = evals < 0.8
    assert cropped.any() and (maps[np.broadcast_to(cropped[..., None, :], maps.shape)] == 0).all()


def test_pics_maps_flag_with_the_scans_own_maps_is_bit_identical(oracle_backend, radial, tmp_path):
    path = radial[0]
    own = os.path.join(str(tmp_path), "own.npy")
    np.save(own, np.load(path)['maps'])
    a = _pics(oracle_backend, PICS + [path])
    b = _pics(oracle_backend, PICS + ["--maps", own, path])
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_ecalib_then_pics_reconstructs_the_phantom(oracle_backend, radial, tmp_path, caplog):
    path, S, sup = radial
    z = np.load(path)
    bare = os.path.join(str(tmp_path), "bare.npz")                     # the scan without any maps
    np.savez(bare, data=z['data'], traj=z['traj'])
    with pytest.raises(ValueError, match=r"holds no `maps`.*--maps"):
        _pics(oracle_backend, PICS + [bare])
    _main(oracle_backend, ["-m", "1", "--dims", "32:32:32"] + e64.NC_ARGS + [bare])
    est = os.path.join(str(tmp_path), "bare.maps.npy")
    assert np.load(est).shape == (1, 3) + e64.NC_DIMS[::-1]
    out = _pics(oracle_backend, PICS + ["--maps", est, bare])
    true = os.path.join(str(tmp_path), "true.npy")
    np.save(true, e64.normalised(S).astype(C64).T)
    ref = _pics(oracle_backend, PICS + ["--maps", true, bare])
    assert out.shape == ref.shape == e64.NC_DIMS + (1,)
    diff = e64.rel_on(out, ref, np.ones(out.shape, dtype=bool))
    print("pics on the estimated maps against pics on the true normalised maps: %.3e" % diff)
    assert diff <= PICS_DIFFERENCE
    # two sets drive the soft-SENSE path
    _main(oracle_backend, ["-m", "2", "--dims", "32:32:32"] + e64.NC_ARGS + [bare])
    with caplog.at_level(logging.INFO, logger="pics"):
        oracle_backend._scratch = None
        soft = pics.main(["-i", "2"] + PICS[2:] + ["--maps", est, bare], backend=oracle_backend)
        oracle_backend._scratch = None
    assert soft.shape == e64.NC_DIMS + (1, 2) and np.isfinite(soft).all()
    assert any("sets of maps 2" in r.getMessage() for r in caplog.records)


def test_refusals(oracle_backend, tmp_path):
    big = e64.write_calib(tmp_path, rand64c(8 ** 3 * 9, 1, seed=3).reshape((8, 8, 8, 9), order='F'), "big.npz")
    with pytest.raises(ValueError, match=r"-k.*compress the coils"):
        _main(oracle_backend, ["-k", "8", "--dims", "32:32:32", big])
    small = e64.write_calib(tmp_path, rand64c(6 ** 3 * 2, 1, seed=4).reshape((6, 6, 6, 2), order='F'), "small.npz")
    with pytest.raises(ValueError, match="sets of maps from 2 coils"):
        _main(oracle_backend, ["-k", "3", "-m", "3", "--dims", "16:16:16", small])
    with pytest.raises(ValueError, match="needs an image of at least"):
        _main(oracle_backend, ["-k", "3", "-m", "1", "--dims", "16:4:16", small])
