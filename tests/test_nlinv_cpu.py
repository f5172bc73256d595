"""NLINV on the CPU with the numpy oracle backend: the host forms of Backend.nlinv_product and Backend.sobolev_weight against the
float64 restatement in tests/nlinv64.py, the forward/adjoint pairs and the bilinearity of the model, the pipeline of indigo_amd.nlinv
against the restatement's own figures, and the command lines of nlinv and pics --maps."""
import os

import numpy as np
import pytest

import nlinv64 as n64
from indigo_amd import nlinv, pics
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
MARGIN = 1.5                # the pipeline stays within this factor of the float64 restatement's own figures for the same options


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _main(B, argv):
    B._scratch = None
    try:
        return nlinv.main(argv + ["--debug", "40"], backend=B)
    finally:
        B._scratch = None


def _pics(B, argv):
    B._scratch = None
    try:
        return pics.main(argv + ["--debug", "40"], backend=B)
    finally:
        B._scratch = None


# ---- the host forms -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,C", [(1, 1), (255, 3), (2048, 8), (5049, 9)], ids=str)
def test_host_nlinv_product_is_the_restatement_rounded_once(oracle_backend, n, C):
    """the host form computes in float64 and rounds once: bit for bit the restatement rounded to complex64"""
    B = oracle_backend
    pad = 3
    rho, coils = rand64c(n, 1, seed=n).reshape(-1), rand64c(n, C, seed=n + 1)
    for adjoint in (False, True):
        cols_x, cols_y = (C, 1 + C) if adjoint else (1 + C, C)
        x, y0 = rand64c(n, cols_x, seed=n + 2), rand64c(n, cols_y, seed=n + 3)
        for alpha, beta in ((1, 0), (0.75 - 0.5j, 0), (0.75 - 0.5j, -0.25 + 1.5j)):
            host = np.full((n + pad, cols_y), np.nan, dtype=C64, order='F')
            if beta != 0:
                host[:n] = y0
            y_d = B.copy_array(host)
            B.nlinv_product(y_d[:n], B.copy_array(x), B.copy_array(rho), B.copy_array(coils), n, C, adjoint=adjoint, alpha=alpha, beta=beta)
            got = y_d.to_host()
            want = n64.product(rho, coils, x, y0, adjoint, alpha, beta).astype(C64)
            assert np.array_equal(_bits(got[:n]), _bits(np.asfortranarray(want))), (adjoint, alpha, beta)
            assert np.isnan(got[n:]).all()
    with pytest.raises(RuntimeError, match="coils"):
        B.nlinv_product(y_d[:n], B.copy_array(x), B.copy_array(rho), B.copy_array(coils), n, 0)


@pytest.mark.parametrize("dims", [(16, 12, 10), (17, 9, 5), (1, 1, 7)], ids=str)
@pytest.mark.parametrize("ab", [(220, 32), (10, 32), (30, 15)], ids=str)
def test_host_sobolev_weight_matches_the_restatement(oracle_backend, dims, ab):
    """the host form rounds w and scale * w to float32 like the kernel: within 1e-6 of the restatement, element by element"""
    B = oracle_backend
    N, ncols, pad, scale = int(np.prod(dims)), 3, 5, 0.37
    x = rand64c(N, ncols, seed=N)
    want = n64.weight(x, dims, ab[0], ab[1], scale)
    host = np.full((N + pad, ncols), np.nan, dtype=C64, order='F')
    y_d = B.copy_array(host)
    B.sobolev_weight(y_d[:N], B.copy_array(x), dims, ncols, ab[0], ab[1], scale=scale)
    got = y_d.to_host()
    assert np.isnan(got[N:]).all()
    assert (np.abs(got[:N] - want) <= 1e-6 * np.abs(want)).all()
    host[:N] = x                                                            # in place
    y_d = B.copy_array(host)
    B.sobolev_weight(y_d[:N], y_d[:N], dims, ncols, ab[0], ab[1], scale=scale)
    assert np.array_equal(_bits(y_d.to_host()[:N]), _bits(got[:N]))
    w = n64.weights(dims, *ab)
    assert w[0, 0, 0] == 1.0 and np.array_equal(w, w[(-np.arange(dims[0])) % dims[0]][:, (-np.arange(dims[1])) % dims[1]][:, :, (-np.arange(dims[2])) % dims[2]])


# ---- the forward / adjoint pairs and the bilinearity ------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(12, 10, 8), (9, 7, 5)], ids=str)
def test_adjoint_pairs(oracle_backend, dims):
    B, C = oracle_backend, 3
    N = int(np.prod(dims))
    A, P, S, DF = n64.backend_model(B, dims, C, 10.0, 32.0)
    keep = n64.set_point(B, P, S, rand64c(N * (1 + C), 1, seed=5))
    for name, node in (("NlinvProduct", P), ("SobolevCoils", S), ("DF", DF)):
        defect = n64.adjoint_defect(B, node, seed=11)
        print("%s %s: adjoint defect %.3e" % (name, dims, defect))
        assert defect <= 1e-5, name
    del keep


@pytest.mark.parametrize("dims", [(12, 10, 8), (9, 7, 5)], ids=str)
def test_operators_match_the_restatement_and_the_model_is_bilinear(oracle_backend, dims):
    """F(u + v) - F(u) - DF(u) v = A vec(d rho * W d c^) to 1e-5 of its own norm; SobolevCoils and DF against float64 to 1e-5"""
    B, C, a, b = oracle_backend, 3, 10.0, 32.0
    N = int(np.prod(dims))
    A, P, S, DF = n64.backend_model(B, dims, C, a, b)
    u, v = rand64c(N * (1 + C), 1, seed=21).reshape(-1), rand64c(N * (1 + C), 1, seed=22).reshape(-1)
    for adjoint in (False, True):
        got = n64.evaluate(B, S, u, forward=not adjoint)
        want = n64.sobolev_coils(u, dims, C, a, b, adjoint=adjoint)
        assert np.linalg.norm(got - want) <= 1e-5 * np.linalg.norm(want)

    def F(w):
        """A vec(rho * c) through the backend: the point of w, the map product with one set of maps, the transforms"""
        p = n64.evaluate(B, S, w)
        pc = B.zero_array((N * C, 1), C64)
        B.coil_maps(pc, B.copy_array(np.asfortranarray(p[:N].reshape(-1, 1))), B.copy_array(np.asfortranarray(p[N:].reshape(-1, 1))), N, C, 1)
        return n64.evaluate(B, A, pc.to_host()).astype(np.complex128)

    keep = n64.set_point(B, P, S, u)
    second = F((u + v).astype(C64)) - F(u) - n64.evaluate(B, DF, v).astype(np.complex128)
    pv = n64.sobolev_coils(v, dims, C, a, b).reshape((N, 1 + C), order='F')
    want = n64.apply64(A, (pv[:, :1] * pv[:, 1:]).reshape(-1, 1, order='F')).reshape(-1)
    err = np.linalg.norm(second - want) / np.linalg.norm(want)
    print("bilinearity %s: %.3e of the second-order term's norm" % (dims, err))
    assert err <= 1e-5
    df64 = n64.apply64(A, n64.product(keep.to_host().reshape((N, 1 + C), order='F')[:, 0], keep.to_host().reshape((N, 1 + C), order='F')[:, 1:],
                                      pv).reshape(-1, 1, order='F')).reshape(-1)
    assert np.linalg.norm(n64.evaluate(B, DF, v) - df64) <= 1e-5 * np.linalg.norm(df64)
    with pytest.raises(RuntimeError, match="set_point"):
        n64.evaluate(B, B.NlinvProduct(N, C), v)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scan(tmp_path_factory, oracle_backend):
    return n64.write_scan(tmp_path_factory.mktemp("nlinv"), oracle_backend)


def test_oracle_pipeline_stays_within_the_restatements_figures(oracle_backend, scan):
    """dims (24, 20, 16), 4 coils, 48 x 300 radial samples, osf 2, half-width 2, a = 10, b = 32, 10 Newton steps of 10 CG iterations.
    Measured with this file, restatement / oracle pipeline: residual after steps 0, 3, 5, 7, 9: 0.6645 0.1933 0.0735 0.0294 0.0122 /
    0.6645 0.1933 0.0733 0.0297 0.0122; image error 0.0581 / 0.0589; maps error 0.0399 / 0.0407; image * maps against
    rho c / (s sqrt L): 3.4e-8."""
    B = oracle_backend
    ref, ph = n64.reference(B), n64.phantom(B)
    z, state = np.load(scan), {}
    B._scratch = None
    image, maps, history = nlinv.nlinv(B, z['data'].T, z['traj'].T, n64.DIMS, iters=n64.ITERS, cg_iters=n64.CG_ITERS, a=n64.SOBOLEV[0],
                                       b=n64.SOBOLEV[1], osf=n64.OSF, width=n64.WIDTH, state=state)
    res = [h['residual'] for h in history]
    res64 = [h['residual'] for h in ref['history']]
    err_i, err_m = n64.image_error(image, ph), n64.maps_error(maps, ph)
    print("residuals: restatement %s" % " ".join("%.4f" % v for v in res64))
    print("residuals: oracle      %s" % " ".join("%.4f" % v for v in res))
    print("image error %.4f (restatement %.4f), maps error %.4f (restatement %.4f)" % (err_i, ref['image_error'], err_m, ref['maps_error']))
    # (the first system, at c = 0, has few distinct eigenvalues: its CG reaches the tolerance of Backend.cg before the tenth iteration)
    assert len(history) == n64.ITERS and all(1 <= h['cg_iters'] <= n64.CG_ITERS for h in history)
    assert [h['alpha'] for h in history] == [2.0 ** -n for n in range(n64.ITERS)]
    assert all(later < earlier for earlier, later in zip([1.0] + res, res))
    assert all(later < earlier for earlier, later in zip([1.0] + res64, res64))
    assert res[-1] <= MARGIN * res64[-1]
    assert err_i <= MARGIN * ref['image_error'] and err_m <= MARGIN * ref['maps_error']
    n64.check_results(image, maps, state)


# ---- the command line -------------------------------------------------------------------------------------------------------------

def test_nlinv_writes_both_files_and_pics_reads_the_maps(oracle_backend, scan, tmp_path):
    B = oracle_backend
    z = np.load(scan)
    path = os.path.join(str(tmp_path), "short.npz")
    np.savez(path, data=z['data'], traj=z['traj'])
    image, maps, history = _main(B, ["-i", "3", "--cg-iters", "4"] + n64.ARGS[8:] + ["--sobolev-a", "10", path])
    stem = os.path.splitext(path)[0]
    fi, fm = np.load(stem + ".nlinv.npy"), np.load(stem + ".maps.npy")
    assert fi.shape == n64.DIMS[::-1] and fi.dtype == C64
    assert fm.shape == (1, n64.COILS) + n64.DIMS[::-1] and fm.dtype == C64
    assert np.array_equal(fi.T, image) and np.array_equal(fm.T[..., 0], maps)
    assert len(history) == 3 and all(1 <= h['cg_iters'] <= 4 for h in history)
    with pytest.raises(ValueError, match=r"holds no `maps`"):
        _pics(B, ["-i", "5", "--osf", str(n64.OSF), "--width", str(n64.WIDTH), path])
    rec = _pics(B, ["-i", "5", "--osf", str(n64.OSF), "--width", str(n64.WIDTH), "--maps", stem + ".maps.npy", path])
    assert rec.shape[:3] == n64.DIMS and np.isfinite(rec).all() and np.abs(rec).max() > 0
    # coil compression in passing: two virtual coils
    image2, maps2, _ = _main(B, ["-i", "2", "--cg-iters", "3", "--cc", "2"] + n64.ARGS[8:] + ["--sobolev-a", "10", path])
    assert maps2.shape == n64.DIMS + (2,) and image2.shape == n64.DIMS


def test_refusals(oracle_backend, scan, tmp_path):
    B = oracle_backend
    z = np.load(scan)
    ksp, traj = z['data'].T, z['traj'].T
    frames = os.path.join(str(tmp_path), "frames.npz")
    k2 = np.stack([ksp, ksp], axis=-1).reshape(ksp.shape + (1,) * 6 + (2,))
    np.savez(frames, data=k2.T, traj=traj.T)
    with pytest.raises(ValueError, match="one time frame only"):
        _main(B, n64.ARGS + [frames])
    bare = os.path.join(str(tmp_path), "bare.npz")
    np.savez(bare, data=ksp.T)
    with pytest.raises(ValueError, match="has no `traj`"):
        _main(B, n64.ARGS + [bare])
    with pytest.raises(SystemExit, match="only .npz"):
        _main(B, n64.ARGS + [os.path.join(str(tmp_path), "scan.h5")])
