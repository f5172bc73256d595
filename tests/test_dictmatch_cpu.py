"""Dictionary matching on the numpy oracle backend: the host form of Backend.dict_match against the float64 restatement in
tests/dict64.py, the `basis` command for both models, `fit` end to end on a T2 phantom whose voxels sit on grid values, `fit_frames`,
the error messages, and one run through pics --basis on the written phi followed by `fit` on what pics wrote."""
import os

import numpy as np
import pytest

import basis64
import dict64
from indigo_amd import dictmatch, pics

C64 = np.dtype('complex64')


def _dm(B, argv):
    return dictmatch.main(argv + ["--debug", "40"], backend=B)


@pytest.mark.parametrize("stacked", [False, True], ids=["panel", "stacked"])
@pytest.mark.parametrize("n,K,N", [(105, 3, 31), (2048, 4, 1000), (1, 1, 1), (77, 32, 33)], ids=lambda v: str(v))
def test_host_form_matches_the_float64_restatement(oracle_backend, n, K, N, stacked):
    B = oracle_backend
    x, d = dict64.random_case(n, K, N, seed=n + K)
    x[n // 2] = 0                                                                      # a zero voxel: (0, 0)
    want_idx, want_ip, _ = dict64.match(d, x)
    x_d = B.copy_array(np.asfortranarray(x.reshape((-1, 1), order='F')) if stacked else x)
    idx, ip = B.dict_match(x_d, B.copy_array(d), n, chunk=100)                         # several chunks and a ragged last one
    assert idx.dtype == np.int32 and ip.dtype == C64 and idx.shape == (n,) and ip.shape == (n,)
    assert np.array_equal(idx, want_idx)
    assert np.abs(ip - want_ip).max() <= 2e-7 * np.abs(want_ip).max() + 0.0
    assert idx[n // 2] == 0 and ip[n // 2] == 0
    assert np.array_equal(x_d.to_host().ravel(order='F'), x.ravel(order='F'))          # the input is not written


def test_host_form_returns_the_lowest_index_of_equal_scores(oracle_backend):
    B = oracle_backend
    x, d = dict64.random_case(50, 4, 64, seed=1)
    d[:, 40] = d[:, 5]
    d[:, 63] = d[:, 5]
    x[:] = (np.arange(1, 51)[:, None] * d[:, 5][None, :]).astype(C64)
    idx, ip = B.dict_match(B.copy_array(x), B.copy_array(d), 50)
    assert np.array_equal(idx, np.full(50, 5))
    with pytest.raises(RuntimeError, match="33 coefficients, between 1 and 32"):
        B.dict_match(B.copy_array(dict64.random_case(4, 33, 2, seed=2)[0]), B.copy_array(dict64.random_case(4, 33, 2, seed=2)[1]), 4)


# ---- basis ----------------------------------------------------------------------------------------------------------------------------

def test_basis_t2_model(tmp_path):
    out = os.path.join(str(tmp_path), "t2")
    atoms, params, phi = _dm(None, ["basis"] + dict64.T2_ARGS + [out])
    assert atoms.shape == (32, 16) and params.shape == (32, 1) and phi.shape == (16, 4)
    t2 = np.geomspace(0.02, 0.3, 32)
    assert np.allclose(params[:, 0], t2, rtol=1e-14)
    assert np.allclose(atoms, np.exp(-0.01 * np.arange(1, 17)[None, :] / t2[:, None]), rtol=1e-13)
    assert np.abs(phi.conj().T @ phi - np.eye(4)).max() < 1e-12                       # orthonormal
    # the files round-trip
    for name, a in (("atoms", atoms), ("params", params), ("phi", phi)):
        assert np.array_equal(np.load("%s.%s.npy" % (out, name)), a)
    # the part of the dictionary outside the subspace shrinks with K
    res = []
    for K in range(1, 7):
        p = dictmatch.basis_of(atoms, rank=K)[0]
        res.append(np.linalg.norm(atoms - (atoms @ p.conj()) @ p.T) / np.linalg.norm(atoms))
    print("T2 dictionary, relative residual of the subspace at K = 1 ... 6:", " ".join("%.2e" % r for r in res))
    assert all(b < a for a, b in zip(res, res[1:])) and res[3] < 1e-3
    # --energy: the smallest K that holds the fraction
    sv = np.linalg.svd(atoms, compute_uv=False)
    e = np.cumsum(sv ** 2) / (sv ** 2).sum()
    want = int(np.argmax(e >= 0.99999)) + 1
    phi_e = _dm(None, ["basis"] + dict64.T2_ARGS[:-2] + ["--energy", "0.99999", out + "_e"])[2]
    assert phi_e.shape == (16, want) and 1 < want < 16


def test_basis_ir_model_and_external_atoms(tmp_path):
    tmp = str(tmp_path)
    ti = np.linspace(0.05, 3.0, 12)
    np.save(os.path.join(tmp, "ti.npy"), ti)
    out = os.path.join(tmp, "ir")
    atoms, params, phi = _dm(None, ["basis", "--model", "ir", "--ti", os.path.join(tmp, "ti.npy"), "--t1", "0.2:3:40", "--rank", "3", out])
    t1 = np.geomspace(0.2, 3.0, 40)
    assert atoms.shape == (40, 12) and np.allclose(params[:, 0], t1, rtol=1e-14)
    assert np.allclose(atoms, 1 - 2 * np.exp(-ti[None, :] / t1[:, None]), rtol=1e-13, atol=1e-15)
    assert phi.shape == (12, 3) and np.abs(phi.conj().T @ phi - np.eye(3)).max() < 1e-12
    assert np.array_equal(np.load(out + ".phi.npy"), phi)
    # a dictionary simulated elsewhere, two parameters per atom: the same basis as the model's
    np.save(os.path.join(tmp, "a.npy"), atoms)
    np.save(os.path.join(tmp, "p.npy"), np.concatenate([params, params ** 2], axis=1))
    a2, p2, phi2 = _dm(None, ["basis", "--atoms", os.path.join(tmp, "a.npy"), "--params", os.path.join(tmp, "p.npy"), "--rank", "3",
                              os.path.join(tmp, "ext")])
    assert np.array_equal(a2, atoms) and p2.shape == (40, 2) and np.array_equal(phi2, phi)


# ---- fit ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def phantom(tmp_path_factory):
    """the T2 dictionary of `basis` (32 T2 values from 20 to 300 ms, 16 echoes of 10 ms, K = 4) and a 12 x 10 x 8 volume of its atoms"""
    tmp = str(tmp_path_factory.mktemp("dict_phantom"))
    stem = os.path.join(tmp, "t2")
    atoms, params, phi = _dm(None, ["basis"] + dict64.T2_ARGS + [stem])
    coeffs, index, rho, inside = dict64.t2_phantom(atoms, phi)
    rec = os.path.join(tmp, "scan.rec.npy")
    np.save(rec, coeffs.T)
    argv = ["fit", "--atoms", stem + ".atoms.npy", "--params", stem + ".params.npy", "--basis", stem + ".phi.npy"]
    return dict(tmp=tmp, stem=stem, atoms=atoms, params=params, phi=phi, coeffs=coeffs, index=index, rho=rho, inside=inside, rec=rec, argv=argv)


def check_phantom_fit(ph, out):
    """what `fit` must return on the phantom, and what it must have written (used by the GPU test as well)"""
    X, Y, Z = dict64.PHANTOM_DIMS
    inside, index = ph['inside'], ph['index']
    assert out['qmaps'].shape == (X, Y, Z, 1) and out['qmaps'].dtype == np.float32
    assert out['pd'].shape == (X, Y, Z) and out['pd'].dtype == C64
    assert out['index'].shape == (X, Y, Z) and out['index'].dtype == np.int32
    assert out['misfit'].shape == (X, Y, Z) and out['misfit'].dtype == np.float32
    assert 0 < inside.sum() < inside.size
    assert np.array_equal(out['index'][inside], index[inside])                        # every unmasked voxel, no voxel excused
    assert np.array_equal(out['qmaps'][inside][:, 0], ph['params'][index[inside], 0].astype(np.float32))
    err = np.abs(out['pd'][inside] - ph['rho'][inside]).max() / np.abs(ph['rho'][inside]).max()
    print("phantom: proton density within %.3e, largest misfit %.3e" % (err, out['misfit'][inside].max()))
    assert err <= 1e-5
    assert np.abs(out['misfit'][inside]).max() <= 1e-5
    for name in ('qmaps', 'pd', 'index', 'misfit'):
        assert not out[name][~inside].any()                                           # the masked voxels are zero
        on_disk = np.load("%s.%s.npy" % (os.path.splitext(ph['rec'])[0], name))
        assert on_disk.dtype == out[name].dtype and np.array_equal(on_disk.T, out[name])     # stored reversed, like every array of a scan


def test_fit_recovers_the_phantom(phantom, oracle_backend):
    out = _dm(oracle_backend, phantom['argv'] + ["--chunk", "300", phantom['rec']])
    check_phantom_fit(phantom, out)
    # a mask threshold above the faint voxels removes them and nothing else
    a = np.abs(phantom['rho'])
    out = _dm(oracle_backend, phantom['argv'] + ["--mask-rel", "0.6", phantom['rec']])
    cn = np.linalg.norm(phantom['coeffs'].reshape(dict64.PHANTOM_DIMS + (-1,)).astype(np.complex128), axis=3)
    keep = cn >= 0.6 * cn.max()
    assert 0 < keep.sum() < phantom['inside'].sum() and a[keep].min() > 0
    assert np.array_equal(out['index'], np.where(keep, phantom['index'], 0)) and not out['pd'][~keep].any()


def test_fit_frames(phantom, oracle_backend):
    """the frames of the phantom, matched through their projection on phi: the same maps as from the coefficients"""
    ph = phantom
    n = int(np.prod(dict64.PHANTOM_DIMS))
    frames = (ph['rho'].reshape(-1, order='F')[:, None] * ph['atoms'][ph['index'].reshape(-1, order='F')]).astype(C64)
    assert frames.shape == (n, 16)
    out = dictmatch.fit_frames(oracle_backend, frames, ph['phi'], ph['atoms'], ph['params'], chunk=250)
    inside = ph['inside'].reshape(-1, order='F')
    assert np.array_equal(out['mask'], inside)
    assert np.array_equal(out['index'][inside], ph['index'].reshape(-1, order='F')[inside])
    # (the projection of rho s_a is rho Phi^H s_a whatever part of s_a lies outside the subspace: pd is rho itself)
    rho = ph['rho'].reshape(-1, order='F')
    assert np.abs(out['pd'][inside] - rho[inside]).max() <= 1e-5 * np.abs(rho).max()
    assert out['qmaps'].shape == (n, 1) and not out['qmaps'][~inside].any()


def test_error_messages(phantom, oracle_backend, tmp_path):
    ph, tmp = phantom, str(tmp_path)

    def save(name, a):
        path = os.path.join(tmp, name)
        np.save(path, a)
        return path
    fit = lambda atoms, params, basis, rec, extra=(): _dm(oracle_backend, ["fit", "--atoms", atoms, "--params", params, "--basis", basis]
                                                          + list(extra) + [rec])
    A, P, F = ph['stem'] + ".atoms.npy", ph['stem'] + ".params.npy", ph['stem'] + ".phi.npy"
    with pytest.raises(ValueError, match="the basis has 15 rows, the atoms have 16 time points"):
        fit(A, P, save("phi15.npy", np.ones((15, 4))), ph['rec'])
    with pytest.raises(ValueError, match="33 coefficients, between 1 and 32"):
        fit(save("a40.npy", np.ones((5, 40))), save("p5.npy", np.ones((5, 1))), save("phi33.npy", np.eye(40)[:, :33]), ph['rec'])
    with pytest.raises(ValueError, match=r"expected the coefficient images of pics --basis, \(X, Y, Z, 1, 1, 1, K\) with K = 3"):
        fit(A, P, F, ph['rec'], ["--basis-rank", "3"])
    with pytest.raises(ValueError, match="expected the coefficient images"):
        fit(A, P, F, save("flat.npy", np.ones((4, 8, 10, 12), dtype=C64)))
    with pytest.raises(ValueError, match="a row per atom: 32 atoms, parameters of shape"):
        fit(A, save("p31.npy", np.ones((31, 1))), F, ph['rec'])
    with pytest.raises(ValueError, match="--basis-rank 5, the basis has 4 columns"):
        fit(A, P, F, ph['rec'], ["--basis-rank", "5"])
    with pytest.raises(ValueError, match="a parameter grid is lo:hi:N"):
        _dm(None, ["basis", "--model", "t2", "--te", "0.01", "--echoes", "4", "--t2", "0.02-0.3", "--rank", "2", os.path.join(tmp, "x")])
    with pytest.raises(ValueError, match="--model t2 needs --te, --echoes and --t2"):
        _dm(None, ["basis", "--model", "t2", "--rank", "2", os.path.join(tmp, "x")])
    with pytest.raises(ValueError, match="--rank 9, between 1 and"):
        _dm(None, ["basis", "--model", "t2", "--te", "0.01", "--echoes", "4", "--t2", "0.02:0.3:8", "--rank", "9", os.path.join(tmp, "x")])
    with pytest.raises(ValueError, match="atom 1 has no component in the subspace"):
        dictmatch.compress(np.array([[1.0, 0.0], [0.0, 1.0]]), np.array([[1.0], [0.0]]))


def test_pics_basis_then_fit(oracle_backend, tmp_path):
    """pics --basis on a phi that `basis` wrote, then `fit` on the file pics wrote: the file conventions of the two ends agree"""
    tmp = str(tmp_path)
    stem = os.path.join(tmp, "t2")
    atoms, params, phi = _dm(None, ["basis", "--model", "t2", "--te", "0.01", "--echoes", "6", "--t2", "0.02:0.3:24", "--rank", "2", stem])
    N = (16, 16, 8)
    path = basis64.subspace_scan(tmp, oracle_backend, N, 2, phi, nro=32, nsp=24, osf=2.0)
    oracle_backend._scratch = None
    coef = pics.main(["--basis", stem + ".phi.npy", "-i", "3", "--osf", "2.0", "--width", "2", "--lamda", "1e-3", "--debug", "40", path],
                     backend=oracle_backend)
    oracle_backend._scratch = None
    rec = os.path.splitext(path)[0] + ".rec.npy"
    assert coef.shape == N + (1, 1, 1, 2) and np.load(rec).shape == (2, 1, 1, 1) + N[::-1]
    out = _dm(oracle_backend, ["fit", "--atoms", stem + ".atoms.npy", "--params", stem + ".params.npy", "--basis", stem + ".phi.npy", rec])
    c = coef.reshape((-1, 2), order='F')
    d, norms = dictmatch.compress(atoms, phi)
    idx, ip, s = dict64.match(d.astype(C64), c)
    cn = np.linalg.norm(c.astype(np.complex128), axis=1)
    mask = cn >= 0.02 * cn.max()
    assert 0 < mask.sum() and np.array_equal(out['index'].reshape(-1, order='F')[mask], idx[mask])
    assert np.array_equal(out['qmaps'].reshape(-1, order='F')[mask], params[idx[mask], 0].astype(np.float32))
    assert np.load(os.path.splitext(rec)[0] + ".qmaps.npy").shape == (1,) + N[::-1]
    assert np.load(os.path.splitext(rec)[0] + ".misfit.npy").shape == N[::-1]
    assert np.allclose(out['misfit'].reshape(-1, order='F')[mask], (1 - s[np.arange(c.shape[0]), idx] / cn ** 2)[mask], atol=1e-5)
