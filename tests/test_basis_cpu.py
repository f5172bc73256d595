"""The temporal-subspace operator and pics --basis on the numpy oracle backend: Backend.frame_basis against the float64
restatement in tests/basis64.py, operators.FrameBasis, and the driver -- a unitary basis must reproduce the frame-by-frame
reconstruction, a basis of fewer columns than frames must converge, every regulariser must run on the coefficient images."""
import logging
import os
import re

import numpy as np
import pytest

import basis64
from test_hip_llr import _scan
from indigo_amd import pics
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _basis(T, K, seed):
    return rand64c(T, K, seed=seed)


@pytest.mark.parametrize("stacked", [False, True], ids=["panel", "stacked"])
@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
@pytest.mark.parametrize("alpha,beta", [(1, 0), (0.7 - 0.3j, 0), (0.7 - 0.3j, 0.5 + 0.25j)])
def test_host_form_matches_the_float64_restatement(oracle_backend, adjoint, alpha, beta, stacked):
    B = oracle_backend
    n, K, T = 105, 3, 7
    phi = _basis(T, K, 1)
    cols_x, cols_y = (T, K) if adjoint else (K, T)
    x, y = rand64c(n, cols_x, seed=2), rand64c(n, cols_y, seed=3)
    want = basis64.apply(phi, x, y, adjoint, alpha, beta)
    if beta == 0:
        y = np.full_like(y, np.nan)                                       # not read
    shape = (lambda a: np.asfortranarray(a.reshape((-1, 1), order='F'))) if stacked else (lambda a: a)
    x_d, y_d = B.copy_array(shape(x)), B.copy_array(shape(y))
    B.frame_basis(y_d, x_d, B.copy_array(phi), n, adjoint=adjoint, alpha=alpha, beta=beta)
    got = y_d.to_host().reshape((n, cols_y), order='F')
    assert got.dtype == C64 and _rel(got, want) < 2e-7, _rel(got, want)


def test_adjoint_identity(oracle_backend):
    B = oracle_backend
    n, K, T = 231, 5, 9
    phi_d = B.copy_array(_basis(T, K, 4))
    x, y = rand64c(n, K, seed=5), rand64c(n, T, seed=6)
    px = B.zero_array((n, T), C64)
    phy = B.zero_array((n, K), C64)
    B.frame_basis(px, B.copy_array(x), phi_d, n)
    B.frame_basis(phy, B.copy_array(y), phi_d, n, adjoint=True)
    lhs = np.vdot(y.astype(np.complex128), px.to_host().astype(np.complex128))
    rhs = np.vdot(phy.to_host().astype(np.complex128), x.astype(np.complex128))
    assert abs(lhs - rhs) < 1e-6 * abs(lhs), (lhs, rhs)


def test_frame_basis_operator(oracle_backend):
    B = oracle_backend
    n, K, T = 60, 2, 6
    phi = _basis(T, K, 7)
    P = B.FrameBasis(phi, n)
    assert P.shape == (n * T, n * K) and P.H.shape == (n * K, n * T) and P.dtype == C64
    x = rand64c(n * K, 2, seed=8)                                         # two columns: one product per column
    frames = P * x
    want = np.stack([basis64.forward(phi, x[:, j].reshape((n, K), order='F')).reshape(-1, order='F') for j in range(2)], axis=1)
    assert _rel(frames, want) < 2e-7
    back = P.H * frames
    gram = phi.astype(np.complex128).conj().T @ phi.astype(np.complex128)
    want = np.stack([(x[:, j].reshape((n, K), order='F').astype(np.complex128) @ gram.T).reshape(-1, order='F') for j in range(2)], axis=1)
    assert _rel(back, want) < 1e-6
    assert P.H.H is P
    # a real basis converts; what is not a T x K matrix of at most 32 columns is refused
    assert B.FrameBasis(np.eye(3), 4).shape == (12, 12)
    for bad in (np.zeros(5, C64), np.zeros((40, 33), C64), np.zeros((4, 0), C64), np.zeros((2, 2, 2), C64)):
        with pytest.raises(ValueError, match="FrameBasis"):
            B.FrameBasis(bad, 4)
    with pytest.raises(NotImplementedError, match="FrameBasis"):
        K_ = B.Kron(B.DenseMatrix(phi), B.Eye(n))
        K_ * rand64c(n * K, 1, seed=9)


def _pics(B, argv):
    B._scratch = None
    out = pics.main(argv, backend=B)
    B._scratch = None
    return out


def _frames(phi, coef):
    """the frames (X, Y, Z, T) that the coefficient images (X, Y, Z, 1, 1, 1, K) stand for"""
    return np.einsum('tk,xyzk->xyzt', np.asarray(phi, dtype=np.complex128), coef.reshape(coef.shape[:3] + (-1,)).astype(np.complex128))


@pytest.fixture(scope="module")
def unitary_scan(tmp_path_factory, oracle_backend):
    tmp = tmp_path_factory.mktemp("basis_unitary")
    path = _scan(tmp, oracle_backend, (16, 16, 8), 2, 4, nro=32, nsp=24, osf=2.0)
    oracle_backend._scratch = None
    args = ["-i", "8", "--lamda", "1e-3", "--osf", "2.0", "--width", "2", "--debug", "40", path]
    plain = _pics(oracle_backend, args)
    return str(tmp), args, plain.reshape(plain.shape[:3] + (4,))


@pytest.mark.parametrize("which,tol", [("dft", 1e-4), ("identity", 1e-6)])
def test_pics_with_a_unitary_basis_reproduces_the_frames(unitary_scan, oracle_backend, which, tol):
    """CG under a unitary change of variables produces the transformed iterates: Phi alpha is the no-basis result.  The driver
    normalises A^H y by its own largest magnitude, which differs between the two runs: each side is divided by its 2-norm."""
    tmp, args, plain = unitary_scan
    T = 4
    phi = np.exp(-2j * np.pi * np.outer(np.arange(T), np.arange(T)) / T) / np.sqrt(T) if which == "dft" else np.eye(T)
    np.save(os.path.join(tmp, which + ".npy"), phi)
    coef = _pics(oracle_backend, ["--basis", os.path.join(tmp, which + ".npy")] + args)
    assert coef.shape == (16, 16, 8, 1, 1, 1, T)
    frames = _frames(phi, coef)
    err = _rel(frames / np.linalg.norm(frames), plain / np.linalg.norm(plain))
    print("unitary basis (%s): relative difference %.3e" % (which, err))
    assert err < tol, err


@pytest.fixture(scope="module")
def subspace(tmp_path_factory, oracle_backend):
    tmp = tmp_path_factory.mktemp("basis_subspace")
    phi = basis64.exponential_basis(6)
    np.save(os.path.join(str(tmp), "phi.npy"), phi)
    path = basis64.subspace_scan(tmp, oracle_backend, (16, 16, 8), 2, phi, nro=32, nsp=24, osf=2.0)
    return os.path.join(str(tmp), "phi.npy"), path


COMMON = ["--osf", "2.0", "--width", "2", "--lamda", "1e-3", "--power-iters", "6"]


def test_pics_with_fewer_coefficients_than_frames(subspace, oracle_backend, caplog):
    """The residuals of CG decrease: what CG makes monotone is the energy norm of the error, not the 2-norm of the residual that
    the driver logs, and on SENSE systems that norm zigzags from one iteration to the next (the frame-by-frame driver logs
    2.9e-1 1.3e-1 1.1e-1 6.1e-2 5.4e-2 2.7e-2 3.4e-2 1.6e-2 on such a scan).  So: every residual is below the one two iterations
    earlier, and the last is below a tenth of the first."""
    phi, path = subspace
    with caplog.at_level(logging.INFO):
        out = _pics(oracle_backend, ["--basis", phi, "-i", "8"] + COMMON + [path])
    assert out.shape == (16, 16, 8, 1, 1, 1, 2) and np.isfinite(out).all()
    msgs = [r.getMessage() for r in caplog.records]
    assert not any("scratch arena too small" in m for m in msgs), msgs
    gram = [float(m.group(1)) for m in (re.search(r"basis: 6 frames, 2 coefficients, \|\|Phi\^H Phi - I\|\| (\S+)", s) for s in msgs) if m]
    assert len(gram) == 1 and gram[0] < 1e-6, (gram, msgs)                # orthonormal up to its complex64 rounding
    res = [float(v) for m in msgs if m.startswith("residuals:") for v in m.split()[1:]]
    assert len(res) == 8 and res[1] < res[0] and all(b < a for a, b in zip(res, res[2:])) and res[-1] < 0.1 * res[0], res
    # --basis-rank keeps the first column
    one = _pics(oracle_backend, ["--basis", phi, "--basis-rank", "1", "-i", "2", "--debug", "40"] + COMMON + [path])
    assert one.shape == (16, 16, 8, 1, 1, 1, 1)


@pytest.mark.parametrize("extra", [["--llr", "0.02", "--llr-block", "6"], ["--tv", "0.01"], ["--l1", "0.01", "--levels", "2"]],
                         ids=["llr", "tv", "l1"])
def test_every_regulariser_runs_on_the_coefficients(subspace, oracle_backend, caplog, extra):
    phi, path = subspace
    with caplog.at_level(logging.INFO):
        out = _pics(oracle_backend, ["--basis", phi, "-i", "3"] + extra + COMMON + [path])
    assert out.shape == (16, 16, 8, 1, 1, 1, 2) and np.isfinite(out).all() and np.abs(out).max() > 0
    msgs = [r.getMessage() for r in caplog.records]
    assert not any("scratch arena too small" in m for m in msgs), msgs
    if extra[0] == "--llr":
        assert any("locally low rank" in m and "2 frames" in m for m in msgs), msgs


def test_parse_and_basis_errors(subspace, oracle_backend, tmp_path, capsys):
    phi, path = subspace
    with pytest.raises(SystemExit):
        pics.parse(["--basis", phi, "--tv-time", "0.1", path])
    assert "differences between coefficients are not differences in time" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pics.parse(["--basis", phi, "--basis-rank", "0", path])
    assert "--basis-rank must be at least 1" in capsys.readouterr().err

    def run(basis, extra=()):
        f = os.path.join(str(tmp_path), "b.npy")
        np.save(f, basis)
        return _pics(oracle_backend, ["--basis", f, "-i", "1", "--debug", "40"] + list(extra) + COMMON + [path])
    with pytest.raises(ValueError, match="the basis has 5 rows, the scan has 6 time frames"):
        run(np.ones((5, 2)))
    with pytest.raises(ValueError, match="33 coefficients, at most 32"):
        run(np.ones((6, 33)))
    with pytest.raises(ValueError, match="needs a scan with several time frames"):
        run(np.ones((1, 1)), ["--crop", "TIME:1"])
    with pytest.raises(ValueError, match="--basis-rank must be at least 1"):
        pics.subspace_basis(np.ones((6, 2)), 6, 0)
