"""The Toeplitz normal operator and pics --toeplitz on the numpy oracle backend: Backend.psf_mix against the float64 restatement
in tests/toep64.py, operators.ToeplitzNormal with an arbitrary Hermitian kernel, the built kernel against the exact NUDFT normal
operator, and the driver."""
import logging
import os
import re

import numpy as np
import pytest

import basis64
import toep64
from test_hip_llr import _scan
from indigo_amd import pics
from indigo_amd.toeplitz import pack_planes, psf_kernel
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
WIDTH, OSF = 3, 2.0          # of the accuracy test and of the driver runs that take their bar from it


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _hermitian(K, grid, seed):
    """(K, K) + grid complex128, Hermitian at every grid point"""
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((K, K) + tuple(grid)) + 1j * rng.standard_normal((K, K) + tuple(grid))
    return H + np.conj(H.transpose(1, 0, 2, 3, 4))


@pytest.mark.parametrize("interleaved", [False, True], ids=["coil-major", "interleaved"])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_host_form_matches_the_float64_restatement(oracle_backend, K, interleaved):
    B = oracle_backend
    n, C = 105, 3
    kern = pack_planes(_hermitian(K, (7, 5, 3), K))                       # (K^2, n)
    x = rand64c(n * C * K, 1, seed=2).reshape((n, C, K), order='F')
    want = toep64.mix(kern, x)
    mem = x.transpose(1, 0, 2) if interleaved else x                      # (c, g, k) or (g, c, k), first index fastest
    panel = np.asfortranarray(mem.reshape((n * C, K), order='F'))
    kern_d = B.copy_array(np.ascontiguousarray(kern).reshape(-1))
    x_d = B.copy_array(panel)
    y_d = B.copy_array(np.full_like(panel, np.nan))                       # not read
    B.psf_mix(y_d, x_d, kern_d, n, C, interleaved=interleaved)
    B.psf_mix(x_d, x_d, kern_d, n, C, interleaved=interleaved)            # in place
    for got in (y_d.to_host(), x_d.to_host()):
        got = got.reshape(((C, n, K) if interleaved else (n, C, K)), order='F')
        got = got.transpose(1, 0, 2) if interleaved else got
        assert got.dtype == C64 and _rel(got, want) < 2e-7, _rel(got, want)


def test_toeplitz_normal_with_an_arbitrary_hermitian_kernel(oracle_backend):
    B = oracle_backend
    dims, C, K = (6, 5, 4), 3, 3
    grid = tuple(2 * n for n in dims)
    N = int(np.prod(dims))
    maps = rand64c(N, C, seed=4).reshape(dims + (C,), order='F')
    H = _hermitian(K, grid, 1)
    T = B.ToeplitzNormal(dims, maps, pack_planes(H), K)
    assert T.shape == (N * K, N * K) and T.dtype == C64 and T.H is T
    x, y = rand64c(N * K, 2, seed=5), rand64c(N * K, 2, seed=6)           # two columns
    Tx, Ty = (T * x).astype(np.complex128), (T * y).astype(np.complex128)
    for j in range(2):
        lhs, rhs = np.vdot(y[:, j].astype(np.complex128), Tx[:, j]), np.vdot(Ty[:, j], x[:, j].astype(np.complex128))
        assert abs(lhs - rhs) < 1e-6 * abs(lhs), (lhs, rhs)
    # the same kernel handed over in the other memory order is the same operator
    assert _rel(B.ToeplitzNormal(dims, maps, pack_planes(H, 'xzy'), K, order='xzy') * x, Tx) < 1e-6
    alpha, beta = 0.7 - 0.3j, 0.5 + 0.25j
    y_d = B.copy_array(y)
    T.eval(y_d, B.copy_array(x), alpha=alpha, beta=beta)
    assert _rel(y_d.to_host(), alpha * Tx + beta * y) < 1e-6
    # against the definition, in float64: sum_c S_c^H crop F^-1 P F zpad S_c
    Pg = toep64.unpack(pack_planes(H), int(np.prod(grid)), K).reshape(grid + (K, K), order='F')
    sl = tuple(slice(m // 2 + int(np.ceil(-n / 2)), m // 2 + int(np.ceil(-n / 2)) + n) for m, n in zip(grid, dims))
    xa = x[:, 0].reshape(dims + (K,), order='F').astype(np.complex128)
    acc = np.zeros(dims + (K,), dtype=np.complex128)
    for c in range(C):
        full = np.zeros(grid + (K,), dtype=np.complex128)
        full[sl] = maps[..., c, None] * xa
        mixed = np.einsum('xyzab,xyzb->xyza', Pg, np.fft.fftn(full, axes=(0, 1, 2)))
        acc += np.conj(maps[..., c, None]) * (np.fft.ifftn(mixed, axes=(0, 1, 2)) * np.prod(grid))[sl]
    assert _rel(Tx[:, 0], acc.reshape(-1, order='F')) < 1e-6
    with pytest.raises(ValueError, match="between 1 and 8"):
        B.ToeplitzNormal(dims, maps, np.zeros((81, 8 * N), np.float32), 9)


def test_the_unfused_composition_is_the_same_operator(oracle_backend):
    """a backend without zero-pad-aware transforms for the grid runs Crop * UnscaledFFT * Zpad, with the kernel in F order"""
    from oracle.np_backend import NumpyBackend
    plain = NumpyBackend()
    plain.supports_padded_fft = lambda grid, ncoils=None: False
    dims, C, K = (6, 5, 4), 3, 2
    N = int(np.prod(dims))
    maps = rand64c(N, C, seed=4).reshape(dims + (C,), order='F')
    kern = pack_planes(_hermitian(K, tuple(2 * n for n in dims), 2))
    x = rand64c(N * K, 2, seed=5)
    T0, T1 = oracle_backend.ToeplitzNormal(dims, maps, kern, K), plain.ToeplitzNormal(dims, maps, kern, K, chunk=2)
    assert (T0._order, T1._order) == ('xzy', 'xyz') and len(T1._parts) == 2
    assert _rel(T1 * x, T0 * x) < 1e-6
    y = rand64c(N * K, 2, seed=6)
    y_d = plain.copy_array(y)
    T1.eval(y_d, plain.copy_array(x), alpha=0.7 - 0.3j, beta=0.5 + 0.25j)
    assert _rel(y_d.to_host(), (0.7 - 0.3j) * (T0 * x) + (0.5 + 0.25j) * y) < 1e-6


# ---- accuracy against the exact NUDFT ----------------------------------------------------------------------------------

DIMS, COILS, FRAMES, SAMPLES = (12, 10, 8), 2, 4, 300


def _gridding_normal(B, dims, maps, trajs, phi):
    """the EXISTING operator: FrameBasis^H * BlockDiag(A_t^H A_t) * FrameBasis"""
    C = maps.shape[3]
    ops = []
    for trj in trajs:
        F1 = B.NUFFT((1,) + trj.shape[1:], dims, trj, width=WIDTH, oversamp=(OSF,) * 3, dtype=C64)
        A = B.KronI(C, F1) * B.VStack([B.Diag(maps[..., c:c + 1]) for c in range(C)])
        ops.append(A.H * A)
    Phi = B.FrameBasis(phi, int(np.prod(dims)))
    return Phi.H * B.BlockDiag(ops) * Phi


def _exact_scale(dims):
    """the constant between the NUFFT's normal operator and the unscaled NUDFT's: the centred transform is unitary over the
    oversampled grid, and the Kaiser-Bessel kernel is not normalised (indigo_amd.toeplitz.nufft_gain, restated)"""
    from scipy.special import i0
    beta = np.pi * np.sqrt(((WIDTH * 2. / OSF) * (OSF - 0.5)) ** 2 - 0.8)
    gain = 2.0 * WIDTH * np.sinh(beta) / (beta * i0(beta))
    return gain ** 6 / np.prod([int(n * OSF) for n in dims])


@pytest.fixture(scope="module")
def accuracy(oracle_backend):
    """e_grid and e_toep of the accuracy test, computed once: the driver test takes its bar from e_grid"""
    B = oracle_backend
    B._scratch = None
    rng = np.random.default_rng(0)
    distinct = [rng.random((3, SAMPLES, 1)) - 0.5 for _ in range(3)]
    which = [0, 1, 0, 2]                                                  # frames 0 and 2 share a trajectory
    trajs = [distinct[w] for w in which]
    phi = rand64c(FRAMES, 2, seed=3)
    N = int(np.prod(DIMS))
    maps = rand64c(N, COILS, seed=4).reshape(DIMS + (COILS,), order='F')
    alpha = rand64c(N * 2, 1, seed=5)
    want = toep64.normal_exact([t.reshape(3, -1) for t in trajs], phi, maps, alpha.reshape((N, 2), order='F'),
                               scale=_exact_scale(DIMS)).reshape((-1, 1), order='F')
    e_grid = _rel(_gridding_normal(B, DIMS, maps, trajs, phi) * alpha, want)
    B._scratch = None
    kern = psf_kernel(B, DIMS, distinct, which, phi, WIDTH, OSF)
    B._scratch = None
    e_toep = _rel(B.ToeplitzNormal(DIMS, maps, kern, 2) * alpha, want)
    return e_grid, e_toep


def test_accuracy_against_the_exact_nudft(accuracy):
    """The gridding operator carries the NUFFT's approximation twice; the point-spread functions carry it once, but on the image
    of twice the size, whose roll-off is deeper at large lags: hence the factor 3.  Measured on the oracle backend, half-width 3,
    oversampling 2: e_grid 2.38e-02, e_toep 9.90e-03."""
    e_grid, e_toep = accuracy
    print("exact NUDFT: e_grid %.3e, e_toep %.3e" % (e_grid, e_toep))
    assert e_toep <= 3 * e_grid, (e_toep, e_grid)


def test_exact_point_spread_functions_give_the_exact_normal_operator(oracle_backend):
    """the embedding itself: with P the transform of the point-spread functions summed directly (lag d at index d mod 2 n_a, the
    unscaled inverse transform's 1 / (8 N) folded in) the operator IS the exact NUDFT normal operator, to the complex64 rounding
    of its transforms -- the project's 1e-5"""
    B = oracle_backend
    dims, C = (6, 5, 4), 2
    grid = tuple(2 * n for n in dims)
    N = int(np.prod(dims))
    rng = np.random.default_rng(1)
    trajs = [(rng.random((3, 80)) - 0.5) for _ in range(3)]
    phi = rand64c(3, 2, seed=3)
    maps = rand64c(N, C, seed=4).reshape(dims + (C,), order='F')
    psf = toep64.psf_exact(trajs, phi, dims, scale=1.0 / 80)
    psf[:, :, 0, :, :] = psf[:, :, :, 0, :] = psf[:, :, :, :, 0] = 0      # the lag -n_a is never used (i - j lies in (-n_a, n_a)) and has no partner +n_a
    P = np.fft.fftn(np.fft.ifftshift(psf, axes=(2, 3, 4)), axes=(2, 3, 4)) / np.prod(grid)
    assert np.abs(P - np.conj(P.transpose(1, 0, 2, 3, 4))).max() < 1e-12 * np.abs(P).max()
    alpha = rand64c(N * 2, 1, seed=5)
    want = toep64.normal_exact(trajs, phi, maps, alpha.reshape((N, 2), order='F'), scale=1.0 / 80)
    got = B.ToeplitzNormal(dims, maps, pack_planes(P), 2) * alpha
    err = _rel(got, want.reshape((-1, 1), order='F'))
    print("exact point-spread functions: relative error %.3e" % err)
    assert err < 1e-5, err


def test_identity_basis_on_a_shared_trajectory_is_the_single_frame_operator(oracle_backend):
    B = oracle_backend
    rng = np.random.default_rng(2)
    trj = rng.random((3, SAMPLES, 1)) - 0.5
    N = int(np.prod(DIMS))
    maps = rand64c(N, COILS, seed=4).reshape(DIMS + (COILS,), order='F')
    T3 = B.ToeplitzNormal(DIMS, maps, psf_kernel(B, DIMS, [trj], [0, 0, 0], np.eye(3), WIDTH, OSF), 3)
    B._scratch = None
    T1 = B.ToeplitzNormal(DIMS, maps, psf_kernel(B, DIMS, [trj], [0], None, WIDTH, OSF), 1)
    B._scratch = None
    x = rand64c(N * 3, 1, seed=7)
    each = np.concatenate([T1 * np.asfortranarray(x[k * N:(k + 1) * N]) for k in range(3)])
    assert _rel(T3 * x, each) < 1e-6
    # a shared trajectory with a general basis: (Phi^H Phi) (x) T_1
    phi = rand64c(5, 2, seed=8)
    T2 = B.ToeplitzNormal(DIMS, maps, psf_kernel(B, DIMS, [trj], [0] * 5, phi, WIDTH, OSF), 2)
    B._scratch = None
    gram = phi.astype(np.complex128).conj().T @ phi.astype(np.complex128)
    x = rand64c(N * 2, 1, seed=9)
    t1x = np.stack([(T1 * np.asfortranarray(x[k * N:(k + 1) * N]))[:, 0] for k in range(2)], axis=1).astype(np.complex128)
    assert _rel(T2 * x, (t1x @ gram.T).reshape((-1, 1), order='F')) < 1e-6


# ---- the driver ------------------------------------------------------------------------------------------------------------

def _pics(B, argv):
    B._scratch = None
    out = pics.main(argv, backend=B)
    B._scratch = None
    return out


@pytest.fixture(scope="module")
def scan(tmp_path_factory, oracle_backend):
    tmp = tmp_path_factory.mktemp("toeplitz")
    path = _scan(tmp, oracle_backend, (16, 16, 8), 2, 4, nro=32, nsp=24, osf=OSF, width=WIDTH)
    oracle_backend._scratch = None
    phi = os.path.join(str(tmp), "phi.npy")
    np.save(phi, basis64.exponential_basis(4))
    return str(tmp), phi, path


COMMON = ["--osf", str(OSF), "--width", str(WIDTH), "--lamda", "1e-3", "--power-iters", "6"]


def test_pics_basis_toeplitz_agrees_with_basis_alone(scan, oracle_backend, accuracy, caplog):
    """8 CG iterations: the bar is the operator-level e_grid of the accuracy test (same half-width and oversampling) times 10 for
    CG's amplification; each result divided by its own 2-norm"""
    tmp, phi, path = scan
    args = ["--basis", phi, "-i", "8"] + COMMON + [path]
    plain = _pics(oracle_backend, ["--debug", "40"] + args)
    with caplog.at_level(logging.INFO):
        toep = _pics(oracle_backend, ["--toeplitz"] + args)
    assert toep.shape == plain.shape == (16, 16, 8, 1, 1, 1, 2)
    msgs = [r.getMessage() for r in caplog.records]
    assert not any("scratch arena too small" in m for m in msgs), msgs
    assert any("ToeplitzNormal" in m for m in msgs) and any("kernel of 2 x 2 point-spread functions" in m for m in msgs), msgs
    err = _rel(toep / np.linalg.norm(toep), plain / np.linalg.norm(plain))
    print("pics --basis --toeplitz against --basis: relative difference %.3e, bar %.3e" % (err, 10 * accuracy[0]))
    assert err < 10 * accuracy[0], (err, accuracy)


@pytest.mark.parametrize("extra", [["--llr", "0.02", "--llr-block", "6"], ["--tv", "0.01"], ["--l1", "0.01", "--levels", "2"]],
                         ids=["llr", "tv", "l1"])
def test_every_regulariser_runs_on_the_toeplitz_operator(scan, oracle_backend, caplog, extra):
    tmp, phi, path = scan
    with caplog.at_level(logging.INFO):
        out = _pics(oracle_backend, ["--toeplitz", "--basis", phi, "-i", "12"] + extra + COMMON + [path])
    assert out.shape == (16, 16, 8, 1, 1, 1, 2) and np.isfinite(out).all() and np.abs(out).max() > 0
    msgs = [r.getMessage() for r in caplog.records]
    assert not any("scratch arena too small" in m for m in msgs), msgs
    obj = [float(m.group(1)) for s in msgs for m in [re.search(r"iter \d+, objective (\S+)", s)] if m]
    assert len(obj) == 2 and obj[-1] < obj[0], obj


def test_frames_without_a_basis_and_one_frame(scan, oracle_backend, accuracy, caplog):
    tmp, phi, path = scan
    with caplog.at_level(logging.INFO):
        frames = _pics(oracle_backend, ["--toeplitz", "-i", "3"] + COMMON + [path])
        one = _pics(oracle_backend, ["--toeplitz", "-i", "3", "--crop", "TIME:1"] + COMMON + [path])
        tvt = _pics(oracle_backend, ["--toeplitz", "-i", "3", "--tv-time", "0.01"] + COMMON + [path])
    assert frames.shape == tvt.shape == (16, 16, 8) + (1,) * 7 + (4,) and one.shape[:3] == (16, 16, 8)
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in (frames, one, tvt))
    msgs = [r.getMessage() for r in caplog.records]
    assert not any("scratch arena too small" in m for m in msgs), msgs
    assert sum("kernel of 1 x 1 point-spread functions" in m for m in msgs) == 4 + 1 + 4, msgs
    # one frame with --toeplitz against the gridding operator, 3 CG iterations: the bar of the --basis comparison
    plain = _pics(oracle_backend, ["-i", "3", "--crop", "TIME:1", "--debug", "40"] + COMMON + [path])
    assert _rel(one / np.linalg.norm(one), plain / np.linalg.norm(plain)) < 10 * accuracy[0]


def test_nine_coefficients_are_refused(scan, oracle_backend, capsys):
    tmp, phi, path = scan
    nine = os.path.join(tmp, "nine.npy")
    np.save(nine, np.ones((4, 9)))
    with pytest.raises(ValueError, match="9 coefficients, at most 8"):
        _pics(oracle_backend, ["--toeplitz", "--basis", nine, "-i", "1", "--debug", "40"] + COMMON + [path])
    with pytest.raises(SystemExit):
        pics.parse(["--toeplitz", "--basis", nine, "--basis-rank", "9", path])
    assert "at most 8 coefficient images" in capsys.readouterr().err
    with pytest.raises(ValueError, match="at most 8 are supported"):
        psf_kernel(oracle_backend, (4, 4, 4), [np.zeros((3, 5, 1))], [0] * 9, np.ones((9, 9)), 2, 2.0)


def test_parser_and_the_default_run(scan, oracle_backend, monkeypatch):
    tmp, phi, path = scan
    assert pics.parse(["--toeplitz", path]).toeplitz is True and pics.parse([path]).toeplitz is False

    def refuse(*args, **kwargs):
        raise AssertionError("a run without --toeplitz constructs no ToeplitzNormal")
    monkeypatch.setattr(type(oracle_backend), "ToeplitzNormal", refuse, raising=False)
    out = _pics(oracle_backend, ["--basis", phi, "-i", "1", "--debug", "40"] + COMMON + [path])
    assert out.shape == (16, 16, 8, 1, 1, 1, 2)
    with pytest.raises(AssertionError, match="constructs no ToeplitzNormal"):
        _pics(oracle_backend, ["--toeplitz", "--basis", phi, "-i", "1", "--debug", "40"] + COMMON + [path])
