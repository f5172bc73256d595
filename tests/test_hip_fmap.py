"""The off-resonance kernels and pics --fmap on the MI355X: ig_fmap_phase_c64 and ig_fmap_combine_c64 against the float64
restatement in tests/fmap64.py, operators.SegmentPhase / SegmentCombine inside a product, and the driver against the same driver
on the numpy oracle backend."""
import ctypes
import logging
import re

import numpy as np
import pytest

import fmap64
from indigo_amd import pics
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
TOL = 1e-5          # the project's bar on the relative 2-norm; the phase is good to 2e-7 rad, the sums have at most 16 terms
ALPHA, BETA = 0.7 - 0.3j, 0.5 + 0.25j
PAD = 37

NS = (1, 105, 2048, 5049)                       # one row; 5 * 7 * 3; whole workgroups; 33 * 17 * 9: several workgroups and a tail
LS = (1, 2, 3, 8, 9, 16)                        # one segment, both sides of the unroll factors, and the limit
CYCLES = (0.3, 5.0, 50.0)                       # max|f tau|: below one cycle, a few, and where a float32 product is 1e-5 rad off

# every (n, L) once, with the field's span and the table's period rotating, and the corner that the rotation may miss
CASES = [(n, L, (i + j) % 3) for i, L in enumerate(LS) for j, n in enumerate(NS)]
CASES += [c for c in [(5049, 16, 2), (2048, 16, 2)] if c not in CASES]


def _periods(n):
    return [P for P in (1, 7, n) if n % P == 0]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _bits(a):
    """the bit patterns of a complex64 array (NaN payloads included), whatever its memory order"""
    return np.ascontiguousarray(a).view(np.uint32)


def _padded(hip, a, pad):
    """the panel a on the device with `pad` extra rows of NaN under every column, and the host copy"""
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _run(call, hip, n, x, y, pad):
    """call(y_d, x_d) on panels with `pad` NaN rows under every column of x and y, which must come back bit-identical"""
    x_d, xp = _padded(hip, x, pad)
    y_d, yp = _padded(hip, y, pad)
    call(y_d[:n], x_d[:n])
    out = y_d.to_host()
    assert np.array_equal(_bits(x_d.to_host()), _bits(xp))
    assert np.array_equal(_bits(out[n:]), _bits(yp[n:]))
    return out[:n]


def _taus(L):
    return 2e-3 + 1.5e-3 * np.arange(L), 2e-3, 1.5e-3


def _field(n, cycles, taus, seed):
    """n float32 field values with max|f tau| = cycles"""
    f = np.random.default_rng(seed).uniform(-1, 1, n)
    return (f * (cycles / (np.abs(f).max() * np.abs(taus).max()))).astype(np.float32)


def _phase_call(hip, f_d, L, n, adjoint, alpha, beta):
    _, tau0, dtau = _taus(L)
    return lambda y_d, x_d: hip.segment_phase(y_d, x_d, f_d, tau0, dtau, L, n, adjoint=adjoint, alpha=alpha, beta=beta)


def _combine_call(hip, b_d, P, n, adjoint, alpha, beta):
    return lambda y_d, x_d: hip.segment_combine(y_d, x_d, b_d, P, n, adjoint=adjoint, alpha=alpha, beta=beta)


WORST = {"phase": 0.0, "combine": 0.0}


@pytest.mark.parametrize("n,L,rot", CASES, ids=lambda v: str(v))
def test_kernels_match_the_float64_restatement(hip, n, L, rot):
    taus = _taus(L)[0]
    f = _field(n, CYCLES[rot], taus, seed=n + L)
    f_d = hip.copy_array(f)
    periods = _periods(n)
    P = periods[rot % len(periods)]
    table = rand64c(P, L, seed=L * 100 + P)
    b_d, _ = _padded(hip, table, 3)                                       # ldb = P + 3, the padding NaN
    for adjoint in (False, True):
        for which in ("phase", "combine"):
            wide_x = adjoint == (which == "phase")                         # the side with L columns
            x, y = rand64c(n, L if wide_x else 1, seed=n + 1), rand64c(n, 1 if wide_x else L, seed=n + 2)
            for beta, y0 in ((0, np.full_like(y, np.nan)), (BETA, y)):
                if which == "phase":
                    got = _run(_phase_call(hip, f_d, L, n, adjoint, ALPHA, beta), hip, n, x, y0, PAD)
                    want = fmap64.phase(f, taus, x, y, adjoint, ALPHA, beta)
                else:
                    got = _run(_combine_call(hip, b_d[:P], P, n, adjoint, ALPHA, beta), hip, n, x, y0, PAD)
                    want = fmap64.combine(table, P, x, y, adjoint, ALPHA, beta)
                err = _rel(got, want)
                WORST[which] = max(WORST[which], err)
                assert np.isfinite(got).all() and err < TOL, (which, adjoint, beta, err)
    print("n %d L %d, %g cycles, period %d: worst relative error so far, phase %.3e, combine %.3e"
          % (n, L, CYCLES[rot], P, WORST["phase"], WORST["combine"]))


@pytest.mark.parametrize("n,L,P", [(2048, 3, 1), (2048, 16, 2048), (5049, 9, 17), (105, 8, 7)], ids=lambda v: str(v))
def test_layout_forms_give_the_same_bits(hip, n, L, P):
    """the stacked vectors, the plain panels (both with 16-byte accesses when n is even) and panels with an odd leading
    dimension (8-byte accesses) hold the same bits"""
    taus = _taus(L)[0]
    f_d = hip.copy_array(_field(n, 5.0, taus, seed=3))
    b_d = hip.copy_array(rand64c(P, L, seed=4))
    for adjoint in (False, True):
        for which in ("phase", "combine"):
            wide_x = adjoint == (which == "phase")
            x, y = rand64c(n, L if wide_x else 1, seed=5), rand64c(n, 1 if wide_x else L, seed=6)
            call = (_phase_call(hip, f_d, L, n, adjoint, ALPHA, BETA) if which == "phase"
                    else _combine_call(hip, b_d, P, n, adjoint, ALPHA, BETA))
            outs = [_run(call, hip, n, x, y, pad) for pad in (PAD, 0, 2)]
            xs, ys = (hip.copy_array(np.asfortranarray(a.reshape((-1, 1), order='F'))) for a in (x, y))
            call(ys, xs)
            outs.append(ys.to_host().reshape(y.shape, order='F'))
            for o in outs[1:]:
                assert np.array_equal(_bits(o), _bits(outs[0])), (which, adjoint)


def test_adjointness_on_the_device(hip):
    n, L, P = 5049, 5, 17
    taus, tau0, dtau = _taus(L)
    f_d = hip.copy_array(_field(n, 5.0, taus, seed=6))
    b_d = hip.copy_array(rand64c(P, L, seed=7))
    x, z = rand64c(n, 1, seed=8), rand64c(n, L, seed=9)
    for fwd, adj in (((lambda y_d, x_d: hip.segment_phase(y_d, x_d, f_d, tau0, dtau, L, n)),
                      (lambda y_d, x_d: hip.segment_phase(y_d, x_d, f_d, tau0, dtau, L, n, adjoint=True))),
                     ((lambda y_d, x_d: hip.segment_combine(y_d, x_d, b_d, P, n, adjoint=True)),       # (n -> n x L is Combine^H)
                      (lambda y_d, x_d: hip.segment_combine(y_d, x_d, b_d, P, n)))):
        px, phz = hip.zero_array((n, L), C64), hip.zero_array((n, 1), C64)
        fwd(px, hip.copy_array(x))
        adj(phz, hip.copy_array(z))
        lhs = np.vdot(z.astype(np.complex128), px.to_host().astype(np.complex128))
        rhs = np.vdot(phz.to_host().astype(np.complex128), x.astype(np.complex128))
        assert abs(lhs - rhs) < 1e-5 * abs(lhs), (lhs, rhs)


def test_limits(hip):
    n, P = 64, 8
    f = _field(n, 5.0, _taus(16)[0], seed=1)
    f_d = hip.copy_array(f)
    x = rand64c(n, 1, seed=2)
    x_d, y17 = hip.copy_array(x), hip.copy_array(rand64c(n, 17, seed=3))
    before = y17.to_host()
    with pytest.raises(RuntimeError, match="17 segments"):
        hip.segment_phase(y17, x_d, f_d, 2e-3, 1.5e-3, 17, n)
    with pytest.raises(RuntimeError, match="17 segments"):
        hip.segment_combine(y17, x_d, hip.copy_array(rand64c(P, 17, seed=4)), P, n, adjoint=True)
    assert np.array_equal(y17.to_host(), before)
    y1 = hip.copy_array(x)
    with pytest.raises(RuntimeError, match="17 segments"):
        hip.segment_phase(y1, y17, f_d, 2e-3, 1.5e-3, 17, n, adjoint=True)
    assert np.array_equal(y1.to_host(), x)
    y16 = hip.zero_array((n, 16), C64)                                    # the limit itself is served
    hip.segment_phase(y16, x_d, f_d, 2e-3, 1.5e-3, 16, n)
    assert _rel(y16.to_host(), fmap64.phase(f, _taus(16)[0], x)) < TOL
    table = rand64c(P, 16, seed=5)
    hip.segment_combine(y16, x_d, hip.copy_array(table), P, n, adjoint=True)
    assert _rel(y16.to_host(), fmap64.combine(table, P, x, adjoint=True)) < TOL
    before = y16.to_host()
    with pytest.raises(RuntimeError, match="no multiple of the table's period 7"):
        hip.segment_combine(y16, x_d, hip.copy_array(rand64c(7, 16, seed=6)), 7, n, adjoint=True)
    assert np.array_equal(y16.to_host(), before)


def test_overlapping_panels_raise(hip):
    n, L, P = 64, 3, 8
    # complex64 elements: y may start anywhere; x = [192, 256); b = [520, 544); f (64 floats) = [560, 592)
    host = rand64c(600, 1, seed=9)
    host[560:592] = np.linspace(-300, 300, 64).astype(np.float32).view(C64).reshape((-1, 1))
    buf = hip.copy_array(host)

    def at(off):
        return ctypes.c_void_p(buf._arr + 8 * off)

    def phase(y_off):
        return hip._L.ig_fmap_phase_c64(hip._ctx, n, L, at(560), ctypes.c_double(2e-3), ctypes.c_double(1.5e-3), 0, at(192), n,
                                        1.0, 0.0, 0.0, 0.0, at(y_off), n)

    def combine(y_off):
        return hip._L.ig_fmap_combine_c64(hip._ctx, n, L, P, at(520), P, 1, at(192), n, 1.0, 0.0, 0.0, 0.0, at(y_off), n)
    for off in (1, 255, 200, 400, 591):          # x's first element, its last, inside it; f's first float, its last
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(phase(off), "ig_fmap_phase_c64")
    for off in (1, 255, 200, 329, 543):          # x's first element, its last, inside it; b's first element, its last
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(combine(off), "ig_fmap_combine_c64")
    assert np.array_equal(_bits(buf.to_host()), _bits(host))
    f = np.ascontiguousarray(host[560:592, 0]).view(np.float32)
    for call, want in ((phase, fmap64.phase(f, _taus(L)[0], host[192:256, 0])),
                       (combine, fmap64.combine(host[520:544, 0].reshape((P, L), order='F'), P, host[192:256, 0], adjoint=True))):
        hip._check(call(0), call.__name__)                                 # adjacent to x, not overlapping
        after = buf.to_host()
        assert np.array_equal(_bits(after[192:]), _bits(host[192:]))
        assert _rel(after[:192, 0].reshape((n, L), order='F'), want) < TOL


def test_the_operators_inside_a_product(hip):
    n, L, P = 105, 3, 7
    taus = np.linspace(1e-3, 6e-3, L)
    f = _field(n, 5.0, taus, seed=10)
    table = rand64c(P, L, seed=11)
    d = rand64c(n, 1, seed=12)
    A = hip.SegmentCombine(table, P, n) * hip.BlockDiag([hip.Diag(d)] * L) * hip.SegmentPhase(f, taus, n)
    assert A.shape == (n, n) and A.H.shape == (n, n)
    x = rand64c(n, 1, seed=20)
    want = fmap64.combine(table, P, fmap64.phase(f, taus, x) * d.astype(np.complex128))
    assert _rel(A * x, want) < TOL
    z = rand64c(n, 1, seed=21)
    want = fmap64.phase(f, taus, fmap64.combine(table, P, z, adjoint=True) * np.conj(d.astype(np.complex128)), adjoint=True)
    assert _rel(A.H * z, want) < TOL


@pytest.fixture(scope="module")
def scan(tmp_path_factory, hip, oracle_backend):
    """32^3, 2 coils, a smooth field map of 2 cycles span over an 8 ms readout.  Regularisation as in tests/test_hip_softsense.py:
    complex64 iterates of two realisations of one operator drift apart by about (condition number) x (their 5e-7 rounding
    difference) per iteration, and a radial scan without density compensation has eigenvalues from the largest down to zero; with
    the project's bars of 1e-5 after one iteration and 1e-4 after ten the comparison runs at lamda = a tenth of the largest
    eigenvalue of A^H A (the oracle's power iteration at lamda = 0, from which the proximal solvers also take their step), i.e. a
    condition number of eleven.  (At lamda = 1e-3 the two backends are 5.3e-07 apart after one CG iteration and 3.4e-03 after ten.)"""
    tmp = tmp_path_factory.mktemp("fmap_scan")
    N, nro = (32, 32, 32), 64
    times = 1e-3 + np.arange(nro) * (8e-3 / (nro - 1))
    path, fmap, tpath = fmap64.fmap_scan(tmp, hip, N, fmap64.smooth_field(N, 250.0, seed=3), times, nro=nro, nsp=100, osf=2.0, width=2)
    opts = ["--fmap", fmap, "--times", tpath, "--osf", "2.0", "--width", "2"]
    handler_records = []

    class Keep(logging.Handler):
        def emit(self, record):
            handler_records.append(record.getMessage())
    keep = Keep(level=logging.INFO)
    plog = logging.getLogger("pics")
    old = plog.level
    plog.addHandler(keep)
    plog.setLevel(logging.INFO)
    try:
        pics.main(["-i", "0", "--power-iters", "6", "--no-fuse", "--l1", "0.01", "--debug", "40", "--lamda", "0"] + opts + [path],
                  backend=oracle_backend)
    finally:
        plog.removeHandler(keep)
        plog.setLevel(old)
    oracle_backend._scratch = None
    est = [float(m.group(1)) for s in handler_records for m in [re.search(r"largest eigenvalue of A\^H A \+ lamda I (\S+)", s)] if m][0]
    return opts + ["--lamda", "%.8e" % (est / 10), path], ["--step", "%.8e" % (0.9 / (1.1 * est))]


# (CG chooses the segments itself, 8 of them here; the proximal solvers fix 4 and the Toeplitz form 2 to keep the oracle's side short: the
# Toeplitz form sets up L (L + 1) / 2 point-spread functions on the doubled grid)
@pytest.mark.parametrize("extra", [[], ["--l1", "0.01", "--fmap-segments", "4"], ["--tv", "0.01", "--fmap-segments", "4"],
                                   ["--toeplitz", "--fmap-segments", "2"]], ids=["cg", "l1", "tv", "toeplitz"])
def test_pics_fmap_on_the_gpu_matches_the_oracle_backend(scan, hip, oracle_backend, caplog, extra):
    args, step = scan
    with caplog.at_level(logging.WARNING):
        for iters, tol in (("1", 1e-5), ("10", 1e-4)):
            argv = extra + ["-i", iters, "--debug", "40"] + (step if extra and extra[0] != "--toeplitz" else []) + args
            out = pics.main(argv, backend=hip)
            ref = pics.main(["--no-fuse"] + argv, backend=oracle_backend)
            oracle_backend._scratch = None
            assert out.shape == (32, 32, 32, 1)
            print("pics --fmap %s, %s iterations: relative difference %.3e" % (extra, iters, _rel(out, ref)))
            assert _rel(out, ref) < tol, (extra, iters, _rel(out, ref))
    assert not any("scratch arena too small" in r.getMessage() for r in caplog.records)
