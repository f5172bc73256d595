"""pics --l1 on the CPU: the float64 wavelet restatement (tests/dwt64.py) against its definition, the coarse-box rule, the host
forms of Backend.dwt3 / soft_threshold, operators.Wavelet, Backend.fista against a plain numpy FISTA, and the driver against a
float64 FISTA on the dense matrix of the same operator -- all on the numpy oracle backend."""
import logging
import os

import numpy as np
import pytest

import dwt64
import dwt_cases
from conftest import check_misc_leaves
from indigo_amd import pics
from indigo_amd.backends.backend import WAVELETS, dwt_coarse_box, dwt_plan
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
SHAPES = [(16, 8, 1), (12, 10, 3), (16, 6, 5), (9, 16, 4)]


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


@pytest.mark.parametrize("wavelet", ["haar", "db2", "db4"])
def test_filters_from_the_spectral_factorisation(wavelet):
    h = dwt64.daubechies(dwt64.TAPS[wavelet])
    assert np.abs(h - np.array(WAVELETS[wavelet])).max() < 1e-12
    # orthogonality of the filter to its even shifts and vanishing moments of the high-pass filter
    g = dwt64.highpass(h)
    for s in range(0, h.size, 2):
        assert abs(np.dot(h[s:], h[:h.size - s]) - (s == 0)) < 1e-12
    for p in range(h.size // 2):
        assert abs(np.dot(g, np.arange(h.size) ** p)) < 1e-9


@pytest.mark.parametrize("wavelet", ["haar", "db2", "db4"])
@pytest.mark.parametrize("dims", SHAPES)
def test_float64_transform_is_orthogonal(wavelet, dims):
    W = dwt64.dense(dims, wavelet, 3)
    assert np.abs(W @ W.T - np.eye(W.shape[0])).max() < 1e-12
    x = np.random.default_rng(1).standard_normal(W.shape[0])
    np.testing.assert_allclose(dwt64.dwt(x, dims, wavelet, 3, inverse=True), W.T @ x, atol=1e-12)


def test_coarse_box_rule():
    assert dwt_coarse_box((480, 208, 308), 'db4', 3) == (60, 26, 77)
    assert dwt_coarse_box((480, 208, 308), 'db4', 5) == (15, 13, 77)
    assert dwt_coarse_box((64, 48, 1), 'db2', 3) == (8, 6, 1)              # 2-D: the third axis never splits
    assert dwt_coarse_box((8, 8, 8), 'haar', 9) == (2, 2, 2)                # stops after two levels, no error
    for dims in SHAPES + [(480, 208, 308), (8, 8, 8)]:
        for w in WAVELETS:
            for levels in (1, 3, 5, 9):
                assert dwt_coarse_box(dims, w, levels) == dwt64.coarse_box(dims, w, levels)


@pytest.mark.parametrize("wavelet", ["haar", "db2", "db4"])
def test_host_forms_match_the_float64_transform(oracle_backend, wavelet):
    B = oracle_backend
    for dims in SHAPES + [(32, 24, 40)]:
        for levels in (1, 3, 5):
            n = int(np.prod(dims))
            x = rand64c(n, 2, seed=levels) - (0.5 + 0.5j)
            y0 = rand64c(n, 2, seed=9)
            for inverse in (False, True):
                ref = dwt64.dwt(x, dims, wavelet, levels, inverse=inverse)
                y = B.copy_array(np.full((n, 2), np.nan, dtype=C64, order='F'))
                B.dwt3(y, B.copy_array(x), dims, wavelet, levels, inverse=inverse)
                assert _rel(y.to_host(), ref) < 1e-6
                y = B.copy_array(y0)
                B.dwt3(y, B.copy_array(x), dims, wavelet, levels, inverse=inverse, alpha=0.5j, beta=2 - 1j)
                assert _rel(y.to_host(), 0.5j * ref + (2 - 1j) * y0) < 1e-6


def test_host_soft_threshold(oracle_backend):
    dims, tau = (16, 20, 7), np.float32(0.25)
    keep = dwt64.coarse_box(dims, 'db2', 2)                # (4, 5, 7): the rows below lie outside it
    n = int(np.prod(dims))
    u = (rand64c(n, 2, seed=3) - (0.5 + 0.5j)).astype(C64)
    u[-80:-50, 0] = 0
    u[-40:-20, 0] = tau
    u[-20:, 1] = 1j * tau
    u_d = oracle_backend.copy_array(u)
    oracle_backend.soft_threshold(u_d, tau, dims, keep)
    out = u_d.to_host().reshape(dims + (2,), order='F')
    ref = dwt64.soft(u, tau, dims, keep).reshape(dims + (2,), order='F')
    vol = u.reshape(dims + (2,), order='F')
    box = tuple(slice(0, c) for c in keep)
    assert np.array_equal(out[box], vol[box])
    zero = np.abs(ref) == 0
    assert zero.sum() > 100 and np.all(out[zero] == 0)
    assert out.reshape((n, 2), order='F')[-40:-20, 0].tolist() == [0] * 20
    assert np.abs(out - ref).max() < 1e-6


def test_wavelet_operator(oracle_backend):
    B = oracle_backend
    dims = (16, 20, 7)
    W = B.Wavelet(dims, wavelet='db4', levels=3)
    assert W.shape == (16 * 20 * 7,) * 2 and W.coarse == dwt64.coarse_box(dims, 'db4', 3)
    x = rand64c(W.shape[1], 2, seed=4)
    np.testing.assert_allclose(W.H * (W * x), x, atol=1e-6)
    np.testing.assert_allclose(W * x, dwt64.dwt(x, dims, 'db4', 3), atol=1e-6)
    with pytest.raises(ValueError):
        B.Wavelet((1025, 4, 4))
    with pytest.raises(ValueError):
        B.Wavelet((16, 16, 16), wavelet='db8')


def test_fista_reproduces_a_numpy_loop(oracle_backend):
    B = oracle_backend
    rng = np.random.default_rng(2)
    M = (rng.standard_normal((40, 24)) + 1j * rng.standard_normal((40, 24))).astype(C64)
    b = (rng.standard_normal((40, 1)) + 1j * rng.standard_normal((40, 1))).astype(C64)
    A = B.DenseMatrix(M)
    AH_b = B.copy_array(np.asfortranarray(M.conj().T @ b))
    tmp = B.zero_array((40, 1), C64)

    def gradf(g, z):                                  # grad of 1/2 ||M z - b||^2
        A.eval(tmp, z)
        A.H.eval(g, tmp)
        B.axpby(1, g, -1, AH_b)

    def proxg(v, alpha):                              # prox of 0.3 ||v||_1 (complex soft threshold, no box kept)
        B.soft_threshold(v, alpha * 0.3, (24, 1, 1), (0, 0, 0))

    step = 0.9 / np.linalg.norm(M.astype(np.complex128), 2) ** 2
    seen = []
    x0 = rand64c(24, 1, seed=1)
    x = x0.copy(order='F')
    B.fista(gradf, proxg, step, x, maxiter=12, callback=lambda k, xk: seen.append(xk.to_host().copy()))
    # the same iteration in numpy, complex128
    Md = M.astype(np.complex128)

    def soft(v, t):
        r = np.abs(v)
        return np.where(r <= t, 0, v * (1 - t / np.maximum(r, 1e-300)))
    xk = zk = x0.astype(np.complex128)
    t = 1.0
    for k in range(12):
        xn = soft(zk - step * (Md.conj().T @ (Md @ zk - b)), step * 0.3)
        tn = (1 + np.sqrt(1 + 4 * t * t)) / 2
        zk = xn + (t - 1) / tn * (xn - xk)
        xk, t = xn, tn
        assert _rel(seen[k], xk) < 1e-5, k
    assert _rel(x, xk) < 1e-5
    # and the proximal-gradient iteration with the reference's constant momentum is still what the golden vectors hold
    check_misc_leaves(B, 1e-5)


def test_pics_parses_the_l1_options():
    a = pics.parse(["--l1", "0.01", "--wavelet", "db4", "--levels", "4", "--power-iters", "7", "--step", "0.5", "x.npz"])
    assert (a.l1, a.wavelet, a.levels, a.power_iters, a.step, a.data) == (0.01, "db4", 4, 7, 0.5, "x.npz")
    a = pics.parse(["x.npz"])
    assert (a.l1, a.wavelet, a.levels, a.power_iters, a.step) == (0, "db2", 3, 15, None)
    with pytest.raises(SystemExit):
        pics.parse(["--wavelet", "sym4", "x.npz"])


@pytest.fixture(scope="module")
def scan16(tmp_path_factory, oracle_backend):
    N, C, nro, nsp, osf = (16, 16, 16), 2, 16, 30, 1.5
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    img = (np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + g[2] ** 2)) * (1 + 0.3j)).astype(C64)
    img[(np.abs(g[0]) < 0.4) & (np.abs(g[1]) < 0.3)] += 0.5
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph)
                    for cx, cy, ph in [(-1, 0, 0.3), (1, 0.5, -0.4)]], axis=3).astype(C64)
    coord = radial_trajectory(nsp, nro, seed=2)
    traj = coord * np.array(N, dtype=np.float64)[:, None, None]
    B = oracle_backend
    B._scratch = None
    F1 = B.NUFFT((1, nro, nsp), N, coord, width=3, oversamp=(osf,) * 3, dtype=C64)
    A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
    ksp = (A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F')
    # the operator's dense matrix, through its adjoint (fewer rows than columns), a block of rows at a time
    m = A.shape[0]
    AdH = np.concatenate([A.H * np.asfortranarray(np.eye(m, dtype=C64)[:, j:j + 480]) for j in range(0, m, 480)], axis=1)
    Ad = AdH.conj().T
    B._scratch = None
    path = os.path.join(str(tmp_path_factory.mktemp("scan16")), "scan.npz")
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path, N, ksp, Ad.astype(np.complex128)


def test_pics_l1_zero_is_the_cg_driver(scan16, oracle_backend):
    path, N, _, _ = scan16
    args = ["-i", "4", "--osf", "1.5", "--lamda", "1e-3", "--debug", "40", path]
    oracle_backend._scratch = None
    a = pics.main(args, backend=oracle_backend)
    oracle_backend._scratch = None
    b = pics.main(["--l1", "0"] + args, backend=oracle_backend)
    oracle_backend._scratch = None
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_pics_l1_matches_a_float64_fista(scan16, oracle_backend, caplog):
    path, N, ksp, Ad = scan16
    lamda, l1, iters = 1e-3, 0.2, 10
    y = ksp.reshape(-1, order='F').astype(np.complex128)
    AHy = Ad.conj().T @ y
    b = AHy / np.abs(AHy).max()
    AHA = Ad.conj().T @ Ad + lamda * np.eye(Ad.shape[1])
    lam = np.linalg.eigvalsh(AHA)[-1]
    step = 0.9 / lam
    keep = dwt64.coarse_box(N, 'db2', 3)
    x = z = np.zeros_like(b)
    t = 1.0
    for _ in range(iters):
        v = z - step * (AHA @ z - b)
        xn = dwt64.dwt(dwt64.soft(dwt64.dwt(v, N, 'db2', 3), step * l1, N, keep), N, 'db2', 3, inverse=True)
        tn = (1 + np.sqrt(1 + 4 * t * t)) / 2
        z = xn + (t - 1) / tn * (xn - x)
        x, t = xn, tn
    W = dwt64.dwt(x, N, 'db2', 3).reshape(N, order='F')
    inside = np.zeros(N, dtype=bool)
    inside[tuple(slice(0, c) for c in keep)] = True
    assert (abs(W[~inside]) < 1e-12).mean() > 0.3        # the threshold is doing something
    oracle_backend._scratch = None
    with caplog.at_level(logging.INFO, logger="pics"):
        out = pics.main(["-i", str(iters), "--osf", "1.5", "--lamda", str(lamda), "--l1", str(l1), "--step", "%.12e" % step,
                         "--debug", "40", path], backend=oracle_backend)
    oracle_backend._scratch = None
    assert out.shape == N + (1, 1)
    assert _rel(out.reshape(-1, order='F'), x) < 1e-4, _rel(out.reshape(-1, order='F'), x)
    # the logged objective is the float64 one of the same iterate
    logged = [r.getMessage() for r in caplog.records if "objective" in r.getMessage()]
    assert logged and logged[-1].startswith("fista iter %d" % iters)
    obj = 0.5 * np.linalg.norm(Ad @ x - y / np.abs(AHy).max()) ** 2 + 0.5 * lamda * np.linalg.norm(x) ** 2 + l1 * np.abs(W[~inside]).sum()
    assert abs(float(logged[-1].split()[-1]) - obj) < 1e-4 * abs(obj)
    # the power iteration finds the largest eigenvalue of A^H A + lamda I
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="pics"):
        pics.main(["-i", "0", "--osf", "1.5", "--lamda", str(lamda), "--l1", str(l1), "--power-iters", "40", "--debug", "40",
                   path], backend=oracle_backend)
    oracle_backend._scratch = None
    est = [r.getMessage() for r in caplog.records if "largest eigenvalue" in r.getMessage()]
    assert est and abs(float(est[0].split("lamda I ")[1].split()[0]) - lam) < 1e-2 * lam


# ---- the case table of the GPU tests (tests/dwt_cases.py) and the elementwise bound they use (dwt64.dwt_bound) ----------------

def test_the_case_table_reaches_what_it_claims():
    """from dwt64.passes: the empty plans, the first passes on another axis than 0, the strips above 64 KB of LDS and the lines of
    every pass's last group"""
    geo = {dwt_cases.case_id(c): dwt_cases.launches(*c) for c in dwt_cases.CASES}
    assert len(geo) == len(dwt_cases.CASES)                                # the ids are distinct
    assert sorted(k for k, g in geo.items() if not g) == ["16x16x16_db2_0", "2x2x2_haar_1", "7x9x5_db2_3"]
    first = {k: g[0][0] for k, g in geo.items() if g}
    assert {k: a for k, a in first.items() if a != 0} == {"9x16x4_db2_3": 1, "1x1x64_db4_5": 2, "12x16x3_db4_2": 1,
                                                          "41x4x6_haar_2": 1, "5x4x1024_db4_9": 2}
    # (axis, d, LDS bytes) of every pass that has to ask for more than 64 KB: 65 536 itself (d = 512) does not
    big = {k: [(a, d, lds) for a, d, _, _, _, lds, _ in g if lds > dwt_cases.LDS_DEFAULT] for k, g in geo.items()}
    assert {k: v for k, v in big.items() if v} == {"20x640x3_db4_2": [(1, 640, 81920)], "5x4x1024_db4_9": [(2, 1024, 131072)]}
    assert (2, 512, 65536) in [(a, d, lds) for a, d, _, _, _, lds, _ in geo["5x4x1024_db4_9"]]
    assert max(lds for g in geo.values() for *_, lds, _ in g) <= 160 * 1024
    # passes, and for each (axis, lines P, lines of the last group)
    lines = {k: [(a, P, last) for a, _, P, _, _, _, last in g] for k, g in geo.items()}
    assert lines["9x16x4_db2_3"] == [(1, 9, 9), (1, 9, 9)]
    assert lines["12x10x3_haar_3"] == [(0, 10, 10), (1, 6, 6), (0, 5, 5)]
    assert lines["16x8x1_db2_3"] == [(0, 8, 8), (1, 8, 8), (0, 4, 4)]
    assert lines["1x1x64_db4_5"] == [(2, 1, 1)] * 3 and dwt64.coarse_box((1, 1, 64), "db4", 5) == (1, 1, 8)
    assert lines["40x6x34_haar_2"] == [(0, 6, 6), (1, 20, 4), (2, 20, 4), (0, 3, 3)]
    assert dwt64.coarse_box((40, 6, 34), "haar", 2) == (10, 3, 17)
    assert lines["12x16x3_db4_2"] == [(1, 12, 12)]
    assert lines["41x4x6_haar_2"] == [(1, 41, 9), (2, 41, 9)]
    assert lines["48x20x24_db4_3"] == [(0, 20, 4), (1, 24, 8), (2, 24, 8), (0, 10, 10)]
    assert lines["20x640x3_db4_2"] == [(0, 640, 16), (1, 10, 10), (1, 10, 10)]
    assert lines["5x4x1024_db4_9"] == [(2, 5, 5)] * 7
    assert lines["1024x4x2_db2_9"] == [(0, 4, 4)] * 8 and geo["1024x4x2_db2_9"][0][4] == 4      # W = 4 lines at d = 1024
    dims, wavelet, levels, ncols = dwt_cases.MANY_COLUMNS
    assert ncols > 65535 and len(dwt64.passes(dims, wavelet, levels)[0]) == 3
    for dims, wavelet, levels in dwt_cases.CASES:                          # the product's plan is the restatement's
        assert dwt_plan(dims, wavelet, levels) == dwt64.passes(dims, wavelet, levels)


@pytest.mark.parametrize("case", dwt_cases.CASES, ids=dwt_cases.case_id)
def test_host_forms_match_the_float64_transform_on_the_case_table(oracle_backend, case):
    B = oracle_backend
    dims, wavelet, levels = case
    n = int(np.prod(dims))
    x, y0 = dwt_cases.make_input(dims, 2, seed=1), dwt_cases.make_input(dims, 2, seed=9)
    for inverse in (False, True):
        ref = dwt64.dwt(x, dims, wavelet, levels, inverse=inverse)
        y = B.copy_array(np.full((n, 2), np.nan, dtype=C64, order='F'))
        B.dwt3(y, B.copy_array(x), dims, wavelet, levels, inverse=inverse)
        assert _rel(y.to_host(), ref) < 1e-6
        y = B.copy_array(y0)
        B.dwt3(y, B.copy_array(x), dims, wavelet, levels, inverse=inverse, alpha=0.5j, beta=2 - 1j)
        assert _rel(y.to_host(), 0.5j * ref + (2 - 1j) * y0) < 1e-6


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64, and the one rounding of the sum to float64 before the rounding
    to float32 changes the result in no case that matters here"""
    return _f32(np.float64(a) * np.float64(b) + np.float64(c))


def _cmul32(a, vr, vi):
    """ig_common.h's cmul(a, v): (fma(a.x, v.x, -(a.y v.y)), fma(a.x, v.y, a.y v.x))"""
    ar, ai = np.float32(a.real), np.float32(a.imag)
    return _fma(ar, vr, -(ai * vi)), _fma(ar, vi, ai * vr)


def _emulate_split(v, h, inverse):
    """one split along axis 0 of the float32 array v, tap by tap in the order of k_dwt_lines"""
    taps, d = h.size, v.shape[0]
    half = d // 2
    g = _f32([(-1.0 if j & 1 else 1.0) * h[taps - 1 - j] for j in range(taps)])
    out = np.zeros_like(v)
    k = np.arange(half)
    if not inverse:
        for t in range(taps):
            src = v[(2 * k + t) % d]
            out[:half] = _fma(h[t], src, out[:half])
            out[half:] = _fma(g[t], src, out[half:])
    else:
        for t in range(taps // 2):
            m = (k - t) % half
            lo, hi = v[m], v[half + m]
            for r in (0, 1):
                out[r::2] = _fma(h[2 * t + r], lo, out[r::2])
                out[r::2] = _fma(g[2 * t + r], hi, out[r::2])
    return out


def _emulate(x, dims, wavelet, levels, inverse, alpha=1):
    """alpha * T x in float32 the way ig_wavelet.hip's transform() goes about it: forward, alpha rides on the first pass's outputs;
    inverse (or no pass), a scaling pass comes first"""
    h = _f32(WAVELETS[wavelet])
    plan = dwt64.passes(dims, wavelet, levels)[0]
    v = [np.array(p, dtype=np.float32).reshape(tuple(dims) + (-1,), order='F') for p in (x.real, x.imag)]
    if alpha != 1 and (inverse or not plan):
        v = list(_cmul32(alpha, *v))
    for i, (box, a) in enumerate(reversed(plan) if inverse else plan):
        sl = tuple(slice(0, c) for c in box)
        new = [np.moveaxis(_emulate_split(np.moveaxis(p[sl], a, 0), h, inverse), 0, a) for p in v]
        if alpha != 1 and not inverse and i == 0:
            new = _cmul32(alpha, *new)
        for p, q in zip(v, new):
            p[sl] = q
    return (v[0] + 1j * v[1]).reshape(x.shape, order='F')


@pytest.mark.parametrize("case", dwt_cases.CASES, ids=dwt_cases.case_id)
def test_a_float32_transform_stays_inside_the_elementwise_bound(case):
    """a plain numpy float32 restatement of the kernel's arithmetic (not the backend's host form, which computes in float64) against
    dwt64.dwt_bound: the bound the GPU tests use is attainable, with room, by a correct float32 transform"""
    dims, wavelet, levels = case
    x, y0 = dwt_cases.make_input(dims, dwt_cases.NCOLS, seed=1), dwt_cases.make_input(dims, dwt_cases.NCOLS, seed=2)
    alpha, beta = 0.75 - 0.5j, -0.25 + 1.5j
    worst = 0.0
    for inverse in (False, True):
        ref = dwt64.dwt(x, dims, wavelet, levels, inverse)
        for a in (1, alpha):
            err = np.abs(_emulate(x, dims, wavelet, levels, inverse, a) - a * ref)
            bound = dwt64.dwt_bound(x, dims, wavelet, levels, inverse, alpha=a)
            assert (bound > 0).all() or (a == 1 and not bound.any())       # alpha == 1 and no pass: an exact copy
            assert (err <= bound).all(), (inverse, a, dwt64.worst_ratio(err, bound))
            worst = max(worst, dwt64.worst_ratio(err, bound))
        # beta != 0: T (beta T^H y0 + alpha x), the combining pass as k_dwt_combine has it
        z = _emulate(y0, dims, wavelet, levels, not inverse)
        rr, ri = _cmul32(alpha, _f32(x.real), _f32(x.imag))
        br, bi = np.float32(beta.real), np.float32(beta.imag)
        rr, ri = _fma(-bi, _f32(z.imag), _fma(br, _f32(z.real), rr)), _fma(bi, _f32(z.real), _fma(br, _f32(z.imag), ri))
        out = _emulate(np.asfortranarray(rr + 1j * ri), dims, wavelet, levels, inverse)
        err = np.abs(out - (alpha * ref + beta * y0))
        bound = dwt64.dwt_bound(x, dims, wavelet, levels, inverse, alpha=alpha, beta=beta, y0=y0)
        assert (err <= bound).all(), (inverse, "beta", dwt64.worst_ratio(err, bound))
        worst = max(worst, dwt64.worst_ratio(err, bound))
    print("%s: worst error / bound %.3f" % (dwt_cases.case_id(case), worst))
    assert worst < 0.5                                                     # a correct transform leaves a margin of two at least


def test_the_bound_on_unit_vectors_rejects_a_wrong_tap():
    """the last db4 tap (0.0106 of the largest) off by a relative 2^-18, 64 float32 roundings: on dense data that is less than one
    rounding of an output and no bound can see it; on unit vectors every coefficient is a product of single taps, the bound is
    relative to each of them, and the wrong tap leaves it -- which is why the GPU tests transform the unit vectors too"""
    dims, wavelet, levels = (1, 1, 64), "db4", 5
    h = dwt64.daubechies(8)
    h[-1] *= 1 + 2.0 ** -18
    wrong = np.eye(64)
    for box, a in dwt64.passes(dims, wavelet, levels)[0]:
        wrong[:box[a]] = dwt64.analysis_matrix(box[a], h) @ wrong[:box[a]]
    assert np.abs(wrong - dwt64.dense(dims, wavelet, levels)).max() < 1e-7
    eye = np.asfortranarray(np.eye(64, dtype=C64))
    bound = dwt64.dwt_bound(eye, dims, wavelet, levels)
    assert dwt64.worst_ratio(np.abs(wrong - dwt64.dense(dims, wavelet, levels)), bound) > 4
    dense_x = dwt_cases.make_input(dims, 1, seed=1)
    err = np.abs(wrong @ dense_x.astype(np.complex128) - dwt64.dwt(dense_x, dims, wavelet, levels))
    assert dwt64.worst_ratio(err, dwt64.dwt_bound(dense_x, dims, wavelet, levels)) < 0.1
    out = _emulate(eye, dims, wavelet, levels, False)                      # and the float32 transform itself stays inside
    assert dwt64.worst_ratio(np.abs(out - dwt64.dense(dims, wavelet, levels)), bound) < 0.5
