"""Dictionary matching on the MI355X: ig_dict_match_c64 against the float64 restatement in tests/dict64.py, exact indices on voxels
built on known atoms, ties and padding, the layout forms, the limits, and the `fit` driver on the T2 phantom of the CPU tests."""
import ctypes

import numpy as np
import pytest

import dict64
from test_dictmatch_cpu import check_phantom_fit, phantom  # noqa: F401  (the module-scoped fixture and its check)
from indigo_amd import dictmatch

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
PAD = 37            # NaN rows under every column of the voxel panel
PAD_D = 3           # NaN rows under every atom: ldd = K + 3
PAD_OUT = 5         # sentinel rows below idx and ip

NS = (1, 105, 2048, 5049)                       # one voxel; part of a group of 32; whole workgroups; several workgroups and a tail
KS = (1, 3, 4, 5, 8, 9, 16, 17, 32)             # exact widths up to 8, both sides of the padded widths 16 and 32, the limit
NAS = (1, 31, 33, 1000, 4097)                   # one atom; a ragged tile; a tile and one atom; several chunks; a chunk boundary and one

# every (n, K) once, with N rotating through its five values, and the corners
CASES = [(n, K, NAS[(i + j) % 5]) for i, K in enumerate(KS) for j, n in enumerate(NS)]
CASES += [c for c in [(5049, 32, 4097), (1, 1, 1)] if c not in CASES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _padded(hip, a, pad):
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _call(hip, n, K, N, x_d, ldx, d_d, ldd):
    """the C entry on outputs with PAD_OUT sentinel rows below them -> (rc, idx, ip) with the sentinels checked"""
    idx_h = np.full((n + PAD_OUT, 1), -7, dtype=np.int32, order='F')
    ip_h = np.full((n + PAD_OUT, 1), np.nan, dtype=C64, order='F')
    idx_d, ip_d = hip.copy_array(idx_h), hip.copy_array(ip_h)
    rc = hip._L.ig_dict_match_c64(hip._ctx, n, K, N, ctypes.c_void_p(x_d._arr), ldx, ctypes.c_void_p(d_d._arr), ldd,
                                  ctypes.c_void_p(idx_d._arr), ctypes.c_void_p(ip_d._arr))
    idx, ip = idx_d.to_host(), ip_d.to_host()
    assert np.array_equal(idx[n:], idx_h[n:]) and np.array_equal(_bits(ip[n:]), _bits(ip_h[n:]))
    return rc, idx[:n, 0], ip[:n, 0]


WORST = {"score": 0.0, "ip": 0.0}


@pytest.mark.parametrize("n,K,N", CASES, ids=lambda v: str(v))
def test_kernel_matches_the_float64_restatement(hip, n, K, N):
    """The criterion: the chosen atom's float64 score is within 4 (2K + 2) 2^-24 ||c||^2 of the largest float64 score.  Each of Re and
    Im of d_a^H c is a chain of 2K float32 fmas on exact products (relative error (2K) 2^-24 of sum |d||c| <= ||c|| for unit atoms),
    squaring doubles the relative error and two scores are compared: 1.6e-5 ||c||^2 at K = 32."""
    x, d = dict64.random_case(n, K, N, seed=1000 * K + n + N)
    x_d, x_h = _padded(hip, x, PAD)
    d_d, d_h = _padded(hip, d, PAD_D)
    rc, idx, ip = _call(hip, n, K, N, x_d, n + PAD, d_d, K + PAD_D)
    hip._check(rc, "ig_dict_match_c64")
    assert np.array_equal(_bits(x_d.to_host()), _bits(x_h)) and np.array_equal(_bits(d_d.to_host()), _bits(d_h))
    assert idx.min() >= 0 and idx.max() < N
    P = dict64.products(d, x)
    s = P.real ** 2 + P.imag ** 2
    c2 = (np.abs(x.astype(np.complex128)) ** 2).sum(axis=1)
    rows = np.arange(n)
    short = (s.max(axis=1) - s[rows, idx]) / c2
    err_ip = np.abs(ip - P[rows, idx]) / np.sqrt(c2)
    WORST["score"], WORST["ip"] = max(WORST["score"], short.max()), max(WORST["ip"], err_ip.max())
    print("dict_match n %d K %d N %d: score short of the best by %.3e ||c||^2 (bound %.3e), ip %.3e ||c||; worst so far %.3e / %.3e"
          % (n, K, N, short.max(), 4 * (2 * K + 2) * 2.0 ** -24, err_ip.max(), WORST["score"], WORST["ip"]))
    assert np.isfinite(ip).all()
    assert short.max() <= 4 * (2 * K + 2) * 2.0 ** -24
    assert err_ip.max() <= 1e-5
    # the backend method on the same panels: the same bits
    idx_b, ip_b = hip.dict_match(x_d[:n], d_d[:K], n)
    assert idx_b.dtype == np.int32 and ip_b.dtype == C64 and idx_b.shape == (n,) and ip_b.shape == (n,)
    assert np.array_equal(idx_b, idx) and np.array_equal(_bits(ip_b), _bits(ip))


@pytest.mark.parametrize("n,K,N", [(5049, 4, 1000), (2048, 3, 31), (2048, 17, 100), (5049, 32, 4097)], ids=lambda v: str(v))
def test_exact_indices_of_planted_atoms(hip, n, K, N):
    """voxels rho d_m + 1e-3 noise: idx == m for every voxel.  In float64 the planted atom leads every other by at least
    1.3e-2 ||c||^2 (asserted below), against a float32 error of at most 1.6e-5 ||c||^2."""
    x, d, m = dict64.planted_case(n, K, N, seed=K * N)
    idx64, _, s = dict64.match(d, x)
    c2 = (np.abs(x.astype(np.complex128)) ** 2).sum(axis=1)
    lead = s[np.arange(n), m].copy()
    s[np.arange(n), m] = -1
    assert np.array_equal(idx64, m) and ((lead - s.max(axis=1)) / c2).min() >= 1.3e-2
    idx, ip = hip.dict_match(hip.copy_array(x), hip.copy_array(d), n)
    assert np.array_equal(idx, m)


@pytest.mark.parametrize("K,N", [(4, 1000), (8, 600), (17, 200), (3, 33)], ids=lambda v: str(v))
def test_ties_return_the_lowest_index(hip, K, N):
    """atom 5 again at 40 (the next tile, the other half of the lanes) and at N - 1 (another chunk), atom 2 again at 6 (the same
    tile, the other half of the lanes): bitwise equal scores, and the lowest index must win.  A zero voxel gives (0, 0)."""
    n = 300
    rng = np.random.default_rng(K + N)
    d = dict64.normalised_atoms(K, N, rng)
    if N > 40:
        d[:, 40] = d[:, 5]
    d[:, N - 1] = d[:, 5]
    d[:, 6] = d[:, 2]
    rho = (0.5 + rng.random(n)) * np.exp(2j * np.pi * rng.random(n))
    which = np.where(np.arange(n) % 2 == 0, 5, 2)
    x = np.asfortranarray((rho[:, None] * d.astype(np.complex128).T[which]).astype(C64))
    x[7] = 0
    want = which.copy()
    want[7] = 0
    x_d, d_d = hip.copy_array(x), hip.copy_array(d)
    idx, ip = hip.dict_match(x_d, d_d, n)
    assert np.array_equal(idx, want), np.flatnonzero(idx != want)
    assert ip[7] == 0
    keep = np.arange(n) != 7
    assert np.abs(ip[keep] - rho[keep]).max() <= 1e-5 * 1.5
    idx2, ip2 = hip.dict_match(x_d, d_d, n)                                           # two calls give the same bits
    assert np.array_equal(idx2, idx) and np.array_equal(_bits(ip2), _bits(ip))


@pytest.mark.parametrize("n,K,N", [(2048, 4, 1000), (5049, 5, 33), (2048, 9, 100), (105, 32, 31)], ids=lambda v: str(v))
def test_layout_forms_give_the_same_bits(hip, n, K, N):
    """the stacked (n K, 1) vector, the plain panel and panels with odd leading dimensions hold the same results"""
    x, d = dict64.random_case(n, K, N, seed=3)
    d_d = hip.copy_array(d)
    outs = []
    for pad in (PAD, 0, 2):
        x_d, _ = _padded(hip, x, pad)
        outs.append(hip.dict_match(x_d[:n], d_d, n))
    outs.append(hip.dict_match(hip.copy_array(np.asfortranarray(x.reshape((-1, 1), order='F'))), d_d, n))
    d_p, _ = _padded(hip, d, PAD_D)
    outs.append(hip.dict_match(hip.copy_array(x), d_p[:K], n))
    for idx, ip in outs[1:]:
        assert np.array_equal(idx, outs[0][0]) and np.array_equal(_bits(ip), _bits(outs[0][1]))


def test_limits(hip):
    n = 64
    x33, d33 = dict64.random_case(n, 33, 10, seed=1)
    with pytest.raises(RuntimeError, match="33 coefficients, between 1 and 32"):
        hip.dict_match(hip.copy_array(x33), hip.copy_array(d33), n)
    x32, d32 = dict64.random_case(n, 32, 10, seed=2)                                  # the limit itself is served
    idx, _ = hip.dict_match(hip.copy_array(x32), hip.copy_array(d32), n)
    assert np.array_equal(idx, dict64.match(d32, x32)[0])
    # elements of one buffer: x = [192, 320) (n = 64, K = 2), d = [520, 526) (N = 3); ip and idx anywhere
    K, N = 2, 3
    host = np.asfortranarray(dict64.random_case(700, 1, 1, seed=3)[0])
    buf = hip.copy_array(host)

    def at(ip_off, idx_off):
        return hip._L.ig_dict_match_c64(hip._ctx, n, K, N, ctypes.c_void_p(buf._arr + 8 * 192), n, ctypes.c_void_p(buf._arr + 8 * 520), K,
                                        ctypes.c_void_p(buf._arr + 8 * idx_off), ctypes.c_void_p(buf._arr + 8 * ip_off))
    for ip_off, idx_off in ((129, 600), (319, 600), (200, 600), (457, 600), (525, 600),      # ip on x's first and last element, inside, on d
                            (0, 161), (0, 319), (0, 489), (0, 525), (0, 40), (600, 631)):    # idx on x, on d, on ip
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(at(ip_off, idx_off), "ig_dict_match_c64")
    for bad, text in (((0, K, N), "0 voxels"), ((n, K, 0), "0 atoms"), ((n, 0, N), "0 coefficients")):
        with pytest.raises(RuntimeError, match=text):
            hip._check(hip._L.ig_dict_match_c64(hip._ctx, bad[0], bad[1], bad[2], ctypes.c_void_p(buf._arr + 8 * 192), n,
                                                ctypes.c_void_p(buf._arr + 8 * 520), K, ctypes.c_void_p(buf._arr + 8 * 600),
                                                ctypes.c_void_p(buf._arr)), "ig_dict_match_c64")
    assert np.array_equal(_bits(buf.to_host()), _bits(host))                           # nothing was written
    hip._check(at(128, 600), "ig_dict_match_c64")                                      # adjacent to x, not overlapping
    after = buf.to_host()
    xs, ds = host[192:320, 0].reshape((n, K), order='F'), host[520:526, 0].reshape((K, N), order='F')
    idx64, ip64, _ = dict64.match(ds, xs)
    assert np.array_equal(after[600:632, 0].view(np.int32), idx64)
    assert np.abs(after[128:192, 0] - ip64).max() <= 1e-5 * np.abs(ip64).max()
    rest = np.ones(700, dtype=bool)
    rest[128:192] = rest[600:632] = False
    assert np.array_equal(_bits(after[rest]), _bits(host[rest]))


def test_fit_on_the_gpu_recovers_the_phantom(hip, phantom):  # noqa: F811
    """the T2 phantom of the CPU tests through the `fit` driver on the device: N = 32 T2 values from 20 to 300 ms, 16 echoes of
    10 ms, K = 4.  Neighbouring compressed atoms differ by at least 1.85e-4 in normalised score (asserted below), against the
    float32 bound 4 (2K + 2) 2^-24 = 2.4e-6 at K = 4: the indices equal the float64 ones on every unmasked voxel."""
    d, _ = dictmatch.compress(phantom['atoms'], phantom['phi'])
    assert 1 - dict64.largest_cross_score(d.astype(C64)) >= 1.85e-4
    out = dictmatch.main(phantom['argv'] + ["--chunk", "300", "--debug", "40", phantom['rec']], backend=hip)
    check_phantom_fit(phantom, out)
