"""CPU checks behind the GPU route matrix of the fused SENSE leaf (tests/test_hip_sense_routes.py):

  * the float64 SENSE reference (oracle/sense64.py) against the reference's goldens, on an odd grid (18 x 19 x 21: the centring
    convention) and an even one (128^3);
  * the gridding-matrix caches of SenseProblem hold one matrix per set of phases (a leaf rebuilt under another tuning asks for
    another matrix);
  * the separable records decline samples with no tap on an axis, and describe the stored matrix at narrow and wide kernels,
    including samples exactly on grid points.
"""
import numpy as np
import pytest
from scipy.signal.windows import kaiser

from conftest import golden, rel_err
from indigo_amd.interp import interp_mat, interp_sep_records, sep_expand
from indigo_amd.sense import SenseProblem, _mod_axis_phases, radial_trajectory
from indigo_amd.util import rand64c
from oracle.sense64 import SenseF64

PIN = 1e-6


@pytest.fixture(scope="module")
def odd_golden():
    g = golden("sense")
    C, width, ntab, osf, ro, tr = g["params"]
    p = SenseProblem(tuple(int(n) for n in g["N"]), g["coord"], np.asfortranarray(g["maps"]),
                     width=int(width), ntable=int(ntab), oversamp=float(osf))
    assert p.oN == (18, 19, 21)
    return p, g


def test_sense64_nufft_on_an_odd_grid(odd_golden):
    p, g = odd_golden
    one = SenseProblem(p.N, p.coord, np.ones(p.N + (1,), dtype=np.complex64, order='F'), width=p.width, ntable=p.ntable, oversamp=p.oversamp)
    A = SenseF64(one)
    assert rel_err(A.forward(g["nufft_x"]), g["nufft_fwd"]) < PIN
    assert rel_err(A.adjoint(g["nufft_k"]), g["nufft_adj"]) < PIN


def test_sense64_sense_on_an_odd_grid(odd_golden):
    p, g = odd_golden
    A = SenseF64(p)
    assert A.shape == (g["sense_k"].shape[0], g["sense_x"].shape[0])
    assert rel_err(A.forward(g["sense_x"]), g["sense_Ax"]) < PIN
    assert rel_err(A.adjoint(g["sense_k"]), g["sense_AHk"]) < PIN
    assert rel_err(A.normal(g["sense_x"], float(g["lamda"])), g["sense_AHAx"]) < PIN
    # a coil subset is the matching block of rows
    A1 = SenseF64(p, coils=[1])
    assert rel_err(A1.forward(g["sense_x"]), g["sense_Ax"][p.T:2 * p.T]) < PIN


def test_sense64_sense_on_an_even_grid():
    g = golden("sense_even")
    C, width, ntab, osf, ro, nsp = g["params"]
    s_coord, s_maps, s_x, s_k, _ = (int(v) for v in g["seeds"])
    N = tuple(int(n) for n in g["N"])
    p = SenseProblem(N, radial_trajectory(int(nsp), int(ro), seed=s_coord), np.asfortranarray(rand64c(*N, int(C), seed=s_maps)),
                     width=int(width), ntable=int(ntab), oversamp=float(osf))
    x = rand64c(int(np.prod(N)), 1, seed=s_x)
    k = rand64c(p.T * int(C), 1, seed=s_k)
    A = SenseF64(p)
    pick = g["pick"]
    assert rel_err(A.forward(x), g["sense_Ax"]) < PIN
    scale = np.sqrt(pick.size / float(A.shape[1]))          # a sample of n of P entries carries ~sqrt(n / P) of the norm
    AHk = A.adjoint(k)[pick]
    assert np.linalg.norm(AHk - g["sense_AHk_pick"]) < PIN * scale * float(g["sense_AHk_norm"])
    AHAx = A.normal(x)[pick]
    assert np.linalg.norm(AHAx - g["sense_AHAx_pick"]) < PIN * scale * float(g["sense_AHAx_norm"])


# -- the gridding-matrix caches ----------------------------------------------------------------------------------------------
def _small_problem(N=(12, 10, 9), width=2, osf=2.0, C=2, seed=4):
    return SenseProblem.synthetic(N, C, nspokes=17, nreadout=24, width=width, oversamp=osf, seed=seed)


def _phase_sets(oN):
    ph = _mod_axis_phases(oN)
    other = [a - a[0] for a in ph]                         # what HipBackend.split_gridding_constant hands over
    return ph, other


def test_folded_gridding_matrix_is_cached_per_phase_set():
    p = _small_problem()
    ph, other = _phase_sets(p.oN)
    for layout in (0, 1):
        for first, second in ((ph, other), (other, ph)):
            p.drop_cache()
            a = p.fused_interp(layout, phases=first)
            b = p.fused_interp(layout, phases=second)
            fresh = _small_problem()
            fa, fb = fresh.fused_interp(layout, phases=first), _small_problem().fused_interp(layout, phases=second)
            assert (a != fa).nnz == 0 and (b != fb).nnz == 0
            assert abs(b - a).max() > 0.1 * abs(a).max()      # (the two sets really give two matrices)
            assert p.fused_interp(layout, phases=first) is a            # ... and each is still cached
            assert p.fused_interp(layout, phases=[np.array(v) for v in second]) is b


def test_separable_records_are_cached_per_phase_set():
    p = _small_problem()
    ph, other = _phase_sets(p.oN)
    for first, second in ((ph, other), (other, ph)):
        p.drop_cache()
        a = p.fused_interp_sep(1, phases=first)
        b = p.fused_interp_sep(1, phases=second)
        fa, fb = _small_problem().fused_interp_sep(1, phases=first), _small_problem().fused_interp_sep(1, phases=second)
        for got, exp in ((a, fa), (b, fb)):
            assert got is not None and got['gconst'] == exp['gconst'] and np.array_equal(got['records'], exp['records'])
        assert a['gconst'] != b['gconst']
        assert p.fused_interp_sep(1, phases=first) is a


# -- the separable records at the edges of the kernel widths --------------------------------------------------------------------
def _edge_coords(oN, T, seed):
    """coordinates of which a third lie exactly on grid points, a third on the grid's faces and corners, the rest uniform"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.5, 0.5, size=(3, T))
    k = T // 3
    for d in range(3):
        c[d, :k] = (rng.integers(0, oN[d], size=k) - oN[d] // 2) / oN[d]
        c[d, k:2 * k] = rng.choice([-0.5, -0.5 + 1.0 / oN[d], 0.5 - 1.0 / oN[d], 0.0], size=k)
    return c


def _table(ntable=128, beta=5.0):
    return kaiser(2 * ntable + 1, beta)[ntable:]


@pytest.mark.parametrize("width", [0.5, 0.75])
def test_separable_records_decline_samples_without_taps(width):
    oN, T = (32, 24, 20), 300
    coord = _edge_coords(oN, T, seed=1)
    G = interp_mat(T, oN, width, _table(), coord).tocsr()
    assert np.any(np.diff(G.indptr) == 0)                  # (the trajectory has samples without taps)
    for phases in (None, _mod_axis_phases(oN)):
        for order in (0, 1):
            assert interp_sep_records(T, oN, width, _table(), coord, phases=phases, grid_order=order) is None


def _grid_order_cols(cols, oN, grid_order):
    if grid_order == 0:
        return cols
    n0, n1, n2 = oN
    kx, ky, kz = cols % n0, (cols // n0) % n1, cols // (n0 * n1)
    return kx + n0 * (kz + n2 * ky)


@pytest.mark.parametrize("width,tw", [(1, 4), (1.5, 4), (2, 4), (2.5, 6), (3, 6), (3.5, 8), (4, 8)])
@pytest.mark.parametrize("grid_order", [0, 1])
def test_separable_records_expand_to_the_gridding_matrix(width, tw, grid_order):
    oN, T = (32, 24, 20), 400
    coord = _edge_coords(oN, T, seed=2)
    table = _table()
    G = interp_mat(T, oN, width, table, coord).tocoo()
    sep = interp_sep_records(T, oN, width, table, coord, grid_order=grid_order)
    assert sep is not None and sep['tw'] == tw and sep['gconst'] == 1
    on_grid = np.all(np.abs(coord[:, :T // 3] * np.array(oN)[:, None] - np.round(coord[:, :T // 3] * np.array(oN)[:, None])) < 1e-12, axis=0)
    assert on_grid.all()
    if width == int(width):                               # a sample on a grid point has 2 width taps per axis, the outermost weighing 0
        assert np.all(np.diff(G.tocsr().indptr)[:T // 3] == (2 * int(width)) ** 3)
    rows, cols, vals = sep_expand(sep)
    n = T * int(np.prod(oN))
    key_exp = G.row.astype(np.int64) * int(np.prod(oN)) + _grid_order_cols(G.col.astype(np.int64), oN, grid_order)
    key_got = rows.astype(np.int64) * int(np.prod(oN)) + cols.astype(np.int64)
    ie, ig = np.argsort(key_exp), np.argsort(key_got)
    assert key_got.max() < n
    np.testing.assert_array_equal(key_got[ig], key_exp[ie])
    np.testing.assert_allclose(vals[ig], G.data[ie], rtol=1e-6, atol=1e-6 * np.abs(G.data).max())


# -- panels of several columns through the coil-interleaved tree -------------------------------------------------------------------
@pytest.mark.parametrize("layout,C", [(None, 4), (None, 5), (None, 3), (1, 4)])
def test_fused_tree_with_two_columns(oracle_backend, layout, C):
    """A, A^H and A^H A + 0.2 I of the fused tree on two columns at once: in the coil-interleaved layout every column's grid is a panel
    of its own (a 4-coil chunk given two columns is not one 8-coil panel)"""
    from indigo_amd.sense import normal_operator
    B = oracle_backend
    p = SenseProblem.synthetic((16, 16, 12), C, nspokes=20, nreadout=32, width=2, oversamp=2.0, seed=4)
    A = p.build_zpadfft(B, layout=layout)
    assert (A._coil_chunks[0][2] > 1) == (layout is None)
    R = SenseF64(p)
    X = rand64c(A.shape[1], 2, seed=1)
    K = rand64c(A.shape[0], 2, seed=2)
    B._scratch = None
    assert rel_err(A * X, R.forward(X)) < 1e-5
    assert rel_err(A.H * K, R.adjoint(K)) < 1e-5
    y = B.zero_array((A.shape[1], 2), np.dtype('complex64'))
    normal_operator(A, lamda=0.2, ncols=2).eval(y, B.copy_array(X))
    assert rel_err(y.to_host(), R.normal(X, 0.2)) < 1e-5
    B._scratch = None


# -- which axes the zero-pad-aware transform takes ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind,words", [(256, 3, (16, 16)), (128, 4, (16, 8)), (135, 4, (15, 9)), (58, 5, (12, 12)), (62, 5, (16, 16)),
                                          (69, 5, (12, 12)), (102, 5, (15, 15)), (277, 5, (28, 28)), (410, 5, (32, 32)),
                                          (32, 0, None), (48, 0, None), (64, 0, None), (96, 0, None)])
def test_padded_axis_kinds(n, kind, words):
    """ig_fft_padded_axis_kind / ig_fft_support_words: a chirp-z axis is one with a prime factor above 7 -- 64 or 96 (radix-8 stages of the
    LDS kernel) are none, and no zero-pad-aware pass takes them: a grid with such a y or z axis has no fused leaf (supports_padded_fft)"""
    import ctypes
    from indigo_amd import _lib
    L = _lib.lib()
    k = ctypes.c_int(-1)
    assert L.ig_fft_padded_axis_kind(n, ctypes.byref(k)) == 0 and k.value == kind
    zi, zo = ctypes.c_int(), ctypes.c_int()
    rc = L.ig_fft_support_words(n, ctypes.byref(zi), ctypes.byref(zo))
    assert (rc == 0) == (words is not None) and (words is None or (zi.value, zo.value) == words)
