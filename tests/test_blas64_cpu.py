"""tests/blas64.py on the CPU: that the exact comparisons of tests/test_hip_blas.py are legitimate (on the integer inputs every value the
kernels of ig_blas.hip form -- products, updated elements, float32 run partials -- is a float32 number, so no summation order and no
grid can change a bit), that blas64.cg_iteration is the loop the project already pins to the reference (Backend.cg on the numpy
oracle backend), and that the restatement has every gate of the header."""
import itertools

import numpy as np
import pytest

import blas64 as b64
from blas64 import C64, C128, N_BIG, N_MID, SMALL_N

RTOL = 1e-5                         # the project's tolerance for complex64 results
SHAPES = SMALL_N + (N_MID,)


def _units(values, gran):
    """the largest |value| in units of `gran`; every value must be a whole number of them"""
    v = np.abs(np.asarray(values, dtype=np.float64)) / gran
    assert np.array_equal(v, np.rint(v)), "not a multiple of %g" % gran
    return float(v.max()) if v.size else 0.0


def _parts(z):
    z = np.asarray(z)
    return np.concatenate([z.real.ravel(), z.imag.ravel()])


# ---- 1. the exact cases have no rounding -------------------------------------------------------------------------------------------------

def test_exact_inputs_are_nonzero_integers_up_to_8():
    a, b = b64.exact_inputs(1023, 5, 2)
    for v in (a, b):
        assert v.dtype == C64 and v.shape == (1023,)
        parts = _parts(v)
        assert np.array_equal(parts, np.rint(parts)) and np.abs(parts).min() >= 1 and np.abs(parts).max() == 8
    assert not np.array_equal(a, b)
    assert np.array_equal(b64.exact_inputs(1023, 5, 2)[1], b)


@pytest.mark.parametrize("n", SHAPES)
def test_elementwise_references_are_float32_numbers(n):
    x, y = b64.exact_inputs(n, n, 2)
    for beta, alpha in b64.AXPBY_SCALARS:
        ref = b64.axpby(beta, y, alpha, x)
        assert b64.is_f32(ref), (beta, alpha)
        # the kernel forms b y first and adds a x one real product at a time: every intermediate is a partial sum of these four
        # products per component, all multiples of 1/4 (the scalars' granularity), so it is enough that their magnitudes add up to
        # far fewer than 2^24 quarters
        mag = (abs(np.float64(complex(beta).real)) + abs(np.float64(complex(beta).imag))) * 8 + (abs(complex(alpha).real) + abs(complex(alpha).imag)) * 8
        assert _units(_parts(ref), 0.25) <= mag / 0.25 < 2 ** 24
    for d_beta, bs, d_alpha in b64.DEV_COMBOS:
        ref = b64.axpby_dev(d_beta, bs, y, d_alpha, b64.DEV_ALPHA_SCALE, x)
        assert b64.is_f32(ref), (d_beta, bs, d_alpha)
        # the factors themselves: beta_scale * (float)*d_beta is formed in float32 on the device
        b = b64.f32(bs) * (1.0 if d_beta is None else d_beta)
        a = b64.DEV_ALPHA_SCALE * (1.0 if d_alpha is None else d_alpha)
        assert b64.f32(b) == b and b64.f32(a) == a
        assert _units(_parts(ref), 2.0 ** -3) < 2 ** 24


@pytest.mark.parametrize("n", SHAPES + (N_BIG,))
def test_reduction_run_partials_are_exact(n):
    """k_reduce: a float32 run is 16 elements of two (the norm) or four (the dot) fused multiply-adds on integers"""
    x, y = b64.exact_inputs(n, n + 1, 2)
    xr, xi, yr, yi = (v.astype(np.float64) for v in (x.real, x.imag, y.real, y.imag))
    for terms in (np.abs(xr * yr) + np.abs(xi * yi), np.abs(xr * yi) + np.abs(xi * yr), xr * xr + xi * xi):
        assert b64.RUN_ELEMS * _units(terms, 1.0) < 2 ** 24
    re, im = b64.dotc(x, y)
    assert re == np.vdot(x.astype(C128), y.astype(C128)).real and im == np.vdot(x.astype(C128), y.astype(C128)).imag
    assert abs(re) < 2 ** 53 and abs(im) < 2 ** 53 and b64.nrm2sq(x) < 2 ** 53           # the double sums are whole numbers below 2^53


@pytest.mark.parametrize("n,lamda,k", list(itertools.product(SHAPES, b64.CG_LAMDAS, b64.CG_KS)) + [(N_BIG, 0.5, 3)])
def test_cg_references_are_float32_numbers_and_run_partials_exact(n, lamda, k):
    c = b64.exact_cg_case(n, 7 * n + k, lamda, k)
    ref = b64.cg_iteration(n, c['p'], c['Ap'], c['r'], c['x'], lamda, c['rr'], c['r0'], c['tol2'])
    assert ref['pap'] > 0 and ref['alpha'] == 2.0 ** -k and c['rr'] / ref['alpha'] == ref['pap']
    for name in ('Ap', 'r', 'x'):
        assert b64.is_f32(ref[name]), name
    if lamda == 0:
        assert np.array_equal(ref['Ap'], c['Ap'].astype(C128))
    # k_cg_dot: Ap' in halves; a run holds 16 elements' px ax' + py ay'
    p = c['p'].astype(C128)
    assert _units(_parts(ref['Ap']), 0.5) <= 24
    terms = np.abs(p.real * ref['Ap'].real) + np.abs(p.imag * ref['Ap'].imag)
    assert b64.RUN_ELEMS * _units(terms, 0.5) < 2 ** 24
    # k_cg_step_r: r' in units of 2^-(k+1), its squares in units of 2^-(2k+2); a run holds 16 elements' |r'|^2
    g = 2.0 ** -(k + 1)
    assert _units(_parts(ref['r']), g) <= 20 / g
    sq = ref['r'].real ** 2 + ref['r'].imag ** 2
    assert b64.RUN_ELEMS * _units(sq, g * g) < 2 ** 24
    assert ref['r2'] == float(np.sum(sq)) and ref['r2'] / (g * g) < 2 ** 53 and ref['pap'] / 0.5 < 2 ** 53
    # k_cg_step_xp: x' in units of 2^-k; p' is the one rounded value: a single fma whose exact value the float64 reference holds
    assert _units(_parts(ref['x']), 2.0 ** -k) <= 16 * 2 ** k
    beta32 = b64.f32(ref['beta'])
    exact = [ref['r'].real + beta32 * p.real, ref['r'].imag + beta32 * p.imag]
    assert np.array_equal(ref['p'].real, exact[0]) and np.array_equal(ref['p'].imag, exact[1])
    # (24 bits of beta times 4 bits of p against r', below 32 in units of 2^-4: with beta between 2^-20 and 2^20 the two span fewer
    # than 53 bits, so the float64 sum above is the exact value and one rounding to float32 gives the device's fma)
    assert 2.0 ** -20 < beta32 < 2.0 ** 20
    assert ref['rr_next'] == ref['r2'] and ref['hist'] == ref['r2'] / c['r0']


@pytest.mark.parametrize("ncols", b64.CSUM_NCOLS)
def test_coil_sum_references_are_float32_numbers(ncols):
    for rows in b64.CSUM_ROWS:
        X = b64.exact_inputs(rows * ncols, rows + ncols, 1)[0].reshape(rows, ncols)
        y = b64.exact_inputs(rows, rows, 1)[0]
        for beta, alpha in b64.CSUM_SCALARS:
            ref = b64.csum_il(X, alpha, beta, y)
            assert b64.is_f32(ref)
            assert _units(_parts(ref), 0.5) <= (1.5 * 8 * ncols + 4) / 0.5 < 2 ** 24     # sums of <= 64 integers, then halves
            assert np.array_equal(ref, b64.csum_cols(X, alpha, beta, y))


# ---- 2. the restatements themselves -----------------------------------------------------------------------------------------------------

def test_axpby_rules():
    x = np.array([1 + 2j, -3 + 0.5j], dtype=C64)
    y = np.array([np.nan + 1j * np.nan, 2 - 1j], dtype=C64)
    assert np.array_equal(b64.axpby(0, y, 2j, x), np.array([-4 + 2j, -1 - 6j]))              # beta == 0: y is not read
    assert np.array_equal(b64.axpby(0, y, 0, x), np.zeros(2))
    assert np.array_equal(b64.axpby(2, x, 0, None), np.array([2 + 4j, -6 + 1j]))              # ig_cscal
    out = b64.axpby(1, y, 0, x)
    assert np.isnan(out[0]) and out[1] == 2 - 1j
    # the scalars are rounded to float32 first
    assert b64.axpby(0, x, 0.1, x)[0] == complex(np.float32(0.1)) * (1 + 2j)
    assert np.array_equal(b64.axpby_dev(None, 0.5, x, 3.0, -1.0, x), -2.5 * x.astype(C128))
    assert np.array_equal(b64.axpby_dev(0.1, 1.0, x, None, 1.0, x), (float(np.float32(0.1)) + 1.0) * x.astype(C128))
    assert np.isnan(b64.axpby_dev(None, 0.0, y, None, 1.0, x)[0])                             # the device form always reads y


def test_reductions_and_sums():
    x = np.array([1 + 2j, -3 + 0.5j], dtype=C64)
    y = np.array([2 - 1j, 4 + 4j], dtype=C64)
    z = np.vdot(x.astype(C128), y.astype(C128))
    assert b64.dotc(x, y) == (z.real, z.imag) and b64.nrm2sq(x) == 1 + 4 + 9 + 0.25
    assert b64.dotc(x[:0], y[:0]) == (0.0, 0.0) and b64.nrm2sq(x[:0]) == 0.0
    X = np.array([[1 + 1j, 2, 3], [4, 5j, 6]], dtype=C64)
    assert np.array_equal(b64.csum_cols(X, 2, 0, np.full(2, np.nan, C64)), np.array([12 + 2j, 20 + 10j]))
    assert np.array_equal(b64.csum_il(X, 1, 0.5, np.array([2, 4j], C64)), np.array([7 + 1j, 10 + 7j]))
    assert np.array_equal(b64.csum_cols(X[:, :0], 1, 0.5, np.array([2, 4j], C64)), np.array([1, 2j]))
    a = np.array([-1.5, 0.25, 3, -0.0], dtype=np.float32)
    assert np.array_equal(b64.smax(0.25, a), np.array([0.25, 0.25, 3, 0.25], dtype=np.float32)) and b64.smax(0.25, a).dtype == np.float32


def test_scalar_programs():
    assert b64.scalar_ratio(3.0, 4.0, -2.0) == -1.5 and b64.scalar_ratio(3.0, 0.0, 1.0) == 0.0 and b64.scalar_ratio(0.0, 0.0, 1.0) == 0.0
    assert b64.scalar_ratio_gated(3.0, 4.0, 1.0, 1.0, 4.0, 0.25) == 0.75               # equality at the gate: not stopped
    assert b64.scalar_ratio_gated(3.0, 4.0, 1.0, np.nextafter(1.0, 0), 4.0, 0.25) == 0.0
    assert b64.scalar_ratio_gated(3.0, 4.0, 1.0, 2.0, 4.0, 0.25) == 0.75
    assert b64.scalar_ratio_gated(3.0, 0.0, 1.0, 2.0, 4.0, 0.25) == 0.0
    assert b64.scalar_ratio_gated(3.0, 4.0, 1.0, np.nan, 4.0, 0.25) == 0.0             # a NaN residual stops, too


def test_cg_gates():
    n = 1000
    c = b64.exact_cg_case(n, 3, 0.5, 1)
    args = (n, c['p'], c['Ap'], c['r'], c['x'], c['lamda'])
    r64, x64 = c['r'].astype(C128), c['x'].astype(C128)
    # stopped by the tolerance: rr just below tol2 * r0
    tol2, r0 = 2.0 ** -10, c['rr'] * 2.0 ** 10
    assert tol2 * r0 == c['rr']
    out = b64.cg_iteration(*args, np.nextafter(c['rr'], 0), r0, tol2)
    assert out['alpha'] == 0.0 and np.array_equal(out['r'], r64) and np.array_equal(out['x'], x64) and out['rr_next'] == b64.nrm2sq(c['r'])
    # equality at the threshold is not stopped
    out = b64.cg_iteration(*args, c['rr'], r0, tol2)
    assert out['alpha'] == 0.5 and not np.array_equal(out['r'], r64)
    # <p, Ap> == 0: a zero step, nothing NaN or Inf
    out = b64.cg_iteration(n, c['p'], np.zeros(n, C64), c['r'], c['x'], 0.0, c['rr'], c['r0'], c['tol2'])
    assert out['pap'] == 0.0 and out['alpha'] == 0.0 and np.array_equal(out['r'], r64) and np.array_equal(out['x'], x64)
    assert all(np.isfinite(np.asarray(v)).all() for v in out.values())
    # rr == 0: beta = 0, p' = r'
    out = b64.cg_iteration(*args, 0.0, c['r0'], 0.0)
    assert out['alpha'] == 0.0 and out['beta'] == 0.0 and np.array_equal(out['p'], r64) and np.isfinite(out['hist'])
    # r0 == 0: the history entry is 0, the step is taken
    out = b64.cg_iteration(*args, c['rr'], 0.0, c['tol2'])
    assert out['hist'] == 0.0 and out['alpha'] == 0.5
    # a NaN residual stops
    assert b64.cg_iteration(*args, np.nan, c['r0'], c['tol2'])['alpha'] == 0.0


# ---- 3. cg_iteration is the loop the project pins to the reference ----------------------------------------------------------------------

def test_cg_iteration_matches_backend_cg_on_the_oracle(oracle_backend):
    B = oracle_backend
    n, lamda, iters = 64, 0.05, 3
    rng = np.random.default_rng(12)
    G = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(n)
    M = np.asfortranarray((G.conj().T @ G + 0.5 * np.eye(n)).astype(C64))             # Hermitian positive definite
    b = np.asfortranarray((rng.standard_normal((n, 1)) + 1j * rng.standard_normal((n, 1))).astype(C64))
    x_ref = np.zeros((n, 1), dtype=C64, order='F')
    h_ref = B.cg(B.DenseMatrix(M), b.copy(order='F'), x_ref, lamda=lamda, maxiter=iters, tol=1e-10)
    assert len(h_ref) == iters
    M64 = M.astype(C128)
    x = np.zeros(n, dtype=C128)
    r = b[:, 0].astype(C128)
    p = r.copy()
    rr = r0 = b64.nrm2sq(r)
    hist = []
    for _ in range(iters):
        out = b64.cg_iteration(n, p, M64 @ p, r, x, lamda, rr, r0, 1e-20)
        x, r, p, rr = out['x'], out['r'], out['p'], out['rr_next']
        hist.append(np.sqrt(out['hist']))
    np.testing.assert_allclose(hist, h_ref, rtol=RTOL)
    assert np.linalg.norm(x - x_ref[:, 0]) <= RTOL * np.linalg.norm(x_ref)
