"""The image-axis permutation that lets the fused SENSE leaf run grids whose x axis it has no zero-pad-aware pass for
(indigo_amd.fused.image_permutation, operators.AxisPermute), on the host: the choice rule on a stub backend, the operator on
the numpy oracle, and the permuted route of build_zpadfft and FuseZpadFFT on an oracle that refuses a chirp-z x axis."""
import itertools

import numpy as np
import pytest

from conftest import rel_err
from indigo_amd import fused
from indigo_amd import operators as op
from indigo_amd.sense import SenseProblem, normal_operator
from indigo_amd.transforms import FuseZpadFFT
from indigo_amd.util import rand64c
from oracle.np_backend import NumpyBackend

C64 = np.dtype('complex64')
PERMS = list(itertools.permutations(range(3)))


def _smooth(n):
    n = int(n)
    for f in (2, 3, 5, 7):
        while n > 1 and n % f == 0:
            n //= f
    return n == 1


class KindStub(object):
    """supports_padded_fft as the HIP backend decides it, from a table of axis kinds: 3 / 4 zero-pad-aware passes, 5 chirp-z,
    0 none -- x must be 3 or 4, y and z any of 3, 4, 5"""

    def __init__(self, kinds):
        self.kinds = kinds

    def supports_padded_fft(self, grid, ncoils=None):
        k = [self.kinds.get(int(n), 0) for n in grid]
        return len(grid) == 3 and k[0] in (3, 4) and all(v in (3, 4, 5) for v in k[1:])


STUB = KindStub({256: 3, 512: 3, 160: 4, 240: 4, 320: 4, 138: 4, 96: 4, 225: 4,
                 69: 5, 102: 5, 205: 5, 277: 5, 410: 5, 17: 5, 20: 0})


@pytest.mark.parametrize("grid, expected", [
    ((69, 160, 102), (1, 0, 2)),          # the swap with y: 160 = 16 * 10 on x
    ((69, 102, 160), (2, 1, 0)),          # only a swap with z puts a multiple of 16 on x
    ((277, 320, 320), (1, 0, 2)),         # both y and z qualify: swaps before 3-cycles, then the lowest
    ((69, 225, 160), (2, 1, 0)),          # 225 is accepted on x but not a multiple of 16: 160 first
    ((69, 225, 102), (1, 0, 2)),          # no multiple of 16 anywhere: the swap with the accepted axis
    ((102, 69, 225), (2, 1, 0)),
])
def test_image_permutation_picks_the_documented_axis_order(grid, expected):
    assert not STUB.supports_padded_fft(grid)
    perm = fused.image_permutation(STUB, grid, 8)
    assert perm == expected
    assert STUB.supports_padded_fft(tuple(grid[a] for a in perm))


@pytest.mark.parametrize("grid", [(160, 69, 102), (256, 256, 256), (225, 69, 102), (320, 277, 410)])
def test_image_permutation_keeps_accepted_grids_as_they_are(grid):
    assert STUB.supports_padded_fft(grid)
    assert fused.image_permutation(STUB, grid, 8) is None


@pytest.mark.parametrize("grid", [(69, 69, 69), (277, 277, 277), (69, 102, 205), (20, 20, 20), (69, 160)])
def test_image_permutation_is_none_without_a_smooth_axis(grid):
    assert fused.image_permutation(STUB, grid, 8) is None


def test_the_oracle_takes_every_grid_as_it_is():
    assert fused.image_permutation(NumpyBackend(), (69, 160, 102), 8) is None


def test_permute_grid_columns_default_is_the_layout_1_order():
    import scipy.sparse as spp
    rng = np.random.default_rng(1)
    oN = (6, 5, 4)
    P = int(np.prod(oN))
    G = spp.random(7, P, density=0.3, format='csr', random_state=rng).astype(C64)
    vol = rand64c(P, 1, seed=3)[:, 0]
    for order in PERMS:
        Gp = fused.permute_grid_columns(G.copy(), oN, order)
        volp = vol.reshape(oN, order='F').transpose(order).ravel(order='F')
        assert rel_err(Gp @ volp, G @ vol) < 1e-6
    assert (fused.permute_grid_columns(G.copy(), oN) != fused.permute_grid_columns(G.copy(), oN, (0, 2, 1))).nnz == 0


def _host_permute(x, dims, perm):
    n = int(np.prod(dims))
    return x.reshape(tuple(dims) + (-1,), order='F').transpose(tuple(perm) + (3,)).reshape((n, -1), order='F')


@pytest.mark.parametrize("dims", [(7, 5, 3), (1, 64, 1)])
@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("ncols", [1, 3])
def test_axis_permute_on_the_oracle(dims, perm, ncols):
    B = NumpyBackend()
    n = int(np.prod(dims))
    P = B.AxisPermute(dims, perm)
    assert P.shape == (n, n)
    x = rand64c(n, ncols, seed=7)
    ref = _host_permute(x, dims, perm)
    assert np.array_equal(P * x, ref)
    # P^H P = I, and the adjoint is the inverse permutation
    assert np.array_equal(P.H * (P * x), x)
    assert np.array_equal(P.H * ref, x)
    # alpha and beta as for any leaf; beta = 0 does not read y
    y0 = rand64c(n, ncols, seed=8)
    a, b = 0.5 - 1.25j, -0.75 + 0.5j
    y_d = B.copy_array(y0)
    P.eval(y_d, B.copy_array(x), alpha=a, beta=b)
    assert rel_err(y_d.to_host(), np.complex64(b) * y0 + np.complex64(a) * ref) < 1e-6
    y_d = B.copy_array(np.full((n, ncols), np.nan, dtype=C64))
    P.eval(y_d, B.copy_array(ref), alpha=a, beta=0, forward=False)
    assert rel_err(y_d.to_host(), np.complex64(a) * x) < 1e-6


def test_axis_permute_books_its_bytes():
    from indigo_amd.util import Trace
    B = NumpyBackend()
    B.trace = Trace()
    P = B.AxisPermute((7, 5, 3), (2, 0, 1))
    P * rand64c(105, 1, seed=1)
    assert B.trace.total_bytes('permute') == 2 * 105 * 8


class ChirpXRefused(NumpyBackend):
    """the oracle with the HIP backend's restriction on x: a grid whose x axis has a prime factor above 7 is refused"""

    def supports_padded_fft(self, grid, ncoils=None):
        return len(grid) == 3 and _smooth(grid[0])


def _problem():
    p = SenseProblem.synthetic((13, 24, 15), 3, nspokes=24, nreadout=20, width=2, oversamp=4 / 3, seed=5)
    assert p.oN == (17, 32, 20)
    return p


def _check_against_oracle(A, A_o, shape):
    x = rand64c(shape[1], 1, seed=1)
    k = rand64c(shape[0], 1, seed=2)
    assert rel_err(A * x, A_o * x) < 1e-5
    assert rel_err(A.H * k, A_o.H * k) < 1e-5
    assert rel_err(normal_operator(A, lamda=0.2) * x, normal_operator(A_o, lamda=0.2) * x) < 1e-5


def test_build_zpadfft_runs_a_refused_grid_through_a_permutation():
    p = _problem()
    B = ChirpXRefused()
    assert fused.image_permutation(B, p.oN, p.C) == (1, 0, 2)
    A = p.build_zpadfft(B)
    assert A.has(op.ZpadFFT) and A.has(op.AxisPermute) and not A.has(op.UnscaledFFT)
    assert isinstance(A.right, op.AxisPermute) and A.right._perm == (1, 0, 2)
    zs = []
    stack = [A.left]
    while stack:
        n = stack.pop()
        if isinstance(n, op.ZpadFFT):
            zs.append(n)
        stack.extend(getattr(n, '_children', []))
    assert zs and all(z._grid == (32, 17, 20) and z._box == (24, 13, 15) for z in zs)
    A_o = p.build_zpadfft(NumpyBackend(), layout=0, support=False)
    assert not A_o.has(op.AxisPermute)
    _check_against_oracle(A, A_o, A_o.shape)


def test_build_zpadfft_with_lazy_maps_and_a_coil_subset():
    p = SenseProblem.synthetic((13, 24, 15), 5, nspokes=24, nreadout=20, width=2, oversamp=4 / 3, seed=5, lazy_maps=True)
    A = p.build_zpadfft(ChirpXRefused(), coils=[1, 2, 4])
    assert A.has(op.AxisPermute)
    A_o = p.build_zpadfft(NumpyBackend(), coils=[1, 2, 4], layout=0, support=False)
    _check_against_oracle(A, A_o, A_o.shape)


def test_fuse_zpadfft_runs_a_refused_grid_through_a_permutation():
    p = _problem()
    B = ChirpXRefused()
    A = p.build_tree(B, level=3)
    assert A.has(op.UnscaledFFT)
    A = FuseZpadFFT().visit(A)
    assert A.has(op.ZpadFFT) and A.has(op.AxisPermute) and not A.has(op.UnscaledFFT)
    A_o = p.build_zpadfft(NumpyBackend(), layout=0, support=False)
    _check_against_oracle(A, A_o, A_o.shape)


def test_fuse_zpadfft_permutes_the_scipy_gridding_matrix_without_a_description():
    """a recipe whose G' lost its description (a plain scipy matrix): its columns are renumbered for the permuted grid"""
    p = _problem()
    B = ChirpXRefused()
    A = p.build_tree(B, level=3)
    G = A.left.right
    G._m = G._matrix
    G._struct = None
    A = FuseZpadFFT().visit(A)
    assert A.has(op.ZpadFFT) and A.has(op.AxisPermute)
    _check_against_oracle(A, p.build_zpadfft(NumpyBackend(), layout=0, support=False), A.shape)


def test_scratch_arena_covers_the_permuted_tree():
    """the Product temporary that holds P x is the only extra buffer: the arena reserved for the normal operator serves every
    request of an evaluation without falling back to dynamic allocations"""
    from indigo_amd.analyses import ScratchUsage
    p = _problem()
    B = ChirpXRefused()
    A = p.build_zpadfft(B)
    inner = ScratchUsage().measure(A.left)
    assert ScratchUsage().measure(A) >= inner + A.shape[1]
    AHA = normal_operator(A, lamda=0.2)
    served = []
    real = B.zero_array

    def watch(shape, dtype, name=''):
        served.append(name)
        return real(shape, dtype, name=name)
    B.zero_array = watch
    y = B.zero_array((A.shape[1], 1), C64)
    served.clear()
    AHA.eval(y, B.copy_array(rand64c(A.shape[1], 1, seed=3)))
    assert 'scratch(dynamic)' not in served
