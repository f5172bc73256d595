"""The z-contiguous y <-> z intermediate of the fused SENSE leaf (plan option 'fft.zc_intermediate', indigo_amd/csrc/ig_fft_zc.h).

The option changes where the y and z passes of the zero-padded / cropped transform keep what they exchange, nothing else: the
arithmetic, the kernels and their order are the same, so every result must be BIT-identical with the option off (the grid's own
order, as before) and on -- the k-space grid on the segments the support table flags, and the image.  Over NaN-poisoned memory:
with the option on nobody writes an unflagged segment of the grid (the y pass no longer passes through it), and the cropped
transform reads none.

Shapes: the smallest at which the addressing can go wrong -- both tile widths (16 columns on 256-point axes, 32 on 512-point
ones), the half box and a run-time box, mixed axis lengths with ny != nz either way round, 8 / 4 / 2 interleaved coils, and a
12-coil tree whose 8- and 4-wide chunks share one scratch arena."""
import ctypes

import numpy as np
import pytest

from conftest import rel_err
from indigo_amd.sense import SenseProblem
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
RTOL = 1e-5           # the bar of the route tests of this path (tests/test_hip_configs.py)
NAN = np.nan + 1j * np.nan

SHAPES = [((128, 128, 128), 2.0),      # grid 256^3, half box: the 256-point route
          ((160, 160, 160), 1.6),      # grid 256^3, run-time box
          ((256, 128, 128), 2.0),      # grid 512 x 256 x 256: 512 points on x only
          ((128, 128, 256), 2.0)]      # grid 256 x 256 x 512: ny != nz, 16-column y tiles inside 32-column pieces


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _problem(image, osf, coils, nspokes=300):
    p = SenseProblem.synthetic(image, coils, nspokes=nspokes, nreadout=2 * image[0], width=2, ntable=128, oversamp=osf, seed=5,
                               lazy_maps=True)
    return p


def _leaf(tree):
    from indigo_amd import operators as op
    tree = tree.child if isinstance(tree, op.HeadRows) else tree
    Z = tree.right
    assert isinstance(Z, op.ZpadFFT) and Z._layout == 2
    return Z


def _flags(p, Z):
    """[ky, kz, kx tile] -> whether the support table flags the segment (as tests/stress_adjoint.py reads it)"""
    n0, n1, n2 = p.oN
    tile = int(Z._tile_kw.get('support_tile', 16))
    _, _, bits = p.split_support(Z._support_h, tile)
    kz = np.arange(n2)
    b = bits.reshape(n1, n0 // tile, 16)
    return ((b[:, :, kz % 16] >> (kz // 16).astype(np.uint32)) & 1).astype(bool).transpose(0, 2, 1), tile


def _leaf_both_ways(hip, p, Z, x):
    """forward and adjoint of the leaf with the option at 0 and at 1 -> {option: (grid, image)}; the adjoint's input is the grid
    of option 0 with NaN in every unflagged segment"""
    n0, n1, n2 = p.oN
    C = Z._C
    flag, tile = _flags(p, Z)
    assert flag.any() and not flag.all() and not flag.any(axis=(1,)).all(), "the table has empty tiles and ragged hulls"
    poison_d = hip.copy_array(np.full((n0 * n1 * n2 * C, 1), NAN, dtype=C64))
    nan_img_d = hip.copy_array(np.full((Z.shape[1], 1), NAN, dtype=C64))
    x_d = hip.copy_array(x)
    out, g_in_d = {}, None
    for opt in (0, 1):
        hip.set_option('fft.zc_intermediate', opt)
        g_d = hip.empty_array((n0 * n1 * n2 * C, 1), C64)
        g_d._copy(poison_d)
        Z.eval(g_d, x_d, forward=True)
        g = g_d.to_host().reshape(n1, n2, n0 // tile, tile, C)
        if opt == 0:
            gin = g.copy()
            gin[~flag] = NAN
            g_in_d = hip.copy_array(gin.reshape(-1, 1))
            del gin
        img_d = hip.empty_array((Z.shape[1], 1), C64)
        img_d._copy(nan_img_d)
        Z.eval(img_d, g_in_d, forward=False)
        out[opt] = (g, img_d.to_host().reshape(-1))
        del g_d, img_d
    hip.set_option('fft.zc_intermediate', 1)
    return out, flag


@pytest.mark.parametrize("coils", [8, 4, 2])
@pytest.mark.parametrize("image,osf", SHAPES)
def test_results_are_bit_identical_with_the_old_addressing(hip, image, osf, coils):
    p = _problem(image, osf, coils)
    hip._scratch = None
    try:
        A = p.build_zpadfft(hip, layout=2)
        Z = _leaf(A)
        assert Z._C == coils
        out, flag = _leaf_both_ways(hip, p, Z, rand64c(int(np.prod(p.N)), 1, seed=1))
        (g0, i0), (g1, i1) = out[0], out[1]
        assert not np.isnan(g0[flag].real).any() and not np.isnan(i0.real).any()
        assert np.array_equal(_bits(g0[flag]), _bits(g1[flag])), "k-space grid, flagged segments"
        assert np.isnan(g1[~flag].real).all() and np.isnan(g1[~flag].imag).all(), "an unflagged segment of the grid was written"
        assert np.array_equal(_bits(i0), _bits(i1)), "image"
    finally:
        hip.set_option('fft.zc_intermediate', 1)
        hip._scratch = None
        p.drop_cache()


def test_chunks_of_two_piece_widths_share_the_arena(hip):
    """12 coils as 8 + 4 on the 256 x 256 x 512 grid: both chunks' intermediates in ONE scratch arena, one after the other"""
    from indigo_amd import operators as op
    from indigo_amd.transforms import reserve_for
    p = _problem((128, 128, 256), 2.0, 12)
    hip._scratch = None
    try:
        A = p.build_zpadfft(hip, layout=2, chunk=8)
        assert isinstance(A, op.VStack) and [_leaf(ch)._C for ch in A.children] == [8, 4]
        x_d = hip.copy_array(rand64c(A.shape[1], 1, seed=1))
        leaves = [_leaf(ch) for ch in A.children]
        # (the adjoint of the whole tree scatters with float atomics and is not repeatable bit for bit even at one setting:
        # tests/stress_adjoint.py; the leaves' adjoints are, so they are compared leaf by leaf, on fixed grids, inside the arena)
        grids = [hip.copy_array(rand64c(int(np.prod(p.oN)) * Z._C, 1, seed=3 + i)) for i, Z in enumerate(leaves)]
        res = {}
        for opt in (0, 1):
            hip.set_option('fft.zc_intermediate', opt)
            reserve_for(A, 1)
            y_d = hip.copy_array(np.full((A.shape[0], 1), NAN, dtype=C64))
            A.eval(y_d, x_d)
            imgs = []
            for Z, g_d in zip(leaves, grids):
                z_d = hip.copy_array(np.full((Z.shape[1], 1), NAN, dtype=C64))
                Z.eval(z_d, g_d, forward=False)
                imgs.append(z_d.to_host())
            res[opt] = (y_d.to_host(), np.concatenate(imgs))
        assert not np.isnan(res[0][0].real).any() and not np.isnan(res[0][1].real).any()
        assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])), "forward of the tree"
        assert np.array_equal(_bits(res[0][1]), _bits(res[1][1])), "adjoint of the chunks' leaves"
    finally:
        hip.set_option('fft.zc_intermediate', 1)
        hip._scratch = None
        p.drop_cache()


def test_against_the_float64_evaluation(hip):
    """image 128^3 on the 256^3 grid, 8 coils, option on: forward (k-space of coil 5) and adjoint (a panel that is non-zero in
    the columns of coils 2 and 7) against oracle/precise.py"""
    from oracle.precise import CoilOperatorF64
    p = _problem((128, 128, 128), 2.0, 8)
    hip._scratch = None
    try:
        hip.set_option('fft.zc_intermediate', 1)
        A = p.build_zpadfft(hip, layout=2)
        T = p.T
        x = rand64c(int(np.prod(p.N)), 1, seed=1)
        k = np.zeros((T, 8), dtype=C64, order='F')
        k[:, 2] = rand64c(T, seed=2)
        k[:, 7] = rand64c(T, seed=3)
        Ax = (A * x).reshape(T, 8, order='F')
        AHk = A.H * k.reshape(-1, 1, order='F')
        fwd = rel_err(Ax[:, 5], CoilOperatorF64(p, 5).forward(x))
        exact = CoilOperatorF64(p, 2).adjoint(k[:, 2]) + CoilOperatorF64(p, 7).adjoint(k[:, 7])
        adj = rel_err(AHk.reshape(-1), exact)
        assert fwd < RTOL and adj < RTOL, "forward %.3e, adjoint %.3e against the float64 evaluation (bar %.0e)" % (fwd, adj, RTOL)
    finally:
        hip._scratch = None
        p.drop_cache()


@pytest.mark.parametrize("image,osf,coils", [((128, 128, 128), 2.0, 8), ((160, 160, 160), 1.6, 4), ((128, 128, 256), 2.0, 12)])
def test_scratch_accounting_holds_with_the_option_on(hip, image, osf, coils):
    """analyses.ScratchUsage of the tree is what an evaluation really takes: an arena of exactly that size serves forward and
    adjoint without a dynamic allocation, Backend.mem_usage() grows by exactly the arena, the leaf's own figure is the plan's
    workspace, and the intermediate fits the part of it that the full-size array had"""
    from indigo_amd import operators as op
    from indigo_amd.analyses import ScratchUsage
    from indigo_amd._lib import lib
    p = _problem(image, osf, coils)
    hip._scratch = None
    real = hip.zero_array
    try:
        hip.set_option('fft.zc_intermediate', 1)
        A = p.build_zpadfft(hip, layout=2, chunk=8)
        x_d = hip.copy_array(rand64c(A.shape[1], 1, seed=1))
        y_d = hip.zero_array((A.shape[0], 1), C64)
        A.eval(y_d, x_d)                                                  # formats and plans are made on first use
        A.eval(x_d, y_d, forward=False)
        hip._scratch = None
        elems = ScratchUsage().measure(A, 1)
        before = hip.mem_usage()
        hip.reserve_scratch(elems)
        assert hip.mem_usage() - before == elems * 8
        served = []

        def watch(shape, dtype, name=''):
            served.append(name)
            return real(shape, dtype, name=name)
        hip.zero_array = watch
        A.eval(y_d, x_d)
        A.eval(x_d, y_d, forward=False)
        hip.barrier()
        assert 'scratch(dynamic)' not in served
        assert hip.mem_usage() - before == elems * 8
        a3 = ctypes.c_int64 * 3
        for ch in (A.children if isinstance(A, op.VStack) else [A]):
            Z = _leaf(ch)
            ws = hip._fft_padded_workspace(Z._grid, Z._lo, Z._box, Z._C, 2)
            assert Z._ws_bytes() == ws
            piece = 256 if Z._grid[2] == 512 else 128
            size = lib().ig_fft_zc_size(a3(*Z._grid), a3(*Z._box), Z._C, piece)
            assert 0 < size <= int(np.prod(Z._grid)) * Z._C * 8 <= ws
    finally:
        hip.zero_array = real
        hip._scratch = None
        p.drop_cache()
