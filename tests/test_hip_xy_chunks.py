"""The x and y passes of the fused SENSE leaf in chunks of image planes on alternating streams (plan options 'fft.xy_chunk_planes',
'fft.xy_chunk_streams'; indigo_amd/csrc/ig_fft_xy.h).

The options change in how many launches, and on which streams, the two passes run -- nothing else: every tile is transformed by the
same arithmetic over the same addresses, so every result must be BIT-identical with K = 0 (one launch per pass) and with any (K, S):
the k-space grid on the segments the support table flags, and the image, over NaN-poisoned memory; unflagged segments of the grid
stay NaN.  What the caller enqueues next (an axpby, a copy to the host) must see the finished image: the chunks' streams are joined
into the backend's stream before the call returns.

Shapes: those of tests/test_hip_zc_intermediate.py -- both tile widths, the half box and a run-time box, mixed axis lengths,
8 / 4 / 2 interleaved coils, a 12-coil tree whose chunks share the arena.  Settings: one plane per chunk, a chunk size that divides
the planes and ones that leave a ragged last chunk, one chunk for all planes, one, two and three streams.  The reference of a group
of cases (one shape, one coil count) is evaluated once at K = 0 and shared by the group's settings."""
import numpy as np
import pytest

from indigo_amd.sense import SenseProblem
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
NAN = np.nan + 1j * np.nan
DEFAULT = (-1, 2)        # the library's default (K, S; -1: chunks of 128 MiB): restored after every test (the backend is shared by the session)

SHAPES = [((128, 128, 128), 2.0),      # grid 256^3, half box: the 256-point route
          ((160, 160, 160), 1.6),      # grid 256^3, run-time box
          ((256, 128, 128), 2.0),      # grid 512 x 256 x 256: 512 points on x only
          ((128, 128, 256), 2.0)]      # grid 256 x 256 x 512: ny != nz
COILS = [8, 4, 2]
# (K, S): one plane per chunk; 3 planes (ragged on 128 and 160 and 256 planes alike); 2 planes on three streams; 5 planes, a ragged last
# chunk on 128 and 256 planes; K >= planes, a single chunk; three planes on the backend's stream alone
SETTINGS = [(1, 2), (3, 2), (2, 3), (5, 3), (1 << 20, 2), (3, 1)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _set(hip, K, S):
    hip.set_option('fft.xy_chunk_planes', K)
    hip.set_option('fft.xy_chunk_streams', S)


def _problem(image, osf, coils, nspokes=300):
    return SenseProblem.synthetic(image, coils, nspokes=nspokes, nreadout=2 * image[0], width=2, ntable=128, oversamp=osf, seed=5,
                                  lazy_maps=True)


def _leaf(tree, layout=2):
    from indigo_amd import operators as op
    tree = tree.child if isinstance(tree, op.HeadRows) else tree
    Z = tree.right
    assert isinstance(Z, op.ZpadFFT) and Z._layout == layout
    return Z


def _flags(p, Z):
    """[ky, kz, kx tile] -> whether the support table flags the segment (as tests/test_hip_zc_intermediate.py reads it)"""
    n0, n1, n2 = p.oN
    tile = int(Z._tile_kw.get('support_tile', 16))
    _, _, bits = p.split_support(Z._support_h, tile)
    kz = np.arange(n2)
    b = bits.reshape(n1, n0 // tile, 16)
    return ((b[:, :, kz % 16] >> (kz // 16).astype(np.uint32)) & 1).astype(bool).transpose(0, 2, 1), tile


class _Group:
    """one shape and coil count: the leaf, its poisoned inputs on the device, and the K = 0 results"""

    def __init__(self, hip, image, osf, coils):
        self.p = p = _problem(image, osf, coils)
        hip._scratch = None
        self.Z = Z = _leaf(p.build_zpadfft(hip, layout=2))
        assert Z._C == coils
        n0, n1, n2 = p.oN
        self.nel = n0 * n1 * n2 * coils
        flag, tile = _flags(p, Z)
        assert flag.any() and not flag.all(), "the table has flagged and unflagged segments"
        self.poison_d = hip.copy_array(np.full((self.nel, 1), NAN, dtype=C64))
        self.nan_img_d = hip.copy_array(np.full((Z.shape[1], 1), NAN, dtype=C64))
        self.x_d = hip.copy_array(rand64c(int(np.prod(p.N)), 1, seed=1))
        _set(hip, 0, 1)
        g, _ = self.run(hip)
        g5 = g.reshape(n1, n2, n0 // tile, tile, coils)
        assert not np.isnan(g5[flag].real).any(), "flagged segments are written"
        assert np.isnan(g5[~flag].real).all() and np.isnan(g5[~flag].imag).all(), "an unflagged segment of the grid was written"
        # the adjoint's input: the grid of K = 0, NaN in every unflagged segment (it already is: nobody writes them)
        self.g_in_d = hip.copy_array(g)
        self.grid0 = _bits(g).copy()
        _, img = self.run(hip, adjoint=True)
        assert not np.isnan(img.real).any()
        self.img0 = _bits(img).copy()

    def run(self, hip, adjoint=False):
        """forward over a poisoned grid -> the grid; adjoint of g_in over a poisoned image -> the image"""
        Z = self.Z
        if not adjoint:
            g_d = hip.empty_array((self.nel, 1), C64)
            g_d._copy(self.poison_d)
            Z.eval(g_d, self.x_d, forward=True)
            return g_d.to_host(), None
        img_d = hip.empty_array((Z.shape[1], 1), C64)
        img_d._copy(self.nan_img_d)
        Z.eval(img_d, self.g_in_d, forward=False)
        return None, img_d.to_host().reshape(-1)

    def drop(self, hip):
        hip._scratch = None
        self.p.drop_cache()


_group = {}


@pytest.fixture
def group(hip, request):
    """the group of the case's (image, osf, coils): kept while consecutive cases ask for the same one"""
    key = request.param
    if _group.get('key') != key:
        if 'g' in _group:
            _group.pop('g').drop(hip)
            _group.pop('key')
        try:
            _group['g'] = _Group(hip, *key)
            _group['key'] = key
        finally:
            _set(hip, *DEFAULT)
    yield _group['g']
    _set(hip, *DEFAULT)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "K%d-S%d" % s)
@pytest.mark.parametrize("group", [(im, osf, c) for im, osf in SHAPES for c in COILS], indirect=True,
                         ids=lambda k: "%s-osf%s-%dcoils" % ("x".join(map(str, k[0])), k[1], k[2]))
def test_results_are_bit_identical_with_one_launch_per_pass(hip, group, setting):
    _set(hip, *setting)
    g, _ = group.run(hip)
    # (the whole grid, bit for bit: the flagged segments are equal and the unflagged ones still hold the poison's NaN)
    assert np.array_equal(_bits(g), group.grid0), "k-space grid"
    del g
    _, img = group.run(hip, adjoint=True)
    assert np.array_equal(_bits(img), group.img0), "image"


def test_chunks_of_a_twelve_coil_tree_share_the_arena(hip):
    """12 coils as 8 + 4 on the 256 x 256 x 512 grid, both leaves in ONE scratch arena: forward of the tree, adjoint of its leaves"""
    from indigo_amd import operators as op
    from indigo_amd.transforms import reserve_for
    p = _problem((128, 128, 256), 2.0, 12)
    hip._scratch = None
    try:
        A = p.build_zpadfft(hip, layout=2, chunk=8)
        assert isinstance(A, op.VStack) and [_leaf(ch)._C for ch in A.children] == [8, 4]
        x_d = hip.copy_array(rand64c(A.shape[1], 1, seed=1))
        leaves = [_leaf(ch) for ch in A.children]
        # (the adjoint of the whole tree scatters with float atomics and is not repeatable bit for bit even at one setting; the leaves'
        # adjoints are, so they are compared leaf by leaf, on fixed grids, inside the arena)
        grids = [hip.copy_array(rand64c(int(np.prod(p.oN)) * Z._C, 1, seed=3 + i)) for i, Z in enumerate(leaves)]
        res = []
        for K, S in [(0, 1)] + SETTINGS:
            _set(hip, K, S)
            reserve_for(A, 1)
            y_d = hip.copy_array(np.full((A.shape[0], 1), NAN, dtype=C64))
            A.eval(y_d, x_d)
            imgs = []
            for Z, g_d in zip(leaves, grids):
                z_d = hip.copy_array(np.full((Z.shape[1], 1), NAN, dtype=C64))
                Z.eval(z_d, g_d, forward=False)
                imgs.append(z_d.to_host())
            res.append((_bits(y_d.to_host()), _bits(np.concatenate(imgs))))
        assert not np.isnan(res[0][0].view(np.float32)).any() and not np.isnan(res[0][1].view(np.float32)).any()
        for (K, S), r in zip(SETTINGS, res[1:]):
            assert np.array_equal(res[0][0], r[0]), "forward of the tree, K = %d on %d streams" % (K, S)
            assert np.array_equal(res[0][1], r[1]), "adjoint of the chunks' leaves, K = %d on %d streams" % (K, S)
    finally:
        _set(hip, *DEFAULT)
        hip._scratch = None
        p.drop_cache()


@pytest.fixture(scope="module")
def small(hip):
    """image 128^3 on the 256^3 grid, 8 coils: the leaf, a grid for its adjoint and the K = 0 image of that grid"""
    p = _problem((128, 128, 128), 2.0, 8)
    hip._scratch = None
    Z = _leaf(p.build_zpadfft(hip, layout=2))
    x_d = hip.copy_array(rand64c(int(np.prod(p.N)), 1, seed=2))
    g_d = hip.zero_array((int(np.prod(p.oN)) * 8, 1), C64)
    _set(hip, 0, 1)
    Z.eval(g_d, x_d, forward=True)
    img_d = hip.copy_array(np.full((Z.shape[1], 1), NAN, dtype=C64))
    Z.eval(img_d, g_d, forward=False)
    img0 = img_d.to_host().reshape(-1)
    assert not np.isnan(img0.real).any()
    _set(hip, *DEFAULT)
    yield dict(p=p, Z=Z, x_d=x_d, g_d=g_d, img0=img0)
    _set(hip, *DEFAULT)
    hip._scratch = None
    p.drop_cache()


def _cropped_sum(hip, Z, g_d, slabs=None):
    """ifft_cropped_sum of the leaf's grid over a poisoned image: one call, or the z pass and then the given slabs"""
    P, C = int(np.prod(Z._grid)), Z._C
    img_d = hip.copy_array(np.full((Z.shape[1], 1), NAN, dtype=C64))
    with hip.scratch(nbytes=Z._ws_bytes()) as ws:
        args = (img_d, g_d.reshape((P, C)), Z._weights(), Z._grid, Z._lo, Z._box, ws, Z._support())
        if slabs is None:
            hip.ifft_cropped_sum(*args, **Z._tile_kw)
        else:
            hip.ifft_cropped_sum(*args, slab='z', **Z._tile_kw)
            for z0, z1 in slabs:
                hip.ifft_cropped_sum(*args, slab=(z0, z1), **Z._tile_kw)
    return img_d.to_host().reshape(-1)


@pytest.mark.parametrize("setting", [(3, 2), (5, 3), (2, 1)], ids=lambda s: "K%d-S%d" % s)
def test_the_slab_route_chunks_inside_every_slab(hip, small, setting):
    """slab = 'z', then slabs of 7, 1, 42 and 78 planes -- none a multiple of K but the last at K = 3 and 2, one a single plane --
    against the unchunked single call"""
    Z, g_d = small['Z'], small['g_d']
    try:
        _set(hip, *setting)
        img = _cropped_sum(hip, Z, g_d, slabs=[(0, 7), (7, 8), (8, 50), (50, 128)])
        assert np.array_equal(_bits(img), _bits(small['img0']))
        img = _cropped_sum(hip, Z, g_d)
        assert np.array_equal(_bits(img), _bits(small['img0']))
    finally:
        _set(hip, *DEFAULT)


def test_what_follows_the_call_sees_the_finished_image(hip, small):
    """an axpby and a copy to the host issued right behind the adjoint, on the backend's stream: the chunks' streams were joined"""
    Z, g_d = small['Z'], small['g_d']
    want = None
    try:
        for K, S in [(0, 1), (2, 3), (5, 3), (1, 2)]:
            _set(hip, K, S)
            img_d = hip.copy_array(np.full((Z.shape[1], 1), NAN, dtype=C64))
            acc_d = hip.zero_array((Z.shape[1], 1), C64)
            Z.eval(img_d, g_d, forward=False)
            hip.axpby(0, acc_d, 2, img_d)                 # acc = 2 * img, right behind the last chunk
            got = acc_d.to_host().reshape(-1)
            want = got if want is None else want          # (the same two calls at K = 0)
            assert np.allclose(want, 2 * small['img0'], rtol=1e-6, atol=0)
            assert np.array_equal(_bits(img_d.to_host().reshape(-1)), _bits(small['img0'])), "K = %d on %d streams" % (K, S)
            assert np.array_equal(_bits(got), _bits(want)), "axpby behind the call, K = %d on %d streams" % (K, S)
    finally:
        _set(hip, *DEFAULT)


def test_twenty_evaluations_repeat_bit_for_bit(hip, small):
    """forward into a fresh grid, adjoint of that grid, twenty times at (2, 3): every image equals the first and the K = 0 one"""
    Z, x_d = small['Z'], small['x_d']
    try:
        _set(hip, 2, 3)
        g_d = hip.zero_array((int(np.prod(Z._grid)) * Z._C, 1), C64)
        img_d = hip.zero_array((Z.shape[1], 1), C64)
        for it in range(20):
            Z.eval(g_d, x_d, forward=True)
            Z.eval(img_d, g_d, forward=False)
            img = img_d.to_host().reshape(-1)
            assert np.array_equal(_bits(img), _bits(small['img0'])), "evaluation %d" % it
    finally:
        _set(hip, *DEFAULT)


@pytest.mark.parametrize("K,S,chunks", [(0, 1, 1), (3, 2, 43), (5, 3, 26), (128, 2, 1), (200, 3, 1)])
def test_every_call_site_reports_one_launch_per_chunk(hip, small, K, S, chunks):
    Z, x_d, g_d = small['Z'], small['x_d'], small['g_d']
    out_d = hip.zero_array((int(np.prod(Z._grid)) * Z._C, 1), C64)
    img_d = hip.zero_array((Z.shape[1], 1), C64)
    try:
        _set(hip, K, S)
        Z.eval(out_d, x_d, forward=True)              # (plans are made on first use)
        hip.barrier()
        hip.profile(True)
        Z.eval(out_d, x_d, forward=True)
        Z.eval(img_d, g_d, forward=False)
        hip.profile(False)
        prof = hip.profile_report()
        for site in ('fft_pad_x', 'fft_pad_y', 'fft_crop_y', 'fft_crop_x'):
            assert prof[site]['launches'] == chunks, (site, prof[site])
            assert prof[site]['total_ms'] > 0
        for site in ('fft_pad_z', 'fft_crop_z'):
            assert prof[site]['launches'] == 1
        if chunks > 1:       # each chunk carries its share of the pass's bytes
            _set(hip, 0, 1)
            hip.profile(True)
            Z.eval(out_d, x_d, forward=True)
            Z.eval(img_d, g_d, forward=False)
            hip.profile(False)
            whole = hip.profile_report()
            for site in ('fft_pad_x', 'fft_pad_y', 'fft_crop_y', 'fft_crop_x'):
                assert abs(prof[site]['bytes'] - whole[site]['bytes']) <= 1e-9 * whole[site]['bytes'] + chunks, site
    finally:
        hip.profile(False)
        _set(hip, *DEFAULT)


def _both_ways(hip, Z, nel, seed):
    """forward and adjoint of a leaf at K = 0 and at (2, 3), with the launches per call site -> [(grid bits, image bits, launches)]"""
    x_d = hip.copy_array(rand64c(Z.shape[1], 1, seed=seed))
    out = []
    for K, S in [(0, 1), (2, 3)]:
        _set(hip, K, S)
        g_d = hip.zero_array((nel, 1), C64)
        img_d = hip.copy_array(np.full((Z.shape[1], 1), NAN, dtype=C64))
        Z.eval(g_d, x_d, forward=True)
        hip.barrier()
        hip.profile(True)
        Z.eval(g_d, x_d, forward=True)
        Z.eval(img_d, g_d, forward=False)
        hip.profile(False)
        prof = hip.profile_report()
        out.append((_bits(g_d.to_host()), _bits(img_d.to_host()), {k: v['launches'] for k, v in prof.items() if k.startswith('fft_')}))
    return out


def test_the_option_is_a_no_op_off_its_route(hip):
    """a one-coil leaf of the per-coil layout 1, and a coil-interleaved grid of A x B axes (160^3): the same launches, the same bits"""
    try:
        for image, osf, coils, layout in [((128, 128, 128), 2.0, 1, 1), ((128, 128, 128), 1.25, 8, 2)]:
            p = _problem(image, osf, coils)
            hip._scratch = None
            try:
                Z = _leaf(p.build_zpadfft(hip, layout=layout), layout)
                (g0, i0, l0), (g1, i1, l1) = _both_ways(hip, Z, int(np.prod(p.oN)) * coils, seed=4)
                assert l0 == l1 and l0 and all(v == 1 for v in l0.values()), (l0, l1)
                assert not np.isnan(i0.view(np.float32)).any()
                assert np.array_equal(g0, g1) and np.array_equal(i0, i1), (image, osf, coils, layout)
            finally:
                hip._scratch = None
                p.drop_cache()
    finally:
        hip.profile(False)
        _set(hip, *DEFAULT)
