"""NLINV on the MI355X: ig_nlinv_product_c64 and ig_sobolev_weight_c64 against float64 (tests/nlinv64.py), the operators' adjointness
on the device, the pipeline of indigo_amd.nlinv against the same pipeline on the numpy oracle and against the restatement's own
figures, and the command lines of nlinv and pics --maps."""
import ctypes
import os

import numpy as np
import pytest

import nlinv64 as n64
from indigo_amd import nlinv, pics
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu

C64 = np.dtype('complex64')
PAD = 37
ALPHA, BETA = 0.75 - 0.5j, -0.25 + 1.5j
U = 2.0 ** -24

# HIP pipeline against the oracle pipeline on the scan of nlinv64 (10 Newton steps of up to 10 CG iterations in complex64 on either
# side): each bound is 3 x the figure measured on an MI355X, given in the comment
HIP_ORACLE_RESIDUAL = 3 * 1.79e-2        # residual history, largest element-wise difference relative to the oracle's value: measured 1.781e-2
HIP_ORACLE_IMAGE = 3 * 1.64e-3           # image, relative 2-norm over the support: measured 1.636e-3
HIP_ORACLE_MAPS = 3 * 1.84e-3            # maps, relative 2-norm over the support: measured 1.833e-3
MARGIN = 1.5                             # recovery errors against the truth: within this factor of the float64 restatement's


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _padded(hip, a, pad):
    """the panel a on the device with `pad` extra rows of NaN under every column, and the host copy"""
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _product(hip, rho, coils, x, y, adjoint, alpha, beta, pad, shift=0):
    """nlinv_product on panels with `pad` NaN rows under every column; `shift`: every array starts that many elements into its
    allocation.  Everything the call must not write comes back bit-identical.  -> y as (n, cols)"""
    n = rho.shape[0]

    def place(a):
        a_d, a_h = _padded(hip, np.concatenate([np.full((shift, a.shape[1]), np.nan, dtype=C64), a]), pad)
        return a_d, a_h, a_d[shift:shift + n]
    (r_d, r_h, _), (c_d, c_h, c_v), (x_d, x_h, x_v), (y_d, y_h, y_v) = place(rho.reshape(-1, 1)), place(coils), place(x), place(y)
    r_v = r_d.dense_rows(shift, shift + n)
    hip.nlinv_product(y_v, x_v, r_v, c_v, n, coils.shape[1], adjoint=adjoint, alpha=alpha, beta=beta)
    for a_d, a_h in ((r_d, r_h), (c_d, c_h), (x_d, x_h)):
        assert np.array_equal(_bits(a_d.to_host()), _bits(a_h))
    out = y_d.to_host()
    assert np.array_equal(_bits(out[:shift]), _bits(y_h[:shift])) and np.array_equal(_bits(out[shift + n:]), _bits(y_h[shift + n:]))
    return out[shift:shift + n]


WORST = {"rel": 0.0, "bound": 0.0}


@pytest.mark.parametrize("nc", [1, 3, 8, 9, 32])
@pytest.mark.parametrize("n", [1, 255, 2048, 5049])
def test_product_matches_float64(hip, n, nc):
    """|got - want| <= (nc + 6) 2^-23 (the sum of the magnitudes of the products that form the element, |beta y| included): the
    running-sum bound of float32 complex multiply-adds, derived, not measured.  PAD = 37 rows under every column: an odd leading
    dimension, the 8-byte form; pad 38 on the even n runs the 16-byte form on padded panels."""
    rho, coils = rand64c(n, 1, seed=n + nc).reshape(-1), rand64c(n, nc, seed=n + nc + 1)
    for adjoint in (False, True):
        cols_x, cols_y = (nc, 1 + nc) if adjoint else (1 + nc, nc)
        x, y = rand64c(n, cols_x, seed=n + 2), rand64c(n, cols_y, seed=n + 3)
        for alpha, beta, y0 in ((1, 0, np.full_like(y, np.nan)), (ALPHA, BETA, y)):
            for pad in ((PAD, 38) if n % 2 == 0 else (PAD,)):
                got = _product(hip, rho, coils, x, y0, adjoint, alpha, beta, pad).astype(np.complex128)
                want = n64.product(rho, coils, x, y, adjoint, alpha, beta)
                bound = (nc + 6) * 2.0 ** -23 * n64.product_magnitudes(rho, coils, x, y, adjoint, alpha, beta)
                assert np.isfinite(got).all()
                WORST["rel"] = max(WORST["rel"], np.linalg.norm(got - want) / np.linalg.norm(want))
                WORST["bound"] = max(WORST["bound"], (np.abs(got - want) / bound).max())
                assert (np.abs(got - want) <= bound).all(), (adjoint, beta, pad, (np.abs(got - want) / bound).max())
    print("nlinv_product n %d nc %d: worst relative 2-norm so far %.3e, worst share of the bound %.3f" % (n, nc, WORST["rel"], WORST["bound"]))


@pytest.mark.parametrize("n,nc", [(2048, 8), (2048, 3), (5048, 9)], ids=str)
def test_product_forms_give_the_same_bits(hip, n, nc):
    """an even n on contiguous aligned panels (16-byte accesses), the same with every pointer advanced by one element (8-byte
    accesses on an even n), padded panels with an even and with an odd leading dimension: the same bits"""
    rho, coils = rand64c(n, 1, seed=1).reshape(-1), rand64c(n, nc, seed=2)
    for adjoint in (False, True):
        cols_x, cols_y = (nc, 1 + nc) if adjoint else (1 + nc, nc)
        x, y = rand64c(n, cols_x, seed=3), rand64c(n, cols_y, seed=4)
        outs = [_product(hip, rho, coils, x, y, adjoint, ALPHA, BETA, pad, shift) for pad, shift in ((0, 0), (1, 1), (38, 0), (PAD, 0), (0, 2))]
        for o in outs[1:]:
            assert np.array_equal(_bits(o), _bits(outs[0]))
        # the stacked vectors an operator tree hands over
        xs, ys = (hip.copy_array(np.asfortranarray(a.reshape((-1, 1), order='F'))) for a in (x, y))
        hip.nlinv_product(ys, xs, hip.copy_array(rho), hip.copy_array(np.asfortranarray(coils.reshape((-1, 1), order='F'))), n, nc,
                          adjoint=adjoint, alpha=ALPHA, beta=BETA)
        assert np.array_equal(_bits(ys.to_host().reshape((n, cols_y), order='F')), _bits(outs[0]))


def test_product_argument_checks(hip):
    n, nc = 64, 2
    # elements: rho [0, 64), coils [64, 192), x [192, 384) (forward: 3 columns), y (2 columns, 128) anywhere from 400
    host = rand64c(800, 1, seed=9)
    buf = hip.copy_array(host)

    def call(y_off, n_=n, nc_=nc, ldc=n, ldx=n, ldy=n):
        return hip._L.ig_nlinv_product_c64(hip._ctx, n_, nc_, ctypes.c_void_p(buf._arr), ctypes.c_void_p(buf._arr + 8 * 64), ldc, 0,
                                           ctypes.c_void_p(buf._arr + 8 * 192), ldx, 1.0, 0.0, 0.0, 0.0, ctypes.c_void_p(buf._arr + 8 * y_off), ldy)
    with pytest.raises(RuntimeError, match="0 coils"):
        hip._check(call(400, nc_=0), "ig_nlinv_product_c64")
    with pytest.raises(RuntimeError, match="0 voxels"):
        hip._check(call(400, n_=0), "ig_nlinv_product_c64")
    for kw in ({'ldc': n - 1}, {'ldx': n - 1}, {'ldy': n - 1}):
        with pytest.raises(RuntimeError, match="leading dimension"):
            hip._check(call(400, **kw), "ig_nlinv_product_c64")
    for off, what in ((383, "x"), (200, "x"), (100, "coils"), (63, "rho"), (0, "rho")):
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(call(off), "ig_nlinv_product_c64")
    assert np.array_equal(_bits(buf.to_host()), _bits(host))
    hip._check(call(384), "ig_nlinv_product_c64")                           # adjacent to x, not overlapping
    after = buf.to_host()
    assert np.array_equal(_bits(after[:384]), _bits(host[:384])) and np.array_equal(_bits(after[512:]), _bits(host[512:]))
    want = n64.product(host[:64, 0], host[64:192, 0].reshape((n, nc), order='F'), host[192:384, 0].reshape((n, 3), order='F'))
    got = after[384:512, 0].reshape((n, nc), order='F')
    assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want)


# ---- the weight pass ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ab", [(220, 32), (10, 32), (30, 15)], ids=str)
@pytest.mark.parametrize("ncols", [1, 3, 8])
@pytest.mark.parametrize("dims", [(16, 12, 10), (17, 9, 5), (1, 1, 7), (32, 28, 24)], ids=str)
def test_sobolev_weight_matches_float64(hip, dims, ncols, ab):
    """|got - want| <= 4 2^-24 |want| element by element: one rounding of w, one of scale * w, a real x complex product.  Elements
    whose exact scale * w is below 2^-126 may come back anywhere between 0 and that magnitude times |x|.  A result below 2^-126 is
    a subnormal float32, spaced 2^-149: that spacing is added to the bound (the precision of the format, not of the kernel)."""
    N = int(np.prod(dims))
    x = rand64c(N, ncols, seed=N + ncols)
    for scale in (1.0 / np.sqrt(N), 1e-4):
        want = n64.weight(x, dims, ab[0], ab[1], scale)
        tiny = (scale * n64.weights(dims, *ab).reshape(-1, order='F') < 2.0 ** -126)[:, None] & np.ones((1, ncols), dtype=bool)
        outs = []
        for in_place in (False, True):
            x_d, x_h = _padded(hip, x, PAD)
            y_d, y_h = (x_d, x_h) if in_place else _padded(hip, np.full_like(x, np.nan), PAD)
            hip.sobolev_weight(y_d[:N], x_d[:N], dims, ncols, ab[0], ab[1], scale=scale)
            out = y_d.to_host()
            assert np.array_equal(_bits(out[N:]), _bits(y_h[N:]))
            if not in_place:
                assert np.array_equal(_bits(x_d.to_host()), _bits(x_h))
            outs.append(out[:N])
        got = outs[0].astype(np.complex128)
        assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
        for part in (np.real, np.imag):
            g, w = part(got), part(want)
            assert (np.abs(g - w)[~tiny] <= 4 * U * np.abs(w)[~tiny] + 2.0 ** -149).all(), (scale, (np.abs(g - w)[~tiny] / np.abs(w)[~tiny]).max() / U)
            assert (np.abs(g)[tiny] <= np.abs(w)[tiny] * (1 + 4 * U) + 2.0 ** -149).all() and (g[tiny] * w[tiny] >= 0).all()
    # w(k) and w(-k): identical bits
    ones = np.ones((N, 1), dtype=C64, order='F')
    y = hip.zero_array((N, 1), C64)
    hip.sobolev_weight(y, hip.copy_array(ones), dims, 1, ab[0], ab[1], scale=1.0)
    w = y.to_host().reshape(dims, order='F')
    mirrored = w[(-np.arange(dims[0])) % dims[0]][:, (-np.arange(dims[1])) % dims[1]][:, :, (-np.arange(dims[2])) % dims[2]]
    assert np.array_equal(_bits(w), _bits(mirrored)) and w[0, 0, 0] == 1


def test_sobolev_weight_argument_checks(hip):
    dims, N = (4, 4, 4), 64
    host = rand64c(400, 1, seed=3)
    buf = hip.copy_array(host)

    def call(y_off, ldy=N, ncols=2, a=10.0):
        return hip._L.ig_sobolev_weight_c64(hip._ctx, *dims, ncols, ctypes.c_double(a), ctypes.c_double(32.0), ctypes.c_double(1.0),
                                            ctypes.c_void_p(buf._arr + 8 * 100), N, ctypes.c_void_p(buf._arr + 8 * y_off), ldy)
    for off in (99, 101, 227, 30):                 # x = [100, 228): shifted by one either way, its last element, reaching into it
        with pytest.raises(RuntimeError, match="overlaps"):
            hip._check(call(off), "ig_sobolev_weight_c64")
    with pytest.raises(RuntimeError, match="overlaps"):
        hip._check(call(100, ldy=N + 2), "ig_sobolev_weight_c64")            # the same start with another leading dimension
    with pytest.raises(RuntimeError, match="leading dimensions"):
        hip._check(call(300, ldy=N - 1), "ig_sobolev_weight_c64")
    with pytest.raises(RuntimeError, match="columns"):
        hip._check(call(300, ncols=0), "ig_sobolev_weight_c64")
    with pytest.raises(RuntimeError, match="non-negative"):
        hip._check(call(300, ncols=1, a=-1.0), "ig_sobolev_weight_c64")
    assert np.array_equal(_bits(buf.to_host()), _bits(host))


# ---- the operators ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("dims", [(12, 10, 8), (32, 28, 24)], ids=str)
def test_operators_are_adjoint_pairs_and_follow_the_point(hip, dims, C):
    N = int(np.prod(dims))
    hip._scratch = None
    A, P, S, DF = n64.backend_model(hip, dims, C, 10.0, 32.0)
    u = rand64c(N * (1 + C), 1, seed=5).reshape(-1)
    keep = n64.set_point(hip, P, S, u)
    for name, node in (("NlinvProduct", P), ("SobolevCoils", S), ("DF", DF)):
        defect = n64.adjoint_defect(hip, node, seed=11)
        print("%s %s C %d: adjoint defect %.3e" % (name, dims, C, defect))
        assert defect <= 1e-5, name
    for adjoint in (False, True):
        got = n64.evaluate(hip, S, u, forward=not adjoint)
        want = n64.sobolev_coils(u, dims, C, 10.0, 32.0, adjoint=adjoint)
        assert np.linalg.norm(got - want) <= 1e-5 * np.linalg.norm(want)
    # set_point: the next evaluation reads the new arrays, and an update in place of the old ones as well (no stale device copy)
    v = rand64c(N * (1 + C), 1, seed=6).reshape(-1)
    first = n64.evaluate(hip, P, v)
    point = keep.to_host().reshape((N, 1 + C), order='F')
    assert np.linalg.norm(first - n64.product(point[:, 0], point[:, 1:], v.reshape((N, 1 + C), order='F')).reshape(-1, order='F')) <= 1e-6 * np.linalg.norm(first)
    other = rand64c(N * (1 + C), 1, seed=7)
    keep2 = hip.copy_array(other)
    P.set_point(keep2.dense_rows(0, N), keep2.dense_rows(N, N * (1 + C)))
    second = n64.evaluate(hip, P, v)
    o2 = other.reshape((N, 1 + C), order='F')
    want2 = n64.product(o2[:, 0], o2[:, 1:], v.reshape((N, 1 + C), order='F')).reshape(-1, order='F')
    assert np.linalg.norm(second - want2) <= 1e-6 * np.linalg.norm(want2) and np.linalg.norm(second - first) > 0.1 * np.linalg.norm(first)
    keep2.copy_from(np.asfortranarray(point.reshape((-1, 1), order='F')))
    assert np.array_equal(_bits(n64.evaluate(hip, P, v)), _bits(first))
    with pytest.raises(ValueError, match="set_point"):
        P.set_point(keep2.dense_rows(0, N - 1), keep2.dense_rows(N, N * (1 + C)))
    hip._scratch = None


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scan(tmp_path_factory, oracle_backend):
    return n64.write_scan(tmp_path_factory.mktemp("nlinv"), oracle_backend)


def _pipeline(B, path, state=None):
    z = np.load(path)
    B._scratch = None
    try:
        return nlinv.nlinv(B, z['data'].T, z['traj'].T, n64.DIMS, iters=n64.ITERS, cg_iters=n64.CG_ITERS, a=n64.SOBOLEV[0], b=n64.SOBOLEV[1],
                           osf=n64.OSF, width=n64.WIDTH, state=state)
    finally:
        B._scratch = None


def test_pipeline_matches_the_oracle_and_recovers_the_phantom(hip, oracle_backend, scan):
    """the scan and the options of the CPU test.  Measured on an MI355X: residuals hip 0.66452 0.48674 0.31864 0.19332 0.11782 0.07354
    0.04592 0.02940 0.01889 0.01213, oracle ... 0.07334 0.04608 0.02972 0.01923 0.01218 (the first five agree to five digits; the
    float64 restatement has 0.0735 0.0460 0.0294 0.0189 0.0122: the two complex64 realisations drift apart, the device's stays
    nearer to float64); HIP against the oracle as in the bounds at the top; against the truth image 0.0582 and maps 0.0399, the
    restatement's 0.0581 and 0.0399."""
    ph, ref = n64.phantom(oracle_backend), n64.reference(oracle_backend)
    sup = ph['support']
    state = {}
    image, maps, history = _pipeline(hip, scan, state)
    image_o, maps_o, history_o = _pipeline(oracle_backend, scan)
    res, res_o = np.array([h['residual'] for h in history]), np.array([h['residual'] for h in history_o])
    d_res = (np.abs(res - res_o) / res_o).max()
    d_img = np.linalg.norm((image - image_o)[sup]) / np.linalg.norm(image_o[sup])
    d_map = np.linalg.norm((maps - maps_o)[sup]) / np.linalg.norm(maps_o[sup])
    err_i, err_m = n64.image_error(image, ph), n64.maps_error(maps, ph)
    print("residuals: hip    %s" % " ".join("%.5f" % v for v in res))
    print("residuals: oracle %s" % " ".join("%.5f" % v for v in res_o))
    print("hip against oracle: residual history %.3e, image %.3e, maps %.3e" % (d_res, d_img, d_map))
    print("hip against the truth: image %.4f (restatement %.4f), maps %.4f (restatement %.4f)" % (err_i, ref['image_error'], err_m, ref['maps_error']))
    assert len(history) == n64.ITERS and all(1 <= h['cg_iters'] <= n64.CG_ITERS for h in history)
    assert all(later < earlier for earlier, later in zip([1.0] + list(res), res))
    assert d_res <= HIP_ORACLE_RESIDUAL and d_img <= HIP_ORACLE_IMAGE and d_map <= HIP_ORACLE_MAPS
    assert res[-1] <= MARGIN * ref['history'][-1]['residual']
    assert err_i <= MARGIN * ref['image_error'] and err_m <= MARGIN * ref['maps_error']
    n64.check_results(image, maps, state)


def test_command_line_then_pics(hip, scan, tmp_path):
    z = np.load(scan)
    path = os.path.join(str(tmp_path), "scan.npz")
    np.savez(path, data=z['data'], traj=z['traj'])
    hip._scratch = None
    try:
        image, maps, history = nlinv.main(["-i", "4", "--cg-iters", "5", "--debug", "40"] + n64.ARGS[8:] + ["--sobolev-a", "10", path], backend=hip)
        hip._scratch = None
        stem = os.path.splitext(path)[0]
        fi, fm = np.load(stem + ".nlinv.npy"), np.load(stem + ".maps.npy")
        assert fi.shape == n64.DIMS[::-1] and fm.shape == (1, n64.COILS) + n64.DIMS[::-1] and fi.dtype == C64 and fm.dtype == C64
        assert np.array_equal(fi.T, image) and np.array_equal(fm.T[..., 0], maps) and len(history) == 4
        res = [h['residual'] for h in history]
        assert all(later < earlier for earlier, later in zip([1.0] + res, res))
        rec = pics.main(["-i", "5", "--osf", str(n64.OSF), "--width", str(n64.WIDTH), "--maps", stem + ".maps.npy", "--debug", "40", path], backend=hip)
        assert rec.shape[:3] == n64.DIMS and np.isfinite(rec).all() and np.abs(rec).max() > 0
    finally:
        hip._scratch = None
