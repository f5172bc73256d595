"""Field-map estimation on the MI355X: ig_fmapest_init_r32 and ig_fmapest_step_r32 through HipBackend.fieldmap_init / fieldmap_step
against the float64 restatement in tests/fmapest64.py on the same float32 inputs, voxel by voxel within the derived rounding bounds
(fmapest64.step_bound / init_bound / cost_bound), and the driver indigo_amd.fmapest against itself on the numpy oracle backend."""
import numpy as np
import pytest

import fmapest64
from indigo_amd import fmapest

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
F32 = np.dtype('float32')
PAD = 37
# the seams of the lane layout (8 .. 64 lanes along x, 256 / lanes rows per workgroup, the row loop strides past 64 lanes): every n0
# once with an axis of length 1 and once without, n1 and n2 rotating through 1, 2, 5, 17
SHAPES = [(1, 5, 1), (1, 17, 2), (7, 1, 17), (7, 2, 5), (8, 17, 1), (8, 5, 17), (9, 1, 2), (9, 17, 5), (33, 2, 1), (33, 5, 2),
          (64, 1, 5), (64, 2, 17), (65, 5, 1), (65, 17, 2), (130, 1, 1), (130, 2, 5)]
ECHOES = {2: [0.002, 0.0043], 3: [0.002, 0.004, 0.0065], 4: [0.001, 0.0022, 0.0041, 0.0073],
          8: [0.001, 0.0019, 0.0031, 0.004, 0.0052, 0.0061, 0.0075, 0.0083]}
CYCLES = [0.3, 5.0, 50.0]
CASES = [(s, (2, 3, 4, 8)[i % 4], CYCLES[i % 3]) for i, s in enumerate(SHAPES)] + \
        [((33, 5, 2), E, c) for E in (2, 3, 4, 8) for c in CYCLES if (E, c) not in ((3, 0.3), (2, 0.3))] + \
        [((8, 260, 260), 2, 5.0)]                        # (more groups of rows than the grid holds: they stride)


def _guarded_field(hip, values):
    """N float32 values on the device between PAD NaN guards: (the view, the whole array, its host copy)"""
    host = np.full(values.size + 2 * PAD, np.nan, dtype=F32)
    host[PAD:PAD + values.size] = values
    whole = hip.copy_array(host)
    return whole[PAD:PAD + values.size], whole, host


def _guarded_panel(hip, y):
    """the N x E panel on the device with PAD NaN rows above and below every column"""
    host = np.full((y.shape[0] + 2 * PAD, y.shape[1]), np.nan, dtype=C64, order='F')
    host[PAD:PAD + y.shape[0]] = y
    whole = hip.copy_array(host)
    return whole[PAD:PAD + y.shape[0], :], whole, host


def _bits(a):
    return a.view(np.uint64 if a.dtype == C64 else np.uint32)


def _same(whole, host):
    return np.array_equal(_bits(whole.to_host()), _bits(host))


def _result(view_whole_host, n):
    """the N values of a guarded field after a kernel wrote them, once the guards are seen untouched"""
    _, whole, host = view_whole_host
    out = whole.to_host()
    assert np.array_equal(out[:PAD].view(np.uint32), host[:PAD].view(np.uint32))
    assert np.array_equal(out[PAD + n:].view(np.uint32), host[PAD + n:].view(np.uint32))
    return out[PAD:PAD + n]


def _inputs(dims, E, cycles, seed=0):
    te = ECHOES[E]
    n = int(np.prod(dims))
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((n, E)) + 1j * rng.standard_normal((n, E))).astype(C64)
    y[rng.random(n) < 0.1] *= np.float32(0.01)           # low-signal voxels
    y[::11] = 0                                           # and voxels without any
    f = (rng.uniform(-1.0, 1.0, n) * cycles / (te[-1] - te[0])).astype(F32)
    beta = float(np.float32(0.05 * fmapest.relative_beta_scale(y, te)))
    return te, n, y, f, beta


def _check_step(hip, dims, te, y, f, beta):
    """one step with and without the fused cost, everything the issue asks of it; -> (largest error / bound, cost error / bound)"""
    n = f.size
    yv, yw, yh = _guarded_panel(hip, y)
    old = _guarded_field(hip, f)
    new = _guarded_field(hip, np.full(n, np.nan, dtype=F32))
    assert hip.fieldmap_step(new[0], old[0], yv, te, beta, dims) is None
    out = _result(new, n)
    ref, bound = fmapest64.step(y, f, te, beta, dims), fmapest64.step_bound(y, f, te, beta, dims)
    err = np.abs(out.astype(np.float64) - ref)
    assert np.isfinite(out).all()
    assert (err <= bound).all(), (dims, len(te), beta, float((err / np.maximum(bound, 1e-300)).max()), int(np.argmax(err - bound)))
    costs = []
    for _ in range(2):
        again = _guarded_field(hip, np.full(n, np.nan, dtype=F32))
        costs.append(hip.fieldmap_step(again[0], old[0], yv, te, beta, dims, cost=True))
        assert np.array_equal(_result(again, n).view(np.uint32), out.view(np.uint32))     # f_new is the same bits with the cost
    assert costs[0] == costs[1]                                                            # and the cost from call to call
    ref_cost, cbound = fmapest64.cost(y, f, te, beta, dims), fmapest64.cost_bound(y, f, te, beta, dims)
    assert abs(costs[0] - ref_cost) <= cbound, (costs[0], ref_cost, cbound)
    alone = [hip.fieldmap_cost(old[0], yv, te, beta, dims) for _ in range(2)]                 # the cost without the step
    assert alone[0] == alone[1] and abs(alone[0] - ref_cost) <= cbound, (alone, ref_cost, cbound)
    assert _same(yw, yh) and _same(old[1], old[2])                                         # inputs and their guards untouched
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(bound > 0, err / bound, 0.0).max()
    return float(frac), abs(costs[0] - ref_cost) / cbound if cbound > 0 else 0.0


@pytest.mark.parametrize("dims,E,cycles", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_step_and_init_stay_within_the_rounding_bounds(hip, dims, E, cycles):
    te, n, y, f, beta = _inputs(dims, E, cycles, seed=n_seed(dims, E))
    frac, cfrac = _check_step(hip, dims, te, y, f, beta)
    frac0, _ = _check_step(hip, dims, te, y, f, 0.0)
    # without signal and without a penalty the voxel is left alone, bit for bit
    yv, _, _ = _guarded_panel(hip, y)
    old, new = _guarded_field(hip, f), _guarded_field(hip, np.full(n, np.nan, dtype=F32))
    hip.fieldmap_step(new[0], old[0], yv, te, 0.0, dims)
    assert np.array_equal(_result(new, n)[::11].view(np.uint32), f[::11].view(np.uint32))
    # the initial field, compared modulo the period 1 / dTE: at the wrap either branch is right
    init = _guarded_field(hip, np.full(n, np.nan, dtype=F32))
    hip.fieldmap_init(init[0], yv, dims, te)
    f0 = _result(init, n).astype(np.float64)
    k = 2.0 * np.pi * (te[1] - te[0])
    err0 = np.abs((k * (f0 - fmapest64.init(y, te)) + np.pi) % (2.0 * np.pi) - np.pi) / k
    bound0 = fmapest64.init_bound(y, te) + 2.0 ** -24 * np.abs(f0)
    assert (err0 <= bound0).all(), float((err0 / bound0).max())
    assert np.abs(f0).max() <= (0.5 / (te[1] - te[0])) * (1 + 1e-6)
    print("%s E %d, %.1f cycles: step error / bound %.3f (beta = 0: %.3f), cost %.3f, init %.3f" % (
        dims, E, cycles, frac, frac0, cfrac, float((err0 / bound0).max())))


def n_seed(dims, E):
    return dims[0] * 1000 + dims[1] * 10 + dims[2] + E


def test_exact_zeros_and_the_wrap_of_s(hip):
    """E = 2 with dTE = 2^-9 s, so that f = 512 Hz is one whole cycle and 256 Hz half a one, exactly: voxels with s = 0 exactly (a real
    positive p at f = 0 and at f = 512), with s = +-pi exactly, and with s within 1e-6 of +-pi from either side, through the data
    (p = -0.75 +- i 0.75e-6 c) and through the field (f = 256 +- one float32 spacing, 3e-5 Hz = 3.7e-7 rad); the rest random."""
    dims, te = (9, 5, 2), [2.0 ** -9, 2.0 ** -8]
    _, n, y, f, beta = _inputs(dims, 2, 0.3, seed=7)
    y[:, 0] = np.where(np.arange(n) % 2 == 0, 1.0, y[:, 0])
    special = [(0.75, 0.0), (0.75, 512.0), (0.5, -512.0), (-0.75, 0.0), (0.75, 256.0), (0.75, -256.0),
               (-0.75 + 0.6e-6j, 0.0), (-0.75 - 0.6e-6j, 0.0), (-0.75 + 0.2e-6j, 0.0), (-0.75 - 0.9e-6 * 0.75j, 0.0),
               (0.75, np.nextafter(np.float32(256.0), np.float32(300.0))), (0.75, np.nextafter(np.float32(256.0), np.float32(0.0))),
               (0.75, -np.nextafter(np.float32(256.0), np.float32(300.0))), (0.75, -np.nextafter(np.float32(256.0), np.float32(0.0)))]
    for j, (y1, fj) in enumerate(special):
        v = 2 * (3 * j + 1)                               # even voxels: y_0 = 1; spread over rows and both planes
        y[v, 1], f[v] = y1, fj
    s = [t[2] for t in fmapest64._pair_terms(y, f, te)][0]
    assert (np.abs(s[[2 * (3 * j + 1) for j in range(3)]]) < 1e-15).all()       # (the kernel's reduced phase is 0 exactly)
    assert (np.pi - np.abs(s[[2 * (3 * j + 1) for j in range(3, len(special))]]) < 1e-6).all()
    for b in (beta, 0.0):
        _check_step(hip, dims, te, y, f, b)


def test_the_hip_overrides_refuse_what_they_cannot_do(hip):
    dims, n = (4, 3, 2), 24
    y2, y9 = hip.zero_array((n, 2), C64), hip.zero_array((n, 9), C64)
    f = hip.copy_array(np.arange(2 * n, dtype=F32))
    before = f.to_host()
    a, b = f[:n], f[n:]
    te2, te3 = ECHOES[2], ECHOES[3]
    for y, te in ((hip.zero_array((n, 1), C64), [0.002]), (y9, np.arange(1, 10) * 1e-3)):
        with pytest.raises(ValueError, match="between 2 and 8"):
            hip.fieldmap_step(a, b, y, te, 0.1, dims)
    with pytest.raises(ValueError, match="between 2 and 8"):
        hip.fieldmap_init(a, y9, dims, np.arange(1, 10) * 1e-3)
    for te in ([0.004, 0.002], [0.002, 0.002]):
        with pytest.raises(ValueError, match="strictly increasing"):
            hip.fieldmap_step(a, b, y2, te, 0.1, dims)
        with pytest.raises(ValueError, match="strictly increasing"):
            hip.fieldmap_init(a, y2, dims, te)
    with pytest.raises(ValueError, match="overlaps"):
        hip.fieldmap_step(a, a, y2, te2, 0.1, dims)
    with pytest.raises(ValueError, match="overlaps"):
        hip.fieldmap_step(f[1:n + 1], a, y2, te2, 0.1, dims, cost=True)
    with pytest.raises(ValueError, match="N x E"):
        hip.fieldmap_step(a, b, y2, te3, 0.1, dims)
    with pytest.raises(ValueError, match="N x E"):
        hip.fieldmap_init(a, y2, (4, 3, 3), te2)
    with pytest.raises(ValueError, match="beta"):
        hip.fieldmap_step(a, b, y2, te2, -1e-3, dims)
    assert np.array_equal(f.to_host(), before)
    hip.fieldmap_step(a, b, y2, te2, 0.1, dims)           # adjacent halves of one array: fine (no signal: the penalty alone)
    ref = fmapest64.step(np.zeros((n, 2)), before[n:], te2, float(np.float32(0.1)), dims)
    np.testing.assert_allclose(f.to_host()[:n], ref, rtol=1e-6)


def test_the_driver_on_the_gpu_follows_the_oracle_backend(hip, oracle_backend):
    """24 x 20 x 18 voxels, E = 3, 50 iterations at the default beta.  The tolerance is 50 times the largest one-step bound along
    the iteration: it supposes that the iteration does not amplify errors, which holds near the minimum and is only supposed
    elsewhere.  DESIGN.md §3.21 records the observed fraction."""
    dims, te, iters = (24, 20, 18), ECHOES[3], 50
    y, _, _ = fmapest64.phantom(dims, te, seed=5)
    images = y.reshape(dims + (3,), order='F').astype(C64)
    ref = fmapest.estimate(oracle_backend, images, te, iters=iters, beta=0.1, cost_every=0)
    # the same iteration by hand, for the bound at every iterate
    panel = fmapest.normalised_panel(images)
    beta = float(np.float32(0.1 * fmapest.relative_beta_scale(panel, te)))
    B, n = oracle_backend, int(np.prod(dims))
    yd = B.copy_array(np.asfortranarray(panel))
    f, g = B.zero_array((n,), F32), B.zero_array((n,), F32)
    B.fieldmap_init(f, yd, dims, te)
    largest = float(fmapest64.init_bound(panel, te).max())
    for _ in range(iters):
        largest = max(largest, float(fmapest64.step_bound(panel, f.to_host(), te, beta, dims).max()))
        B.fieldmap_step(g, f, yd, te, beta, dims)
        f, g = g, f
    assert np.array_equal(f.to_host().reshape(dims, order='F'), ref)
    out = fmapest.estimate(hip, images, te, iters=iters, beta=0.1, cost_every=10)
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print("fmapest on hip against the oracle backend: max difference %.3e Hz, %d x the largest one-step bound %.3e Hz = %.3e (fraction %.3f)"
          % (err, iters, largest, iters * largest, err / (iters * largest)))
    assert err <= iters * largest, (err, iters * largest)
