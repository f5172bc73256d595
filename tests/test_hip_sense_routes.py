"""Every route of the fused SENSE leaf (SenseProblem.build_zpadfft -> fused.assemble -> HipBackend.csr_matrix.forward / adjoint,
operators.ZpadFFT) against the float64 SENSE operator of oracle/sense64.py, which is built from the operator's definition and not
from the product's builders of G' (tests/test_sense_routes_cpu.py pins it to the reference's goldens).

Each case names the route it expects -- the chunk widths, the transform's axis shift and support tile, the separable records, the
forward kernel and the adjoint format of every chunk width -- and asserts it on the tree BEFORE anything is evaluated.  Then A,
A^H and A^H A + 0.2 I are compared with the reference on complex-normal inputs, globally and on the samples at the grid's faces,
corners and grid points only (a fault in a few taps hides in the global norm).  The trajectories put a quarter of their samples
there."""
import numpy as np
import pytest

from conftest import rel_err
from indigo_amd import operators as op
from indigo_amd.sense import SenseProblem, normal_operator
from oracle.sense64 import SenseF64

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
RTOL = 1e-5
LAMDA = 0.2

# name -> (image, oversampling, kernel half-width, coils of the problem).  The 'even' grid is 128 x 62 x 58: even axes whose modulation is a
# sign per cell times a constant, chirp-z y and z passes (62 = 2 * 31, 58 = 2 * 29) -- a grid of 0.46 M points
PROBLEMS = {
    'even-w0.75': ((64, 31, 29), 2.0, 0.75, 4),
    'even-w1': ((64, 31, 29), 2.0, 1, 4),
    'even-w1.5': ((64, 31, 29), 2.0, 1.5, 2),
    'even-w2': ((64, 31, 29), 2.0, 2, 8),
    'even-w2.5': ((64, 31, 29), 2.0, 2.5, 4),
    'even-w3': ((64, 31, 29), 2.0, 3, 8),
    'even-w3.5': ((64, 31, 29), 2.0, 3.5, 4),
    'even-w4': ((64, 31, 29), 2.0, 4, 2),
    'even-w4.5': ((64, 31, 29), 2.0, 4.5, 4),
    'odd-smooth-y': ((96, 90, 39), 1.5, 2, 3),           # grid 144 x 135 x 58: 135 = 3^3 * 5, odd and no chirp-z axis
    'x168': ((84, 31, 29), 2.0, 2.5, 4),                 # grid 168 x 62 x 58: x not a multiple of 16
    'chirp': ((120, 52, 77), 640 / 480, 2, 9),           # grid 160 x 69 x 102: 69 odd (chirp-z), 102 = 2 mod 4
}
GRIDS = {'odd-smooth-y': (144, 135, 58), 'x168': (168, 62, 58), 'chirp': (160, 69, 102)}

_cache = {}


def _problem(name):
    """(SenseProblem, per-coil float64 reference, inputs, edge-sample mask) -- built once per module"""
    if name in _cache:
        return _cache[name]
    N, osf, width, C = PROBLEMS[name]
    p = SenseProblem.synthetic(N, C, nspokes=48, nreadout=int(round(N[0] * osf)), width=width, oversamp=osf, seed=5)
    assert p.oN == GRIDS.get(name, tuple(2 * n for n in N))
    c = p.coord.reshape(3, -1, order='F').copy()
    rng = np.random.default_rng(11)
    k = c.shape[1] // 4
    for d in range(3):
        n = p.oN[d]
        # faces, corners and the last cell before the wrap-around (-0.5 is a grid point of an even axis, half a cell off one of an odd
        # axis), and grid points anywhere: a sample on a grid point has 2 width taps per axis
        c[d, :k] = np.where(rng.random(k) < 0.5, rng.choice([-0.5, -0.5 + 1.0 / n, 0.5 - 1.0 / n, 0.5 - 0.5 / n], size=k),
                            (rng.integers(0, n, size=k) - n // 2) / n)
    p.coord = c.reshape(p.coord.shape, order='F')
    p.drop_cache()
    edge = np.zeros(p.T, dtype=bool)
    edge[:k] = True
    Nn = int(np.prod(p.N))
    x = _randn(Nn, 1, seed=1)
    kk = _randn(C * p.T, 1, seed=2)
    ref = []
    for coil in range(C):
        R = SenseF64(p, coils=[coil])
        kc = kk[coil * p.T:(coil + 1) * p.T]
        ref.append(dict(fwd=R.forward(x), adj=R.adjoint(kc), adj_edge=R.adjoint(kc * edge[:, None]), nrm=R.normal(x), op=R))
    _cache[name] = (p, ref, x, kk, edge)
    return _cache[name]


def _randn(*shape, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(C64)


def _expected(ref, coils, x, T):
    fwd = np.concatenate([ref[c]['fwd'] for c in coils])
    adj = sum(ref[c]['adj'] for c in coils)
    adj_edge = sum(ref[c]['adj_edge'] for c in coils)
    nrm = sum(ref[c]['nrm'] for c in coils) + LAMDA * x.astype(np.complex128)
    return fwd, adj, adj_edge, nrm


# -- the route of a tree ------------------------------------------------------------------------------------------------------
def _trees(A):
    return list(A.children) if isinstance(A, op.VStack) else [A]


def _leaves(tree):
    t = tree.child if isinstance(tree, op.HeadRows) else tree
    return t.left.right, t.right            # KronI(w, G') * ZpadFFT


def observed_route(A, tuning):
    """what the tree will run: chunk widths, the transform's axis shift and support tile, the records, the forward kernel, the
    adjoint kernel of every chunk width -- the dispatch of HipBackend.csr_matrix.forward / adjoint, read off the tree's state"""
    widths = tuple(w for _, _, w in A._coil_chunks)
    G, Z = _leaves(_trees(A)[0])
    assert all(_leaves(t)[0] is G for t in _trees(A)), "the chunks share one gridding matrix"
    M = G._get_or_create_device_matrix()
    sep = getattr(M, '_sep', None)
    if sep is not None and tuning.get('sep_gather', True):
        fwd = 'sep' if tuning.get('gather_order', True) else 'sep-unordered'
    else:
        fwd = 'rw' if M._real_values() is not None else 'il'
    adj = {}
    for w in widths:
        sh, br, sl = (M._format(f, w, exact=True) for f in ('_shares', '_bricks', '_slots'))
        if sh is not None and sh['ntasks'] > 0 and tuning.get('sep_scatter', True):
            adj[w] = 'shares'
        elif br is not None:
            adj[w] = 'bricks%d' % br['words']
        elif sl is not None and sl['ntasks'] > 0:
            adj[w] = 'slots%d' % sl['words']
        else:
            adj[w] = 'gather'
    kshift = Z._tile_kw.get('kshift')
    support = None if Z._support_h is None else Z._tile_kw.get('support_tile', 16)
    return dict(widths=widths, kshift=kshift, support=support,
                sep=None if sep is None else (sep['tw'], 'g=1' if sep['gconst'] == 1 else 'g!=1'), fwd=fwd, adj=adj)


def check_route_queries(A, observed):
    """the matrix's own answer (forward_route / adjoint_route) agrees with the restatement above, for every chunk width"""
    import types
    M = _leaves(_trees(A)[0])[0]._get_or_create_device_matrix()
    y = types.SimpleNamespace(contiguous=True)
    for w in observed['widths']:
        assert M.forward_route(w) == {'sep': 'sep', 'sep-unordered': 'sep', 'rw': 'il_rw', 'il': 'il'}[observed['fwd']], (w, observed)
        assert M.adjoint_route(w, 0, y) == {'shares': 'shares', 'bricks': 'bricks', 'slots': 'slots', 'gather': 'gather_il'}[observed['adj'][w].rstrip('234')], \
            (w, observed)


def _route(widths, sep, fwd, adj, kshift=None, support=None):
    return dict(widths=tuple(widths), kshift=kshift, support=support, sep=sep, fwd=fwd, adj=adj)


# -- the checks -------------------------------------------------------------------------------------------------------------
def check_products(hip, A, name, coils):
    """A, A^H and A^H A + 0.2 I against the float64 reference, globally and on the edge samples; returns the worst error"""
    p, ref, x, kk, edge = _problem(name)
    T = p.T
    ksub = np.concatenate([kk[c * T:(c + 1) * T] for c in coils])
    fwd, adj, adj_edge, nrm = _expected(ref, coils, x, T)
    hip._scratch = None
    errs = {}
    y = A * x
    errs['fwd'] = rel_err(y, fwd)
    emask = np.tile(edge, len(coils))
    errs['fwd_edge'] = rel_err(y[emask], fwd[emask])
    errs['adj'] = rel_err(A.H * ksub, adj)
    errs['adj_edge'] = rel_err(A.H * (ksub * emask[:, None]), adj_edge)
    y_d = hip.zero_array((A.shape[1], 1), C64)
    normal_operator(A, lamda=LAMDA).eval(y_d, hip.copy_array(x))
    errs['normal'] = rel_err(y_d.to_host(), nrm)
    hip._scratch = None
    bad = {k: v for k, v in errs.items() if not v < RTOL}
    assert not bad, (name, coils, errs)
    return max(errs.values())


_MISSING = object()


def _with_tuning(hip, tuning, fn):
    """fn() with hip.tuning updated by `tuning` (the route is chosen when the tree is built, when its device matrix is built and
    when it is evaluated)"""
    saved = {k: hip.tuning.get(k, _MISSING) for k in tuning}
    hip.tuning.update(tuning)
    try:
        return fn()
    finally:
        for k, v in saved.items():
            if v is _MISSING:
                hip.tuning.pop(k, None)
            else:
                hip.tuning[k] = v


KS = (0, 34, 0)          # the chirp-z grid's folded shift: 69 // 2 on the y axis
S4 = (4, 'g=1')
CASES = [
    # tw = 4 / 6 / 8 / none, on the even grid
    ('even-w0.75', range(4), {}, _route([4], None, 'rw', {4: 'bricks2'}, support=8)),
    ('even-w0.75', range(2), {}, _route([2], None, 'rw', {2: 'slots3'}, support=16)),
    ('even-w1', range(4), {}, _route([4], S4, 'sep', {4: 'bricks2'}, support=8)),
    ('even-w1.5', range(2), {}, _route([2], S4, 'sep', {2: 'slots3'}, support=16)),
    ('even-w2', range(8), {}, _route([8], S4, 'sep', {8: 'bricks2'}, support=4)),
    ('even-w2.5', range(4), {}, _route([4], (6, 'g=1'), 'sep', {4: 'shares'}, support=8)),
    ('even-w3', range(8), {}, _route([8], (6, 'g=1'), 'sep', {8: 'shares'}, support=4)),
    ('even-w3', range(8), {'sep_scatter': False}, _route([8], (6, 'g=1'), 'sep', {8: 'gather'}, support=4)),
    ('even-w3.5', range(4), {}, _route([4], (8, 'g=1'), 'sep', {4: 'shares'}, support=8)),
    ('even-w4', range(2), {}, _route([2], (8, 'g=1'), 'sep', {2: 'slots3'}, support=16)),
    ('even-w4.5', range(4), {}, _route([4], None, 'rw', {4: 'bricks2'}, support=8)),
    # an odd 7-smooth axis without a chirp-z pass: the modulation stays in G' -- complex weights, stored taps
    ('odd-smooth-y', range(3), {}, _route([4], None, 'il', {4: 'bricks3'}, support=8)),
    ('odd-smooth-y', range(2), {}, _route([2], None, 'il', {2: 'slots4'}, support=16)),
    # an x axis that is no multiple of 16: no support table, no binned adjoint
    ('x168', range(4), {}, _route([4], (6, 'g=1'), 'sep', {4: 'gather'})),
    ('x168', range(2), {}, _route([2], (6, 'g=1'), 'sep', {2: 'gather'})),
    # the odd chirp-z grid, coil counts that are no power of two
    ('chirp', range(1), {}, _route([2], S4, 'sep', {2: 'slots3'}, kshift=KS, support=16)),
    ('chirp', range(3), {}, _route([4], S4, 'sep', {4: 'bricks2'}, kshift=KS, support=8)),
    ('chirp', range(5), {}, _route([4, 2], S4, 'sep', {4: 'bricks2', 2: 'slots3'}, kshift=KS, support=8)),
    ('chirp', range(9), {}, _route([8, 2], S4, 'sep', {8: 'bricks2', 2: 'slots3'}, kshift=KS, support=4)),
]


def _case_id(c):
    return "%s-C%d-%s" % (c[0], len(c[1]), ",".join("%s=%s" % kv for kv in sorted(c[2].items())) or "default")


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_route_against_float64(hip, case):
    name, coils, tuning, expect = case
    p = _problem(name)[0]
    A = _with_tuning(hip, tuning, lambda: p.build_zpadfft(hip, coils=list(coils)))
    assert _with_tuning(hip, tuning, lambda: observed_route(A, hip.tuning)) == expect
    _with_tuning(hip, tuning, lambda: check_route_queries(A, expect))
    err = _with_tuning(hip, tuning, lambda: check_products(hip, A, name, list(coils)))
    print("route %s: worst rel. error %.2e" % (_case_id(case), err))


# every tuning switch on ONE problem (no drop_cache in between), in both orders: a rebuild must not pick up a gridding matrix cached
# for another tuning (the folded / split matrices depend on the phases the tuning selects)
TUNING_SEQUENCE = [
    ({}, None, _route([4], S4, 'sep', {4: 'bricks2'}, kshift=KS, support=8)),
    ({'real_gridding': False}, None, _route([4], (4, 'g!=1'), 'sep', {4: 'bricks3'}, kshift=KS, support=8)),
    ({'fold_odd_axes': False}, None, _route([4], None, 'il', {4: 'bricks3'}, support=8)),
    ({'separable': False}, None, _route([4], None, 'rw', {4: 'bricks2'}, kshift=KS, support=8)),
    ({'sep_gather': False}, None, _route([4], S4, 'rw', {4: 'bricks2'}, kshift=KS, support=8)),
    ({'sep_scatter': False}, None, _route([4], S4, 'sep', {4: 'bricks2'}, kshift=KS, support=8)),
    ({'real_entries': False}, None, _route([4], S4, 'sep', {4: 'bricks3'}, kshift=KS, support=8)),
    ({'real_entries': False, 'separable': False}, None, _route([4], None, 'il', {4: 'bricks3'}, kshift=KS, support=8)),
    ({'gather_order': False}, None, _route([4], S4, 'sep-unordered', {4: 'bricks2'}, kshift=KS, support=8)),
    ({'bricks': ()}, None, _route([4], S4, 'sep', {4: 'gather'}, kshift=KS, support=8)),
    ({}, False, _route([4], S4, 'sep', {4: 'bricks2'}, kshift=KS)),
]


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_tuning_switches_on_one_problem(hip, order):
    p = _problem('chirp')[0]
    seq = TUNING_SEQUENCE if order == "forward" else TUNING_SEQUENCE[::-1]
    for tuning, support, expect in seq:
        A = _with_tuning(hip, tuning, lambda: p.build_zpadfft(hip, coils=[0, 1, 2, 3], support=support))
        assert _with_tuning(hip, tuning, lambda: observed_route(A, hip.tuning)) == expect, (tuning, support)
        _with_tuning(hip, tuning, lambda: check_route_queries(A, expect))
        err = _with_tuning(hip, tuning, lambda: check_products(hip, A, 'chirp', [0, 1, 2, 3]))
        print("tuning %s support=%s: worst rel. error %.2e" % (tuning, support, err))
        del A


def test_alpha_beta_nan_and_two_columns(hip):
    """y = alpha A x + beta y and y = alpha A^H k + beta y with complex alpha; a NaN-filled y at beta = 0 (must not be read); x and k
    with two columns (coil-interleaved grids: one panel per column)"""
    name, coils = 'chirp', [0, 1, 2, 3]
    p, ref, x, kk, edge = _problem(name)
    T = p.T
    A = p.build_zpadfft(hip, coils=coils)
    ksub = np.concatenate([kk[c * T:(c + 1) * T] for c in coils])
    fwd, adj, _, _ = _expected(ref, coils, x, T)
    alpha, beta = 0.5 - 0.25j, 1.5
    hip._scratch = None
    for forward, inp, exp in ((True, x, fwd), (False, ksub, adj)):
        rows = A.shape[0] if forward else A.shape[1]
        y0 = _randn(rows, 1, seed=3)
        y_d = hip.copy_array(y0)
        A.eval(y_d, hip.copy_array(inp), alpha=alpha, beta=beta, forward=forward)
        assert rel_err(y_d.to_host(), alpha * exp + beta * y0) < RTOL, ("alpha, beta", forward)
        y_d = hip.copy_array(np.full((rows, 1), np.nan, dtype=C64))
        A.eval(y_d, hip.copy_array(inp), alpha=alpha, beta=0, forward=forward)
        got = y_d.to_host()
        assert np.isfinite(got).all() and rel_err(got, alpha * exp) < RTOL, ("NaN y at beta = 0", forward)
    # two columns: the second one a different image / k-space vector
    x2 = np.asfortranarray(np.concatenate([x, _randn(x.shape[0], 1, seed=4)], axis=1))
    k2 = np.asfortranarray(np.concatenate([ksub, _randn(ksub.shape[0], 1, seed=5)], axis=1))
    R = SenseF64(p, coils=coils)
    assert rel_err(A * x2, R.forward(x2)) < RTOL
    assert rel_err(A.H * k2, R.adjoint(k2)) < RTOL
    y_d = hip.zero_array((A.shape[1], 2), C64)
    normal_operator(A, lamda=LAMDA, ncols=2).eval(y_d, hip.copy_array(x2))
    assert rel_err(y_d.to_host(), R.normal(x2, LAMDA)) < RTOL
    hip._scratch = None
