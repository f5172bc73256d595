"""Extended-phase-graph simulation on the MI355X: ig_epg_sim_c64 against the float64 restatement in tests/epg64.py evaluated on the
float32-cast parameters, under the bound derived there; bits that do not depend on where an atom stands; the truncation; the limits;
and `basis --model fse` followed by `fit` at toy size."""
import ctypes
import os

import numpy as np
import pytest

import dict64
import epg64
from indigo_amd import dictmatch

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
PAD_OUT = 5         # NaN rows below every atom's records: ldo = nrec + 5

NS = (1, 3, 64, 65, 257)                        # one atom; part of a workgroup; whole workgroups; a workgroup and one; many
SS = (1, 2, 63, 64, 65, 130)                    # both sides of the block of 64 steps, and more than two blocks
KS = (1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256)        # both sides of 1, 2 and 4 states per lane, the limit

# every (S, nstates) once, with N rotating through its five values, and the corners
CASES = [(NS[(i + j) % 5], S, K) for i, K in enumerate(KS) for j, S in enumerate(SS)]
CASES += [c for c in [(257, 130, 256), (1, 1, 1), (257, 130, 1), (65, 130, 64)] if c not in CASES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _call(hip, params, steps, flags, nstates, ldo=None, nsteps=None):
    """the C entry on an output with PAD_OUT sentinel rows below every column -> (rc, (N, nrec) signal) with the sentinels and the
    parameters checked"""
    params = np.ascontiguousarray(params, dtype=np.float32)
    steps, flags = np.ascontiguousarray(steps, dtype=np.float64), np.ascontiguousarray(flags, dtype=np.int32)
    N, nrec = params.shape[0], int(np.count_nonzero(flags & 4))
    rows = nrec + PAD_OUT
    out_h = np.full((rows, N), np.nan, dtype=C64, order='F')
    cols_h = [np.asfortranarray(params[:, c:c + 1]) for c in range(3)]
    out_d, cols_d = hip.copy_array(out_h), [hip.copy_array(c) for c in cols_h]
    rc = hip._L.ig_epg_sim_c64(hip._ctx, N, steps.shape[0] if nsteps is None else nsteps, nstates, *(ctypes.c_void_p(c._arr) for c in cols_d),
                               ctypes.c_void_p(steps.ctypes.data), ctypes.c_void_p(flags.ctypes.data), ctypes.c_void_p(out_d._arr),
                               rows if ldo is None else ldo)
    out = out_d.to_host()
    keep = nrec if rc == 0 else 0
    assert np.array_equal(_bits(out[keep:]), _bits(out_h[keep:]))                       # the pad rows (all rows, after a refusal)
    for c_d, c_h in zip(cols_d, cols_h):
        assert np.array_equal(_bits(c_d.to_host()), _bits(c_h))                         # the parameters are not written
    return rc, out[:keep].T


WORST = {"ratio": 0.0}


@pytest.mark.parametrize("N,S,K", CASES, ids=lambda v: str(v))
def test_kernel_matches_the_float64_restatement(hip, N, S, K):
    """|device - float64| <= C_STEP (steps executed up to the record) 2^-24, C_STEP = 42 as derived in tests/epg64.py.  The
    worst ratio to that bound over all cases is printed: 0.033 on an MI355X."""
    rng = np.random.default_rng(10000 * K + 100 * S + N)
    params = epg64.random_params(N, rng)
    steps, flags = epg64.random_program(S, rng, all_flags=S >= 16)
    want = epg64.simulate(params, steps, flags, K)
    rc, got = _call(hip, params, steps, flags, K)
    hip._check(rc, "ig_epg_sim_c64")
    assert got.shape == want.shape and np.isfinite(got).all()
    ratio = (np.abs(got - want) / epg64.bound(flags)[None, :]).max()
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print("epg N %d S %d states %d: %d records, largest |signal| %.3f, error / bound %.3e; worst so far %.3e"
          % (N, S, K, want.shape[1], np.abs(want).max(), ratio, WORST["ratio"]))
    assert ratio <= 1.0
    # the backend method on the same input, in chunks: the same bits
    sig = hip.epg_signal(params, steps, flags, K, chunk=100)
    assert sig.dtype == C64 and sig.shape == want.shape and np.array_equal(_bits(sig), _bits(got))


@pytest.mark.parametrize("S,K", [(130, 16), (63, 32), (65, 33), (130, 129), (64, 256)], ids=lambda v: str(v))
def test_bits_do_not_depend_on_where_an_atom_stands(hip, S, K):
    """257 atoms, the same atoms in a permuted order, 5 of them alone, and the first call again: every atom's bits are the same"""
    rng = np.random.default_rng(S + K)
    params = epg64.random_params(257, rng)
    steps, flags = epg64.random_program(S, rng, all_flags=True)
    a = hip.epg_signal(params, steps, flags, K)
    perm = rng.permutation(257)
    b = hip.epg_signal(params[perm], steps, flags, K)
    assert np.array_equal(_bits(b), _bits(a[perm]))
    five = np.array([256, 0, 63, 64, 130])
    assert np.array_equal(_bits(hip.epg_signal(params[five], steps, flags, K)), _bits(a[five]))
    assert np.array_equal(_bits(hip.epg_signal(params, steps, flags, K)), _bits(a))
    assert np.abs(a - epg64.simulate(params, steps, flags, K)).max() <= epg64.bound(flags).max()


def test_truncation_is_part_of_the_definition(hip):
    t = epg64.TRUNC
    steps, flags = epg64.cpmg(t['te'], t['echoes'], t['flip'])
    p32 = t['params'].astype(np.float32)
    cut = epg64.simulate(p32, steps, flags, t['nstates'])
    full = epg64.simulate(p32, steps, flags, 2 * t['echoes'] + 2)
    assert np.abs(cut - full).max() > 1e-2
    got = hip.epg_signal(t['params'], steps, flags, t['nstates'])
    assert (np.abs(got - cut) <= epg64.bound(flags)[None, :]).all()
    got_full = hip.epg_signal(t['params'], steps, flags, 2 * t['echoes'] + 2)
    assert (np.abs(got_full - full) <= epg64.bound(flags)[None, :]).all()


def test_limits(hip):
    rng = np.random.default_rng(7)
    params = epg64.random_params(6, rng)
    steps, flags = epg64.cpmg(0.01, 6, 2.0)
    nrec = 6

    def refused(text, st=steps, fl=flags, K=8, **kw):
        rc, _ = _call(hip, params, st, fl, K, **kw)                                     # (_call checks that nothing was written)
        assert rc != 0
        with pytest.raises(RuntimeError, match=text):
            hip._check(rc, "ig_epg_sim_c64")
    refused("0 states, between 1 and 256", K=0)
    refused("257 states, between 1 and 256", K=257)
    refused("0 steps, between 1 and 65535", nsteps=0)
    refused("records nothing", fl=flags & 3)
    bad = flags.copy()
    bad[3] = 16
    refused("step 3 has the flags 16", fl=bad)
    for value, text in ((-1e-3, "step 2 has a negative duration"), (np.nan, "step 2 holds a value that is not finite"),
                        (np.inf, "step 2 holds a value that is not finite")):
        st = steps.copy()
        st[2, 3] = value
        refused(text, st=st)
    refused("leading dimension %d of out below the %d records" % (nrec - 1, nrec), ldo=nrec - 1)
    # out on top of t1: one buffer, t1 = its first 6 floats, out from byte 16 on
    buf_h = np.full((1024, 1), 0.5, dtype=np.float32, order='F')
    buf = hip.copy_array(buf_h)
    cols = [hip.copy_array(np.asfortranarray(params[:, c:c + 1])) for c in (1, 2)]
    st, fl = np.ascontiguousarray(steps), np.ascontiguousarray(flags)
    rc = hip._L.ig_epg_sim_c64(hip._ctx, 6, st.shape[0], 8, ctypes.c_void_p(buf._arr), ctypes.c_void_p(cols[0]._arr), ctypes.c_void_p(cols[1]._arr),
                               ctypes.c_void_p(st.ctypes.data), ctypes.c_void_p(fl.ctypes.data), ctypes.c_void_p(buf._arr + 16), nrec)
    assert rc != 0
    with pytest.raises(RuntimeError, match="out overlaps t1"):
        hip._check(rc, "ig_epg_sim_c64")
    assert np.array_equal(_bits(buf.to_host()), _bits(buf_h))
    # the limits themselves are served
    rc, got = _call(hip, params, steps, flags, 256)
    hip._check(rc, "ig_epg_sim_c64")
    assert (np.abs(got - epg64.simulate(params, steps, flags, 256)) <= epg64.bound(flags)[None, :]).all()
    with pytest.raises(ValueError, match="257 states, between 1 and 256"):
        hip.epg_signal(params, steps, flags, 257)


def _fse_round_trip(B, tmp, tag):
    """`basis --model fse` (12 T2 x 5 B1, 16 echoes, 150 degrees) on backend B, 200 voxels rho * atom through phi, `fit` on B
    -> (atoms, planted index, rho, fitted maps)"""
    stem = os.path.join(tmp, "fse_" + tag)
    atoms, params, phi = dictmatch.main(["basis", "--model", "fse", "--te", "0.01", "--echoes", "16", "--flip", "150", "--t2", "0.02:0.3:12",
                                         "--b1", "0.7:1.1:5", "--rank", "6", "--debug", "40", stem], backend=B)
    assert atoms.shape == (60, 16) and params.shape == (60, 3) and phi.shape == (16, 6)
    rng = np.random.default_rng(11)
    dims = (10, 5, 4)
    index = rng.integers(0, 60, 200)
    rho = (0.5 + 1.5 * rng.random(200)) * np.exp(2j * np.pi * rng.random(200))
    c = (rho[:, None] * (atoms.astype(np.complex128)[index] @ phi.conj())).astype(C64)
    rec = os.path.join(tmp, "scan_%s.rec.npy" % tag)
    np.save(rec, c.reshape(dims + (1, 1, 1, 6), order='F').T)
    out = dictmatch.main(["fit", "--atoms", stem + ".atoms.npy", "--params", stem + ".params.npy", "--basis", stem + ".phi.npy", "--debug", "40",
                          rec], backend=B)
    return atoms, params, phi, index, rho, out


def test_fse_dictionary_then_fit_recovers_t2_and_b1(hip, oracle_backend, tmp_path):
    """every voxel's atom -- its T2 and its B1 -- comes back exactly and rho to 1e-4.  Neighbouring compressed atoms differ by at
    least 1e-4 in normalised score (asserted below) against the float32 bound 4 (2K + 2) 2^-24 = 3.3e-6 of the match at K = 6."""
    atoms, params, phi, index, rho, out = _fse_round_trip(hip, str(tmp_path), "hip")
    d, _ = dictmatch.compress(atoms, phi)
    assert 1 - dict64.largest_cross_score(d.astype(C64)) >= 1e-4
    got = out['index'].reshape(-1, order='F')
    assert np.array_equal(got, index)
    assert np.array_equal(out['qmaps'].reshape((-1, 3), order='F'), params[index].astype(np.float32))
    assert np.abs(out['pd'].reshape(-1, order='F') - rho).max() <= 1e-4 * np.abs(rho).max()
    atoms_np, _, _, index_np, _, out_np = _fse_round_trip(oracle_backend, str(tmp_path), "numpy")
    assert np.array_equal(index_np, index) and np.array_equal(out_np['index'].reshape(-1, order='F'), got)
    assert np.abs(atoms - atoms_np).max() <= epg64.bound(np.array([1] + [7] * 16)).max() + 2e-7
