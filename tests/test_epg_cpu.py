"""Extended-phase-graph simulation on the numpy oracle backend: the float64 restatement in tests/epg64.py against closed forms, the
host form of Backend.epg_signal against the restatement, the program builders, the `basis --model fse | fisp` command line and the
error messages."""
import os

import numpy as np
import pytest

import epg64
from indigo_amd import dictmatch

C64 = np.dtype('complex64')
PARAMS = np.array([[1.0, 0.08, 1.0], [0.6, 0.05, 0.8], [2.5, 0.3, 1.2], [0.3, 0.02, 1.0]])


def _dm(B, argv):
    return dictmatch.main(argv + ["--debug", "40"], backend=B)


# ---- the definition against closed forms ----------------------------------------------------------------------------------------------

def test_cpmg_with_perfect_refocusing_is_exponential_decay():
    te, T = 0.012, 20
    sig = epg64.simulate(PARAMS, *epg64.cpmg(te, T, np.pi), nstates=T + 1)
    want = np.exp(-te * np.arange(1, T + 1)[None, :] / PARAMS[:, 1:2])
    for row in (0, 3):                                                        # the atoms with B1 = 1 (the others: the next test)
        assert np.abs(sig[row] - want[row]).max() <= 1e-15


def test_first_echo_of_an_alpha_train():
    te = 0.01
    for flip in (0.3, 1.0, 2.0, 3.0):
        sig = epg64.simulate(PARAMS, *epg64.cpmg(te, 3, flip), nstates=8)
        want = np.sin(PARAMS[:, 2] * np.pi / 2) * np.sin(PARAMS[:, 2] * flip / 2) ** 2 * np.exp(-te / PARAMS[:, 1])
        assert np.abs(sig[:, 0] - want).max() <= 1e-15


def test_spoiled_train_reaches_the_ernst_steady_state():
    alpha, tr, n = 0.4, 0.05, 400
    steps = np.tile([alpha, 0.0, 0.0, tr], (n, 1))
    flags = np.full(n, epg64.RECORD | epg64.SPOIL, dtype=np.int32)
    sig = epg64.simulate(PARAMS, steps, flags, nstates=4)
    E1 = np.exp(-tr / PARAMS[:, 0])
    th = PARAMS[:, 2] * alpha
    want = np.sin(th) * (1 - E1) / (1 - E1 * np.cos(th))
    assert np.abs(np.abs(sig[:, -1]) - want).max() <= 1e-14
    assert np.abs(sig[:, -1] - (-1j) * want).max() <= 1e-14                   # phase 0: F+ = -i sin(theta) Z


def test_more_states_than_shifts_truncate_nothing():
    rng = np.random.default_rng(3)
    steps, flags = epg64.random_program(20, rng)
    shifts = int(sum(bin(int(f) & 3).count("1") for f in flags))
    a = epg64.simulate(PARAMS, steps, flags, nstates=shifts + 1)
    b = epg64.simulate(PARAMS, steps, flags, nstates=shifts + 40)
    assert np.array_equal(a, b)


def test_truncation_is_part_of_the_definition(oracle_backend):
    t = epg64.TRUNC
    steps, flags = epg64.cpmg(t['te'], t['echoes'], t['flip'])
    cut = epg64.simulate(t['params'].astype(np.float32), steps, flags, t['nstates'])
    full = epg64.simulate(t['params'].astype(np.float32), steps, flags, 2 * t['echoes'] + 2)
    assert np.abs(cut - full).max() > 1e-2
    got = oracle_backend.epg_signal(t['params'], steps, flags, t['nstates'])
    assert got.dtype == C64 and got.shape == (3, t['echoes'])
    assert np.abs(got - cut).max() <= 2e-7


# ---- the host form against the restatement --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,S,K", [(1, 1, 1), (5, 16, 2), (33, 40, 7), (7, 130, 64), (3, 65, 256)], ids=lambda v: str(v))
def test_host_form_matches_the_float64_restatement(oracle_backend, N, S, K):
    rng = np.random.default_rng(100 * N + S + K)
    params = epg64.random_params(N, rng)
    steps, flags = epg64.random_program(S, rng, all_flags=S >= 16)
    assert S < 16 or set(flags.tolist()) == set(range(16))
    assert (steps[:, 2:] == 0).any() or S < 4
    want = epg64.simulate(params, steps, flags, K)
    got = oracle_backend.epg_signal(params.astype(np.float64), steps, flags, K, chunk=4)       # several chunks and a ragged last one
    assert got.dtype == C64 and got.shape == want.shape == (N, int(np.count_nonzero(flags & 4)))
    assert np.abs(got - want).max() <= 2e-7                                                   # the rounding of the result to complex64
    # the parameters are cast to float32 before anything else
    nudged = params.astype(np.float64) * (1 + 1e-9)
    assert np.array_equal(oracle_backend.epg_signal(nudged, steps, flags, K), got)


def test_program_fse_with_180_degrees_reproduces_the_t2_model(oracle_backend):
    t2 = dictmatch.grid("0.02:0.3:12")
    want, _ = dictmatch.atoms_t2(0.01, 16, t2)
    steps, flags = dictmatch.program_fse(0.01, np.full(16, np.pi))
    assert steps.shape == (17, 4) and flags.dtype == np.int32 and np.array_equal(flags, [1] + [7] * 16)
    params = np.stack([np.ones(12), t2, np.ones(12)], axis=1)
    sig = epg64.simulate(params, steps, flags, 17)
    assert np.abs(sig - want).max() <= 1e-12
    got = oracle_backend.epg_signal(params, steps, flags, 17)
    assert np.abs(got - want).max() <= 1e-6                                   # T2 cast to float32, the result to complex64


def test_program_fisp():
    steps, flags = dictmatch.program_fisp([0.1, 0.2, 0.3], [0.010, 0.012, 0.011], 0.003, phases=[0.0, 1.0, 2.0], ti=0.02)
    assert np.array_equal(flags, [8, 6, 6, 6])
    assert np.allclose(steps, [[np.pi, 0, 0.02, 0], [0.1, 0, 0.003, 0.007], [0.2, 1, 0.003, 0.009], [0.3, 2, 0.003, 0.008]], rtol=1e-15, atol=1e-18)
    steps, flags = dictmatch.program_fisp([0.1, 0.2], 0.01, 0.0)
    assert np.array_equal(flags, [6, 6]) and np.array_equal(steps[:, 2:], [[0, 0.01], [0, 0.01]])


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_basis_fse_model(oracle_backend, tmp_path):
    tmp = str(tmp_path)
    out = os.path.join(tmp, "fse")
    argv = ["basis", "--model", "fse", "--te", "0.01", "--echoes", "12", "--flip", "150", "--t2", "0.02:0.3:6", "--b1", "0.8:1.2:3",
            "--rank", "3", "--chunk", "7", out]
    atoms, params, phi = _dm(oracle_backend, argv)
    assert atoms.shape == (18, 12) and atoms.dtype == C64 and params.shape == (18, 3) and phi.shape == (12, 3)
    t2, b1 = np.geomspace(0.02, 0.3, 6), np.linspace(0.8, 1.2, 3)
    assert np.array_equal(params[:, 0], np.ones(18))                          # T1: the default, one value of 1.0
    assert np.allclose(params[:, 1], np.repeat(t2, 3), rtol=1e-14) and np.allclose(params[:, 2], np.tile(b1, 6), rtol=1e-14)     # B1 fastest
    want = epg64.simulate(params.astype(np.float32), *epg64.cpmg(0.01, 12, np.deg2rad(150.0)), nstates=13)      # min(T + 1, 256) states
    assert np.abs(atoms - want).max() <= 2e-7
    for name, a in (("atoms", atoms), ("params", params), ("phi", phi)):
        assert np.array_equal(np.load("%s.%s.npy" % (out, name)), a)
    # --flips and --t1 and --states: T1 slowest
    flips = np.linspace(180, 100, 12)
    np.save(os.path.join(tmp, "flips.npy"), flips)
    atoms2, params2, _ = _dm(oracle_backend, ["basis", "--model", "fse", "--te", "0.01", "--echoes", "12", "--flips", os.path.join(tmp, "flips.npy"),
                                              "--t2", "0.02:0.3:6", "--t1", "0.5:2:2", "--states", "5", "--rank", "3", out + "2"])
    assert atoms2.shape == (12, 12) and np.allclose(params2[:, 0], np.repeat([0.5, 2.0], 6)) and np.allclose(params2[:, 1], np.tile(t2, 2))
    steps, flags = dictmatch.program_fse(0.01, np.deg2rad(flips))
    assert np.abs(atoms2 - epg64.simulate(params2.astype(np.float32), steps, flags, 5)).max() <= 2e-7


def test_basis_fisp_model_and_the_t2_above_t1_drop(oracle_backend, tmp_path):
    tmp = str(tmp_path)
    T = 30
    flips = 10 + 50 * np.sin(np.linspace(0, np.pi, T)) ** 2
    phases = np.where(np.arange(T) % 2 == 0, 0.0, 180.0)
    tr = 0.012 + 0.002 * np.cos(np.arange(T))
    for name, a in (("flips", flips), ("phases", phases), ("tr", tr)):
        np.save(os.path.join(tmp, name + ".npy"), a)
    out = os.path.join(tmp, "fisp")
    argv = ["basis", "--model", "fisp", "--flips", os.path.join(tmp, "flips.npy"), "--tr", os.path.join(tmp, "tr.npy"), "--te", "0.003",
            "--phases", os.path.join(tmp, "phases.npy"), "--ti", "0.02", "--t1", "0.1:2:4", "--t2", "0.05:1:4", "--b1", "0.9:1.1:2",
            "--rank", "4", out]
    atoms, params, phi = _dm(oracle_backend, argv)
    t1, t2, b1 = np.geomspace(0.1, 2, 4), np.geomspace(0.05, 1, 4), np.array([0.9, 1.1])
    rows = [(a, b, c) for a in t1 for b in t2 for c in b1 if b <= a]
    assert 0 < len(rows) < 32 and params.shape == (len(rows), 3) and np.allclose(params, rows, rtol=1e-14)
    assert (params[:, 1] <= params[:, 0]).all()
    assert atoms.shape == (len(rows), T) and phi.shape == (T, 4)
    steps, flags = dictmatch.program_fisp(np.deg2rad(flips), tr, 0.003, phases=np.deg2rad(phases), ti=0.02)
    assert steps.shape == (T + 1, 4)
    assert np.abs(atoms - epg64.simulate(params.astype(np.float32), steps, flags, 32)).max() <= 2e-7              # 32 states by default
    assert np.array_equal(np.load(out + ".params.npy"), params) and np.array_equal(np.load(out + ".atoms.npy"), atoms)
    # one repetition time for all pulses, no inversion, no phases
    atoms1, _, _ = _dm(oracle_backend, argv[:5] + ["--tr", "0.012","--te", "0.003", "--t1", "0.5:2:2", "--t2", "0.05:0.1:2", "--states", "8", "--rank", "2", out + "1"])
    steps, flags = dictmatch.program_fisp(np.deg2rad(flips), 0.012, 0.003)
    p1 = np.array([[0.5, 0.05, 1], [0.5, 0.1, 1], [2, 0.05, 1], [2, 0.1, 1]], dtype=np.float32)
    assert np.abs(atoms1 - epg64.simulate(p1, steps, flags, 8)).max() <= 2e-7


def test_error_messages(oracle_backend, tmp_path):
    tmp = str(tmp_path)
    np.save(os.path.join(tmp, "f3.npy"), np.array([10.0, 20.0, 30.0]))
    np.save(os.path.join(tmp, "tr2.npy"), np.array([0.01, 0.01]))
    np.save(os.path.join(tmp, "trlow.npy"), np.array([0.01, 0.002, 0.01]))
    F3, out = os.path.join(tmp, "f3.npy"), os.path.join(tmp, "x")
    fse = ["basis", "--model", "fse", "--rank", "2"]
    fisp = ["basis", "--model", "fisp", "--rank", "2"]
    with pytest.raises(ValueError, match="--model fse needs --te, --echoes, --t2 and either --flip or --flips"):
        _dm(oracle_backend, fse + ["--te", "0.01", "--echoes", "4", "--t2", "0.02:0.3:4", out])
    with pytest.raises(ValueError, match="--model fse needs --te, --echoes, --t2 and either --flip or --flips"):
        _dm(oracle_backend, fse + ["--te", "0.01", "--echoes", "3", "--t2", "0.02:0.3:4", "--flip", "150", "--flips", F3, out])
    with pytest.raises(ValueError, match="--flips holds 3 angles for --echoes 4"):
        _dm(oracle_backend, fse + ["--te", "0.01", "--echoes", "4", "--t2", "0.02:0.3:4", "--flips", F3, out])
    for bad in ("0", "257"):
        with pytest.raises(ValueError, match="--states %s, between 1 and 256" % bad):
            _dm(oracle_backend, fse + ["--te", "0.01", "--echoes", "4", "--t2", "0.02:0.3:4", "--flip", "150", "--states", bad, out])
    with pytest.raises(ValueError, match="--model fisp needs --flips, --tr, --te, --t1 and --t2"):
        _dm(oracle_backend, fisp + ["--flips", F3, "--tr", "0.01", "--te", "0.003", "--t2", "0.02:0.3:4", out])
    with pytest.raises(ValueError, match="3 flip angles and 2 repetition times"):
        _dm(oracle_backend, fisp + ["--flips", F3, "--tr", os.path.join(tmp, "tr2.npy"), "--te", "0.003", "--t1", "0.5:2:2", "--t2", "0.02:0.3:4", out])
    with pytest.raises(ValueError, match="repetition time 0.002 of pulse 1 is below the echo time 0.003"):
        _dm(oracle_backend, fisp + ["--flips", F3, "--tr", os.path.join(tmp, "trlow.npy"), "--te", "0.003", "--t1", "0.5:2:2", "--t2", "0.02:0.3:4", out])
    with pytest.raises(ValueError, match="every atom of the grid has T2 > T1"):
        _dm(oracle_backend, fisp + ["--flips", F3, "--tr", "0.01", "--te", "0.003", "--t1", "0.01:0.02:2", "--t2", "0.1:0.3:4", out])
    # Backend.epg_signal itself
    steps, flags = epg64.cpmg(0.01, 4, 2.0)
    ok = np.array([[1.0, 0.1, 1.0]])
    for params, text in ((np.array([[0.0, 0.1, 1.0]]), "T1 and T2 must be positive"), (np.array([[1.0, -0.1, 1.0]]), "T1 and T2 must be positive"),
                         (np.array([[1.0, 0.1, np.nan]]), "not finite"), (np.ones((4, 2)), r"\(N, 3\) array of \(T1, T2, B1\)")):
        with pytest.raises(ValueError, match=text):
            oracle_backend.epg_signal(params, steps, flags, 4)
    for st, fl, K, text in ((steps, flags, 0, "0 states, between 1 and 256"), (steps, flags, 257, "257 states, between 1 and 256"),
                            (steps, flags & 3, 4, "records nothing"), (steps, flags + 16, 4, "flags must be in 0 ... 15"),
                            (steps * [1, 1, -1, 1], flags, 4, "negative duration"), (steps * [1, 1, np.nan, 1], flags, 4, "not finite"),
                            (steps[:0], flags[:0], 4, "1 <= S <= 65535"), (steps, flags[:3], 4, "one per step")):
        with pytest.raises(ValueError, match=text):
            oracle_backend.epg_signal(ok, st, fl, K)
