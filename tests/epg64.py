"""A float64 restatement of the extended-phase-graph simulation (Backend.epg_signal, ig_epg_sim_c64, indigo_amd.dictmatch --model
fse / fisp), for the tests, with the generators of their cases and the error bound of the float32 kernel.

The definition (Hargreaves' convention).  An atom (T1, T2, B1) has the state (F+_k, F-_k, Z_k), k = 0 ... nstates - 1, complex, with
Z_0 = 1 and everything else 0 at the start.  Step s of a program holds (flip, phase, a, b, flags) -- radians, seconds, flag bits
1 = SHIFT_A, 2 = SHIFT_B, 4 = RECORD, 8 = SPOIL -- and runs, in this order,

    1. RF(B1 flip, phase)   2. relax(a)   3. shift if SHIFT_A   4. append F+_0 to the output if RECORD
    5. relax(b)             6. shift if SHIFT_B                 7. F+_k = F-_k = 0 for all k if SPOIL

RF, for every k, with theta = B1 flip, c = cos^2(theta/2), s = sin^2(theta/2), e = exp(i phase):
    F+' = c F+ + e^2 s F- - i e sin(theta) Z
    F-' = conj(e)^2 s F+ + c F- + i conj(e) sin(theta) Z
    Z'  = -(i/2) conj(e) sin(theta) F+ + (i/2) e sin(theta) F- + cos(theta) Z
relax(d): F+_k and F-_k times exp(-d/T2), Z_k times exp(-d/T1), then Z_0 gains -expm1(-d/T1); the identity at d = 0.
shift, the assignments in this order: F+_k <- F+_(k-1) for k >= 1; F-_k <- F-_(k+1) for k < nstates - 1; F- at nstates - 1 <- 0;
F+_0 <- conj(new F-_0).  Z is untouched, and the F+ shifted past nstates - 1 is lost: the truncation is part of the definition.

The error bound of the float32 kernel, |device - float64| <= C_STEP * (steps executed up to the record) * 2^-24, u = 2^-24 below.
It counts the roundings of one step against the bound of the state's norm and is first order in u; nothing in it is fitted to what
a device returns.

  The norm.  w = (F+_k, F-_k, sqrt(2) Z_k)_k.  The state is the Fourier series over the voxel of a magnetisation that is nowhere
  longer than 1, with F+_0 = conj(F-_0) counted twice, so by Parseval ||w||_2^2 <= 2.  RF acts on each k by a matrix that is unitary
  in w (it rotates the magnetisation), relaxation shrinks every component, and a shift moves components, drops some and copies
  conj(F-_1) into both F+_0 and F-_0.
  RF.  The kernel holds c, e^2 s, e sin(theta) and cos(theta), rounded once from double (relative error u each).  Each of the six
  real numbers of state k after the pulse is a chain of five float32 fused multiply-adds (five roundings) of such coefficients with
  the six numbers before it: an error of at most 6 u sum |coefficient| |value|.  In w the coefficient rows are
  (c, Re e^2 s, Im e^2 s, Re e sin / sqrt 2, Im e sin / sqrt 2), of squared length c^2 + s^2 + sin^2(theta)/2 = (c + s)^2 = 1, and
  (sin/sqrt 2 twice over, cos), of squared length 1 too, so by Cauchy-Schwarz every one of the six errors is at most 6 u ||w_k|| and
  together, over all k, at most 6 sqrt(6) u ||w|| <= 6 sqrt(12) u = 20.8 u.
  Relaxation, twice a step.  One product with a once-rounded factor per number: 2 u ||w||; the recovery term of Z_0 is one more
  rounded constant below 1 inside the same fma: sqrt(2) u in w.  Two delays: 2 (2 sqrt 2 + sqrt 2) u = 8.5 u.
  Shifts and the spoiler move or clear numbers exactly.
  Propagation.  What a step adds, at most 29.3 u in w, reaches a later F+_0 through maps that do not lengthen it, but for the
  copy at the next shift, which can count one component twice: a factor of at most sqrt 2.  29.3 sqrt(2) = 41.4.
So C_STEP = 42.  (The coefficients' own double arithmetic and the float64 reference add errors of order 1e-16 per step.)
"""
import numpy as np

C64 = np.dtype('complex64')
SHIFT_A, SHIFT_B, RECORD, SPOIL = 1, 2, 4, 8
C_STEP = 42.0
U32 = 2.0 ** -24


def simulate(params, steps, flags, nstates):
    """-> (N, nrec) complex128: the definition above on the float64 values of `params` (N, 3) = (T1, T2, B1) as given"""
    p = np.asarray(params, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.float64).reshape(-1, 4)
    flags = np.asarray(flags).astype(np.int64).ravel()
    assert p.ndim == 2 and p.shape[1] == 3 and steps.shape[0] == flags.size and nstates >= 1
    N, K = p.shape[0], int(nstates)
    T1, T2, B1 = p[:, 0], p[:, 1], p[:, 2]
    S = np.zeros((N, 3, K), dtype=np.complex128)                  # S[:, 0] = F+, S[:, 1] = F-, S[:, 2] = Z
    S[:, 2, 0] = 1.0
    out = []

    def relax(S, d):
        E = np.stack([np.exp(-d / T2), np.exp(-d / T2), np.exp(-d / T1)], axis=1)
        S = S * E[:, :, None]
        S[:, 2, 0] += -np.expm1(-d / T1)
        return S

    def shift(S):
        new = S.copy()
        for k in range(1, K):
            new[:, 0, k] = S[:, 0, k - 1]
        for k in range(K - 1):
            new[:, 1, k] = S[:, 1, k + 1]
        new[:, 1, K - 1] = 0
        new[:, 0, 0] = np.conj(new[:, 1, 0])
        return new

    for (alpha, phi, a, b), f in zip(steps, flags):
        th = B1 * alpha
        c, s, sn, cs = np.cos(th / 2) ** 2, np.sin(th / 2) ** 2, np.sin(th), np.cos(th)
        e = np.exp(1j * phi)
        R = np.zeros((N, 3, 3), dtype=np.complex128)
        R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = c, e ** 2 * s, -1j * e * sn
        R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = np.conj(e) ** 2 * s, c, 1j * np.conj(e) * sn
        R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -0.5j * np.conj(e) * sn, 0.5j * e * sn, cs
        S = np.einsum('nij,njk->nik', R, S)
        S = relax(S, a)
        if f & SHIFT_A:
            S = shift(S)
        if f & RECORD:
            out.append(S[:, 0, 0].copy())
        S = relax(S, b)
        if f & SHIFT_B:
            S = shift(S)
        if f & SPOIL:
            S[:, :2, :] = 0
    assert out, "the program records nothing"
    return np.stack(out, axis=1)


def steps_at_records(flags):
    """the number of steps executed up to and including each record's own"""
    flags = np.asarray(flags).ravel()
    return (np.flatnonzero(flags & RECORD) + 1).astype(np.float64)


def bound(flags):
    """the (nrec,) bound on |float32 kernel - float64| of the module docstring"""
    return C_STEP * steps_at_records(flags) * U32


def random_params(N, rng):
    """(N, 3) float32: T1 in [0.1, 3], T2 in [0.01, T1], B1 in [0.6, 1.3]"""
    t1 = rng.uniform(0.1, 3.0, N)
    t2 = rng.uniform(0.01, t1)
    return np.stack([t1, t2, rng.uniform(0.6, 1.3, N)], axis=1).astype(np.float32)


def random_program(S, rng, all_flags=False):
    """-> (steps (S, 4), flags (S,) int32): flips in [0, pi], phases in [0, 2 pi), durations 0 (a third of them) or in [0, 0.05], random
    flags with at least one RECORD; all_flags: the sixteen values, each at least once (S >= 16)"""
    steps = np.empty((S, 4))
    steps[:, 0] = rng.uniform(0, np.pi, S)
    steps[:, 1] = rng.uniform(0, 2 * np.pi, S)
    steps[:, 2:] = np.where(rng.random((S, 2)) < 1 / 3, 0.0, rng.uniform(0, 0.05, (S, 2)))
    flags = rng.integers(0, 16, S).astype(np.int32)
    if all_flags:
        assert S >= 16
        flags[rng.permutation(S)[:16]] = np.arange(16)
    if not (flags & RECORD).any():
        flags[rng.integers(0, S)] |= RECORD
    return steps, flags


def cpmg(te, echoes, flip):
    """excitation (pi/2, phase pi/2), te/2, shift; per echo RF(flip, 0), te/2, shift, record, te/2, shift"""
    steps = [(np.pi / 2, np.pi / 2, te / 2, 0.0)] + [(flip, 0.0, te / 2, te / 2)] * echoes
    return np.array(steps), np.array([SHIFT_A] + [SHIFT_A | RECORD | SHIFT_B] * echoes, dtype=np.int32)


# the truncation case: 5 states on a 16-echo train of 2.0 rad pulses
TRUNC = dict(te=0.01, echoes=16, flip=2.0, nstates=5, params=np.array([[1.0, 0.08, 1.0], [0.8, 0.05, 0.9], [2.0, 0.2, 1.1]]))
