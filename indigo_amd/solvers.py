"""The proximal solvers of the reconstruction drivers and what they are made of: the power iteration that sizes their steps, the
non-smooth terms with their proximal maps (`ProxTerm`: L1-wavelet, locally low rank), the smooth data term that both solvers share,
and the solvers themselves, `fista_solve`, `tv_solve` and `tgv_solve`, on top of `Backend.fista` and `Backend.primal_dual`.  They log as `pics`,
the driver they serve (`indigo_amd.pics`; nlinv and ecalib take the power iteration)."""
import collections
import logging

import numpy as np

from indigo_amd.util import rand64c

log = logging.getLogger("pics")
_C64 = np.dtype('complex64')


def power_iteration(B, AHA, iters, seed=0):
    """largest eigenvalue of the Hermitian positive semi-definite AHA: `iters` power iterations from a seeded random start,
    the estimate ||AHA v|| for the last unit vector v"""
    n = AHA.shape[1]
    v = B.copy_array(rand64c(n, 1, seed=seed), name='power.v')
    w = B.zero_array((n, 1), _C64, name='power.w')
    B.scale(v, 1.0 / np.sqrt(B.norm2(v)))
    lam = 0.0
    for _ in range(int(iters)):
        AHA.eval(w, v)
        lam = float(np.sqrt(B.norm2(w)))
        if lam == 0:
            break
        B.axpby(0, v, 1.0 / lam, w)
    return lam


def wavelet_prox(B, W, dims, l1):
    """proxg(v, alpha) of l1 ||W v||_1 (W's coarse band excluded): v <- W^H soft_{alpha l1}(W v), in place (W is unitary); a v
    of several frames stacked is the panel of its frames, and W and the threshold act on every column"""
    n = int(np.prod(dims))

    def proxg(v, alpha):
        W.eval(v, v)
        B.soft_threshold(v.reshape((n, -1)), alpha * l1, dims, W.coarse)
        W.H.eval(v, v)
    return proxg


def wavelet_l1(coef, dims, coarse):
    """sum |coef| outside the coarse box of every frame, in complex128; coef: the host (N T, 1) wavelet coefficients"""
    coef = coef.reshape(tuple(dims) + (-1,), order='F')
    inside = np.zeros(tuple(dims), dtype=bool)
    inside[tuple(slice(0, c) for c in coarse)] = True
    return float(np.abs(coef[~inside].astype(np.complex128)).sum())


# a non-smooth term g of the objective, as the solvers take it: proxg(v, alpha) replaces v by prox_{alpha g}(v) in place,
# value(x) is g(x) as a float, text describes it in the log
ProxTerm = collections.namedtuple('ProxTerm', 'proxg value text')


def wavelet_term(B, dims, l1, wavelet='db2', levels=3):
    """l1 ||W x||_1 (W: operators.Wavelet on every frame, coarse band not penalised)"""
    W = B.Wavelet(dims, wavelet=wavelet, levels=levels)
    work = {}

    def value(x):
        if 'w' not in work:
            work['w'] = B.zero_array(x.shape, _C64, name='objective.w')
        W.eval(work['w'], x)
        return l1 * wavelet_l1(work['w'].to_host(), dims, W.coarse)
    return ProxTerm(wavelet_prox(B, W, dims, l1), value,
                    "%s wavelet, %d levels, coarse box %s of %s, l1 %g" % (wavelet, levels, W.coarse, tuple(dims), l1))


def llr_term(B, dims, frames, lam, block=8, shifts=False, seed=0):
    """lam sum_b ||M_b(x)||_*: the locally low-rank penalty on `frames` time frames with blocks of `block` voxels a side (clamped
    to `dims`).  proxg is Backend.llr_threshold with the threshold alpha lam, at shift (0, 0, 0) or, with `shifts`, at a shift
    drawn before every call, uniformly in [0, side) per axis from numpy.random.default_rng(seed) on the host.  value is that of
    shift 0."""
    dims = tuple(int(n) for n in dims)
    T = int(frames)
    sides = tuple(min(int(block), n) for n in dims)
    rng = np.random.default_rng(seed) if shifts else None

    def proxg(v, alpha):
        shift = tuple(int(rng.integers(0, b)) for b in sides) if shifts else (0, 0, 0)
        B.llr_threshold(v, alpha * lam, dims, T, sides, shift)

    def value(x):
        return lam * B.llr_norm(x, dims, T, sides)
    return ProxTerm(proxg, value, "locally low rank, blocks %s of %s, %d frames, lambda %g, %s" % (
        sides, dims, T, lam, "a random shift per prox call (seed %d)" % seed if shifts else "shift (0, 0, 0)"))


def smooth_term(B, AHA, AHy, ynorm2, tag, iters, rest):
    """What fista_solve and tv_solve share: f(x) = 1/2 x^H AHA x - Re(x^H b) + ynorm2 / 2 with b = AHy, copied to the device here
    -> (gradf and callback(k, x) for the backends' solvers, the list [(iteration, objective)] that the callback fills): at every 10th
    iteration and the last, and only when INFO is enabled, it logs the objective rest(f(x), x) as `tag`, with f(x) through the work
    vector `objective.q`, which the first such call allocates"""
    b = B.copy_array(AHy, name='AHy')
    work, objectives = {}, []

    def gradf(g, z):
        AHA.eval(g, z)
        B.axpby(1, g, -1, b)

    def callback(k, x):
        if not (k % 10 == 9 or k == iters - 1) or not log.isEnabledFor(logging.INFO):
            return
        if not work:
            work['q'] = B.zero_array((AHA.shape[1], 1), _C64, name='objective.q')
        AHA.eval(work['q'], x)
        objectives.append((k + 1, rest(0.5 * B.dot(x, work['q']) - B.dot(x, b) + 0.5 * ynorm2, x)))
        log.info("%s iter %d, objective %.9e", tag, *objectives[-1])
    return gradf, callback, objectives


def choose_step(B, AHA, power_iters, step, tag, say_step):
    """-> (L, step): L the largest eigenvalue of AHA (`power_iteration`) and step = 0.9 / L, or the `step` given and L = 0.9 / step.
    Logged as `tag`; say_step: with the step (tv_solve logs its own two steps afterwards)"""
    if step is not None:
        if say_step:
            log.info("%s: step %.6e (given)", tag, step)
        return 0.9 / step, step
    L = power_iteration(B, AHA, power_iters)
    log.info("%s: largest eigenvalue of A^H A + lamda I %.6e (%d power iterations)" + (", step %.6e" % (0.9 / L) if say_step else ""), tag, L, power_iters)
    return L, 0.9 / L


def fista_solve(B, AHA, AHy, dims, iters, l1, wavelet='db2', levels=3, power_iters=15, step=None, ynorm2=0.0, term=None):
    """min_x 1/2 x^H AHA x - Re(x^H AHy) + ynorm2 / 2 + g(x) by Backend.fista from x = 0, g = l1 ||W x||_1 (W's coarse band
    excluded; `wavelet_term`) or the `term` given in its place (`llr_term`);
    with AHA = A^H A + lamda I and AHy = A^H y that is 1/2 ||A x - y||^2 + lamda/2 ||x||^2 + g(x) for ynorm2 = ||y||^2.
    AHA of NT columns is T frames of the `dims` volume stacked: W and the threshold then act on every frame.
    Returns the image as a host (N, 1) array and the objectives logged: [(iteration, value)], every 10 iterations and the last."""
    if term is None:
        term = wavelet_term(B, dims, l1, wavelet, levels)
    _, step = choose_step(B, AHA, power_iters, step, "fista", True)
    log.info("fista: %s", term.text)
    gradf, callback, objectives = smooth_term(B, AHA, AHy, ynorm2, "fista", iters, lambda f, x: f + term.value(x))
    x = np.zeros((AHA.shape[1], 1), dtype=_C64, order='F')
    B.fista(gradf, term.proxg, step, x, maxiter=iters, callback=callback)
    return x, objectives


def tv_solve(B, AHA, AHy, dims, iters, mu, sigma=None, l1=0.0, wavelet='db2', levels=3, power_iters=15, step=None, ynorm2=0.0,
             frames=1, mu_t=0.0, term=None):
    """min_x 1/2 x^H AHA x - Re(x^H AHy) + ynorm2 / 2 + mu sum_i ||(D x)_i||_2 [+ l1 ||W x||_1] by Backend.primal_dual from x = 0,
    u = 0: with AHA = A^H A + lamda I and AHy = A^H y that is 1/2 ||A x - y||^2 + lamda/2 ||x||^2 + mu TV(x) [+ l1 ||W x||_1] for
    ynorm2 = ||y||^2.  D is operators.Gradient; the dual step is u <- proj_mu(u + sigma D(2 x_{k+1} - x_k)), the projection onto
    the 2-norm ball of radius mu at every voxel (Backend.tv_dual_step); proxg is `wavelet_prox` when l1 > 0, that of `term`
    (`llr_term`, whose value the objective then adds) when one is given, else the identity.

    Steps: L is the largest eigenvalue of AHA (`power_iteration`), or 0.9 / step when `step` is given; tau = 0.9 / L and
    sigma = L / 24 unless given.  With ||D||^2 <= 12:  1/tau - 12 sigma = L/0.9 - L/2 = 0.61 L >= L/2, the Condat-Vu condition.

    frames = T > 1: x is T frames stacked, frame t in rows [tN, (t+1)N), and the penalty is mu sum_t TV(x_t) + mu_t sum_{t<T-1}
    sum_i |x_{t+1}[i] - x_t[i]| (the wavelet term on every frame).  D is operators.GradientT, u has 4NT rows, the dual step is
    Backend.tv4_dual_step: the spatial components onto the ball of radius mu, the temporal one onto the disc of radius mu_t.
    With ||D4||^2 <= 16 the default sigma is L / 32:  1/tau - 16 sigma = L/0.9 - L/2 >= L/2, the same margin.  frames = 1 is
    the iteration above unchanged (mu_t does not enter).
    Returns the image as a host (N, 1) array and the objectives logged: [(iteration, value)], every 10 iterations and the last."""
    T = int(frames)
    if T == 1:
        comps, G, step_fn, step_args = 3, B.Gradient(dims), B.tv_dual_step, (mu, dims)
    else:
        comps, G, step_fn, step_args = 4, B.GradientT(dims, T), B.tv4_dual_step, (mu, mu_t, dims, T)
    L, _ = choose_step(B, AHA, power_iters, step, "tv", False)
    tau = 0.9 / L
    if sigma is None:
        sigma = L / (8 * comps)
    log.info("tv: tau %.6e, sigma %.6e, mu %g, %s", tau, sigma, mu, tuple(dims))
    if T > 1:
        log.info("tv: %d frames, mu_t %g", T, mu_t)
    assert term is None or not l1 > 0, "one prox slot: the wavelet term or `term`"
    if l1 > 0:
        term = wavelet_term(B, dims, l1, wavelet, levels)
    if term is not None:
        log.info("tv: %s", term.text)
    n = AHA.shape[1]
    work = {}

    def objective(val, x):
        if not work:
            work['d'] = B.zero_array((comps * n, 1), _C64, name='objective.d')
        G.eval(work['d'], x)
        diffs = work['d'].to_host().reshape((n // T, comps, T), order='F').astype(np.complex128)
        val += mu * float(np.sqrt((np.abs(diffs[:, :3]) ** 2).sum(axis=1)).sum())
        if T > 1:
            val += mu_t * float(np.abs(diffs[:, 3]).sum())
        return val if term is None else val + term.value(x)

    gradf, callback, objectives = smooth_term(B, AHA, AHy, ynorm2, "tv", iters, objective)
    u = B.zero_array((comps * n, 1), _C64, name='tv.u')

    def KH(g, v):
        G.eval(g, v, alpha=1, beta=1, forward=False)

    def dual_step(v, xn, xo):
        step_fn(v, xn, xo, sigma, *step_args)

    x = np.zeros((n, 1), dtype=_C64, order='F')
    B.primal_dual(gradf, term.proxg if term is not None else None, KH, dual_step, tau, x, u, maxiter=iters, callback=callback)
    return x, objectives


def tgv_solve(B, AHA, AHy, dims, iters, a1, a0, sigma=None, l1=0.0, wavelet='db2', levels=3, power_iters=15, step=None, ynorm2=0.0,
              frames=1, term=None):
    """min_{x, v} 1/2 x^H AHA x - Re(x^H AHy) + ynorm2 / 2 + a1 sum_i ||(D x - v)_i||_2 + a0 sum_i ||(E v)_i||_F [+ l1 ||W x||_1]
    by Backend.primal_dual from zero: second-order total generalized variation (Bredies, Kunisch, Pock 2010).  D is
    operators.Gradient, E operators.SymGradient, v a 3-component field that takes up the smooth part of the differences of x.  With
    K (x; v) = (D x - v; E v):  K^H is Backend.tgv_adjoint, the dual step Backend.tgv_dual_step, the projections of p onto the
    2-norm ball of radius a1 over 3 components and of q onto that of radius a0 over 6, at every voxel.  proxg acts on the x rows
    only: `wavelet_prox` when l1 > 0, that of `term` (`llr_term`) when one is given, else the identity.

    Layout, n = N * frames: the primal vector has 4n rows, x in [0, n) and v in [n, 4n) as a 3N x frames panel; the dual has 9n rows,
    p a 3N x frames panel in [0, 3n) and q a 6N x frames panel in [3n, 9n).  The frames (time frames, sets of maps or coefficient
    images) are independent columns: every image has its own v.  gradf evaluates AHA on the x rows and leaves the v rows to K^H,
    which writes them.

    Steps: L and tau = 0.9 / L as in `tv_solve`; sigma = L / 32 unless given.  With ||K||^2 <= 16:  1/tau - 16 sigma = L/0.9 - L/2,
    the margin that `tv_solve` keeps.
    Returns the image as a host (n, 1) array and the objectives logged: [(iteration, value)], every 10 iterations and the last."""
    cols = int(frames)
    N = int(np.prod(dims))
    n = AHA.shape[1]
    assert n == N * cols, (AHA.shape, dims, frames)
    L, _ = choose_step(B, AHA, power_iters, step, "tgv", False)
    tau = 0.9 / L
    if sigma is None:
        sigma = L / 32
    log.info("tgv: tau %.6e, sigma %.6e, a1 %g, a0 %g, %s", tau, sigma, a1, a0, tuple(dims))
    if cols > 1:
        log.info("tgv: %d images, each with its own v", cols)
    assert term is None or not l1 > 0, "one prox slot: the wavelet term or `term`"
    if l1 > 0:
        term = wavelet_term(B, dims, l1, wavelet, levels)
    if term is not None:
        log.info("tgv: %s", term.text)
    G, E = B.Gradient(dims), B.SymGradient(dims)
    work, last = {}, {}

    def objective(val, x):
        if not work:
            work['d'] = B.zero_array((3 * n, 1), _C64, name='objective.d')
            work['e'] = B.zero_array((6 * n, 1), _C64, name='objective.e')
        v = last['z'].dense_rows(n, 4 * n)
        G.eval(work['d'].reshape((3 * N, cols)), x.reshape((N, cols)))
        B.axpby(1, work['d'], -1, v)                                   # D x - v
        E.eval(work['e'].reshape((6 * N, cols)), v.reshape((3 * N, cols)))
        for radius, name, comps in ((a1, 'd', 3), (a0, 'e', 6)):
            t = work[name].to_host().reshape((N, comps, cols), order='F').astype(np.complex128)
            val += radius * float(np.sqrt((np.abs(t) ** 2).sum(axis=1)).sum())
        return val if term is None else val + term.value(x)

    gradf_x, callback_x, objectives = smooth_term(B, AHA, AHy, ynorm2, "tgv", iters, objective)

    def gradf(g, z):
        gradf_x(g.dense_rows(0, n), z.dense_rows(0, n))

    def KH(g, u):
        B.tgv_adjoint(g.dense_rows(0, n), g.dense_rows(n, 4 * n), u.dense_rows(0, 3 * n), u.dense_rows(3 * n, 9 * n), dims)

    def proxg(g, t):
        term.proxg(g.dense_rows(0, n), t)

    def dual_step(u, zn, zo):
        B.tgv_dual_step(u.dense_rows(0, 3 * n), u.dense_rows(3 * n, 9 * n), zn.dense_rows(0, n), zo.dense_rows(0, n),
                        zn.dense_rows(n, 4 * n), zo.dense_rows(n, 4 * n), sigma, a1, a0, dims)

    def callback(k, z):
        last['z'] = z
        callback_x(k, z.dense_rows(0, n))

    u = B.zero_array((9 * n, 1), _C64, name='tgv.u')
    z = np.zeros((4 * n, 1), dtype=_C64, order='F')
    B.primal_dual(gradf, proxg if term is not None else None, KH, dual_step, tau, z, u, maxiter=iters, callback=callback)
    return np.asfortranarray(z[:n]), objectives
