"""A float64 restatement of the BLAS-1 glue and of the fused CG passes (include/indigo_hip.h, csrc/ig_blas.hip), for the tests, and
inputs on which those kernels have no rounding at all.

Everything here is plain numpy in complex128 / float64.  float32 rounding is applied only where the header says the device rounds:
the (float) scalars of ig_caxpby, (float)*d_beta / (float)*d_alpha of ig_caxpby_dev, (float)alpha and (float)beta of the CG passes.

The exact cases: vectors of nonzero integers in [-8, 8] (exact_inputs), dyadic scalars, lamda = 0.5 and a step length 2^-k.  Every
product, every updated element and every float32 partial sum of the kernels is then a small multiple of a power of two and exactly
representable, whatever the grid and the order of the sums (tests/test_blas64_cpu.py establishes this on the CPU), so the kernels
must reproduce the values below bit for bit; the one rounded quantity is p' = r' + (float)beta p (see ulp32)."""
import numpy as np

C64 = np.dtype('complex64')
C128 = np.dtype('complex128')

# the launch geometry of ig_blas.hip that the shapes below are built around
BLK = 256                   # lanes per workgroup, two complex64 each on the 16-byte paths
GRID_CAP = 2048             # IG_MAX_RED_BLOCKS, and 8 workgroups on each of the MI355X's 256 CUs
RUN_ELEMS = 16              # elements a float32 run accumulates before it is flushed into a double (8 trips of two; 16 in k_reduce)

SMALL_N = (1, 2, 3, 511, 512, 513, 1023)                    # around one workgroup of 256 lanes x 2 elements; the odd ones have a tail
N_MID = 2 * GRID_CAP * BLK + 155                            # capped grid, a partial second trip, an odd tail
N_BIG = 2 * (8 * GRID_CAP * BLK + 1000) + 1                 # a ninth trip in the CG passes (the float run restarts); > 16 * cap for k_reduce

# dyadic (beta, alpha) pairs of ig_caxpby: kernel modes 0 (beta = 0), 1 (beta = 1), 2 (general), 3 (alpha = 0)
AXPBY_SCALARS = ((0, 1.5 - 0.25j), (1, -2), (1.5 - 0.25j, 0.5j), (0.5j, 1.5 - 0.25j), (-2, 0), (1.5 - 0.25j, 0))
CG_LAMDAS = (0.0, 0.5)
CG_KS = (0, 3)              # alpha = 2^-k
CSUM_SCALARS = ((0, 1), (0.5, 0.5 - 1j))                    # (beta, alpha) of the coil sums
DEV_BETA, DEV_ALPHA, DEV_ALPHA_SCALE = -0.75, 1.25, -0.5    # dyadic slot values of ig_caxpby_dev (beta_scale is 1 or 0.5)
DEV_COMBOS = tuple((db, bs, da) for db in (None, DEV_BETA) for bs in (1.0, 0.5) for da in (None, DEV_ALPHA))
CSUM_NCOLS = (1, 2, 3, 4, 6, 7, 8, 16, 32, 64)
CSUM_ROWS = (1, 63, 65, 257, 5001)


def f32(v):
    """a real scalar rounded to float32, as a Python float"""
    return float(np.float32(v))


def cf32(v):
    """a complex scalar with both parts rounded to float32"""
    v = complex(v)
    return complex(f32(v.real), f32(v.imag))


def _c(a):
    return np.asarray(a).astype(C128)


# ---- elementwise ------------------------------------------------------------------------------------------------------------------------

def axpby(beta, y, alpha, x):
    """beta y + alpha x with the scalars rounded to float32; beta == 0 does not read y (BLAS rule), alpha == 0 does not read x
    (ig_cscal passes none)"""
    b, a = cf32(beta), cf32(alpha)
    out = np.zeros(np.shape(y), dtype=C128)
    if b != 0:
        out = out + b * _c(y)
    if a != 0:
        out = out + a * _c(x)
    return out


def axpby_dev(d_beta, beta_scale, y, d_alpha, alpha_scale, x):
    """(beta_scale *d_beta) y + (alpha_scale *d_alpha) x, the slots rounded to float32, None standing for 1; y is always read"""
    b = f32(beta_scale) * (1.0 if d_beta is None else f32(d_beta))
    a = f32(alpha_scale) * (1.0 if d_alpha is None else f32(d_alpha))
    return b * _c(y) + a * _c(x)


def smax(val, arr):
    """max(arr[i], (float)val) over float32 values: no arithmetic, so the result is float32 and exact"""
    return np.maximum(np.asarray(arr, dtype=np.float32), np.float32(val))


# ---- reductions -------------------------------------------------------------------------------------------------------------------------

def dotc(x, y):
    """sum conj(x) y as (re, im)"""
    x, y = _c(x), _c(y)
    re = np.sum(x.real * y.real) + np.sum(x.imag * y.imag)
    im = np.sum(x.real * y.imag) - np.sum(x.imag * y.real)
    return float(re), float(im)


def nrm2sq(x):
    x = _c(x)
    return float(np.sum(x.real * x.real) + np.sum(x.imag * x.imag))


def csum_cols(X, alpha, beta, y):
    """beta y + alpha sum_j X[:, j] of a (rows, ncols) panel; beta == 0 does not read y"""
    X = _c(X)
    s = X.sum(axis=1) if X.shape[1] else np.zeros(X.shape[0], dtype=C128)
    b = cf32(beta)
    out = cf32(alpha) * s
    return out if b == 0 else out + b * _c(y)


def csum_il(X_il, alpha, beta, y):
    """the same sum; X_il is the (rows, ncols) array whose ROWS are contiguous in the device's memory"""
    return csum_cols(X_il, alpha, beta, y)


# ---- scalar programs --------------------------------------------------------------------------------------------------------------------

def scalar_ratio(num, den, scale):
    return 0.0 if den == 0.0 else scale * num / den


def scalar_ratio_gated(num, den, scale, gate_num, gate_den, gate_tol):
    stop = not (gate_num >= gate_tol * gate_den)
    return 0.0 if (den == 0.0 or stop) else scale * num / den


# ---- one CG iteration, as the header states its three passes ----------------------------------------------------------------------------

def cg_dot(p, Ap, lamda):
    """-> (Ap + lamda p, pap = sum Re(conj p . Ap'))"""
    p, Ap = _c(p), _c(Ap)
    lam = f32(lamda)
    if lam != 0.0:
        Ap = Ap + lam * p
    return Ap, float(np.sum(p.real * Ap.real) + np.sum(p.imag * Ap.imag))


def cg_step_r(r, Ap, pap, rr, r0, tol2):
    """-> (alpha, r - (float)alpha Ap, r2 = ||r'||^2); alpha = 0 when pap == 0 or once rr < tol2 r0"""
    stop = not (rr >= tol2 * r0)
    alpha = 0.0 if (pap == 0.0 or stop) else rr / pap
    r = _c(r) - f32(alpha) * _c(Ap)
    return alpha, r, nrm2sq(r)


def cg_step_xp(x, p, r, alpha, r2, rr, r0):
    """-> (beta, x + (float)alpha p, r + (float)beta p, hist); beta = 0 when rr == 0, hist = 0 when r0 == 0"""
    beta = 0.0 if rr == 0.0 else r2 / rr
    x, p = _c(x), _c(p)
    return beta, x + f32(alpha) * p, _c(r) + f32(beta) * p, (0.0 if r0 == 0.0 else r2 / r0)


def cg_iteration(n, p, Ap, r, x, lamda, rr, r0, tol2):
    """ig_cg_dot -> ig_cg_step_r -> ig_cg_step_xp on vectors of n elements; every output of the three calls"""
    assert all(np.size(v) == n for v in (p, Ap, r, x))
    Ap1, pap = cg_dot(p, Ap, lamda)
    alpha, r1, r2 = cg_step_r(r, Ap1, pap, rr, r0, tol2)
    beta, x1, p1, hist = cg_step_xp(x, p, r1, alpha, r2, rr, r0)
    return dict(Ap=Ap1, pap=pap, alpha=alpha, r=r1, r2=r2, beta=beta, x=x1, p=p1, rr_next=r2, hist=hist)


# ---- exact inputs -----------------------------------------------------------------------------------------------------------------------

def exact_inputs(n, seed, count=1):
    """`count` complex64 vectors of n elements whose real and imaginary parts are nonzero integers in [-8, 8]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        v = rng.integers(1, 9, size=2 * n).astype(np.float32)
        v *= (1 - 2 * rng.integers(0, 2, size=2 * n)).astype(np.float32)
        out.append(v.view(C64))
    return tuple(out)


def exact_cg_case(n, seed, lamda, k):
    """Inputs of one CG iteration without rounding: integer p, Ap, r, x with pap > 0 (Ap negated if the exact pap is negative, the
    next seed if it vanishes) and rr = pap 2^-k, so that alpha = 2^-k exactly; r0 = 3 rr, far above the tolerance gate.
    -> dict(p, Ap, r, x, lamda, rr, r0, tol2, k)"""
    while True:
        p, Ap, r, x = exact_inputs(n, seed, 4)
        pap = cg_dot(p, Ap, lamda)[1]
        if pap != 0.0:
            break
        seed += 1000003
    if pap < 0:
        Ap = -Ap
        pap = cg_dot(p, Ap, lamda)[1]
    assert pap > 0
    rr = pap * 2.0 ** -k
    return dict(p=p, Ap=Ap, r=r, x=x, lamda=lamda, rr=rr, r0=3.0 * rr, tol2=2.0 ** -20, k=k)


# ---- comparing ---------------------------------------------------------------------------------------------------------------------------

def is_f32(a):
    """True where the float64 / complex128 values are float32 numbers already"""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return bool(np.array_equal(a.astype(C64).astype(C128), a))
    return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


def ulp32(got, ref):
    """largest distance of the complex64 `got` from the float64 `ref` rounded to float32, in float32 ulps of that rounding, over both
    components: the measure for p' = r' + (float)beta p, a single correctly rounded fma on the device (1 ulp allows for the double
    rounding of the reference, float64 first and float32 after)"""
    g = np.ascontiguousarray(got, dtype=C64).view(np.float32).astype(np.float64)
    r32 = np.ascontiguousarray(np.asarray(ref).astype(C64)).view(np.float32)
    d = np.abs(g - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
    return float(d.max()) if d.size else 0.0


def ulp64(got, ref):
    """|got - ref| in ulps of the double ref"""
    return abs(got - ref) / np.spacing(abs(ref)) if ref != 0 else (0.0 if got == 0 else np.inf)
