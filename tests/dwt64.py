"""Float64 restatement of the wavelet transform of pics --l1, written from its definition and not from the
product's code: the Daubechies filters come from the spectral factorisation of the Daubechies polynomial, and every split is
an explicit per-axis analysis matrix.  Test infrastructure, no GPU."""
from math import comb

import numpy as np
import scipy.sparse as spp

TAPS = {'haar': 2, 'db2': 4, 'db4': 8}


def daubechies(taps):
    """minimum-phase Daubechies low-pass filter with `taps` = 2p coefficients, sum sqrt(2):
    H(z) = sqrt(2) ((1 + 1/z) / 2)^p Q(z) with |Q(e^iw)|^2 = P(sin^2(w/2)), P(y) = sum_{k<p} C(p-1+k, k) y^k; every root y_k of P
    gives the pair z, 1/z of z^2 - (2 - 4 y_k) z + 1 = 0 (y = (2 - z - 1/z) / 4), of which Q keeps the one inside the unit circle"""
    p = taps // 2
    P = [comb(p - 1 + k, k) for k in range(p)]                 # ascending powers of y
    inside = []
    for yk in np.roots(P[::-1]) if p > 1 else []:
        z = np.roots([1.0, -(2.0 - 4.0 * yk), 1.0])
        inside.append(z[np.argmin(np.abs(z))])
    q = np.real(np.poly(inside)) if inside else np.ones(1)     # coefficients of z^0, z^-1, ...
    binom = np.array([comb(p, k) for k in range(p + 1)], dtype=np.float64)
    h = np.convolve(binom, q)
    return h * (np.sqrt(2.0) / h.sum())


def highpass(h):
    return h[::-1] * (-1.0) ** np.arange(h.size)


def analysis_matrix(d, h):
    """the d x d matrix (scipy CSR) of one split of a line of length d: rows k < d/2 low-pass, rows d/2 + k high-pass, periodic"""
    g = highpass(h)
    M = np.zeros((d, d))
    for k in range(d // 2):
        for j in range(h.size):
            M[k, (2 * k + j) % d] += h[j]
            M[d // 2 + k, (2 * k + j) % d] += g[j]
    return spp.csr_matrix(M)


def passes(dims, wavelet, levels):
    """[(box, axis)] in forward order and the coarse box: an axis splits while its length is even and >= 2 taps"""
    taps = TAPS[wavelet]
    c = list(dims)
    out = []
    for _ in range(levels):
        before = len(out)
        for a in range(3):
            if c[a] % 2 == 0 and c[a] >= 2 * taps:
                out.append((tuple(c), a))
                c[a] //= 2
        if len(out) == before:
            break
    return out, tuple(c)


def coarse_box(dims, wavelet, levels):
    return passes(dims, wavelet, levels)[1]


def _apply(v, box, axis, M):
    sl = tuple(slice(0, c) for c in box)
    sub = np.moveaxis(v[sl], axis, 0)
    v[sl] = np.moveaxis((M @ sub.reshape((sub.shape[0], -1))).reshape(sub.shape), 0, axis)


def dwt(x, dims, wavelet, levels, inverse=False):
    """W x (inverse: W^T x) for x of shape (prod dims,) or (prod dims, ncols), F-ordered volumes, in complex128"""
    x = np.asarray(x)
    cols = x.reshape((int(np.prod(dims)), -1), order='F')
    v = cols.astype(np.complex128).reshape(tuple(dims) + (cols.shape[1],), order='F').copy()
    h = daubechies(TAPS[wavelet])
    plan, _ = passes(dims, wavelet, levels)
    for box, a in (reversed(plan) if inverse else plan):
        M = analysis_matrix(box[a], h)
        _apply(v, box, a, M.T if inverse else M)
    return v.reshape(x.shape, order='F')


def dwt_abs(a, dims, wavelet, levels, inverse=False):
    """the same passes with |M| in place of every analysis matrix, on a non-negative real array of the shape `dwt` takes: the
    magnitudes a transform's roundings scale with.  Every pass of a float32 transform computes an output as TAPS fmas on exact
    products of rounded filter constants, an error of at most (TAPS + 2) 2^-24 sum_j |M_kj| |v_j|; later passes carry it on through
    their own |M|, so a whole transform of complex x is elementwise within
        npasses (TAPS + 2) 2^-24 dwt_abs(|x|)
    of the exact one (first order in 2^-24; for the moduli of complex values by the triangle inequality)"""
    a = np.asarray(a, dtype=np.float64)
    assert (a >= 0).all()
    cols = a.reshape((int(np.prod(dims)), -1), order='F')
    v = cols.reshape(tuple(dims) + (cols.shape[1],), order='F').copy()
    h = daubechies(TAPS[wavelet])
    plan, _ = passes(dims, wavelet, levels)
    for box, ax in (reversed(plan) if inverse else plan):
        M = abs(analysis_matrix(box[ax], h))
        _apply(v, box, ax, M.T if inverse else M)
    return v.reshape(a.shape, order='F')


U32 = 2.0 ** -24                                                   # the unit roundoff of float32


def dwt_bound(x, dims, wavelet, levels, inverse=False, alpha=1, beta=0, y0=None):
    """elementwise bound on |y - (alpha T x + beta y0)| for y = ig_dwt3_c64's float32 result, T = W or W^T (see dwt_abs).
    beta == 0: the passes, and one complex multiply by alpha when alpha != 1 (two roundings per component, 2 sqrt(2) < 3 for the
    modulus).  beta != 0: the kernel computes T (beta T^H y0 + alpha x) in three stages, whose errors add up."""
    per_transform = len(passes(dims, wavelet, levels)[0]) * (TAPS[wavelet] + 2) * U32
    ax = abs(alpha) * np.abs(np.asarray(x, dtype=np.complex128))
    if beta == 0:
        scaling = 0.0 if alpha == 1 else 3 * U32
        return (per_transform + scaling) * dwt_abs(ax, dims, wavelet, levels, inverse)
    thy = dwt(y0, dims, wavelet, levels, not inverse)              # T^H y0
    z1, z2 = np.abs(thy), np.abs(beta * thy + alpha * np.asarray(x, dtype=np.complex128))
    # stage 1, z1 = T^H y0 in place: the passes of the opposite direction; the combine then multiplies what they left by beta
    e1 = abs(beta) * per_transform * dwt_abs(np.abs(np.asarray(y0, dtype=np.complex128)), dims, wavelet, levels, not inverse)
    # stage 2, z2 = alpha x + beta z1: a complex multiply (2 roundings per component) and two fmas per component on top of it,
    # each rounding a partial sum of at most |alpha x| + |beta z1|: 4 roundings per component, 4 sqrt(2) < 6 for the modulus
    e2 = 6 * U32 * (ax + abs(beta) * z1)
    # stage 3, T z2 in place: carries e1 + e2 through |T| and adds its own passes' roundings
    return dwt_abs(e1 + e2, dims, wavelet, levels, inverse) + per_transform * dwt_abs(z2, dims, wavelet, levels, inverse)


def worst_ratio(err, bound):
    """max of err / bound; where the bound is 0 (an exact operation) any error at all is infinitely far out"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def dense(dims, wavelet, levels):
    """the transform's N x N matrix"""
    n = int(np.prod(dims))
    return dwt(np.eye(n), dims, wavelet, levels).real


def soft(u, tau, dims, keep):
    """complex soft threshold outside the coarse box `keep`, in float64"""
    u = np.asarray(u, dtype=np.complex128)
    v = u.reshape(tuple(dims) + (-1,), order='F')
    r = np.abs(v)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = np.where(r <= tau, 0.0, v * (1.0 - tau / r))
    sl = tuple(slice(0, c) for c in keep)
    out[sl] = v[sl]
    return out.reshape(u.shape, order='F')
