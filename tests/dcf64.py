"""Float64 / exact-integer restatement of the density-compensation kernels (ig_dcf_spread_r32, ig_dcf_gather_div_r32; DESIGN.md
§3.17), independent of the Backend host forms: the taps come from `interp.sep_expand`, the dense form of the separable records
in the kernels' float32 arithmetic ((w1 * w2) * w0), and everything after them is plain numpy / scipy.

    spread(sep, w, scale)            exact int64  acc = sum rint(tap * w * scale)
    gather_div(sep, acc, w, scale)   float64 s = sum tap * acc / scale, w_out = float32(w / s) (0 where s == 0)
    pipe_menon(sep, iters)           the iteration w <- w / (G G^H w) in float64 from w = 1 (mean 1)
    pipe_menon32(sep, iters)         the same iteration EMULATED in float32 numpy: every sum rounds
    weighted_cg(B, A, y, w, iters)   float64 CG on A^H W A x = A^H W y for an operator tree A of backend B
"""
import numpy as np
import scipy.sparse as spp

from indigo_amd.interp import sep_expand


def taps(sep, lo=0, hi=None):
    """(rows, cells, float32 values) of the records' taps: those inside every axis's tap count"""
    rows, cols, vals = sep_expand(sep, lo, hi)
    assert np.all(vals.imag == 0)
    return rows, cols, np.ascontiguousarray(vals.real, dtype=np.float32)


def matrix(sep, dtype=np.float64):
    """G as a CSR matrix, samples x grid cells (in the records' memory order), float32 tap values cast to `dtype`"""
    rows, cols, vals = taps(sep)
    n0, nm, ns = sep['dims']
    return spp.csr_matrix((vals.astype(dtype), (rows, cols)), shape=(sep['records'].shape[0], n0 * nm * ns))


def spread(sep, w, scale):
    rows, cols, vals = taps(sep)
    n0, nm, ns = sep['dims']
    q = np.rint(vals.astype(np.float64) * np.asarray(w, dtype=np.float32).astype(np.float64)[rows] * float(scale)).astype(np.int64)
    acc = np.zeros(n0 * nm * ns, dtype=np.int64)
    np.add.at(acc, cols, q)
    return acc


def gather_div(sep, acc, w, scale):
    """(w_out float32, s float64)"""
    rows, cols, vals = taps(sep)
    M = sep['records'].shape[0]
    s = np.bincount(rows, weights=vals.astype(np.float64) * acc[cols].astype(np.float64), minlength=M) / float(scale)
    wv = np.asarray(w, dtype=np.float32).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(s == 0, 0.0, wv / s).astype(np.float32)
    return q, s


def pipe_menon(sep, iters=30, normalise=True):
    G = matrix(sep, np.float64)
    w = np.ones(G.shape[0])
    for _ in range(iters):
        w = w / (G @ (G.T @ w))
    return w / w.mean() if normalise else w


def pipe_menon32(sep, iters=30):
    G = matrix(sep, np.float32)
    w = np.ones(G.shape[0], dtype=np.float32)
    for _ in range(iters):
        w = (w / (G @ (G.T @ w))).astype(np.float32)
    w = w.astype(np.float64)
    return w / w.mean()


def weighted_cg(A, y, w, iters, lamda=0.0, ncoils=1):
    """`iters` CG iterations from zero on (A^H W A + lamda I) x = A^H W y / max|A^H W y| -- the normalisation of pics -- with the
    recursion in float64 and A, A^H applied through the operator tree `A` (complex64).  w: one weight per sample, shared by the
    `ncoils` coils stacked in y; None: W = I."""
    c64 = np.complex64
    y = np.asarray(y, dtype=np.complex128).reshape((-1, 1), order='F')
    W = np.ones(y.shape[0]) if w is None else np.tile(np.asarray(w, dtype=np.float64).reshape(-1, order='F'), ncoils)
    W = W.reshape(-1, 1)

    def fwd(v):
        return (A * np.asfortranarray(v.astype(c64))).astype(np.complex128)

    def adj(v):
        return (A.H * np.asfortranarray(v.astype(c64))).astype(np.complex128)

    def normal(v):
        return adj(W * fwd(v)) + lamda * v
    b = adj(W * y)
    b = b / np.abs(b).max()
    x = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rr = np.vdot(r, r).real
    for _ in range(iters):
        q = normal(p)
        a = rr / np.vdot(p, q).real
        x = x + a * p
        r = r - a * q
        rn = np.vdot(r, r).real
        p = r + (rn / rr) * p
        rr = rn
    return x
