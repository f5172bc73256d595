"""Float64 restatement of the second-order total generalized variation of pics --tgv, written from its definition
with numpy slicing and not from the product's code: the symmetrised backward difference E, its adjoint, K (x; v) = (D x - v; E v)
and K^H, the per-voxel projections, the dual step, the Condat-Vu iteration on (x; v) and power-iteration norm estimates.  Test
infrastructure, no GPU.

A volume is F-ordered `dims` (axis 0 fastest); x has shape (N,) or (N, ncols), v and p shape (3N[, ncols]) with component a in rows
[aN, (a+1)N), q shape (6N[, ncols]) with the components xx, yy, zz, xy, xz, yz in rows [cN, (c+1)N).  The gradient D is tv64's."""
import numpy as np

import tv64

PAIRS = [(0, 1), (0, 2), (1, 2)]                           # xy, xz, yz: components 3, 4, 5
R = 1.0 / np.sqrt(2.0)


def _field(u, dims, comps):
    """u as a complex128 array of shape (comps,) + dims + (ncols,): component first"""
    n = int(np.prod(dims))
    u = np.asarray(u).reshape((comps * n, -1), order='F').astype(np.complex128)
    return np.stack([u[c * n:(c + 1) * n].reshape(tuple(dims) + (-1,), order='F') for c in range(comps)])


def _rows(f, like):
    """the inverse of _field: components stacked in rows, with the trailing shape of `like`"""
    cols = f.shape[-1]
    out = np.concatenate([c.reshape((-1, cols), order='F') for c in f], axis=0)
    return out.reshape((out.shape[0],) + np.shape(like)[1:], order='F')


def _face(w, a):
    shape = list(w.shape)
    shape[a] = 1
    return np.zeros(shape, dtype=w.dtype)


def fwd(w, a):
    """D_a w: w[i + e_a] - w[i] where i_a < n_a - 1, else 0 (w: dims + (ncols,))"""
    return np.concatenate([np.diff(w, axis=a), _face(w, a)], axis=a)


def bwd(w, a):
    """B_a w = -D_a^H w: (i_a < n_a - 1 ? w[i] : 0) - (i_a > 0 ? w[i - e_a] : 0)"""
    inner = np.take(w, np.arange(w.shape[a] - 1), axis=a)               # w where i_a < n_a - 1
    return np.concatenate([inner, _face(w, a)], axis=a) - np.concatenate([_face(w, a), inner], axis=a)


def symgrad(v, dims):
    """E v: (E v)_aa = B_a v_a, (E v)_ab = (B_b v_a + B_a v_b) / sqrt(2)"""
    f = _field(v, dims, 3)
    out = [bwd(f[a], a) for a in range(3)] + [(bwd(f[a], b) + bwd(f[b], a)) * R for a, b in PAIRS]
    return _rows(np.stack(out), v)


def symgradh(q, dims):
    """E^H q: (E^H q)_a = -D_a q_aa - sum_{b != a} D_b q_ab / sqrt(2)"""
    f = _field(q, dims, 6)
    out = [-fwd(f[a], a) for a in range(3)]
    for c, (a, b) in enumerate(PAIRS):
        out[a] = out[a] - fwd(f[3 + c], b) * R
        out[b] = out[b] - fwd(f[3 + c], a) * R
    return _rows(np.stack(out), q)


def k(x, v, dims):
    """K (x; v) = (D x - v; E v) -> (3N rows, 6N rows)"""
    return tv64.grad(x, dims) - np.asarray(v, dtype=np.complex128), symgrad(v, dims)


def kh(p, q, dims):
    """K^H (p; q) = (D^H p; E^H q - p) -> (N rows, 3N rows)"""
    return tv64.gradh(p, dims), symgradh(q, dims) - np.asarray(p, dtype=np.complex128)


def radius(u, dims, comps):
    """r[i] = sqrt(sum_c |u_c[i]|^2) over the `comps` components, shape dims + (ncols,)"""
    return np.sqrt((np.abs(_field(u, dims, comps)) ** 2).sum(axis=0))


def proj(u, rad, dims, comps):
    """per voxel: u_c[i] *= (r <= rad ? 1 : rad / r)"""
    r = radius(u, dims, comps)
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(r <= rad, 1.0, rad / r)
    return _rows(_field(u, dims, comps) * f[None], u)


def unprojected(p, q, xn, xo, vn, vo, sigma, dims):
    """(p + sigma (D w_x - w_v), q + sigma E w_v) with w = 2 (xn; vn) - (xo; vo)"""
    wx = 2.0 * np.asarray(xn, dtype=np.complex128) - np.asarray(xo, dtype=np.complex128)
    wv = 2.0 * np.asarray(vn, dtype=np.complex128) - np.asarray(vo, dtype=np.complex128)
    dp, dq = k(wx, wv, dims)
    return np.asarray(p, dtype=np.complex128) + sigma * dp, np.asarray(q, dtype=np.complex128) + sigma * dq


def dual_step(p, q, xn, xo, vn, vo, sigma, a1, a0, dims):
    """(proj_{a1}(p + sigma (D w_x - w_v)), proj_{a0}(q + sigma E w_v))"""
    tp, tq = unprojected(p, q, xn, xo, vn, vo, sigma, dims)
    return proj(tp, a1, dims, 3), proj(tq, a0, dims, 6)


def tgv(x, v, a1, a0, dims):
    """a1 sum_i ||(D x - v)_i||_2 + a0 sum_i ||(E v)_i||_F"""
    dp, dq = k(x, v, dims)
    return float(a1 * radius(dp, dims, 3).sum() + a0 * radius(dq, dims, 6).sum())


def condat_vu(gradf, prox, tau, sigma, a1, a0, dims, x0, iters):
    """x_{k+1} = prox(x_k - tau (gradf(x_k) + D^H p_k), tau), v_{k+1} = v_k - tau (E^H q_k - p_k), (p, q)_{k+1} = the dual step at
    2 z_{k+1} - z_k, from v_0 = 0, p_0 = q_0 = 0, in complex128; prox None is the identity (it acts on x only).  Returns the iterates
    [(x_1, v_1), ..., (x_iters, v_iters)] and the last (p, q)."""
    x = np.asarray(x0, dtype=np.complex128)
    rest = x.shape[1:]
    v = np.zeros((3 * x.shape[0],) + rest, dtype=np.complex128)
    p, q = np.zeros_like(v), np.zeros((6 * x.shape[0],) + rest, dtype=np.complex128)
    seen = []
    for _ in range(iters):
        gx, gv = kh(p, q, dims)
        t = x - tau * (gradf(x) + gx)
        xn = t if prox is None else prox(t, tau)
        vn = v - tau * gv
        p, q = dual_step(p, q, xn, x, vn, v, sigma, a1, a0, dims)
        x, v = xn, vn
        seen.append((x, v))
    return seen, (p, q)


def norm2_estimate(dims, which='K', iters=300, seed=0):
    """power-iteration estimate of ||K||^2 (which = 'K') or ||E||^2 ('E'): a lower bound that converges to it"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    z = rng.standard_normal(4 * n) + 1j * rng.standard_normal(4 * n)
    lam = 0.0
    for _ in range(iters):
        z /= np.linalg.norm(z)
        if which == 'E':
            w = np.concatenate([np.zeros(n), symgradh(symgrad(z[n:], dims), dims)])
        else:
            w = np.concatenate(kh(*k(z[:n], z[n:], dims), dims))
        lam = np.linalg.norm(w)
        z = w
    return lam
