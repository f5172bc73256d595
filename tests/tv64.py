"""Float64 restatement of the total-variation pieces of pics --tv, written from their definition with numpy
slicing and not from the product's code: the forward-difference gradient, its adjoint, the per-voxel projection onto the
2-norm ball, the dual step and the Condat-Vu iteration.  Test infrastructure, no GPU.

A volume is F-ordered `dims` (axis 0 fastest); x has shape (N,) or (N, ncols), u shape (3N,) or (3N, ncols) with component a
in rows [aN, (a+1)N)."""
import numpy as np


def _vol(x, dims):
    """x as a complex128 array of shape dims + (ncols,)"""
    x = np.asarray(x)
    return x.reshape((int(np.prod(dims)), -1), order='F').astype(np.complex128).reshape(tuple(dims) + (-1,), order='F')


def _comp(u, dims):
    """u as a complex128 array of shape dims + (3, ncols)"""
    u = np.asarray(u)
    return u.reshape((3 * int(np.prod(dims)), -1), order='F').astype(np.complex128).reshape(tuple(dims) + (3, -1), order='F')


def grad(x, dims):
    """D x: (D_a x)[i] = x[i + e_a] - x[i] where i_a < n_a - 1, else 0"""
    v = _vol(x, dims)
    out = np.zeros(tuple(dims) + (3, v.shape[3]), dtype=np.complex128)
    out[:-1, :, :, 0] = np.diff(v, axis=0)
    out[:, :-1, :, 1] = np.diff(v, axis=1)
    out[:, :, :-1, 2] = np.diff(v, axis=2)
    shape = (3 * v[..., 0].size,) + np.shape(x)[1:]
    return out.reshape(shape, order='F')


def gradh(u, dims):
    """D^H u: (D^H u)[i] = sum_a ((i_a > 0 ? u_a[i - e_a] : 0) - (i_a < n_a - 1 ? u_a[i] : 0))"""
    t = _comp(u, dims)
    out = np.zeros(tuple(dims) + (t.shape[4],), dtype=np.complex128)
    for a in range(3):
        inner = [slice(None)] * 3
        inner[a] = slice(0, dims[a] - 1)                   # the voxels with a forward neighbour along a
        shifted = list(inner)
        shifted[a] = slice(1, dims[a])
        c = t[tuple(inner) + (a,)]
        out[tuple(shifted)] += c
        out[tuple(inner)] -= c
    shape = (out[..., 0].size,) + np.shape(u)[1:]
    return out.reshape(shape, order='F')


def radius(u, dims):
    """r[i] = sqrt(sum_a |u_a[i]|^2), shape dims + (ncols,)"""
    return np.sqrt((np.abs(_comp(u, dims)) ** 2).sum(axis=3))


def proj(u, mu, dims):
    """per voxel: u_a[i] *= (r <= mu ? 1 : mu / r)"""
    t = _comp(u, dims)
    r = radius(u, dims)[:, :, :, None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(r <= mu, 1.0, mu / r)
    return (t * f).reshape(np.shape(u), order='F')


def dual_step(u, xn, xo, sigma, mu, dims):
    """proj_mu(u + sigma D(2 xn - xo))"""
    w = 2.0 * np.asarray(xn, dtype=np.complex128) - np.asarray(xo, dtype=np.complex128)
    return proj(np.asarray(u, dtype=np.complex128) + sigma * grad(w, dims), mu, dims)


def tv(x, dims):
    """sum_i ||(D x)_i||_2"""
    return float(radius(grad(x, dims), dims).sum())


def condat_vu(gradf, prox, tau, sigma, mu, dims, x0, iters):
    """x_{k+1} = prox(x_k - tau (gradf(x_k) + D^H u_k), tau), u_{k+1} = proj_mu(u_k + sigma D(2 x_{k+1} - x_k)) from u_0 = 0, in
    complex128; prox None is the identity.  Returns the iterates [x_1, ..., x_iters] and the last u."""
    x = np.asarray(x0, dtype=np.complex128)
    u = np.zeros((3 * x.shape[0],) + x.shape[1:], dtype=np.complex128)
    seen = []
    for _ in range(iters):
        v = x - tau * (gradf(x) + gradh(u, dims))
        xn = v if prox is None else prox(v, tau)
        u = dual_step(u, xn, x, sigma, mu, dims)
        x = xn
        seen.append(x)
    return seen, u


def norm2_estimate(dims, iters=200, seed=0):
    """power-iteration estimate of ||D||^2 (a lower bound that converges to it)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    lam = 0.0
    for _ in range(iters):
        v /= np.linalg.norm(v)
        w = gradh(grad(v, dims), dims)
        lam = np.linalg.norm(w)
        v = w
    return lam
