"""Float64 restatement of the spatio-temporal total-variation pieces of pics --tv / --tv-time on several time frames (DESIGN.md
§3.8), written from their definition with numpy slicing and not from the product's code: the gradient with a fourth, temporal
difference, its adjoint, the two projections, the dual step and the Condat-Vu iteration.  Test infrastructure, no GPU.

A frame is an F-ordered `dims` volume of N voxels (axis 0 fastest).  x holds T frames: the panel (N, T), or the same stacked as
(N T,) or (N T, 1), frame t in rows [tN, (t+1)N).  u holds four components per frame: (4N, T), or stacked (4N T,) / (4N T, 1),
component a of frame t in rows [aN, (a+1)N) of that frame's 4N; components 0..2 are the spatial differences, 3 the temporal."""
import numpy as np


def _vol(x, dims, T):
    """x as a complex128 array of shape dims + (T,)"""
    return np.asarray(x).astype(np.complex128).reshape(tuple(dims) + (T,), order='F')


def _comp(u, dims, T):
    """u as a complex128 array of shape dims + (4, T)"""
    return np.asarray(u).astype(np.complex128).reshape(tuple(dims) + (4, T), order='F')


def _like(out, src, rows, T):
    """`out` (any shape of rows * T elements, F-ordered) shaped the way `src` is: a panel of T columns, or stacked"""
    src = np.asarray(src)
    if src.ndim == 2 and src.shape[1] == T and T > 1:
        return out.reshape((rows, T), order='F')
    return out.reshape((rows * T,) + src.shape[1:], order='F')


def grad(x, dims, T):
    """D4 x: (D_a x_t)[i] = x_t[i + e_a] - x_t[i] where i_a < n_a - 1, else 0 (a = 0, 1, 2);  component 3 is x_{t+1}[i] - x_t[i]
    where t < T - 1, else 0"""
    v = _vol(x, dims, T)
    out = np.zeros(tuple(dims) + (4, T), dtype=np.complex128)
    out[:-1, :, :, 0] = np.diff(v, axis=0)
    out[:, :-1, :, 1] = np.diff(v, axis=1)
    out[:, :, :-1, 2] = np.diff(v, axis=2)
    out[:, :, :, 3, :-1] = np.diff(v, axis=3)
    return _like(out, x, 4 * int(np.prod(dims)), T)


def gradh(u, dims, T):
    """D4^H u: (D4^H u)_t[i] = sum_{a<3} ((i_a > 0 ? u_{a,t}[i - e_a] : 0) - (i_a < n_a - 1 ? u_{a,t}[i] : 0))
    + (t > 0 ? u_{3,t-1}[i] : 0) - (t < T - 1 ? u_{3,t}[i] : 0)"""
    c = _comp(u, dims, T)
    shape4 = tuple(dims) + (T,)
    out = np.zeros(shape4, dtype=np.complex128)
    for a in range(4):
        inner = [slice(None)] * 4
        inner[a] = slice(0, shape4[a] - 1)                 # the entries with a forward neighbour along a
        shifted = list(inner)
        shifted[a] = slice(1, shape4[a])
        part = c[:, :, :, a, :][tuple(inner)]
        out[tuple(shifted)] += part
        out[tuple(inner)] -= part
    return _like(out, u, int(np.prod(dims)), T)


def radius(u, dims, T):
    """the spatial radius r[i, t] = sqrt(sum_{a<3} |u_{a,t}[i]|^2), shape dims + (T,)"""
    return np.sqrt((np.abs(_comp(u, dims, T)[:, :, :, :3]) ** 2).sum(axis=3))


def modulus_t(u, dims, T):
    """the temporal modulus |u_{3,t}[i]|, shape dims + (T,)"""
    return np.abs(_comp(u, dims, T)[:, :, :, 3])


def proj(u, mu, mu_t, dims, T):
    """per voxel and frame: u_a *= (r <= mu ? 1 : mu / r) for a < 3, r the spatial radius;  u_3 *= (|u_3| <= mu_t ? 1 : mu_t / |u_3|)"""
    c = _comp(u, dims, T)
    r = radius(u, dims, T)[:, :, :, None, :]
    m = modulus_t(u, dims, T)
    with np.errstate(divide='ignore', invalid='ignore'):
        c[:, :, :, :3] *= np.where(r <= mu, 1.0, mu / r)
        c[:, :, :, 3] *= np.where(m <= mu_t, 1.0, mu_t / m)
    return c.reshape(np.shape(u), order='F')


def dual_step(u, xn, xo, sigma, mu, mu_t, dims, T):
    """proj(u + sigma D4(2 xn - xo))"""
    w = 2.0 * np.asarray(xn, dtype=np.complex128) - np.asarray(xo, dtype=np.complex128)
    step = grad(w, dims, T).reshape(np.shape(u), order='F')
    return proj(np.asarray(u, dtype=np.complex128) + sigma * step, mu, mu_t, dims, T)


def tv(x, dims, T):
    """sum_t sum_i ||(D x_t)_i||_2"""
    return float(radius(grad(x, dims, T), dims, T).sum())


def tv_time(x, dims, T):
    """sum_{t<T-1} sum_i |x_{t+1}[i] - x_t[i]|"""
    return float(modulus_t(grad(x, dims, T), dims, T).sum())


def condat_vu(gradf, prox, tau, sigma, mu, mu_t, dims, T, x0, iters):
    """x_{k+1} = prox(x_k - tau (gradf(x_k) + D4^H u_k), tau), u_{k+1} = proj(u_k + sigma D4(2 x_{k+1} - x_k)) from u_0 = 0, in
    complex128 on stacked vectors; prox None is the identity.  Returns the iterates [x_1, ..., x_iters] and the last u."""
    x = np.asarray(x0, dtype=np.complex128)
    u = np.zeros((4 * x.shape[0],) + x.shape[1:], dtype=np.complex128)
    seen = []
    for _ in range(iters):
        v = x - tau * (gradf(x) + gradh(u, dims, T))
        xn = v if prox is None else prox(v, tau)
        u = dual_step(u, xn, x, sigma, mu, mu_t, dims, T)
        x = xn
        seen.append(x)
    return seen, u


def norm2_estimate(dims, T, iters=300, seed=0):
    """power-iteration estimate of ||D4||^2 (a lower bound that converges to it)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims)) * T
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    lam = 0.0
    for _ in range(iters):
        v /= np.linalg.norm(v)
        w = gradh(grad(v, dims, T), dims, T)
        lam = np.linalg.norm(w)
        v = w
    return lam
