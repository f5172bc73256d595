"""A float64 restatement of NLINV (indigo_amd.nlinv, Backend.nlinv_product, Backend.sobolev_weight, operators.NlinvProduct,
operators.SobolevCoils), for the tests: the two kernels, W, F, DF, DF^H and the whole IRGNM with a plain float64 CG,
and the synthetic radial scan the pipeline tests run on.

The NUFFT here is the scipy matrices of `B.NUFFT`'s factors (roll-off, zero-pad, modulation, gridding: complex64 values as the
factories make them, applied in complex128) around numpy's float64 transforms: `apply64` walks the operator tree.  No backend kernel
and no complex64 intermediate is involved."""
import os

import numpy as np

import maps64

C64 = np.dtype('complex64')


# ---- the two kernels ------------------------------------------------------------------------------------------------------------

def product(rho, coils, x, y=None, adjoint=False, alpha=1, beta=0):
    """beta*y + alpha * (the linearised coil product or its adjoint), complex128.  rho (n,), coils (n, C); forward x (n, 1 + C) ->
    (n, C), adjoint x (n, C) -> (n, 1 + C); y is not read when beta == 0"""
    rho, coils, x = (np.asarray(v, dtype=np.complex128) for v in (rho, coils, x))
    if adjoint:
        out = np.concatenate([(np.conj(coils) * x).sum(axis=1, keepdims=True), np.conj(rho)[:, None] * x], axis=1)
    else:
        out = x[:, :1] * coils + rho[:, None] * x[:, 1:]
    out = complex(alpha) * out
    if beta != 0:
        out = out + complex(beta) * np.asarray(y, dtype=np.complex128)
    return out


def product_magnitudes(rho, coils, x, y=None, adjoint=False, alpha=1, beta=0):
    """the sum of the magnitudes of the products that form each element of `product`, |beta y| included"""
    rho, coils, x = (np.abs(np.asarray(v, dtype=np.complex128)) for v in (rho, coils, x))
    if adjoint:
        out = np.concatenate([(coils * x).sum(axis=1, keepdims=True), rho[:, None] * x], axis=1)
    else:
        out = x[:, :1] * coils + rho[:, None] * x[:, 1:]
    out = abs(complex(alpha)) * out
    if beta != 0:
        out = out + abs(complex(beta)) * np.abs(np.asarray(y, dtype=np.complex128))
    return out


def weights(dims, a, b):
    """w(k) = (1 + a |kappa|^2)^(-b/2), kappa_a = k'_a / n_a, k'_a = k_a if 2 k_a <= n_a else k_a - n_a: float64, dims-shaped"""
    r2 = np.zeros(dims, dtype=np.float64)
    for ax, n in enumerate(dims):
        k = np.arange(n)
        kp = np.where(2 * k <= n, k, k - n) / float(n)
        r2 = r2 + (kp ** 2).reshape([-1 if j == ax else 1 for j in range(3)])
    return (1.0 + float(a) * r2) ** (-float(b) / 2.0)


def weight(x, dims, a, b, scale=1.0):
    """scale * w(k) * x[k, j] for an (N, ncols) panel of F-ordered volumes, complex128"""
    return float(scale) * weights(dims, a, b).reshape(-1, order='F')[:, None] * np.asarray(x, dtype=np.complex128)


def W(chat, dims, a, b):
    """(N, C) c^ -> c = (1 / sqrt N) ifftn(w * c^) with the unnormalised inverse transform (numpy's times N)"""
    N, C = int(np.prod(dims)), chat.shape[1]
    v = weight(chat, dims, a, b).reshape(tuple(dims) + (C,), order='F')
    return (np.fft.ifftn(v, axes=(0, 1, 2)) * np.sqrt(N)).reshape((N, C), order='F')


def WH(z, dims, a, b):
    """(N, C) z -> w * fftn(z) / sqrt N"""
    N, C = int(np.prod(dims)), z.shape[1]
    v = np.fft.fftn(np.asarray(z, dtype=np.complex128).reshape(tuple(dims) + (C,), order='F'), axes=(0, 1, 2)).reshape((N, C), order='F')
    return weight(v, dims, a, b, scale=1.0 / np.sqrt(N))


def sobolev_coils(u, dims, C, a, b, adjoint=False):
    """operators.SobolevCoils on one column u of N (1 + C) values: rho passes, the coil part goes through W (or W^H)"""
    N = int(np.prod(dims))
    p = np.asarray(u, dtype=np.complex128).reshape((N, 1 + C), order='F')
    coil = (WH if adjoint else W)(p[:, 1:], dims, a, b)
    return np.concatenate([p[:, :1], coil], axis=1).reshape(-1, order='F')


# ---- the NUFFT in float64 -------------------------------------------------------------------------------------------------------

_MATRICES = {}          # id(leaf) -> (leaf, its matrix in complex128): converted once


def apply64(node, x, forward=True):
    """node (a tree of SpMatrix, UnscaledFFT, Product, Scale, Adjoint and KronI nodes, as B.NUFFT and B.KronI build it) applied to
    the complex128 (rows, ncols) array x: the leaves' scipy matrices and numpy's float64 transforms"""
    from indigo_amd import operators as op
    x = np.asarray(x, dtype=np.complex128)
    if isinstance(node, op.SpMatrix):
        if id(node) not in _MATRICES:
            _MATRICES[id(node)] = (node, node._matrix.astype(np.complex128).tocsr())
        M = _MATRICES[id(node)][1]
        return (M @ x) if forward else (M.conj().T @ x)
    if isinstance(node, op.UnscaledFFT):
        shape = node._ft_shape
        v = x.reshape(shape + (x.shape[1],), order='F')
        ax = tuple(range(len(shape)))
        out = np.fft.fftn(v, axes=ax) if forward else np.fft.ifftn(v, axes=ax) * int(np.prod(shape))
        return out.reshape(x.shape, order='F')
    if isinstance(node, op.Product):
        L, R = node._children
        return apply64(L, apply64(R, x, True), True) if forward else apply64(R, apply64(L, x, False), False)
    if isinstance(node, op.Scale):
        return (node._val if forward else np.conj(node._val)) * apply64(node.child, x, forward)
    if isinstance(node, op.Adjoint):
        return apply64(node.child, x, not forward)
    if isinstance(node, op.Kron) and isinstance(node.left, op.Eye):
        c = node.left.shape[0]
        cols = node.right.shape[1] if forward else node.right.shape[0]
        out = apply64(node.right, x.reshape((cols, c * x.shape[1]), order='F'), forward)
        return out.reshape((-1, x.shape[1]), order='F')
    raise TypeError("apply64: no float64 form of %s" % type(node).__name__)


class Model(object):
    """F, DF and DF^H of the module docstring of indigo_amd.nlinv on one radial trajectory, in float64"""

    def __init__(self, B, dims, C, coord, a, b, osf, width, power_iters=10):
        from indigo_amd.util import rand64c
        self.dims, self.C, self.a, self.b = tuple(dims), int(C), float(a), float(b)
        self.N = int(np.prod(dims))
        self.F1 = B.NUFFT((1,) + tuple(coord.shape[1:]), self.dims, coord, width=width, oversamp=(osf, osf, osf), dtype=C64)
        # pics.power_iteration: a seeded random start, `power_iters` products, the estimate ||F^H F v|| for the last unit vector
        v = rand64c(self.N, 1, seed=0).astype(np.complex128)
        v /= np.linalg.norm(v)
        lam = 0.0
        for _ in range(power_iters):
            w = apply64(self.F1, apply64(self.F1, v, True), False)
            lam = float(np.linalg.norm(w))
            v = w / lam
        self.L = lam

    def A(self, z, forward=True):
        """L^(-1/2) KronI(C, NUFFT) on (N, C) coil images (forward) or (samples, C) k-space (adjoint)"""
        return apply64(self.F1, z, forward) / np.sqrt(self.L)

    def point(self, u):
        p = sobolev_coils(u, self.dims, self.C, self.a, self.b).reshape((self.N, 1 + self.C), order='F')
        return p[:, 0], p[:, 1:]

    def F(self, u):
        rho, c = self.point(u)
        return self.A(rho[:, None] * c)

    def DF(self, u, v):
        rho, c = self.point(u)
        dv = sobolev_coils(v, self.dims, self.C, self.a, self.b).reshape((self.N, 1 + self.C), order='F')
        return self.A(product(rho, c, dv))

    def DFH(self, u, r):
        rho, c = self.point(u)
        z = product(rho, c, self.A(r, forward=False), adjoint=True)
        return sobolev_coils(z.reshape(-1, order='F'), self.dims, self.C, self.a, self.b, adjoint=True)


def cg(apply, b, lamda, maxiter, tol=1e-10):
    """Backend.cg's sequence from x = 0 in float64 -> (x, iterations)"""
    x = np.zeros_like(b)
    r = b.copy()
    d = r.copy()
    rho = rho0 = np.vdot(r, r).real
    its = 0
    for _ in range(maxiter):
        q = apply(d) + lamda * d
        step = rho / np.vdot(d, q).real
        x += step * d
        r -= step * q
        rho, rho_old = np.vdot(r, r).real, rho
        d = r + (rho / rho_old) * d
        its += 1
        if np.sqrt(rho / rho0) < tol:
            break
    return x, its


def irgnm(model, y_file, iters=8, cg_iters=10, alpha=1.0, redu=2.0):
    """-> (image dims, maps dims + (C,), history, rho c / (s sqrt L) as (N, C)): the IRGNM and the results of indigo_amd.nlinv"""
    N, C = model.N, model.C
    y_file = np.asarray(y_file, dtype=np.complex128).reshape((-1, C), order='F')
    s = 100.0 / np.linalg.norm(y_file)
    y = s * y_file
    u0 = np.zeros(N * (1 + C), dtype=np.complex128)
    u0[:N] = 1
    u = u0.copy()
    history = []
    for n in range(iters):
        alpha_n = alpha * redu ** (-n)
        r = y - model.F(u)
        rhs = model.DFH(u, r) + alpha_n * (u0 - u)
        at = u.copy()
        du, its = cg(lambda v: model.DFH(at, model.DF(at, v)), rhs, alpha_n, cg_iters)
        u = u + du
        history.append({'alpha': alpha_n, 'cg_iters': its, 'residual': float(np.linalg.norm(y - model.F(u)) / 100.0)})
    rho, c = model.point(u)
    rss = np.sqrt((np.abs(c) ** 2).sum(axis=1))
    image = rho * rss / (s * np.sqrt(model.L))
    with np.errstate(divide='ignore', invalid='ignore'):
        maps = np.where(rss[:, None] > 0, c / rss[:, None], 0)
    return (image.reshape(model.dims, order='F'), maps.reshape(model.dims + (C,), order='F'), history,
            rho[:, None] * c / (s * np.sqrt(model.L)))


# ---- the phantom and the figures of merit -----------------------------------------------------------------------------------------

# the pipeline scan: image, coils, readout, spokes, oversampling, kernel half-width, and the options of both pipeline tests.  The
# default a = 220 is useless at this size (the second k-space point already has w = 0.04, the maps stay constant): a = 10
DIMS, COILS, NRO, NSP, OSF, WIDTH = (24, 20, 16), 4, 48, 300, 2.0, 2
SOBOLEV = (10.0, 32.0)
ITERS, CG_ITERS = 10, 10
ARGS = ["--sobolev-a", "10", "--sobolev-b", "32", "-i", str(ITERS), "--cg-iters", str(CG_ITERS), "--osf", str(OSF), "--width", str(WIDTH),
        "--dims", ":".join(str(n) for n in DIMS)]

_CACHE = {}


def phantom(B):
    """maps64.smooth_maps x maps64.objects on sense.radial_trajectory(NSP, NRO, seed=2), the k-space from the float64 NUFFT, rounded
    to complex64 as a file holds it -> dict(ksp (1, NRO, NSP, C), traj in pixels, coord, S, img, support), once per process"""
    if 'phantom' not in _CACHE:
        from indigo_amd.sense import radial_trajectory
        S = maps64.smooth_maps(DIMS, COILS, 1)[..., 0].astype(np.complex128)
        img = maps64.objects(DIMS, 1)[0].astype(np.complex128)
        coord = radial_trajectory(NSP, NRO, seed=2)
        F1 = B.NUFFT((1, NRO, NSP), DIMS, coord, width=WIDTH, oversamp=(OSF, OSF, OSF), dtype=C64)
        N = int(np.prod(DIMS))
        ksp = apply64(F1, (S * img[..., None]).reshape((N, COILS), order='F'))
        _CACHE['phantom'] = dict(ksp=ksp.astype(C64).reshape((1, NRO, NSP, COILS), order='F'), coord=coord,
                                 traj=coord * np.array(DIMS, dtype=np.float64)[:, None, None], S=S, img=img,
                                 support=np.abs(img) > 0.05 * np.abs(img).max())
    return _CACHE['phantom']


def write_scan(tmpdir, B, name="nlinv.npz"):
    ph = phantom(B)
    path = os.path.join(str(tmpdir), name)
    np.savez(path, data=ph['ksp'].T, traj=ph['traj'].T)
    return path


def reference(B):
    """the float64 IRGNM on the phantom with the options of ARGS, once per process -> dict(image, maps, history, product, errors)"""
    if 'reference' not in _CACHE:
        ph = phantom(B)
        model = Model(B, DIMS, COILS, ph['coord'], SOBOLEV[0], SOBOLEV[1], OSF, WIDTH)
        image, maps, history, prod = irgnm(model, ph['ksp'], iters=ITERS, cg_iters=CG_ITERS)
        _CACHE['reference'] = dict(image=image, maps=maps, history=history, product=prod, L=model.L,
                                   image_error=image_error(image, ph), maps_error=maps_error(maps, ph))
    return _CACHE['reference']


def normalised(S):
    """dims + (C,) sensitivities -> S_c / sqrt(sum |S|^2) with the phase of coil 0 removed (espirit64.normalised)"""
    import espirit64
    return espirit64.normalised(S)


def image_error(image, ph):
    """the image, fitted to img * rss(S) by one complex scale, against it: relative 2-norm over the support"""
    sup = ph['support']
    truth = (ph['img'] * np.sqrt((np.abs(ph['S']) ** 2).sum(axis=-1)))[sup]
    got = np.asarray(image, dtype=np.complex128)[sup]
    lam = np.vdot(got, truth) / np.vdot(got, got)
    return float(np.linalg.norm(lam * got - truth) / np.linalg.norm(truth))


def maps_error(maps, ph):
    """the maps in espirit64.normalised form against the true ones in that form: relative 2-norm over the support"""
    sup = ph['support']
    got, truth = normalised(np.asarray(maps, dtype=np.complex128)[sup]), normalised(ph['S'][sup])
    return float(np.linalg.norm(got - truth) / np.linalg.norm(truth))


# ---- the operators of a backend, for the adjointness and bilinearity tests on either backend ---------------------------------------

def backend_model(B, dims, C, a, b, nro=16, nsp=20, osf=2.0, width=2):
    """-> (A = KronI(C, NUFFT), P = NlinvProduct, S = SobolevCoils, DF = A * P * S) of backend B on a small radial trajectory"""
    from indigo_amd.sense import radial_trajectory
    coord = radial_trajectory(nsp, nro, seed=2)
    A = B.KronI(C, B.NUFFT((1, nro, nsp), dims, coord, width=width, oversamp=(osf, osf, osf), dtype=C64))
    P, S = B.NlinvProduct(int(np.prod(dims)), C), B.SobolevCoils(dims, C, a, b)
    return A, P, S, A * P * S


def set_point(B, P, S, u_h):
    """the point of the host column u_h on P -> the device array (rho, c), which the caller keeps alive"""
    N, C = P._n, P._C
    cu = B.zero_array((N * (1 + C), 1), C64)
    S.eval(cu, B.copy_array(np.asfortranarray(u_h.reshape((-1, 1)))))
    P.set_point(cu.dense_rows(0, N), cu.dense_rows(N, N * (1 + C)))
    return cu


def evaluate(B, op, x_h, forward=True):
    rows = op.shape[0] if forward else op.shape[1]
    y = B.zero_array((rows, 1), C64)
    op.eval(y, B.copy_array(np.asfortranarray(x_h.reshape((-1, 1)).astype(C64))), forward=forward)
    return y.to_host().reshape(-1)


def adjoint_defect(B, op, seed):
    """|<op v, r> - <v, op^H r>| / (||op v|| ||r||) for seeded random v and r"""
    from indigo_amd.util import rand64c
    v, r = rand64c(op.shape[1], 1, seed=seed).reshape(-1), rand64c(op.shape[0], 1, seed=seed + 1).reshape(-1)
    fv, ar = evaluate(B, op, v).astype(np.complex128), evaluate(B, op, r, forward=False).astype(np.complex128)
    lhs, rhs = np.vdot(r.astype(np.complex128), fv), np.vdot(ar, v.astype(np.complex128))
    return abs(lhs - rhs) / (np.linalg.norm(fv) * np.linalg.norm(r))


def check_results(image, maps, state):
    """image * maps = rho c / (s sqrt L) to 1e-5 for the iterate `state` of indigo_amd.nlinv.nlinv, and rss(maps) = 1 where non-zero"""
    rho, c = state['rho'].astype(np.complex128), state['coils'].astype(np.complex128)
    want = rho[:, None] * c / (state['s'] * np.sqrt(state['L']))
    prod = (image[..., None].astype(np.complex128) * maps).reshape(want.shape, order='F')
    d = np.linalg.norm(prod - want) / np.linalg.norm(want)
    rss = np.sqrt((np.abs(maps.astype(np.complex128)) ** 2).sum(axis=-1))
    print("image * maps against rho c / (s sqrt L): %.3e; rss(maps) off 1 by at most %.3e" % (d, np.abs(rss[rss > 0] - 1).max()))
    assert d <= 1e-5
    assert (rss > 0).any() and (np.abs(rss[rss > 0] - 1) <= 1e-6).all()
