"""A float64 restatement of ESPIRiT calibration (indigo_amd.ecalib, Backend.place_wrapped, Backend.espirit_eig), for
the tests, and the synthetic scans they calibrate on.

The definition.  s[p, c] is a fully sampled Cartesian block of k-space, (cx, cy, cz, C), centred the way Backend.FFTc centres k-space
(origin at index c_a // 2).  The kernel has side k per axis, clamped to the block; K3 = k0 k1 k2.  For every window origin q at which
the window fits, h_q is the column vector of s[q + kappa, c] over (kappa, c).  Gamma = sum_q h_q h_q^H, eigenpairs (sigma_j^2, w_j);
P = sum w_j w_j^H over sigma_j > t sigma_1.  R_cc'[delta] = sum_{kappa - kappa' = delta} P[(kappa, c), (kappa', c')];
G(x)_cc' = (1 / K3) sum_delta R_cc'[delta] exp(+2 pi i delta . xi / N), xi = the voxel's coordinate from index n_a // 2.  The maps are the
M leading eigenpairs of G(x), descending, unit 2-norm, coil 0 real and >= 0 (unrotated below 1e-6), zero where lambda_m < crop.

Everything here is plain loops and direct sums in complex128: no transform, no window view, nothing shared with the product."""
import os

import numpy as np

C64 = np.dtype('complex64')


# ---- the definition -----------------------------------------------------------------------------------------------------------

def projector(s, k, t=0.001):
    """-> (P as an array (k0, k1, k2, C, k0, k1, k2, C), (k0, k1, k2))"""
    s = np.asarray(s, dtype=np.complex128)
    cx, cy, cz, C = s.shape
    kd = (min(k, cx), min(k, cy), min(k, cz))
    L = kd[0] * kd[1] * kd[2] * C
    gamma = np.zeros((L, L), dtype=np.complex128)
    rows = []
    for q0 in range(cx - kd[0] + 1):
        for q1 in range(cy - kd[1] + 1):
            for q2 in range(cz - kd[2] + 1):
                rows.append(s[q0:q0 + kd[0], q1:q1 + kd[1], q2:q2 + kd[2], :].reshape(-1))
    H = np.array(rows)                                                       # row q: h_q^T
    gamma = H.T @ H.conj()                                                   # sum_q h_q h_q^H
    ev, w = np.linalg.eigh(gamma)
    sigma = np.sqrt(np.clip(ev, 0, None))
    P = np.zeros_like(gamma)
    for j in range(L):
        if sigma[j] > t * sigma.max():
            P += np.outer(w[:, j], w[:, j].conj())
    return P.reshape(kd + (C,) + kd + (C,)), kd


def correlations(P8, kd):
    """R[delta + k - 1, c, c']"""
    C = P8.shape[3]
    R = np.zeros(tuple(2 * k - 1 for k in kd) + (C, C), dtype=np.complex128)
    for a0 in range(kd[0]):
        for a1 in range(kd[1]):
            for a2 in range(kd[2]):
                for b0 in range(kd[0]):
                    for b1 in range(kd[1]):
                        for b2 in range(kd[2]):
                            R[a0 - b0 + kd[0] - 1, a1 - b1 + kd[1] - 1, a2 - b2 + kd[2] - 1] += P8[a0, a1, a2, :, b0, b1, b2, :]
    return R


def gmatrices(R, kd, dims):
    """G(x), dims + (C, C), by the direct sum over delta"""
    E = []
    for a in range(3):
        xi = np.arange(dims[a]) - dims[a] // 2
        delta = np.arange(2 * kd[a] - 1) - (kd[a] - 1)
        E.append(np.exp(2j * np.pi * np.outer(xi, delta) / dims[a]))
    return np.einsum('xa,yb,zc,abcpq->xyzpq', E[0], E[1], E[2], R, optimize=True) / (kd[0] * kd[1] * kd[2])


def eigenmaps(G, M, crop=0.8):
    """G: (..., C, C) Hermitian -> (maps (..., C, M) complex128, evals (..., M)), the conventions of the definition"""
    G = np.asarray(G, dtype=np.complex128)
    G = 0.5 * (G + np.conj(np.swapaxes(G, -1, -2)))
    lam, vec = np.linalg.eigh(G)
    lam, vec = lam[..., ::-1][..., :M], vec[..., ::-1][..., :M]
    vec = vec / np.linalg.norm(vec, axis=-2, keepdims=True)
    v0 = vec[..., 0:1, :]
    big = np.abs(v0) >= 1e-6
    vec = vec * np.where(big, np.conj(v0) / np.where(big, np.abs(v0), 1), 1)
    return np.where((lam < crop)[..., None, :], 0, vec), lam


def all_evals(G):
    G = np.asarray(G, dtype=np.complex128)
    return np.linalg.eigvalsh(0.5 * (G + np.conj(np.swapaxes(G, -1, -2))))[..., ::-1]


def espirit(s, dims, k, t=0.001, M=2, crop=0.8):
    """-> (maps dims + (C, M), evals dims + (M,), G dims + (C, C))"""
    P8, kd = projector(s, k, t)
    G = gmatrices(correlations(P8, kd), kd, dims)
    maps, lam = eigenmaps(G, M, crop)
    return maps, lam, G


# ---- the kernels' arguments -----------------------------------------------------------------------------------------------------

def pack_triangle(G):
    """(n, C, C) -> the (n, C (C + 1) / 2) panel of the row-wise upper triangle"""
    C = G.shape[-1]
    return np.stack([G[:, p, q] for p in range(C) for q in range(p, C)], axis=1)


def unpack_triangle(tri, C):
    """the (n, C, C) complex128 Hermitian matrices of a triangle panel; the imaginary part of the diagonal is ignored"""
    tri = np.asarray(tri, dtype=np.complex128)
    G = np.zeros((tri.shape[0], C, C), dtype=np.complex128)
    col = 0
    for p in range(C):
        for q in range(p, C):
            G[:, p, q] = tri[:, col]
            G[:, q, p] = np.conj(tri[:, col])
            col += 1
        G[:, p, p] = G[:, p, p].real
    return G


def prescribed(n, C, seed):
    """n Hermitian C x C matrices U diag(1, 0.5, 0.25, 0.125, <= 0.03 ...) U^H with a random unitary U per voxel, complex128"""
    rng = np.random.default_rng(seed)
    lam = np.array([1.0, 0.5, 0.25, 0.125] + list(0.03 * rng.random(max(C - 4, 0))))[:C]
    X = rng.standard_normal((n, C, C)) + 1j * rng.standard_normal((n, C, C))
    U, _ = np.linalg.qr(X)
    return (U * lam) @ np.conj(np.swapaxes(U, 1, 2))


def place_wrapped(box, dims):
    """box: (b0, b1, b2) -> the `dims` volume with box element j at (j - b // 2) mod n, zeros elsewhere"""
    out = np.zeros(dims, dtype=box.dtype)
    for j0 in range(box.shape[0]):
        for j1 in range(box.shape[1]):
            for j2 in range(box.shape[2]):
                out[(j0 - box.shape[0] // 2) % dims[0], (j1 - box.shape[1] // 2) % dims[1], (j2 - box.shape[2] // 2) % dims[2]] = box[j0, j1, j2]
    return out


# ---- synthetic scans ------------------------------------------------------------------------------------------------------------

def ellipsoid(dims, radii=(0.75, 0.75, 0.75), centre=(0.0, 0.0, 0.0)):
    """a smooth complex object inside an ellipsoid of the given radii (the volume spans [-1, 1] per axis) -> (image, support)"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in dims)]
    rho2 = sum(((g[a] - centre[a]) / radii[a]) ** 2 for a in range(3))
    support = rho2 < 1
    img = np.where(support, (1.0 + 0.5 * np.cos(3 * g[0]) * np.cos(2 * g[1]) + 0.3 * g[2]) * np.exp(1j * (0.8 * g[0] - 0.5 * g[1] * g[2])), 0)
    return img.astype(np.complex128), support


def centred_fft(x):
    """the unitary transform with both origins at index n // 2, over the first three axes: what Backend.FFTc computes"""
    ax = (0, 1, 2)
    return np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(x, axes=ax), axes=ax), axes=ax) / np.sqrt(np.prod(x.shape[:3]))


def cut_centre(ksp, c):
    """the block of side c (per axis, clamped) around the origin of a centred k-space, its own origin at index c // 2"""
    sl = tuple(slice(n // 2 - min(c, n) // 2, n // 2 - min(c, n) // 2 + min(c, n)) for n in ksp.shape[:3])
    return ksp[sl]


def normalised(S):
    """dims + (C,) sensitivities -> S_c / sqrt(sum |S|^2) with the phase of coil 0 removed"""
    S = np.asarray(S, dtype=np.complex128)
    out = S / np.sqrt((np.abs(S) ** 2).sum(axis=-1, keepdims=True))
    return out * np.exp(-1j * np.angle(out[..., 0:1]))


def rel_on(a, b, mask):
    return np.linalg.norm((a - b)[mask]) / np.linalg.norm(b[mask])


def span_residual(S, V, mask):
    """the relative 2-norm, over the voxels of `mask`, of what is left of the unit vectors S / |S| (dims + (C,)) after projection
    onto span(V[..., m]) (dims + (C, M), orthonormal columns)"""
    u = np.asarray(S, dtype=np.complex128)
    u = u / np.linalg.norm(u, axis=-1, keepdims=True)
    V = np.asarray(V, dtype=np.complex128)
    coef = np.einsum('...cm,...c->...m', np.conj(V), u)
    res = u - np.einsum('...cm,...m->...c', V, coef)
    return np.linalg.norm(res[mask]) / np.linalg.norm(u[mask])


PHANTOM_DIMS, PHANTOM_COILS, PHANTOM_CALIB, PHANTOM_K = (32, 28, 24), 4, 16, 4
GAP = 0.2               # maps are compared where the float64 gap lambda_1 - lambda_2 is at least this


def phantom_calib(dims=PHANTOM_DIMS, C=PHANTOM_COILS, calib=PHANTOM_CALIB):
    """An ellipsoid seen through C smooth coils -> (the central block of the exact transform of the coil images, rounded to complex64 as
    a file holds it, maps dims + (C,), image, support).

    The ellipsoid spans 75 % of every axis.  A larger one does not separate the eigenvalues better but worse: with 4 coils and a 4^3
    kernel the vectors S(x) exp(-2 pi i kappa xi / N) of a larger support span more of the 256-dimensional window space, and the second
    eigenvalue of G(x) rises with it.  Measured with this file (radius as a fraction of the half axis: share of the support with
    lambda_1 - lambda_2 >= 0.2, median lambda_2 there, recovery error): 0.5: 100 %, 0.45, 5e-4; 0.7: 100 %, 0.56, 8e-4; 0.75: 96 %,
    0.60, 7e-4; 0.8: 87 %, 0.66, 8e-4; 0.9: 56 %, 0.78, 4e-3; 1.0: 29 %, 0.87, 4e-2; 1.2: 2 %, 0.98, 0.21."""
    import maps64
    S = maps64.smooth_maps(dims, C, 1)[..., 0].astype(np.complex128)
    img, support = ellipsoid(dims)
    ksp = centred_fft(S * img[..., None])
    return cut_centre(ksp, calib).astype(C64), S, img, support


_CACHE = {}


def phantom_reference():
    """the restatement on the phantom at k = 4, M = 1, crop = 0, computed once per process:
    dict(calib, S, support, maps, lam, ev (all eigenvalues), well (gap >= GAP), truth)"""
    if 'phantom' not in _CACHE:
        calib, S, img, support = phantom_calib()
        maps, lam, G = espirit(calib, PHANTOM_DIMS, PHANTOM_K, M=1, crop=0.0)
        ev = all_evals(G)
        _CACHE['phantom'] = dict(calib=calib, S=S, support=support, maps=maps, lam=lam, ev=ev, well=(ev[..., 0] - ev[..., 1]) >= GAP,
                                 truth=normalised(S))
    return _CACHE['phantom']


def two_set_reference():
    """the restatement on the two-set calibration data at k = 4, M = 2, crop = 0, computed once per process"""
    if 'two' not in _CACHE:
        calib, S, both = two_set_calib()
        maps, lam, G = espirit(calib, PHANTOM_DIMS, PHANTOM_K, M=2, crop=0.0)
        _CACHE['two'] = dict(calib=calib, S=S, both=both, maps=maps, lam=lam,
                             residual=[span_residual(S[..., m], maps, both) for m in range(2)])
    return _CACHE['two']


def write_calib(tmpdir, calib, name):
    path = os.path.join(str(tmpdir), name)
    np.savez(path, calib=np.asarray(calib, dtype=C64).T)
    return path


def two_set_calib(dims=(32, 28, 24), C=4, calib=16):
    """calibration data of the soft-SENSE model: two sets of maps on two overlapping images -> (block, S dims + (C, 2), both non-zero)"""
    import maps64
    S = maps64.smooth_maps(dims, C, 2).astype(np.complex128)
    img0, sup0 = ellipsoid(dims, radii=(0.8, 0.85, 0.9), centre=(-0.1, 0.0, 0.0))
    img1, sup1 = ellipsoid(dims, radii=(0.7, 0.8, 0.85), centre=(0.2, 0.05, 0.0))
    img1 = img1 * np.exp(1j * 0.7) * 0.8
    ksp = centred_fft(S[..., 0] * img0[..., None] + S[..., 1] * img1[..., None])
    return cut_centre(ksp, calib).astype(C64), S, sup0 & sup1


# the radial scan of the non-Cartesian route: image, coils, readout, spokes, oversampling, kernel half-width
NC_DIMS, NC_COILS, NC_NRO, NC_NSP, NC_OSF, NC_WIDTH = (32, 32, 32), 3, 64, 400, 2.0, 2
# -t 0.01 there: width-2 gridding at osf 2 and 15 CG iterations without density compensation leave the 16^3 block within 9 % of the exact
# transform (measured), far above 1e-3 of the largest singular value; at t = 0.001 every error direction is kept, P is close to the
# identity and the maps are arbitrary (recovery error 1.3), at 0.01 the error is 0.021, at 0.03 signal directions go too (0.18)
NC_ARGS = ["-r", "16", "-k", "4", "-t", "0.01", "--osf", str(NC_OSF), "--width", str(NC_WIDTH)]


def noncart_scan(tmpdir, B, name="radial.npz", nsp=NC_NSP):
    """maps64.softsense_scan with one set of maps and no `calib` -> (path, true maps dims + (C,), the object's support)"""
    import maps64
    B._scratch = None
    path = maps64.softsense_scan(tmpdir, B, NC_DIMS, NC_COILS, 1, NC_NRO, nsp, NC_OSF, NC_WIDTH, name=name)
    B._scratch = None
    img = maps64.objects(NC_DIMS, 1)[0]
    return path, maps64.smooth_maps(NC_DIMS, NC_COILS, 1)[..., 0].astype(np.complex128), np.abs(img) > 0.05 * np.abs(img).max()
