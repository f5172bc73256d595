"""The K x K kernel of transformed point-spread functions that `operators.ToeplitzNormal` applies (pics --toeplitz).

The exact normal operator of frame t of a non-Cartesian scan is Toeplitz, (A_t^H A_t x)[i] = sum_j q_t[i - j] x[j] with
q_t[d] = s sum_m exp(2 pi i k_{t,m} . d), and in a temporal subspace x_t = sum_k Phi[t, k] alpha_k

    (A^H A alpha)_k = sum_k' psf_kk' * alpha_k',        psf_kk' = sum_t conj(Phi[t, k]) Phi[t, k'] q_t.

On the grid of twice the image size the convolution is a product with P_kk' = FFT(psf_kk'), Hermitian at every grid point.
q_t comes from ONE adjoint NUFFT of a vector of ones onto the image of twice the size, per distinct trajectory.
"""
import logging
import time

import numpy as np

log = logging.getLogger(__name__)
_C64 = np.dtype('complex64')

MAXK = 8


def kernel_bytes(K, dims):
    """bytes of the kernel array for K coefficient images of a `dims` volume: 4 K^2 floats' worth per point of the 2x grid"""
    return 4 * int(K) ** 2 * 8 * int(np.prod([int(n) for n in dims], dtype=np.int64))


def nufft_gain(width, osf):
    """the amplitude gain per axis of `Backend.NUFFT` over the NUDFT divided by the root of its oversampled grid's size: its
    Kaiser-Bessel kernel is not normalised, a sample collects sum_taps kb(|tap - pos| / width) ~ width * int_{-1}^{1} kb(u) du =
    2 width sinh(beta) / (beta I0(beta)) per axis, and the roll-off is 1 at the image centre"""
    from scipy.special import i0
    from indigo_amd.backends.backend import Backend
    beta = Backend.nufft_params(width, osf)[1]
    return 2.0 * width * np.sinh(beta) / (beta * i0(beta))


def pack_planes(P, order='xyz'):
    """(K, K) + grid complex array of Hermitian matrices -> the (K^2, prod grid) float32 planes of `Backend.psf_mix`: the K real
    diagonals, then re and im of every pair (k < k'), row-major over the upper triangle; every plane flattened in the grid's
    memory order: 'xyz' (F order) or 'xzy'"""
    K = P.shape[0]
    out = np.empty((K * K, int(np.prod(P.shape[2:]))), dtype=np.float32)

    def flat(v):
        return (v.transpose(0, 2, 1) if order == 'xzy' else v).reshape(-1, order='F')
    for k in range(K):
        out[k] = flat(P[k, k].real)
    pair = 0
    for a in range(K):
        for b in range(a + 1, K):
            out[K + 2 * pair] = flat(P[a, b].real)
            out[K + 2 * pair + 1] = flat(P[a, b].imag)
            pair += 1
    return out


def psf_kernel(B, dims, trajs, which, phi, width, osf, order='xyz', recipe=None, sample_weights=None, density=None):
    """The kernel array of `ToeplitzNormal` for an image of `dims` voxels: host float32 (K^2, 8 prod dims), planes as in
    `pack_planes`, in the grid memory order `order`.

    trajs   the DISTINCT trajectories, each (3, readout, views) in cycles per pixel of the image (what `Backend.NUFFT` takes)
    which   for every frame t the index of its trajectory in `trajs`
    phi     the T x K temporal basis, or None: K = 1 with a weight of one per frame (one frame: which = [0])
    width, osf   the Kaiser-Bessel half-width and the oversampling of the run's own NUFFT: q_t is computed with the same
    recipe  optional pass list (indigo_amd.transforms.Optimize) for the set-up transform's tree
    sample_weights   optional (samples, L) complex array for ONE trajectory and no basis, the per-sample interpolator of a
            time-segmented field-map model (indigo_amd.fmap): K = L, and pair (a, b) is the adjoint NUFFT of
            conj(w[:, a]) w[:, b] in place of W[a, b] times that of ones: L (L + 1) / 2 set-up transforms.  The kernel stays
            Hermitian at every grid point, psf_ba[d] = conj(psf_ab[-d]).  None: the planes are what they were without it.
    density   optional: one real non-negative array per DISTINCT trajectory, a weight per sample (pics --dcf):
            the kernel of A^H W A.  q_t becomes the adjoint NUFFT of w in place of that of ones, and with `sample_weights` the
            pair products are multiplied by w.  None: the planes are what they were without it.

    q_t is computed once per distinct trajectory: B.NUFFT(..., N = 2 dims).H applied to ones.  The sample at image index j is the
    lag d = j - dims (the centred transform's origin), and psf[d] belongs at index d mod 2 dims: a circular shift by half the
    grid, which is the sign (-1)^(gx + gy + gz) after the transform.  The constants: the NUFFT's centred transform is unitary over
    ITS oversampled grid, int(2 dims osf) here and int(dims osf) in the operator that is being replaced, so
    psf = sqrt(prod int(2 dims osf)) / prod int(dims osf) * q; and the unscaled inverse transform of `ToeplitzNormal` needs
    1 / (8 prod dims).  Both are folded into P."""
    from indigo_amd.transforms import Optimize, reserve_for
    t0 = time.perf_counter()
    dims = tuple(int(n) for n in dims)
    grid = tuple(2 * n for n in dims)
    P = int(np.prod(grid))
    which = [int(w) for w in which]
    T = len(which)
    if sample_weights is not None:
        if phi is not None or T != 1 or len(trajs) != 1:
            raise ValueError("psf_kernel: sample weights go with one trajectory, one frame and no basis")
        sample_weights = np.asarray(sample_weights, dtype=np.complex128)
        nsamp = int(np.prod(np.asarray(trajs[0]).shape[1:]))
        if sample_weights.ndim != 2 or sample_weights.shape[0] != nsamp:
            raise ValueError("psf_kernel: sample weights of shape %s for %d samples" % (sample_weights.shape, nsamp))
        phi = np.ones((1, sample_weights.shape[1]), dtype=np.complex128)        # (its shape only: K = L)
    phi = np.ones((T, 1), dtype=np.complex128) if phi is None else np.asarray(phi, dtype=np.complex128)
    if phi.ndim != 2 or phi.shape[0] != T:
        raise ValueError("psf_kernel: a basis of shape %s for %d frames" % (phi.shape, T))
    K = phi.shape[1]
    if not 1 <= K <= MAXK:
        raise ValueError("psf_kernel: %d coefficient images, at most %d are supported: the kernel array holds 4 K^2 bytes per grid point, "
                         "%.1f GB here (137 GB at K = 16 on a 512^3 grid)" % (K, MAXK, kernel_bytes(K, dims) / 1e9))
    if density is not None:
        if len(density) != len(trajs):
            raise ValueError("psf_kernel: %d sets of sample weights for %d distinct trajectories" % (len(density), len(trajs)))
        density = [np.asarray(w, dtype=np.float64).reshape(-1, order='F') for w in density]
        for w, trj in zip(density, trajs):
            if w.size != int(np.prod(np.asarray(trj).shape[1:])):
                raise ValueError("psf_kernel: %d sample weights for a trajectory of %d samples" % (w.size, int(np.prod(np.asarray(trj).shape[1:]))))
    pairs = [(a, b) for a in range(K) for b in range(a, K)]
    vols = {}
    for d, trj in enumerate(trajs):
        frames = [t for t in range(T) if which[t] == d]
        if not frames:
            continue
        W = phi[frames].conj().T @ phi[frames]                           # Gram weights of this trajectory's frames
        trj = np.asarray(trj, dtype=np.float64)
        F = B.NUFFT((1,) + tuple(trj.shape[1:]), grid, trj, width=width, oversamp=(osf, osf, osf), dtype=_C64)
        if recipe:
            F = Optimize(recipe).visit(B.KronI(1, F) * B.VStack([B.Diag(np.ones(grid + (1,), dtype=_C64))], name='maps'))
        reserve_for(F, 1, slack_products=4)
        if sample_weights is not None:
            for a, b in pairs:
                w = sample_weights[:, a].conj() * sample_weights[:, b]
                w = (w if density is None else w * density[d]).astype(_C64).reshape((-1, 1))
                w = B.copy_array(np.asfortranarray(w), name='psf.weights')
                vols[(a, b)] = B.zero_array((P, 1), _C64, name='psf.%d.%d' % (a, b))
                F.H.eval(vols[(a, b)], w)
                del w
            del F
            continue
        ones = np.ones((F.shape[0], 1), dtype=_C64, order='F') if density is None else np.asfortranarray(density[d].astype(_C64).reshape((-1, 1)))
        ones = B.copy_array(ones, name='psf.ones')
        q = B.zero_array((P, 1), _C64, name='psf.q')
        F.H.eval(q, ones)
        del ones, F
        for a, b in pairs:
            if W[a, b] == 0 and (a, b) in vols:
                continue
            if (a, b) not in vols:
                vols[(a, b)] = B.zero_array((P, 1), _C64, name='psf.%d.%d' % (a, b))
                B.axpby(0, vols[(a, b)], complex(W[a, b]), q)
            else:
                B.axpby(1, vols[(a, b)], complex(W[a, b]), q)
        del q
    oN1 = [int(n * osf) for n in dims]
    oN2 = [int(n * osf) for n in grid]
    const = nufft_gain(width, osf) ** 3 * np.sqrt(float(np.prod(oN2, dtype=np.float64))) / float(np.prod(oN1, dtype=np.float64)) / P
    sign = 1
    for a, n in enumerate(grid):
        sign = sign * (1.0 - 2.0 * (np.arange(n) % 2)).reshape([-1 if i == a else 1 for i in range(3)])
    sign = (sign * const).astype(np.float32)
    planes = np.empty((K * K, P), dtype=np.float32)
    B.reserve_scratch(B._fft_workspace_size(grid + (1,)) // 8 + 64)       # every volume is transformed in place

    def flat(v):
        return (v.transpose(0, 2, 1) if order == 'xzy' else v).reshape(-1, order='F')
    pair = 0
    for a, b in pairs:
        v = vols.pop((a, b)).reshape(grid + (1,))
        B.fftn(v, v)
        h = v.to_host().reshape(grid, order='F')
        del v
        if a == b:
            planes[a] = flat(h.real * sign)
        else:
            planes[K + 2 * pair] = flat(h.real * sign)
            planes[K + 2 * pair + 1] = flat(h.imag * sign)
            pair += 1
    log.info("toeplitz: kernel of %d x %d point-spread functions on the %s grid from %d distinct trajectories, %.1f MB, set up in %.2f s",
             K, K, grid, len(trajs), planes.nbytes / 1e6, time.perf_counter() - t0)
    return planes
