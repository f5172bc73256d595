"""The `Backend` plugin surface: device arrays, device CSR matrices, the leaf
kernel contract, operator factories, the scratch arena and CG.

Own re-statement of indigo/backends/backend.py (the boundary named by the
north star).  A concrete backend subclasses `Backend`, provides
`dndarray._malloc/_free/_zero/_copy_from/_copy_to/_copy/__getitem__` and the
leaf kernels (`axpby, scale, dot, norm2, fftn, ifftn, ccsrmm, max`).  Method
names, argument order (outputs first: `fftn(y, x)`, `ccsrmm(y, ...)`,
`axpby(beta, y, alpha, x)`) and error behaviour follow the reference:

  dndarray                      backend.py:22-220
  scratch (LIFO bump arena)     backend.py:262-281
  factories Diag..NUFFT         backend.py:287-448
  leaf contract                 backend.py:453-533
  csr_matrix                    backend.py:535-596
  cg                            backend.py:639-689

Differences, all deliberate: structure analysis (`inspect`) comes from the
backend instead of the optional `_customcpu` module (whose absence breaks every
adjoint in the reference, backend.py:564-567 vs :585); `Zpad` indexes with a
tuple of slices (the reference's list indexing is an IndexError on numpy >=
1.23); `beta == 0` never reads `y` (BLAS rule; the numpy oracle multiplies
0 * y and so propagates NaNs from uninitialised memory).
"""
import logging
from contextlib import contextmanager

import numpy as np
import scipy.sparse as spp

import indigo_amd.operators as op

log = logging.getLogger(__name__)
_C64 = np.dtype('complex64')


# Daubechies minimum-phase low-pass filters of the wavelet transform (Backend.dwt3, operators.Wavelet); the
# high-pass filter is g[j] = (-1)^j h[L-1-j].  The same constants are compiled into indigo_amd/csrc/ig_wavelet.hip.
WAVELETS = {
    'haar': (2 ** -0.5, 2 ** -0.5),
    'db2': (0.48296291314453416, 0.8365163037378079, 0.22414386804201339, -0.12940952255126037),
    'db4': (0.23037781330889645, 0.7148465705529156, 0.630880767929859, -0.027983769416859594,
            -0.18703481171909306, 0.03084138183556063, 0.032883011666885176, -0.010597401785069018),
}
WAVELET_IDS = {'haar': 0, 'db2': 1, 'db4': 2}     # the `wavelet` argument of ig_dwt3_c64
DWT_MAX_AXIS = 1024


def dwt_plan(dims, wavelet, levels):
    """-> (passes, coarse): the forward passes of the wavelet transform of an F-ordered `dims` volume, in order, as
    (box before the split, axis split), and the low-pass corner box the last level leaves.  Level 1 splits the whole volume,
    level l+1 the box level l left; within a level the axes go 0, 1, 2 and an axis splits while its current length is even and
    at least twice the filter's length.  The transform stops after `levels` levels or at the first level where nothing splits."""
    taps = len(WAVELETS[wavelet])
    c = [int(n) for n in dims]
    assert len(c) == 3, dims
    passes = []
    for _ in range(int(levels)):
        split = False
        for a in range(3):
            if c[a] % 2 == 0 and c[a] >= 2 * taps:
                passes.append((tuple(c), a))
                c[a] //= 2
                split = True
        if not split:
            break
    return passes, tuple(c)


def _grad_forward(v, comps=3):
    """D v for v of shape dims + (ncols,): shape dims + (comps, ncols) -- the F-ordered 3N-row columns of Backend.grad3 -- forward
    differences, zero at the far face; comps = 4 adds the difference along the columns, the frames of Backend.grad4, zero in
    the last one"""
    out = np.zeros(v.shape[:3] + (comps,) + v.shape[3:], dtype=v.dtype)
    out[:-1, :, :, 0] = v[1:] - v[:-1]
    out[:, :-1, :, 1] = v[:, 1:] - v[:, :-1]
    out[:, :, :-1, 2] = v[:, :, 1:] - v[:, :, :-1]
    if comps == 4:
        out[:, :, :, 3, :-1] = v[..., 1:] - v[..., :-1]
    return out


def _grad_adjoint(t):
    """D^H t for t of shape dims + (3, ncols), D4^H t for dims + (4, ncols): shape dims + (ncols,); t on the far face of its own
    axis, and its fourth component in the last column, is not read"""
    out = np.zeros(t.shape[:3] + t.shape[4:], dtype=t.dtype)
    out[1:] += t[:-1, :, :, 0]
    out[:-1] -= t[:-1, :, :, 0]
    out[:, 1:] += t[:, :-1, :, 1]
    out[:, :-1] -= t[:, :-1, :, 1]
    out[:, :, 1:] += t[:, :, :-1, 2]
    out[:, :, :-1] -= t[:, :, :-1, 2]
    if t.shape[3] == 4:
        out[..., 1:] += t[:, :, :, 3, :-1]
        out[..., :-1] -= t[:, :, :, 3, :-1]
    return out


def _back_diff(w, a):
    """B_a w = -D_a^H w along axis a < 3 of w: (i_a < n_a - 1 ? w[i] : 0) - (i_a > 0 ? w[i - e_a] : 0)"""
    w = np.moveaxis(w, a, 0)
    out = np.zeros_like(w)
    out[:-1] += w[:-1]
    out[1:] -= w[:-1]
    return np.moveaxis(out, 0, a)


def _fwd_diff(w, a):
    """D_a w along axis a < 3 of w: w[i + e_a] - w[i] where i_a < n_a - 1, else 0"""
    w = np.moveaxis(w, a, 0)
    out = np.zeros_like(w)
    out[:-1] = w[1:] - w[:-1]
    return np.moveaxis(out, 0, a)


_SYM_PAIRS = ((0, 1), (0, 2), (1, 2))                     # the off-diagonal components xy, xz, yz of Backend.symgrad3, after xx, yy, zz


def _symgrad_forward(v):
    """E v for v of shape dims + (3, ncols): shape dims + (6, ncols), the 6N-row columns of Backend.symgrad3"""
    out = np.zeros(v.shape[:3] + (6,) + v.shape[4:], dtype=v.dtype)
    for a in range(3):
        out[:, :, :, a] = _back_diff(v[:, :, :, a], a)
    for c, (a, b) in enumerate(_SYM_PAIRS):
        out[:, :, :, 3 + c] = (_back_diff(v[:, :, :, a], b) + _back_diff(v[:, :, :, b], a)) / np.sqrt(2.0)
    return out


def _symgrad_adjoint(q):
    """E^H q for q of shape dims + (6, ncols): shape dims + (3, ncols)"""
    out = np.zeros(q.shape[:3] + (3,) + q.shape[4:], dtype=q.dtype)
    for a in range(3):
        out[:, :, :, a] -= _fwd_diff(q[:, :, :, a], a)
    for c, (a, b) in enumerate(_SYM_PAIRS):
        out[:, :, :, a] -= _fwd_diff(q[:, :, :, 3 + c], b) / np.sqrt(2.0)
        out[:, :, :, b] -= _fwd_diff(q[:, :, :, 3 + c], a) / np.sqrt(2.0)
    return out


def _ball(t, radius):
    """t of shape dims + (comps, ncols) scaled per voxel and column onto the 2-norm ball of `radius` over its components"""
    r = np.sqrt((t.real ** 2 + t.imag ** 2).sum(axis=3, keepdims=True))
    with np.errstate(divide='ignore', invalid='ignore'):
        return t * np.where(r <= float(radius), 1.0, float(radius) / r)


def dwt_coarse_box(dims, wavelet, levels):
    """the coarse (approximation) box that `dwt_plan` leaves: the part of the coefficients soft_threshold keeps"""
    return dwt_plan(dims, wavelet, levels)[1]


def _dwt_split(u, h, inverse):
    """one periodic split along axis 0 of u (complex128, axis 0 of even length d): low to [0, d/2), high to [d/2, d)"""
    h = np.asarray(h, dtype=np.float64)
    L, d = h.size, u.shape[0]
    g = h[::-1] * (-1.0) ** np.arange(L)
    idx = (2 * np.arange(d // 2)[:, None] + np.arange(L)[None, :]) % d          # (d/2, L)
    u2 = u.reshape((d, -1))
    if not inverse:
        taps = u2[idx]                                                          # (d/2, L, rest)
        out = np.concatenate([np.einsum('klr,l->kr', taps, h), np.einsum('klr,l->kr', taps, g)])
    else:
        # v[2m + r] = sum_i h[2i + r] low[(m - i) mod d/2] + g[2i + r] high[(m - i) mod d/2],  r = 0, 1
        half = d // 2
        src = (np.arange(half)[:, None] - np.arange(L // 2)[None, :]) % half    # (d/2, L/2)
        low, high = u2[:half][src], u2[half:][src]
        out = np.empty_like(u2)
        for r in (0, 1):
            out[r::2] = np.einsum('mir,i->mr', low, h[r::2]) + np.einsum('mir,i->mr', high, g[r::2])
    return out.reshape(u.shape)


class Backend(object):

    def __init__(self, device_id=0):
        self.trace = None          # attach an indigo_amd.util.Trace to record leaf calls

    # ---------------------------------------------------------------------------
    # device arrays
    # ---------------------------------------------------------------------------
    class dndarray(object):
        """N-d array in device memory, column-major, with a leading dimension.

        `shape[0]` elements are contiguous; column j of a 2-d view starts
        `_leading_dim * j` elements after column 0.  Views (`own=False`) never free.
        """
        _memory = dict()

        def __init__(self, backend, shape, dtype, ld=None, own=True, data=None, name=''):
            assert isinstance(shape, (tuple, list))
            self.shape = tuple(int(s) for s in shape)
            self.dtype = np.dtype(dtype)
            self._backend = backend
            self._leading_dim = int(ld) if ld else (self.shape[0] if self.shape else 1)
            self._own = own
            self._name = name
            if data is None:
                self._arr = self._malloc(self.shape, self.dtype)
                self._memory[id(self)] = (name, self.shape, self.dtype)
            else:
                self._arr = data

        # -- metadata ---------------------------------------------------------------
        @property
        def size(self):
            return int(np.prod(self.shape, dtype=np.int64))

        @property
        def itemsize(self):
            return self.dtype.itemsize

        @property
        def nbytes(self):
            return self.size * self.dtype.itemsize

        @property
        def ndim(self):
            return len(self.shape)

        @property
        def contiguous(self):
            return self.ndim == 1 or self._leading_dim == self.shape[0]

        def reshape(self, new_shape):
            """View with a new shape.  Mirrors the leading-dimension rules of backend.py:59-89."""
            new_shape = tuple(int(s) for s in new_shape)
            if -1 in new_shape:
                known = -int(np.prod(new_shape, dtype=np.int64))
                assert known > 0 and self.size % known == 0, \
                    "Cannot reshape {} into {}. (size mismatch)".format(self.shape, new_shape)
                new_shape = tuple(self.size // known if s == -1 else s for s in new_shape)
            assert int(np.prod(new_shape, dtype=np.int64)) == self.size, \
                "Cannot reshape {} into {}. (size mismatch)".format(self.shape, new_shape)
            if new_shape[0] > self.shape[0]:
                assert self.shape[0] == self._leading_dim, "Cannot stack non-contiguous columns."
            ld = new_shape[0] if new_shape[0] < self.shape[0] else self._leading_dim
            return self._view(new_shape, ld, self._arr)

        def dense_rows(self, start, stop):
            """rows [start, stop) of every column, as `a[start:stop, :]` gives them; of a one-column array the view is a contiguous
            vector (leading dimension = its length) whatever the parent's leading dimension is"""
            v = self[slice(start, stop), :]
            return v._view(v.shape, v.shape[0], v._arr) if v.shape[1] == 1 else v

        def _view(self, shape, ld, data):
            v = self._backend.dndarray(self._backend, shape, self.dtype, ld=ld, own=False, data=data)
            v._base = getattr(self, '_base', None) or self     # keep the owner alive
            return v

        # -- transfers ----------------------------------------------------------------
        def copy_from(self, arr):
            """host -> device into an existing array"""
            assert isinstance(arr, np.ndarray)
            if self.size != arr.size:
                raise ValueError("size mismatch, expected {} got {}".format(self.shape, arr.shape))
            if self.dtype != arr.dtype:
                raise TypeError("dtype mismatch, expected {} got {}".format(self.dtype, arr.dtype))
            if not arr.flags['F_CONTIGUOUS']:
                raise TypeError("order mismatch, expected 'F' got {}".format(arr.flags['F_CONTIGUOUS']))
            self._copy_from(arr)

        def copy_to(self, arr):
            """device -> host into an existing array"""
            assert isinstance(arr, np.ndarray)
            if self.size != arr.size:
                raise ValueError("size mismatch, expected {} got {}".format(self.shape, arr.shape))
            if self.dtype != arr.dtype:
                raise TypeError("dtype mismatch, expected {} got {}".format(self.dtype, arr.dtype))
            self._copy_to(arr)

        def to_host(self):
            arr = np.ndarray(self.shape, self.dtype, order='F')
            self.copy_to(arr)
            return arr

        @contextmanager
        def on_host(self):
            arr = self.to_host()
            yield arr
            self.copy_from(arr)

        def copy(self, other=None, name=''):
            """`a.copy()` returns a device copy; `a.copy(b)` copies b into a."""
            if other is not None:
                assert isinstance(other, self._backend.dndarray)
                self._copy(other)
                return None
            dup = self._backend.zero_array(self.shape, self.dtype, name=name)
            dup._copy(self)
            return dup

        @classmethod
        def to_device(cls, backend, arr, name=''):
            arr_f = np.require(arr, requirements='F')
            d_arr = cls(backend, arr.shape, arr.dtype, name=name)
            d_arr.copy_from(arr_f)
            return d_arr

        def __setitem__(self, slc, other):
            assert isinstance(slc, slice) and not (slc.start or slc.stop), "dndarray setitem cant slice"
            self._copy(other)

        def __del__(self):
            if getattr(self, '_own', False) and hasattr(self, '_arr'):
                self._memory.pop(id(self), None)
                try:
                    self._free()
                except Exception:       # interpreter shutdown: the library may be gone already
                    pass

        # -- to be provided by the concrete backend ---------------------------------
        def __getitem__(self, slc):
            raise NotImplementedError()

        def _copy_from(self, arr):
            raise NotImplementedError()

        def _copy_to(self, arr):
            raise NotImplementedError()

        def _copy(self, d_arr):
            raise NotImplementedError()

        def _malloc(self, shape, dtype):
            raise NotImplementedError()

        def _free(self):
            raise NotImplementedError()

        def _zero(self):
            raise NotImplementedError()

    def copy_array(self, arr, name=''):
        return self.dndarray.to_device(self, arr, name=name)

    def empty_array(self, shape, dtype, name=''):
        return self.dndarray(self, shape, dtype, name=name)

    def zero_array(self, shape, dtype, name=''):
        d_arr = self.empty_array(shape, dtype, name=name)
        d_arr._zero()
        return d_arr

    def zeros_like(self, other, name=''):
        return self.zero_array(other.shape, other.dtype, name=name)

    def rand_array(self, shape, dtype=_C64, name='', seed=None):
        rng = np.random.default_rng(seed)
        x = rng.random(shape) + 1j * rng.random(shape)
        x = np.require(x, dtype=_C64, requirements='F')
        return self.copy_array(x, name=name)

    def get_max_threads(self):
        return 1

    def barrier(self):
        pass

    def mem_usage(self):
        total = 0
        rows = []
        for name, shape, dtype in list(self.dndarray._memory.values()):
            n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
            rows.append((n, name, shape, dtype))
            total += n
        log.info("Memory report:")
        for n, name, shape, dtype in sorted(rows, key=lambda r: r[0]):
            if n > 1e6:
                log.info("  %40s: % 3.0f MB, %20s, %15s", name, n / 1e6, shape, dtype)
        return total

    # ---------------------------------------------------------------------------
    # scratch arena
    # ---------------------------------------------------------------------------
    def reserve_scratch(self, nelems):
        """Reserve a complex64 arena of `nelems` elements for `scratch()` (LIFO)."""
        self._scratch = self.empty_array((max(int(nelems), 1),), _C64, name='scratch')
        self._scratch_pos = 0

    def release_scratch(self):
        """Drop the arena: `scratch()` allocates dynamically until the next `reserve_scratch`."""
        self._scratch = None

    @contextmanager
    def scratch(self, shape=None, nbytes=None):
        assert not (shape is not None and nbytes is not None), \
            "Specify either shape or nbytes to backend.scratch()."
        if nbytes is not None:
            shape = (int(nbytes) // _C64.itemsize,)
        size = int(np.prod(shape, dtype=np.int64))
        arena = getattr(self, '_scratch', None)
        if arena is not None and self._scratch_pos + size > arena.size:
            # the arena was sized for another tree: serve this request dynamically instead of failing
            # (the reference asserts here, backend.py:272)
            log.warning("scratch arena too small (wanted %d elements at offset %d of %d); allocating dynamically",
                        size, self._scratch_pos, arena.size)
            arena = None
        if arena is not None:
            pos = self._scratch_pos
            mem = arena[pos:pos + size].reshape(tuple(shape))
            # keep successive carvings 256-byte aligned (32 complex64) like fresh allocations
            bump = (size + 31) // 32 * 32
            self._scratch_pos += bump
            try:
                yield mem
            finally:
                self._scratch_pos -= bump
        else:
            mem = self.zero_array(tuple(shape), dtype=_C64, name='scratch(dynamic)')
            yield mem
            del mem

    # ---------------------------------------------------------------------------
    # operator factories
    # ---------------------------------------------------------------------------
    def SpMatrix(self, M=None, **kwargs):
        assert (M is not None and spp.issparse(M)) or kwargs.get('struct') is not None
        return op.SpMatrix(self, M, **kwargs)

    def DenseMatrix(self, M, **kwargs):
        assert isinstance(M, np.ndarray) and M.ndim == 2
        return op.DenseMatrix(self, M, **kwargs)

    def Diag(self, v, **kwargs):
        """diag(v); v is flattened in memory ('A') order, i.e. F order for F arrays"""
        v = np.require(v, requirements='F')
        if v.ndim > 1:
            v = v.flatten(order='A')
        dtype = kwargs.pop('dtype', _C64)
        if np.dtype(dtype) == _C64:
            # (described as the diagonal it is: the scipy matrix is made when somebody asks for it, indigo_amd.structured)
            from indigo_amd.structured import DiagS
            return self.SpMatrix(struct=DiagS(v.size, [('vec', v.astype(_C64))]), **kwargs)
        return self.SpMatrix(spp.diags(v, offsets=0).astype(dtype), **kwargs)

    def Adjoint(self, A, **kwargs):
        return op.Adjoint(self, A, **kwargs)

    def KronI(self, c, B, **kwargs):
        """I_c (x) B"""
        return op.Kron(self, self.Eye(c), B, **kwargs)

    def Kron(self, A, B, **kwargs):
        return op.Kron(self, A, B, **kwargs)

    def BlockDiag(self, Ms, **kwargs):
        return op.BlockDiag(self, *Ms, **kwargs)

    def VStack(self, Ms, **kwargs):
        return op.VStack(self, *Ms, **kwargs)

    def HStack(self, Ms, **kwargs):
        return op.HStack(self, *Ms, **kwargs)

    def UnscaledFFT(self, shape, dtype=_C64, **kwargs):
        return op.UnscaledFFT(self, shape, dtype=dtype, **kwargs)

    def Eye(self, n, dtype=_C64, **kwargs):
        return op.Eye(self, n, dtype=dtype, **kwargs)

    def ZpadFFT(self, grid_shape, box_shape, weights, **kwargs):
        """fused  KronI(C, UnscaledFFT) * zero-pad * diag(weights)  leaf (see operators.ZpadFFT)"""
        return op.ZpadFFT(self, grid_shape, box_shape, weights, **kwargs)

    def One(self, shape, dtype=_C64, **kwargs):
        return op.One(self, shape, dtype=dtype, **kwargs)

    def FFT(self, shape, dtype=_C64, **kwargs):
        """unitary FFT = diag(1/sqrt(n)) * UnscaledFFT"""
        n = int(np.prod(shape))
        if np.dtype(dtype) == _C64:
            from indigo_amd.structured import DiagS
            c = (np.ones(1, dtype=dtype) / np.sqrt(n))[0]          # the value the reference's ones(n) / sqrt(n) holds n times
            return self.SpMatrix(struct=DiagS(n, [('const', c)]), name='scale') * self.UnscaledFFT(shape, dtype, **kwargs)
        s = np.ones(n, order='F', dtype=dtype) / np.sqrt(n)
        return self.Diag(s, name='scale') * self.UnscaledFFT(shape, dtype, **kwargs)

    @staticmethod
    def fftc_mod_phases(ft_shape):
        """per-axis terms (idx_d - c_d/2) c_d / n_d of the modulation's phase (in turns)"""
        return [(np.arange(n) - (n // 2) / 2.0) * ((n // 2) / n) for n in ft_shape]

    @staticmethod
    def fftc_mod(ft_shape, dtype=_C64):
        """Modulation vector of the centred FFT: exp(2 pi i sum_d (idx_d - c_d/2) c_d / n_d), c_d = n_d // 2.  (The phase as a
        broadcast sum of per-axis terms, added in the reference's order: the same numbers without the index grids.)"""
        phase = 0
        for i, ph in enumerate(Backend.fftc_mod_phases(ft_shape)):
            phase = phase + ph.reshape([-1 if j == i else 1 for j in range(len(ft_shape))])
        return np.exp(1j * 2.0 * np.pi * phase).astype(dtype)

    def FFTc(self, ft_shape, dtype=_C64, normalize=True, **kwargs):
        """centred (fftshift-ed) FFT as mod * F * mod"""
        if np.dtype(dtype) == _C64:
            from indigo_amd.structured import DiagS, SepPhase
            M = self.SpMatrix(struct=DiagS(int(np.prod(ft_shape)), [('sep', SepPhase(ft_shape, self.fftc_mod_phases(ft_shape)))]), name='mod')
        else:
            M = self.Diag(self.fftc_mod(ft_shape, dtype), name='mod')
        F = self.FFT(ft_shape, dtype=dtype, **kwargs) if normalize else self.UnscaledFFT(ft_shape, dtype=dtype, **kwargs)
        return M * F * M

    @staticmethod
    def zpad_rows(M, N, mode='center'):
        """Flat (F-order) indices in the padded volume M that receive the N-volume's samples."""
        if mode == 'center':
            slc = tuple(slice(m // 2 + int(np.ceil(-n / 2)), m // 2 + int(np.ceil(n / 2))) for m, n in zip(M, N))
        elif mode == 'edge':
            slc = tuple(slice(n) for n in N)
        else:
            raise ValueError("unknown zpad mode %r" % mode)
        x = np.arange(int(np.prod(M)), dtype=np.int64).reshape(M, order='F')
        return x[slc].flatten(order='F')

    def Zpad(self, M, N, mode='center', dtype=_C64, **kwargs):
        """zero-pad an N-volume into an M-volume; a 0/1 matrix of shape (prod M, prod N)"""
        rows = self.zpad_rows(M, N, mode)
        cols = np.arange(rows.size)
        if np.dtype(dtype) == _C64:
            from indigo_amd.structured import SelectS
            return self.SpMatrix(struct=SelectS((int(np.prod(M)), int(np.prod(N))), rows, cols, np.ones(rows.size, dtype=_C64)), **kwargs)
        mat = spp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(int(np.prod(M)), int(np.prod(N))), dtype=dtype)
        return self.SpMatrix(mat, **kwargs)

    def Crop(self, M, N, dtype=_C64, **kwargs):
        return self.Zpad(N, M, dtype=dtype, **kwargs).H

    def AxisPermute(self, dims, perm, **kwargs):
        """the image -> image relabelling of the axes of an F-ordered `dims` volume: output axis a is input axis perm[a]
        (see operators.AxisPermute)"""
        return op.AxisPermute(self, dims, perm, **kwargs)

    def Wavelet(self, dims, wavelet='db2', levels=3, **kwargs):
        """the unitary wavelet transform of an F-ordered `dims` volume (see operators.Wavelet); .H is its inverse"""
        return op.Wavelet(self, dims, wavelet=wavelet, levels=levels, **kwargs)

    def Gradient(self, dims, **kwargs):
        """the forward-difference gradient of an F-ordered `dims` volume, shape (3N, N) (see operators.Gradient); .H is its adjoint"""
        return op.Gradient(self, dims, **kwargs)

    def SymGradient(self, dims, **kwargs):
        """the symmetrised backward difference of a 3-component field on an F-ordered `dims` volume, shape (6N, 3N) (see
        operators.SymGradient); .H is its adjoint"""
        return op.SymGradient(self, dims, **kwargs)

    def GradientT(self, dims, frames, **kwargs):
        """the gradient of `frames` time frames of a `dims` volume with the forward difference between neighbouring frames as a
        fourth component, shape (4NT, NT) (see operators.GradientT); .H is its adjoint"""
        return op.GradientT(self, dims, frames, **kwargs)

    def FrameBasis(self, phi, n, **kwargs):
        """Phi (x) I_n for the T x K temporal basis `phi` and images of `n` voxels, shape (nT, nK): K coefficient images stacked
        coefficient-major in, T frames stacked frame-major out (see operators.FrameBasis); .H is its adjoint"""
        return op.FrameBasis(self, phi, n, **kwargs)

    def SegmentPhase(self, f, taus, n, **kwargs):
        """the voxel side of the time-segmented off-resonance model for the field map `f` (n values in Hz) and the L equispaced
        segment times `taus`, shape (nL, n): one image in, its L segments stacked segment-major out (see operators.SegmentPhase);
        .H is its adjoint"""
        return op.SegmentPhase(self, f, taus, n, **kwargs)

    def SegmentCombine(self, b, period, n, **kwargs):
        """the sample side of the time-segmented off-resonance model for the P x L interpolator table `b` (P = `period`) and `n`
        sample rows, shape (n, nL): the L segments' samples stacked segment-major in, the samples out (see
        operators.SegmentCombine); .H is its adjoint"""
        return op.SegmentCombine(self, b, period, n, **kwargs)

    def CoilMaps(self, maps, **kwargs):
        """the soft-SENSE map stack for the host array `maps` = dims + (C, M), shape (N C, N M): M images stacked map-major in, C
        coil images stacked coil-major out (see operators.CoilMaps); .H is its adjoint"""
        return op.CoilMaps(self, maps, **kwargs)

    def NlinvProduct(self, n, ncoils, **kwargs):
        """the derivative of NLINV's bilinear coil product at a point set with `set_point`, shape (n C, n (1 + C)): (d rho | d c) in,
        C coil images stacked coil-major out (see operators.NlinvProduct); .H is its adjoint"""
        return op.NlinvProduct(self, n, ncoils, **kwargs)

    def SobolevCoils(self, dims, ncoils, a, b, **kwargs):
        """the coil weighting of NLINV on the unknown (rho, c^_1 ... c^_C) of a `dims` volume, shape (N (1 + C), N (1 + C)): rho
        passes, every c^_c becomes the coil sensitivity W c^_c (see operators.SobolevCoils); .H is its adjoint"""
        return op.SobolevCoils(self, dims, ncoils, a, b, **kwargs)

    def ZpadFFTMaps(self, grid_shape, box_shape, weights, maps, ncoils, **kwargs):
        """the fused ZpadFFT leaf with M images on its image side (see operators.ZpadFFTMaps)"""
        return op.ZpadFFTMaps(self, grid_shape, box_shape, weights, maps, ncoils, **kwargs)

    def Interp(self, N, coord, width, table, dtype=_C64, **kwargs):
        """gridding / interpolation matrix (npts x prod N) from a k-space trajectory"""
        assert len(N) == 3
        ndim = coord.shape[0]
        npts = int(np.prod(coord.shape[1:]))
        coord = coord.reshape((ndim, -1), order='F')
        from indigo_amd.structured import InterpS
        op = self.SpMatrix(struct=InterpS(N, coord, width, table, npts, make_plain=lambda: self._interp_matrix(npts, N, width, table, coord, dtype)), **kwargs)
        op._grid_dims = tuple(int(v) for v in N)        # the columns are the points of this grid, first axis fastest (a hint: hip.py)
        return op

    def _interp_matrix(self, npts, N, width, table, coord, dtype):
        """the gridding matrix itself (scipy): the vectorised numpy formulation of the reference's loop; backends with a native
        builder override this"""
        from indigo_amd.interp import interp_mat
        return interp_mat(npts, N, width, table, coord).astype(dtype)

    def gridding_from_struct(self, s, grid_order=0):
        """CSR (complex64, sorted columns) of an InterpS description with its columns numbered in `grid_order` (0: (x, y, z),
        1: (x, z, y)), built directly -- or None: the caller materialises the scipy matrix and permutes it"""
        return None

    @staticmethod
    def nufft_params(width, oversamp):
        omin = min(oversamp) if isinstance(oversamp, tuple) else oversamp
        beta = np.pi * np.sqrt(((width * 2. / omin) * (omin - 0.5)) ** 2 - 0.8)
        return omin, beta

    def NUFFT(self, M, N, coord, width=3, n=128, oversamp=None, dtype=_C64, **kwargs):
        """non-uniform FFT  G * Fc * Z * R  (interp, centred FFT, zero-pad, roll-off)"""
        assert len(M) == 3 and len(N) == 3
        assert tuple(M[1:]) == tuple(coord.shape[1:])
        from scipy.signal.windows import kaiser
        from indigo_amd.noncart import rolloff3
        omin, beta = self.nufft_params(width, oversamp)
        osf = oversamp if isinstance(oversamp, tuple) else (omin,) * 3
        oN = tuple(int(N[i] * osf[i]) for i in range(3))

        Z = self.Zpad(oN, N, dtype=dtype, name='zpad')
        F = self.FFTc(oN, dtype=dtype, name='fft')
        kb = kaiser(2 * n + 1, beta)[n:]
        G = self.Interp(oN, coord, width, kb, dtype=np.float32, name='interp')
        R = self.Diag(rolloff3(omin, width, beta, N), name='apod')
        return G * F * Z * R

    # ---------------------------------------------------------------------------
    # leaf-kernel contract
    # ---------------------------------------------------------------------------
    def axpby(self, beta, y, alpha, x):
        """y = beta*y + alpha*x"""
        raise NotImplementedError()

    def dot(self, x, y):
        """Re(x^H y)"""
        raise NotImplementedError()

    def norm2(self, x):
        """||x||_2 ** 2"""
        raise NotImplementedError()

    def scale(self, x, alpha):
        """x *= alpha"""
        raise NotImplementedError()

    def pdot(self, x, y, comm):
        v = self.dot(x, y)
        return v if comm is None else comm.allreduce(v)

    def pnorm2(self, x, comm):
        v = self.norm2(x)
        return v if comm is None else comm.allreduce(v)

    def fftn(self, y, x):
        raise NotImplementedError()

    def ifftn(self, y, x):
        raise NotImplementedError()

    def _fft_workspace_size(self, x_shape):
        return 0

    # fused zero-pad/crop transforms used by operators.ZpadFFT (not part of the reference's contract:
    # they replace its Zpad-CSR + FFT composition; see include/indigo_hip.h ig_fft_exec_padded)
    def fft_padded(self, y, x, w, grid, box_lo, box_dims, workspace=None, layout=0, support=None):
        """y[:, c] = FFT(zeropad(w[:, c] * x)); y: (prod grid, C), x: (prod box, 1), w: (prod box, C).
        layout 1 stores each grid in (x, z, y) memory order instead of (x, y, z); layout 2 additionally interleaves
        the coils below x (memory index c + C*(kx + n0*kz + n0*n2*ky)) and expects w interleaved, w[i*C + c]."""
        raise NotImplementedError()

    def ifft_cropped(self, xc, y, w, grid, box_lo, box_dims, workspace, layout=0, support=None):
        """xc[:, c] = conj(w[:, c]) * crop(IFFT(y[:, c])); xc: (prod box, C), y: (prod grid, C) left intact
        (layout 2: y, w and xc are coil-interleaved in memory)"""
        raise NotImplementedError()

    def _fft_padded_workspace(self, grid, box_lo, box_dims, batch, layout=0):
        return 0

    def sum_columns(self, y, X, alpha=1, beta=0, interleaved=False):
        """y = beta*y + alpha * sum_j X[:, j]  (interleaved: X's memory holds element (i, j) at i*ncols + j)"""
        raise NotImplementedError()

    def permute3(self, y, x, dims, perm, alpha=1, beta=0):
        """y[:, j] = beta*y[:, j] + alpha * permute(x[:, j]) for every column j: a column is an F-ordered `dims` volume, output axis
        a is input axis perm[a] (numpy transpose(perm) in F order).  beta == 0: y is not read.  This host form goes through
        to_host / copy_from, so that every backend has it; device backends override it."""
        dims, perm = tuple(int(n) for n in dims), tuple(int(p) for p in perm)
        assert len(dims) == 3 and sorted(perm) == [0, 1, 2], (dims, perm)
        n = int(np.prod(dims))
        assert x.size % n == 0 and x.size == y.size, (x.shape, y.shape, dims)
        ncols = x.size // n
        xh = x.to_host().reshape(dims + (ncols,), order='F')
        out = np.asfortranarray(xh.transpose(perm + (3,))).reshape((n, ncols), order='F')
        out = (out * np.complex64(alpha)).astype(_C64) if alpha != 1 else out.astype(_C64)
        if beta != 0:
            out = (y.to_host().reshape((n, ncols), order='F') * np.complex64(beta) + out).astype(_C64)
        y.copy_from(np.asfortranarray(out.reshape(y.shape, order='F')))

    def dwt3(self, y, x, dims, wavelet, levels, inverse=False, alpha=1, beta=0):
        """y[:, j] = beta*y[:, j] + alpha * W x[:, j] (inverse: W^H = W^-1) for every column j, W the orthonormal periodic wavelet
        transform of an F-ordered `dims` volume (`dwt_plan`; filters `WAVELETS`).  y may be x when beta == 0; beta == 0: y is not
        read.  This host form computes in float64 through to_host / copy_from, so that every backend has it; device backends
        override it."""
        dims = tuple(int(n) for n in dims)
        n = int(np.prod(dims))
        assert x.size % n == 0 and x.size == y.size, (x.shape, y.shape, dims)
        ncols = x.size // n
        passes, _ = dwt_plan(dims, wavelet, levels)
        v = x.to_host().reshape(dims + (ncols,), order='F').astype(np.complex128)
        for box, a in (reversed(passes) if inverse else passes):
            sl = tuple(slice(0, c) for c in box)
            u = np.moveaxis(v[sl], a, 0)
            v[sl] = np.moveaxis(_dwt_split(u, WAVELETS[wavelet], inverse), 0, a)
        out = v.reshape((n, ncols), order='F') * complex(alpha)
        if beta != 0:
            out = out + complex(beta) * y.to_host().reshape((n, ncols), order='F')
        y.copy_from(np.asfortranarray(out.astype(_C64).reshape(y.shape, order='F')))

    def soft_threshold(self, x, tau, dims, keep):
        """x <- x * max(0, 1 - tau / |x|) in place, column by column, for every element of the F-ordered `dims` volume outside the
        box [0, keep[0]) x [0, keep[1]) x [0, keep[2]) (the wavelet transform's coarse band, `dwt_coarse_box`), which is left
        untouched.  |x| <= tau gives exactly 0.  Host form through to_host / copy_from; device backends override it."""
        dims = tuple(int(n) for n in dims)
        n = int(np.prod(dims))
        assert x.size % n == 0 and tau >= 0, (x.shape, dims, tau)
        v = x.to_host().reshape(dims + (-1,), order='F')
        out = v.astype(np.complex128)
        r2 = out.real ** 2 + out.imag ** 2
        with np.errstate(divide='ignore', invalid='ignore'):
            f = np.where(r2 <= float(tau) ** 2, 0.0, 1.0 - float(tau) / np.sqrt(r2))
        inside = np.zeros(dims, dtype=bool)
        inside[tuple(slice(0, int(c)) for c in keep)] = True
        out = np.where(inside[..., None], v, (out * f).astype(_C64))
        x.copy_from(np.asfortranarray(out.astype(_C64).reshape(x.shape, order='F')))

    def grad3(self, y, x, dims, adjoint=False, alpha=1, beta=0):
        """y[:, j] = beta*y[:, j] + alpha * D x[:, j] (adjoint: D^H x[:, j]) for every column j.  D is the forward difference of an
        F-ordered `dims` volume of N voxels along its three axes, zero at the far face: (D_a x)[i] = x[i + e_a] - x[i] where
        i_a < n_a - 1, component a in rows [aN, (a+1)N) of a 3N-row column.  beta == 0: y is not read; y must not
        overlap x.  This host form computes in float64 through to_host / copy_from, so that every backend has it; device
        backends override it."""
        dims = tuple(int(n) for n in dims)
        n = int(np.prod(dims))
        rows_x, rows_y = (3 * n, n) if adjoint else (n, 3 * n)
        assert x.size % rows_x == 0 and x.size // rows_x * rows_y == y.size, (x.shape, y.shape, dims)
        self._grad_host(y, x, dims, 3, x.size // rows_x, adjoint, alpha, beta)

    def _grad_host(self, y, x, dims, comps, ncols, adjoint, alpha, beta):
        """`grad3` (comps = 3) and `grad4` (comps = 4: the ncols columns are the frames) in float64"""
        rows_y = y.size // ncols
        if adjoint:
            out = _grad_adjoint(x.to_host().reshape(dims + (comps, ncols), order='F').astype(np.complex128))
        else:
            out = _grad_forward(x.to_host().reshape(dims + (ncols,), order='F').astype(np.complex128), comps)
        out = out.reshape((rows_y, ncols), order='F') * complex(alpha)
        if beta != 0:
            out = out + complex(beta) * y.to_host().reshape((rows_y, ncols), order='F')
        y.copy_from(np.asfortranarray(out.astype(_C64).reshape(y.shape, order='F')))

    def tv_dual_step(self, u, xn, xo, sigma, mu, dims):
        """u <- proj_mu(u + sigma * D(2*xn - xo)) in place, column by column: the dual step of isotropic total variation.  proj_mu
        scales the three components of u at a voxel by (r <= mu ? 1 : mu / r), r = sqrt(sum_a |u_a[i]|^2).  Host form in float64
        through to_host / copy_from; device backends override it."""
        dims = tuple(int(n) for n in dims)
        n = int(np.prod(dims))
        assert xn.size % n == 0 and xn.size == xo.size and u.size == 3 * xn.size and mu >= 0, (u.shape, xn.shape, xo.shape, dims, mu)
        self._tv_dual_host(u, xn, xo, sigma, (mu,), dims, xn.size // n)

    def _tv_dual_host(self, u, xn, xo, sigma, radii, dims, ncols):
        """`tv_dual_step` (radii = (mu,)) and `tv4_dual_step` (radii = (mu, mu_t): the ncols columns are the frames) in float64"""
        comps = 2 + len(radii)
        w = 2.0 * xn.to_host().astype(np.complex128) - xo.to_host().astype(np.complex128)
        g = float(sigma) * _grad_forward(w.reshape(dims + (ncols,), order='F'), comps)
        t = u.to_host().reshape(dims + (comps, ncols), order='F').astype(np.complex128)
        t[:, :, :, :3] += g[:, :, :, :3]
        r = np.sqrt((t.real ** 2 + t.imag ** 2)[:, :, :, :3].sum(axis=3, keepdims=True))
        with np.errstate(divide='ignore', invalid='ignore'):
            t[:, :, :, :3] *= np.where(r <= float(radii[0]), 1.0, float(radii[0]) / r)
            if comps == 4:
                t[:, :, :, 3, :-1] += g[:, :, :, 3, :-1]
                rt = np.abs(t[:, :, :, 3])
                t[:, :, :, 3] *= np.where(rt <= float(radii[1]), 1.0, float(radii[1]) / rt)
        u.copy_from(np.asfortranarray(t.astype(_C64).reshape(u.shape, order='F')))

    def grad4(self, y, x, dims, frames, adjoint=False, alpha=1, beta=0):
        """y = beta*y + alpha * D4 x (adjoint: D4^H x) for T = `frames` time frames of an F-ordered `dims` volume of N voxels.  x is
        the N x T panel of the frames, or the same as an (N T, 1) vector, frame t in rows [tN, (t+1)N); D4 x is 4N x T, or
        (4N T, 1): components 0..2 of frame t are D x_t as in `grad3`, component 3 (rows [3N, 4N) of the frame's 4N) is
        x_{t+1} - x_t for t < T - 1 and 0 in the last frame.  (D4^H u)_t = D^H u_{0..2, t} + (t > 0 ? u_{3, t-1} : 0) -
        (t < T - 1 ? u_{3, t} : 0): u_3 of the last frame is not read.  beta == 0: y is not read; y must not
        overlap x.  Host form in float64 through to_host / copy_from; device backends override it."""
        dims = tuple(int(n) for n in dims)
        n, T = int(np.prod(dims)), int(frames)
        rows_x, rows_y = (4 * n, n) if adjoint else (n, 4 * n)
        assert T >= 1 and x.size == rows_x * T and y.size == rows_y * T, (x.shape, y.shape, dims, frames)
        self._grad_host(y, x, dims, 4, T, adjoint, alpha, beta)

    def tv4_dual_step(self, u, xn, xo, sigma, mu, mu_t, dims, frames):
        """u <- proj(u + sigma * D4(2*xn - xo)) in place: the dual step of spatial plus temporal total variation on `frames` time
        frames (layouts as in `grad4`).  Per voxel and frame the three spatial components are scaled onto the 2-norm ball of
        radius mu, as `tv_dual_step` does, and the temporal component onto the disc |u_3| <= mu_t, a constraint of its own.
        Host form in float64 through to_host / copy_from; device backends override it."""
        dims = tuple(int(n) for n in dims)
        n, T = int(np.prod(dims)), int(frames)
        assert T >= 1 and xn.size == n * T and xo.size == n * T and u.size == 4 * n * T and mu >= 0 and mu_t >= 0, \
            (u.shape, xn.shape, xo.shape, dims, frames, mu, mu_t)
        self._tv_dual_host(u, xn, xo, sigma, (mu, mu_t), dims, T)

    def symgrad3(self, y, v, dims, adjoint=False, alpha=1, beta=0):
        """y[:, j] = beta*y[:, j] + alpha * E v[:, j] (adjoint: E^H v[:, j]) for every column j.  E is the symmetrised backward
        difference of a 3-component field on an F-ordered `dims` volume of N voxels (component a in rows [aN, (a+1)N) of a 3N-row
        column): with B_a = -D_a^H, (B_a w)[i] = (i_a < n_a - 1 ? w[i] : 0) - (i_a > 0 ? w[i - e_a] : 0), the six components xx,
        yy, zz, xy, xz, yz (component c in rows [cN, (c+1)N) of a 6N-row column) are (E v)_aa = B_a v_a and (E v)_ab = (B_b v_a +
        B_a v_b) / sqrt(2), so that their 2-norm is the Frobenius norm of the symmetric tensor.  beta == 0: y is
        not read; y must not overlap v.  This host form computes in float64 through to_host / copy_from, so that every backend
        has it; device backends override it."""
        dims = tuple(int(n) for n in dims)
        n = int(np.prod(dims))
        comps_v, comps_y = (6, 3) if adjoint else (3, 6)
        assert v.size % (comps_v * n) == 0 and v.size // comps_v * comps_y == y.size, (v.shape, y.shape, dims)
        ncols = v.size // (comps_v * n)
        t = v.to_host().reshape(dims + (comps_v, ncols), order='F').astype(np.complex128)
        out = (_symgrad_adjoint(t) if adjoint else _symgrad_forward(t)).reshape((comps_y * n, ncols), order='F') * complex(alpha)
        if beta != 0:
            out = out + complex(beta) * y.to_host().reshape((comps_y * n, ncols), order='F')
        y.copy_from(np.asfortranarray(out.astype(_C64).reshape(y.shape, order='F')))

    def tgv_adjoint(self, gx, gv, p, q, dims):
        """K^H (p; q) of K (x; v) = (D x - v; E v), column by column: gx += D^H p (gx: N rows per column, read and written) and
        gv = E^H q - p (gv: 3N rows, written and not read); p has 3N rows, q 6N (`grad3`, `symgrad3`).  Host form in float64
        through to_host / copy_from; device backends override it."""
        dims = tuple(int(n) for n in dims)
        n = int(np.prod(dims))
        assert gx.size % n == 0 and gv.size == 3 * gx.size and p.size == 3 * gx.size and q.size == 6 * gx.size, \
            (gx.shape, gv.shape, p.shape, q.shape, dims)
        ncols = gx.size // n
        ph = p.to_host().reshape(dims + (3, ncols), order='F').astype(np.complex128)
        qh = q.to_host().reshape(dims + (6, ncols), order='F').astype(np.complex128)
        out_x = gx.to_host().reshape((n, ncols), order='F') + _grad_adjoint(ph).reshape((n, ncols), order='F')
        out_v = _symgrad_adjoint(qh) - ph
        gx.copy_from(np.asfortranarray(out_x.astype(_C64).reshape(gx.shape, order='F')))
        gv.copy_from(np.asfortranarray(out_v.astype(_C64).reshape(gv.shape, order='F')))

    def tgv_dual_step(self, p, q, xn, xo, vn, vo, sigma, a1, a0, dims):
        """The dual step of second-order total generalized variation in place on p and q, column by column, with w_x = 2*xn - xo
        and w_v = 2*vn - vo:  p <- proj_{a1}(p + sigma (D w_x - w_v)),  q <- proj_{a0}(q + sigma E w_v).  proj_r scales the
        components at a voxel (three of p, six of q) by (norm <= r ? 1 : r / norm), norm their 2-norm.  Host form in float64
        through to_host / copy_from; device backends override it."""
        dims = tuple(int(n) for n in dims)
        n = int(np.prod(dims))
        assert xn.size % n == 0 and xo.size == xn.size and vn.size == 3 * xn.size and vo.size == vn.size and p.size == vn.size \
            and q.size == 6 * xn.size and a1 >= 0 and a0 >= 0, (p.shape, q.shape, xn.shape, xo.shape, vn.shape, vo.shape, dims, a1, a0)
        ncols = xn.size // n
        wx = (2.0 * xn.to_host().astype(np.complex128) - xo.to_host().astype(np.complex128)).reshape(dims + (ncols,), order='F')
        wv = (2.0 * vn.to_host().astype(np.complex128) - vo.to_host().astype(np.complex128)).reshape(dims + (3, ncols), order='F')
        tp = p.to_host().reshape(dims + (3, ncols), order='F').astype(np.complex128) + float(sigma) * (_grad_forward(wx) - wv)
        tq = q.to_host().reshape(dims + (6, ncols), order='F').astype(np.complex128) + float(sigma) * _symgrad_forward(wv)
        p.copy_from(np.asfortranarray(_ball(tp, a1).astype(_C64).reshape(p.shape, order='F')))
        q.copy_from(np.asfortranarray(_ball(tq, a0).astype(_C64).reshape(q.shape, order='F')))

    @staticmethod
    def _llr_block_ids(dims, block, shift):
        """(block number of every voxel as an F-ordered (N,) array, nb, the clamped block) of the locally low-rank partition:
        voxel i has the shifted coordinates j_a = (i_a + s_a) mod n_a and belongs to block (j_0 // b_0, j_1 // b_1, j_2 // b_2),
        the blocks numbered F-order"""
        dims = tuple(int(n) for n in dims)
        block = tuple(min(int(b), n) for b, n in zip(block, dims))
        shift = tuple(int(s) for s in shift)
        assert len(dims) == 3 and all(b >= 1 for b in block) and all(0 <= s < b for s, b in zip(shift, block)), (dims, block, shift)
        nbs = [-(-n // b) for n, b in zip(dims, block)]
        per_axis = [((np.arange(n) + s) % n) // b for n, b, s in zip(dims, block, shift)]
        ids = per_axis[0][:, None, None] + nbs[0] * (per_axis[1][None, :, None] + nbs[1] * per_axis[2][None, None, :])
        return ids.reshape(-1, order='F'), int(np.prod(nbs)), block

    def llr_threshold(self, x, tau, dims, frames, block, shift=(0, 0, 0)):
        """Block-wise singular-value thresholding in place: the proximal map of tau * sum_b ||M_b(x)||_*, the locally low-rank
        penalty.  x is the N x T panel of T = `frames` time frames of an F-ordered `dims` volume, or the same
        as an (N T, 1) vector.  `block` sides are clamped to `dims`, 0 <= shift_a < block_a; the blocks tile the volume shifted
        by `shift` (`_llr_block_ids`), M_b is the (voxels of block b) x T matrix of x, and M_b <- U max(S - tau, 0) V^H.
        Host form in float64 through to_host / copy_from; device backends override it."""
        n, T = int(np.prod(dims)), int(frames)
        assert T >= 1 and x.size == n * T and tau >= 0, (x.shape, dims, frames, tau)
        ids, nb, _ = self._llr_block_ids(dims, block, shift)
        v = x.to_host().reshape((n, T), order='F').astype(np.complex128)
        order = np.argsort(ids, kind='stable')
        bounds = np.searchsorted(ids[order], np.arange(nb + 1))
        for b in range(nb):
            rows = order[bounds[b]:bounds[b + 1]]
            U, S, Vh = np.linalg.svd(v[rows], full_matrices=False)
            v[rows] = (U * np.maximum(S - float(tau), 0.0)) @ Vh
        x.copy_from(np.asfortranarray(v.astype(_C64).reshape(x.shape, order='F')))

    def llr_norm(self, x, dims, frames, block, shift=(0, 0, 0)):
        """sum_b ||M_b(x)||_*, the sum of the singular values of every block's matrix (layouts and blocks as in `llr_threshold`),
        as a float.  Host form in float64; device backends override it."""
        n, T = int(np.prod(dims)), int(frames)
        assert T >= 1 and x.size == n * T, (x.shape, dims, frames)
        ids, nb, _ = self._llr_block_ids(dims, block, shift)
        v = x.to_host().reshape((n, T), order='F').astype(np.complex128)
        order = np.argsort(ids, kind='stable')
        bounds = np.searchsorted(ids[order], np.arange(nb + 1))
        return float(sum(np.linalg.svd(v[order[bounds[b]:bounds[b + 1]]], compute_uv=False).sum() for b in range(nb)))

    def frame_basis(self, y, x, phi, n, adjoint=False, alpha=1, beta=0):
        """y = beta*y + alpha * (Phi (x) I_n) x (adjoint: (Phi^H (x) I_n) x), the temporal-subspace operator between K coefficient
        images and T time frames of `n` voxels.  phi is the T x K basis as a backend array.  Forward, x is the
        n x K panel of the coefficient images, or the same as an (n K, 1) vector, image k in rows [kn, (k+1)n), and y the n x T
        panel of the frames, or (n T, 1):  y[i, t] = sum_k phi[t, k] x[i, k].  Adjoint, x holds the frames and y the images:
        y[i, k] = sum_t conj(phi[t, k]) x[i, t].  beta == 0: y is not read; y must not overlap x or phi.  Host form in float64
        through to_host / copy_from; device backends override it."""
        n = int(n)
        p = phi.to_host().astype(np.complex128)
        assert p.ndim == 2, p.shape
        T, K = p.shape
        cols_x, cols_y = (T, K) if adjoint else (K, T)
        assert n >= 1 and x.size == n * cols_x and y.size == n * cols_y, (x.shape, y.shape, p.shape, n)
        v = x.to_host().reshape((n, cols_x), order='F').astype(np.complex128)
        out = (v @ p.conj() if adjoint else v @ p.T) * complex(alpha)
        if beta != 0:
            out = out + complex(beta) * y.to_host().reshape((n, cols_y), order='F')
        y.copy_from(np.asfortranarray(out.astype(_C64).reshape(y.shape, order='F')))

    def segment_phase(self, y, x, f, tau0, dtau, L, n, adjoint=False, alpha=1, beta=0):
        """y = beta*y + alpha * Phase x (adjoint: Phase^H x), the voxel side of the time-segmented off-resonance model (DESIGN.md
        §3.15): f is a backend array of `n` float32 values of the field map in Hz, tau_l = tau0 + l dtau in seconds, l < L <= 16.
        Forward, x is the image of n voxels and y the n x L panel of its segments, or the same as an (n L, 1) vector, segment l in
        rows [ln, (l+1)n):  y[i, l] = exp(-2 pi i f[i] tau_l) x[i].  Adjoint, x holds the segments and y the image:
        y[i] = sum_l exp(+2 pi i f[i] tau_l) x[i, l].  The field map is what its float32 values say; the phase is formed in
        float64.  beta == 0: y is not read; y must not overlap x or f.  Host form in float64 through to_host / copy_from; device
        backends override it."""
        n, L = int(n), int(L)
        if not 1 <= L <= 16:
            raise RuntimeError("segment_phase: %d segments, between 1 and 16 are supported" % L)
        cols_x, cols_y = (L, 1) if adjoint else (1, L)
        assert n >= 1 and f.size == n and x.size == n * cols_x and y.size == n * cols_y, (x.shape, y.shape, f.shape, n, L)
        taus = float(tau0) + np.arange(L, dtype=np.float64) * float(dtau)
        ph = np.exp(-2j * np.pi * np.outer(f.to_host().reshape(-1).astype(np.float64), taus))
        v = x.to_host().reshape((n, cols_x), order='F').astype(np.complex128)
        out = ((ph.conj() * v).sum(axis=1, keepdims=True) if adjoint else ph * v) * complex(alpha)
        if beta != 0:
            out = out + complex(beta) * y.to_host().reshape((n, cols_y), order='F')
        y.copy_from(np.asfortranarray(out.astype(_C64).reshape(y.shape, order='F')))

    def segment_combine(self, y, x, b, period, n, adjoint=False, alpha=1, beta=0):
        """y = beta*y + alpha * Combine x (adjoint: Combine^H x), the sample side of the time-segmented off-resonance model
        (DESIGN.md §3.15): b is the P x L interpolator table as a backend array, P = `period`, L <= 16; row r of the `n` rows uses
        row r mod P of the table and n is a multiple of P.  Forward, x is the n x L panel of the segments' samples, or the same as
        an (n L, 1) vector, and y the n samples:  y[r] = sum_l b[r mod P, l] x[r, l].  Adjoint, x holds the samples and y the
        panel:  y[r, l] = conj(b[r mod P, l]) x[r].  beta == 0: y is not read; y must not overlap x or b.  Host form in float64
        through to_host / copy_from; device backends override it."""
        n, P = int(n), int(period)
        t = b.to_host().astype(np.complex128)
        assert t.ndim == 2 and t.shape[0] == P, (t.shape, P)
        L = t.shape[1]
        if not 1 <= L <= 16:
            raise RuntimeError("segment_combine: %d segments, between 1 and 16 are supported" % L)
        if P < 1 or n % P:
            raise RuntimeError("segment_combine: %d rows are no multiple of the table's period %d" % (n, P))
        cols_x, cols_y = (1, L) if adjoint else (L, 1)
        assert n >= 1 and x.size == n * cols_x and y.size == n * cols_y, (x.shape, y.shape, t.shape, n)
        t = np.tile(t, (n // P, 1))
        v = x.to_host().reshape((n, cols_x), order='F').astype(np.complex128)
        out = (t.conj() * v if adjoint else (t * v).sum(axis=1, keepdims=True)) * complex(alpha)
        if beta != 0:
            out = out + complex(beta) * y.to_host().reshape((n, cols_y), order='F')
        y.copy_from(np.asfortranarray(out.astype(_C64).reshape(y.shape, order='F')))

    @staticmethod
    def _share_memory(a, b):
        """whether two backend arrays share a byte: host arrays by numpy's bounds, device arrays by their address ranges"""
        if isinstance(a._arr, np.ndarray):
            return bool(np.may_share_memory(a._arr, b._arr))

        def span(v):
            cols = v.shape[1] if v.ndim == 2 else 1
            return int(v._arr), int(v._arr) + ((cols - 1) * v._leading_dim + v.shape[0]) * v.itemsize
        (a0, a1), (b0, b1) = span(a), span(b)
        return a0 < b1 and b0 < a1

    def fieldmap_check(self, what, dims, y, te, fields, beta=0.0):
        """The refusals that fieldmap_init and fieldmap_step share, every one a ValueError: returns (dims, N, E, te as float64,
        beta as what its float32 value says)."""
        dims = tuple(int(n) for n in dims)
        te = np.ascontiguousarray(np.asarray(te, dtype=np.float64).reshape(-1))
        E = te.size
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError("%s: dims %r are not three positive lengths" % (what, dims))
        n = int(np.prod(dims))
        if not 2 <= E <= 8:
            raise ValueError("%s: %d echo times, between 2 and 8 echoes are supported" % (what, E))
        if not (np.isfinite(te).all() and (np.diff(te) > 0).all()):
            raise ValueError("%s: the echo times %r are not strictly increasing" % (what, te.tolist()))
        if y.dtype != _C64 or y.size != n * E:
            raise ValueError("%s: the panel %r of %s is not N x E = %d x %d complex64" % (what, y.shape, y.dtype, n, E))
        for f in fields:
            if f.dtype != np.dtype('float32') or f.size != n or not f.contiguous:
                raise ValueError("%s: a field %r of %s is not N = %d contiguous float32 values" % (what, f.shape, f.dtype, n))
            if self._share_memory(f, y):
                raise ValueError("%s: a field overlaps the panel" % what)
        if len(fields) == 2 and self._share_memory(fields[0], fields[1]):
            raise ValueError("%s: f_new overlaps f_old" % what)
        beta = float(beta)
        if not (np.isfinite(beta) and beta >= 0):
            raise ValueError("%s: beta %r is negative or not finite" % (what, beta))
        return dims, n, E, te, float(np.float32(beta))

    def fieldmap_init(self, f, y, dims, te):
        """f[j] = -angle(y_1 conj(y_0))[j] / (2 pi (te[1] - te[0])), the two-echo phase-difference estimate in Hz that the
        regularised fit starts from.  y is the N x E complex64 panel of the echo images on the F-ordered `dims`
        volume, or the same as an (N E, 1) vector, y_l ~ m exp(-2 pi i f te_l) as in pics --fmap; f a backend array of N float32
        values.  No unwrapping is done: the true field has to satisfy |f| < 1 / (2 (te[1] - te[0])).  Refuses with a ValueError:
        E outside 2..8, echo times not strictly increasing, a panel whose size is not N E.  Host form in float64 through to_host /
        copy_from; device backends override it."""
        dims, n, E, te, _ = self.fieldmap_check("fieldmap_init", dims, y, te, (f,))
        yh = y.to_host().reshape((n, E), order='F').astype(np.complex128)
        f0 = -np.angle(yh[:, 1] * yh[:, 0].conj()) / (2.0 * np.pi * (te[1] - te[0]))
        f.copy_from(np.asfortranarray(f0.astype(np.float32).reshape(f.shape, order='F')))

    def fieldmap_step(self, f_new, f_old, y, te, beta, dims, cost=False):
        """One separable-quadratic-surrogate step of the penalised-likelihood field-map fit of Funai et al. (IEEE TMI 27:1484,
        2008), every voxel from the old iterate.  For the echo pairs l < m with p = y_m conj(y_l), w = |p|,
        k = 2 pi (te_m - te_l) and s the principal value of angle(p) + k f_old in [-pi, pi]:
            g_j = sum_pairs w k sin s + beta sum_{j' ~ j} (f_j - f_j'),    d_j = sum_pairs w k^2 sin(s) / s + 2 beta deg_j,
            f_new[j] = f_old[j] - g_j / d_j        (d_j = 0: unchanged)
        over the nearest neighbours j' along the three axes of the F-ordered `dims` volume, no wrap-around.  It decreases
            Psi(f) = sum_j sum_pairs w (1 - cos s) + beta / 2 sum_edges (f_j - f_j')^2
        monotonically; cost=True returns Psi(f_old), the cost of the INPUT iterate, as a float (else None).  beta is absolute and is
        what its float32 value says.  y as in `fieldmap_init`; f_new and f_old are backend arrays of N float32 values in Hz.  Refuses
        with a ValueError: E outside 2..8, echo times not strictly increasing, overlapping f_new / f_old, a panel whose size is
        not N E, beta < 0.  Host form in float64 through to_host / copy_from; device backends override it."""
        dims, n, E, te, beta = self.fieldmap_check("fieldmap_step", dims, y, te, (f_new, f_old), beta)
        out, psi = self._fieldmap_host(f_old, y, te, beta, dims, n, E)
        f_new.copy_from(np.asfortranarray(out.astype(np.float32).reshape(f_new.shape, order='F')))
        return psi if cost else None

    def fieldmap_cost(self, f, y, te, beta, dims):
        """Psi(f) of `fieldmap_step` as a float, f untouched: what a step with cost=True returns, without the step.  The same
        refusals.  Host form in float64; device backends override it."""
        dims, n, E, te, beta = self.fieldmap_check("fieldmap_cost", dims, y, te, (f,), beta)
        return self._fieldmap_host(f, y, te, beta, dims, n, E)[1]

    @staticmethod
    def _fieldmap_host(f_old, y, te, beta, dims, n, E):
        """(the stepped field as a float64 `dims` array, Psi(f_old)) of the checked arguments of `fieldmap_step`"""
        yh = y.to_host().reshape((n, E), order='F').astype(np.complex128)
        f = f_old.to_host().reshape(dims, order='F').astype(np.float64)
        g, d, psi = np.zeros(dims), np.zeros(dims), 0.0
        for l in range(E):
            for m in range(l + 1, E):
                p = (yh[:, m] * yh[:, l].conj()).reshape(dims, order='F')
                k = 2.0 * np.pi * (te[m] - te[l])
                r = p * np.exp(1j * k * f)
                w, s = np.abs(p), np.angle(r)
                with np.errstate(divide='ignore', invalid='ignore'):
                    g += k * r.imag
                    d += k * k * np.where(s != 0, r.imag / s, w)
                psi += float((w - r.real).sum())
        for a in range(3):
            df = -_fwd_diff(f, a)                             # f_j - f_j' towards the far neighbour, 0 on the far face
            g += beta * df
            g -= beta * np.roll(df, 1, axis=a)                # (df is 0 on the far face, so nothing wraps)
            deg = np.full(dims[a], 2.0 if dims[a] > 1 else 0.0)
            if dims[a] > 1:
                deg[0] = deg[-1] = 1.0
            d += 2.0 * beta * deg.reshape([-1 if b == a else 1 for b in range(3)])
            psi += 0.5 * beta * float((df ** 2).sum())
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(d > 0, f - g / d, f), psi

    def coil_maps(self, y, x, maps, n, ncoils, nmaps, adjoint=False, alpha=1, beta=0, interleaved=False, width=None):
        """y = beta*y + alpha * S x (adjoint: S^H x), the per-voxel coil-map product of soft-SENSE between M = `nmaps` images and
        C = `ncoils` coil images of `n` voxels:  forward y[i, c] = sum_m S[i, c, m] x[i, m], adjoint
        y[i, m] = sum_c conj(S[i, c, m]) x[i, c].  The images are an n x M panel, or the same as an (n M, 1) vector, image m in rows
        [mn, (m+1)n).  The coil images are an n x C panel or the (n C, 1) vector (element (i, c) at i + n c), or, `interleaved`, one
        contiguous array whose memory holds the `width` >= C coil slots of a voxel side by side (element (i, c) at i width + c; width
        2, 4, 8 or 16): slots c >= C are zero-weight padding coils, written as zero on forward and never read on adjoint.  maps is a
        backend array of M dense planes in the form of the coil images (n C elements each, or n width).  beta == 0: y is not read; y
        must not overlap x or maps; M <= 4.  Host form in float64 through to_host / copy_from; device backends override it."""
        n, C, M = int(n), int(ncoils), int(nmaps)
        if not 1 <= M <= 4:
            raise RuntimeError("coil_maps: %d sets of maps, between 1 and 4 are supported" % M)
        w = int(width) if (interleaved and width is not None) else C
        if interleaved and (w not in (2, 4, 8, 16) or C > w):
            raise RuntimeError("coil_maps: %d coils in interleaved rows of width %d (2, 4, 8 or 16, at least the coils)" % (C, w))
        assert n >= 1 and C >= 1 and maps.size == n * w * M, (maps.shape, n, w, M)
        img, coil = (y, x) if adjoint else (x, y)
        assert img.size == n * M and coil.size == n * w, (x.shape, y.shape, n, w, M)
        cshape = (w, n) if interleaved else (n, w)
        S = maps.to_host().reshape(cshape + (M,), order='F').astype(np.complex128)
        S = (S.transpose(1, 0, 2) if interleaved else S)[:, :C]                       # (n, C, M)
        v = x.to_host().reshape(cshape if adjoint else (n, M), order='F').astype(np.complex128)
        if adjoint:
            v = (v.T if interleaved else v)[:, :C]
            out = np.einsum('icm,ic->im', S.conj(), v) * complex(alpha)
            if beta != 0:
                out = out + complex(beta) * y.to_host().reshape((n, M), order='F')
        else:
            prod = np.einsum('icm,im->ic', S, v) * complex(alpha)
            if beta != 0:
                old = y.to_host().reshape(cshape, order='F')
                prod = prod + complex(beta) * (old.T if interleaved else old)[:, :C]
            out = np.zeros((n, w), dtype=np.complex128)
            out[:, :C] = prod
            out = out.T if interleaved else out
        y.copy_from(np.asfortranarray(out.astype(_C64).reshape(y.shape, order='F')))

    def nlinv_product(self, y, x, rho, coils, n, ncoils, adjoint=False, alpha=1, beta=0):
        """y = beta*y + alpha * P x (adjoint: P^H x), the derivative of the bilinear coil product rho * c_c of NLINV at the point
        (rho, coils) (indigo_amd.nlinv).  rho is a backend array of `n` values, coils the n x C panel of the coil
        sensitivities (or the same as an (n C, 1) vector).  Forward, x is the n x (1 + C) panel (d rho | d c_1 ... d c_C), or the same
        as an (n (1 + C), 1) vector, and y the n x C panel of coil images:  y[i, c] = x[i, 0] coils[i, c] + rho[i] x[i, 1 + c].
        Adjoint, x holds the coil images and y the panel:  y[i, 0] = sum_c conj(coils[i, c]) x[i, c],
        y[i, 1 + c] = conj(rho[i]) x[i, c].  beta == 0: y is not read; y must not overlap x, rho or coils.  Host form in float64
        through to_host / copy_from; device backends override it."""
        n, C = int(n), int(ncoils)
        if C < 1 or n < 1:
            raise RuntimeError("nlinv_product: %d voxels and %d coils, at least 1 each is supported" % (n, C))
        cols_x, cols_y = (C, 1 + C) if adjoint else (1 + C, C)
        assert rho.size == n and coils.size == n * C and x.size == n * cols_x and y.size == n * cols_y, (rho.shape, coils.shape, x.shape, y.shape, n, C)
        r = rho.to_host().reshape(n).astype(np.complex128)
        c = coils.to_host().reshape((n, C), order='F').astype(np.complex128)
        v = x.to_host().reshape((n, cols_x), order='F').astype(np.complex128)
        if adjoint:
            out = np.concatenate([(np.conj(c) * v).sum(axis=1, keepdims=True), np.conj(r)[:, None] * v], axis=1)
        else:
            out = v[:, :1] * c + r[:, None] * v[:, 1:]
        out = out * complex(alpha)
        if beta != 0:
            out = out + complex(beta) * y.to_host().reshape((n, cols_y), order='F').astype(np.complex128)
        y.copy_from(np.asfortranarray(out.astype(_C64).reshape(y.shape, order='F')))

    @staticmethod
    def sobolev_weights(dims, a, b):
        """w(k) = (1 + a |kappa|^2)^(-b/2) on the points of an uncentred transform of a `dims` volume, float64 dims-shaped:
        kappa_a = k'_a / n_a with k'_a = k_a if 2 k_a <= n_a else k_a - n_a"""
        r2 = 0.0
        for ax, n in enumerate(dims):
            k = np.arange(n, dtype=np.int64)
            f = np.where(2 * k <= n, k, k - n).astype(np.float64) / float(n)
            r2 = r2 + (f * f).reshape([-1 if j == ax else 1 for j in range(len(dims))])
        return (1.0 + float(a) * r2) ** (-0.5 * float(b))

    def sobolev_weight(self, y, x, dims, ncols, a, b, scale=1.0):
        """y[k, j] = scale * w(k) * x[k, j] for the `ncols` columns of a panel of F-ordered `dims` k-space volumes (or the same as
        one stacked column), w the smoothness weight of NLINV's coil penalty (`sobolev_weights`): w is rounded to float32 once and
        scale * w once more, as the device kernel does.  y may be x (exactly in place); any other overlap is refused.  Host form
        through to_host / copy_from; device backends override it."""
        dims = tuple(int(n) for n in dims)
        n, ncols = int(np.prod(dims)), int(ncols)
        if len(dims) != 3 or min(dims) < 1 or ncols < 1 or not float(a) >= 0:
            raise RuntimeError("sobolev_weight: dims %s, %d columns, a = %g: three positive lengths, at least one column and a >= 0" % (dims, ncols, a))
        assert x.size == n * ncols and y.size == n * ncols, (x.shape, y.shape, dims, ncols)
        w = self.sobolev_weights(dims, a, b).reshape(-1, order='F').astype(np.float32)
        sw = (w.astype(np.float64) * float(scale)).astype(np.float32)
        v = x.to_host().reshape((n, ncols), order='F')
        out = np.empty((n, ncols), dtype=_C64, order='F')
        out.real = sw[:, None] * v.real
        out.imag = sw[:, None] * v.imag
        y.copy_from(np.asfortranarray(out.reshape(y.shape, order='F')))

    def place_wrapped(self, vol, box, dims, box_dims):
        """Zero the columns of the panel `vol` (volumes of `dims`, F-order, one per column) and write column j of `box` (a dense array
        of boxes of `box_dims`, F-order) into column j with the box's centre element b // 2 of every axis at index 0 and its negative
        half wrapped to the top of the axis: box element j_a goes to (j_a - b_a // 2) mod n_a.  The input of the inverse transforms
        that evaluate the ESPIRiT matrices G(x) (indigo_amd.ecalib).  Values are copied: bit-exact.  Rows between
        the columns of a padded vol are not touched.  1 <= b_a <= n_a.  Host form through to_host / copy_from; device backends
        override it."""
        dims, box_dims = tuple(int(n) for n in dims), tuple(int(b) for b in box_dims)
        N, nb = int(np.prod(dims)), int(np.prod(box_dims))
        if not all(1 <= b <= n for b, n in zip(box_dims, dims)):
            raise RuntimeError("place_wrapped: a box of %s in a volume of %s: every side between 1 and the volume's" % (box_dims, dims))
        ncols = box.size // nb
        assert ncols >= 1 and box.size == nb * ncols and vol.size == N * ncols, (vol.shape, box.shape, dims, box_dims)
        b = box.to_host().reshape(box_dims + (ncols,), order='F')
        out = np.zeros(dims + (ncols,), dtype=b.dtype, order='F')
        idx = np.ix_(*[(np.arange(bb) - bb // 2) % n for bb, n in zip(box_dims, dims)])
        out[idx] = b
        vol.copy_from(np.asfortranarray(out.reshape(vol.shape, order='F')))

    @staticmethod
    def espirit_unpack(gram, n, C):
        """the (n, C, C) complex128 Hermitian matrices of an `espirit_eig` panel: column p C - p (p - 1) / 2 + (q - p) holds G[p, q],
        p <= q (the row-wise upper triangle); the imaginary part of the diagonal is ignored"""
        g = np.asarray(gram, dtype=np.complex128).reshape((n, C * (C + 1) // 2), order='F')
        G = np.zeros((n, C, C), dtype=np.complex128)
        col = 0
        for p in range(C):
            for q in range(p, C):
                if p == q:
                    G[:, p, p] = g[:, col].real
                else:
                    G[:, p, q] = g[:, col]
                    G[:, q, p] = np.conj(g[:, col])
                col += 1
        return G

    def espirit_eig(self, maps, evals, gram, n, ncoils, nmaps, iters=30, crop=0.8):
        """The M = `nmaps` leading eigenpairs of the Hermitian C x C matrix G at each of `n` voxels, as ESPIRiT maps (indigo_amd.ecalib,
        DESIGN.md §3.13).  gram is the n x C (C + 1) / 2 panel of the row-wise upper triangle of G (`espirit_unpack`).  maps is the
        n x (C M) panel, column c + C m coil c of set m -- contiguous, the M dense coil-major planes that `coil_maps` and
        operators.CoilMaps take --, evals the n x M float32 panel.  Eigenvalues descend with m; every vector has unit 2-norm over the
        coils and is rotated so that its coil-0 component is real and >= 0 (left unrotated where its coil-0 magnitude is below 1e-6);
        where eigenvalue m < crop the map values of set m are zero (evals keeps the eigenvalue).  `iters` bounds the iterations of an
        iterative method.  1 <= M <= min(4, C), C <= 32.  Host form: numpy.linalg.eigh in complex128 through to_host / copy_from
        (`iters` is not used); device backends override it."""
        n, C, M = int(n), int(ncoils), int(nmaps)
        if not 1 <= C <= 32:
            raise RuntimeError("espirit_eig: %d coils, between 1 and 32 are supported" % C)
        if not 1 <= M <= min(4, C):
            raise RuntimeError("espirit_eig: %d sets of maps from %d coils, between 1 and min(4, coils) are supported" % (M, C))
        assert n >= 1 and gram.size == n * C * (C + 1) // 2 and maps.size == n * C * M and evals.size == n * M, (gram.shape, maps.shape, evals.shape)
        G = self.espirit_unpack(gram.to_host(), n, C)
        lam, vec = np.linalg.eigh(G)
        lam, vec = lam[:, ::-1][:, :M], vec[:, :, ::-1][:, :, :M]                    # (n, M), (n, C, M), descending
        v0 = vec[:, 0, :]
        a0 = np.abs(v0)
        rot = np.where(a0 >= 1e-6, np.conj(v0) / np.where(a0 >= 1e-6, a0, 1), 1)
        vec = vec * rot[:, None, :]
        vec[:, 0, :] = np.where(a0 >= 1e-6, a0, v0)
        vec = np.where((lam < crop)[:, None, :], 0, vec)
        maps.copy_from(np.asfortranarray(vec.astype(_C64).reshape(maps.shape, order='F')))
        evals.copy_from(np.asfortranarray(lam.astype(np.float32).reshape(evals.shape, order='F')))

    def coil_gram(self, x, n, ncoils, slab=None):
        """G[p, q] = sum_i x[i, p] conj(x[i, q]) over the `n` samples of a coil panel, as a host (C, C) complex128 array: Hermitian,
        positive semi-definite, the matrix coil compression and noise prewhitening start from (indigo_amd.cc).  x is
        the n x C panel (coil c is column c, with its leading dimension) or the same as an (n C, 1) vector; it is not written, and
        rows between the columns of a padded panel are not read.  C <= 64.  `slab`: the samples per partial sum of a device backend
        (None: its default), without meaning here.  Host form in float64 through to_host -- real products of [Re x | Im x], as the
        device kernel forms them --; device backends override it."""
        n, C = int(n), int(ncoils)
        if not 1 <= C <= 64:
            raise RuntimeError("coil_gram: %d coils, between 1 and 64 are supported" % C)
        assert n >= 1 and x.size == n * C, (x.shape, n, C)
        v = x.to_host().reshape((n, C), order='F')
        re, im = v.real.astype(np.float64), v.imag.astype(np.float64)
        ri = im.T @ re
        G = (re.T @ re + im.T @ im) + 1j * (ri - ri.T)
        G[np.diag_indices(C)] = G[np.diag_indices(C)].real
        return G

    def coil_mix(self, y, x, A, n):
        """y[i, v] = sum_c A[v, c] x[i, c]: the host V x C matrix `A` applied along the coil axis of the n x C panel x, into the
        n x V panel y (panels with their leading dimensions, or stacked in one column): coil compression and prewhitening of data,
        maps and calibration blocks (indigo_amd.cc).  No kernel of its own: this is `frame_basis` with
        phi = A^H (C x V) and adjoint=True, y[i, v] = sum_c conj(phi[c, v]) x[i, c] -- ig_basis_c64 with nt = C, nk = V on the
        device, whose bound nk <= 32 is the bound on V.  y must not overlap x."""
        A = np.asarray(A)
        assert A.ndim == 2, A.shape
        V, C = A.shape
        if not 1 <= V <= 32:
            raise RuntimeError("coil_mix: %d virtual coils, between 1 and 32 are supported (frame_basis)" % V)
        phi = self.copy_array(np.asfortranarray(A.conj().T.astype(_C64)), name='cc.phi')
        self.frame_basis(y, x, phi, n, adjoint=True)

    def dict_match(self, x, atoms, n, chunk=1 << 16):
        """The atom of a dictionary that best explains each of `n` voxels' subspace coefficients (indigo_amd.dictmatch, DESIGN.md
        §3.16).  x is the n x K panel of the coefficient images (with its leading dimension), or the same as an (n K, 1) vector, as
        `frame_basis` takes it; atoms is the K x N dictionary as a backend array, atom a in column a, normalised by the caller.  With
        c = x[i, :] and s_a = |d_a^H c|^2, returns the host arrays (idx int32[n], ip complex64[n]): idx[i] the smallest a that attains
        max_a s_a, ip[i] = d_a^H c for that a; a zero voxel gives (0, 0).  Neither input is written.  K <= 32.  Host form in float64
        through to_host, `chunk` voxels at a time (a chunk x N matrix of scores); device backends override it."""
        n = int(n)
        assert atoms.ndim == 2, atoms.shape
        K, N = atoms.shape
        if not 1 <= K <= 32:
            raise RuntimeError("dict_match: %d coefficients, between 1 and 32 are supported" % K)
        assert n >= 1 and N >= 1 and x.size == n * K, (x.shape, atoms.shape, n)
        D = atoms.to_host().astype(np.complex128).conj()
        v = x.to_host().reshape((n, K), order='F')
        idx, ip = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=_C64)
        for i0 in range(0, n, max(1, int(chunk))):
            P = v[i0:i0 + chunk].astype(np.complex128) @ D
            best = np.argmax(P.real ** 2 + P.imag ** 2, axis=1)                # (the first of equal maxima: the lowest index)
            idx[i0:i0 + chunk] = best
            ip[i0:i0 + chunk] = P[np.arange(P.shape[0]), best]
        return idx, ip

    EPG_SHIFT_A, EPG_SHIFT_B, EPG_RECORD, EPG_SPOIL = 1, 2, 4, 8
    EPG_MAX_STATES, EPG_MAX_STEPS = 256, 65535

    @classmethod
    def epg_check(cls, params, steps, flags, nstates):
        """-> (params float32 (N, 3), steps float64 (S, 4), flags int32 (S,), nstates, nrec) of `epg_signal`, checked: every refusal
        is a ValueError that says what is wrong"""
        p = np.asarray(params)
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError("epg_signal: the parameters must be an (N, 3) array of (T1, T2, B1), got shape %s" % (p.shape,))
        if np.iscomplexobj(p) or not np.isfinite(p).all():
            raise ValueError("epg_signal: the parameters hold values that are not finite real numbers")
        p = np.ascontiguousarray(p, dtype=np.float32)
        if not (np.isfinite(p).all() and (p[:, :2] > 0).all()):
            raise ValueError("epg_signal: T1 and T2 must be positive (and finite in float32)")
        st = np.asarray(steps, dtype=np.float64)
        fl = np.asarray(flags)
        if st.ndim != 2 or st.shape[1] != 4 or not 1 <= st.shape[0] <= cls.EPG_MAX_STEPS:
            raise ValueError("epg_signal: the program must be an (S, 4) array of (flip, phase, a, b) with 1 <= S <= %d, got shape %s"
                             % (cls.EPG_MAX_STEPS, st.shape))
        if fl.shape != (st.shape[0],) or fl.dtype.kind not in 'iu':
            raise ValueError("epg_signal: the flags must be %d integers, one per step, got %s of shape %s" % (st.shape[0], fl.dtype, fl.shape))
        if ((fl < 0) | (fl > 15)).any():
            raise ValueError("epg_signal: flags must be in 0 ... 15 (1 SHIFT_A, 2 SHIFT_B, 4 RECORD, 8 SPOIL)")
        if not np.isfinite(st).all():
            raise ValueError("epg_signal: the program holds values that are not finite")
        if (st[:, 2:] < 0).any():
            raise ValueError("epg_signal: the program holds a negative duration")
        fl = np.ascontiguousarray(fl, dtype=np.int32)
        nrec = int(np.count_nonzero(fl & cls.EPG_RECORD))
        if nrec < 1:
            raise ValueError("epg_signal: the program records nothing (no step has the RECORD flag, 4)")
        nstates = int(nstates)
        if not 1 <= nstates <= cls.EPG_MAX_STATES:
            raise ValueError("epg_signal: %d states, between 1 and %d are supported" % (nstates, cls.EPG_MAX_STATES))
        return p, np.ascontiguousarray(st), fl, nstates, nrec

    def epg_signal(self, params, steps, flags, nstates, chunk=1 << 16):
        """Extended-phase-graph simulation (indigo_amd.dictmatch --model fse / fisp): the signal of N atoms under one
        pulse program -> a host (N, nrec) complex64 array.  params is a host (N, 3) array of (T1, T2, B1), cast to float32; steps a
        host (S, 4) float64 array of (flip, phase, a, b) per step, radians and seconds; flags S integers, bits 1 = SHIFT_A,
        2 = SHIFT_B, 4 = RECORD, 8 = SPOIL.  An atom's state is (F+_k, F-_k, Z_k), k < nstates, Z_0 = 1 at the start; a step runs
        RF(B1 flip, phase), relax(a), shift if SHIFT_A, record F+_0 if RECORD, relax(b), shift if SHIFT_B, F+ = F- = 0 if SPOIL, with
        the operations of ig_epg_sim_c64 (include/indigo_hip.h).  Host form: float64 arithmetic on the float32-cast parameters,
        vectorised over `chunk` atoms at a time; device backends override it."""
        p, st, fl, K, nrec = self.epg_check(params, steps, flags, nstates)
        N, chunk = p.shape[0], max(1, int(chunk))
        out = np.empty((N, nrec), dtype=_C64)
        for i0 in range(0, N, chunk):
            q = p[i0:i0 + chunk].astype(np.float64)
            T1, T2, B1 = q[:, 0:1], q[:, 1:2], q[:, 2:3]
            n = q.shape[0]
            Fp, Fm, Z = (np.zeros((n, K), dtype=np.complex128) for _ in range(3))
            Z[:, 0] = 1.0

            def relax(d):
                if d == 0:
                    return
                E2 = np.exp(-d / T2)
                Fp[...] *= E2
                Fm[...] *= E2
                Z[...] *= np.exp(-d / T1)
                Z[:, 0] -= np.expm1(-d / T1[:, 0])

            def shift():
                Fp[:, 1:] = Fp[:, :-1].copy()
                Fm[:, :-1] = Fm[:, 1:].copy()
                Fm[:, -1] = 0
                Fp[:, 0] = np.conj(Fm[:, 0])
            r = 0
            for (alpha, phi, a, b), f in zip(st, fl):
                theta = B1 * alpha
                e = np.exp(1j * phi)
                c, s, sn = np.cos(theta / 2) ** 2, np.sin(theta / 2) ** 2, np.sin(theta)
                Fp, Fm, Z = (c * Fp + (e * e) * s * Fm - 1j * e * sn * Z,
                             np.conj(e * e) * s * Fp + c * Fm + 1j * np.conj(e) * sn * Z,
                             -0.5j * np.conj(e) * sn * Fp + 0.5j * e * sn * Fm + np.cos(theta) * Z)
                relax(a)
                if f & self.EPG_SHIFT_A:
                    shift()
                if f & self.EPG_RECORD:
                    out[i0:i0 + n, r] = Fp[:, 0]
                    r += 1
                relax(b)
                if f & self.EPG_SHIFT_B:
                    shift()
                if f & self.EPG_SPOIL:
                    Fp[...] = 0
                    Fm[...] = 0
        return out

    @staticmethod
    def _dcf_taps(rec, tw, dims):
        """(cells, taps) of the separable records `rec` (rows of at least 3 tw + 2 words), each (rows, tw^3): the grid cell of every
        tap in the records' memory order and its value in the kernels' float32 arithmetic, (w1 * w2) * w0; taps beyond an axis's
        tap count are 0 (their cells are valid: they add nothing)"""
        n0, nm, ns = (int(n) for n in dims)
        wts = np.ascontiguousarray(rec[:, :3 * tw]).view(np.float32).reshape(-1, 3, tw)
        h0, h1 = rec[:, 3 * tw].astype(np.int64), rec[:, 3 * tw + 1].astype(np.int64)
        a = np.arange(tw)
        cell, val = [], []
        for axis, (first, count, n) in enumerate(((h0 & 0xffff, (h1 >> 16) & 15, n0), (h0 >> 16, (h1 >> 20) & 15, nm), (h1 & 0xffff, (h1 >> 24) & 15, ns))):
            cell.append((first[:, None] + a) % n)
            val.append(np.where(a < count[:, None], wts[:, axis], np.float32(0)).astype(np.float32))
        cells = cell[0][:, None, None, :] + n0 * (cell[1][:, None, :, None] + nm * cell[2][:, :, None, None])
        taps = (val[1][:, None, :, None] * val[2][:, :, None, None]).astype(np.float32) * val[0][:, None, None, :]
        return cells.reshape(rec.shape[0], -1), taps.astype(np.float32).reshape(rec.shape[0], -1)

    @staticmethod
    def _dcf_records(records, sep, M):
        rec = records.to_host().reshape(-1)
        stride = int(sep.get('stride') or rec.size // max(M, 1))
        assert stride >= 3 * sep['tw'] + 2 and rec.size >= M * stride, (rec.size, M, stride)
        return rec[:M * stride].reshape(M, stride)

    def dcf_spread(self, acc, w, records, sep, scale, tiles):
        """acc = G^H w in fixed point, the first half of a Pipe-Menon iteration (indigo_amd.dcf).  G is the gridding
        matrix in separable form: `records` a backend uint32 array of the records of `interp.interp_sep_records` built with
        phases=None and scale=1, `sep` its description (tw, dims = the grid in memory order, optional stride = words from one
        record to the next).  w: M float32 weights.  acc: int64 over the grid, zeroed here; every tap adds
        rint(tap * w[i] * scale) with the product formed in float64, where it is exact; scale a power of two with
        M * max(w) * scale <= 2^62.  Integer sums do not depend on the order of the adds: the result is the same bits on every
        backend and route.  tiles: the samples binned by grid tile (`grid_formats.dcf_tiles`, as backend arrays) -- how a device
        backend divides the work; without meaning here.  Host form through to_host / copy_from; device backends override it."""
        M = int(w.size)
        tw, dims = int(sep['tw']), tuple(int(n) for n in sep['dims'])
        e = np.frexp(float(scale))
        if not (scale > 0 and e[0] == 0.5):
            raise RuntimeError("dcf_spread: scale %r is no positive power of two" % (scale,))
        assert acc.dtype == np.dtype('int64') and acc.size == int(np.prod(dims)), (acc.shape, dims)
        rec = self._dcf_records(records, sep, M)
        wv = w.to_host().reshape(-1).astype(np.float64) * float(scale)
        out = np.zeros(acc.size, dtype=np.int64)
        for lo in range(0, M, 4096):
            cells, taps = self._dcf_taps(rec[lo:lo + 4096], tw, dims)
            np.add.at(out, cells.reshape(-1), np.rint(taps.astype(np.float64) * wv[lo:lo + 4096, None]).astype(np.int64).reshape(-1))
        acc.copy_from(np.asfortranarray(out.reshape(acc.shape, order='F')))

    def dcf_gather_div(self, w_out, acc, w, records, sep, scale, tiles, s_out=None):
        """The second half of a Pipe-Menon iteration: s_i = sum_taps tap * float64(acc[cell]) / scale in float64 and
        w_out[i] = float32(w[i] / s_i), 0 where s_i == 0; s_out (optional) [i] = float32(s_i).  Arguments as for `dcf_spread`, whose
        acc this reads; w_out may be w.  Returns (max_i w_out[i], max_i |s_i - 1| rounded to float32) as floats: the next
        iteration's scale and the log line.  Host form through to_host / copy_from; device backends override it."""
        M = int(w.size)
        tw, dims = int(sep['tw']), tuple(int(n) for n in sep['dims'])
        rec = self._dcf_records(records, sep, M)
        a = acc.to_host().reshape(-1).astype(np.float64)
        wv = w.to_host().reshape(-1).astype(np.float64)
        s = np.zeros(M)
        for lo in range(0, M, 4096):
            cells, taps = self._dcf_taps(rec[lo:lo + 4096], tw, dims)
            s[lo:lo + 4096] = (taps.astype(np.float64) * a[cells]).sum(axis=1)
        s /= float(scale)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(s == 0, 0.0, wv / s).astype(np.float32)
        w_out.copy_from(np.asfortranarray(q.reshape(w_out.shape, order='F')))
        if s_out is not None:
            s_out.copy_from(np.asfortranarray(s.astype(np.float32).reshape(s_out.shape, order='F')))
        return (float(q.max()), float(np.float32(np.abs(s - 1.0).max()))) if M else (0.0, 0.0)

    def row_scale(self, y, x, w, n, ncols):
        """y[i, c] = w[i] * x[i, c] for the n x ncols complex64 panels x and y (with their leading dimensions, or the same data
        stacked in one column) and the n real float32 weights w shared by all columns: the diagonal of a weighted data term
        (operators.SampleWeights, pics --dcf).  One float32 product per component.  y may be x.  Host form through
        to_host / copy_from; device backends override it."""
        n, C = int(n), int(ncols)
        assert n >= 1 and C >= 1 and w.size == n and x.size == n * C and y.size == n * C, (x.shape, y.shape, w.shape, n, C)
        wv = w.to_host().reshape(-1).astype(np.float32)[:, None]
        v = x.to_host().reshape((n, C), order='F')
        out = np.empty((n, C), dtype=_C64)
        out.real = wv * v.real
        out.imag = wv * v.imag
        y.copy_from(np.asfortranarray(out.reshape(y.shape, order='F')))

    def SampleWeights(self, w, n, ncols, **kwargs):
        """the real diagonal diag(w) (x) I over `ncols` columns of `n` samples each, shape (n ncols, n ncols): one weight per sample,
        shared by the coils (see operators.SampleWeights); .H is itself"""
        return op.SampleWeights(self, w, n, ncols, **kwargs)

    @staticmethod
    def psf_unpack(kern, n, K):
        """the (n, K, K) complex128 Hermitian matrices of a `psf_mix` kernel array: K^2 planes of n floats, the K real diagonals,
        then re and im of every pair (k < k'), the pairs in row-major order of the upper triangle"""
        planes = np.asarray(kern, dtype=np.float64).reshape((K * K, n))
        P = np.zeros((n, K, K), dtype=np.complex128)
        for k in range(K):
            P[:, k, k] = planes[k]
        pair = 0
        for a in range(K):
            for b in range(a + 1, K):
                P[:, a, b] = planes[K + 2 * pair] + 1j * planes[K + 2 * pair + 1]
                P[:, b, a] = np.conj(P[:, a, b])
                pair += 1
        return P

    def psf_mix(self, y, x, kern, n, ncoils, interleaved=False, width=None):
        """y[g, c, k] = sum_k' P[g][k, k'] x[g, c, k'] over g < n grid points and c < ncoils coils: the K x K point-spread mixing
        pass of the Toeplitz normal operator (operators.ToeplitzNormal).  x and y are panels of K columns, or
        the same stacked in one column; a column holds the coils' grids one after the other (element (g, c) at g + n c), or,
        `interleaved`, the `width` >= ncoils coil slots of a grid point side by side (element (g, c) at g width + c; slots
        c >= ncoils are not touched), g in the grid's memory order.  kern is a float32 backend array of K^2 planes of n floats
        in the same grid order (`psf_unpack`).  y may be x.  Host form in float64 through to_host / copy_from; device backends
        override it."""
        n, C = int(n), int(ncoils)
        w = int(width) if (interleaved and width is not None) else C
        K2 = kern.size // n
        K = int(round(np.sqrt(K2)))
        assert n >= 1 and C >= 1 and w >= C and K * K * n == kern.size, (kern.shape, n)
        rows = n * w
        assert x.size == rows * K and y.size == rows * K, (x.shape, y.shape, n, w, K)
        P = self.psf_unpack(kern.to_host(), n, K)
        shape = (w, n, K) if interleaved else (n, w, K)
        v = x.to_host().reshape(shape, order='F').astype(np.complex128)
        out = y.to_host().reshape(shape, order='F').copy()
        if interleaved:
            out[:C] = np.einsum('gab,cgb->cga', P, v[:C]).astype(_C64)
        else:
            out[:] = np.einsum('gab,gcb->gca', P, v).astype(_C64)
        y.copy_from(np.asfortranarray(out.reshape(y.shape, order='F')))

    def ToeplitzNormal(self, dims, maps, kern, K, **kwargs):
        """A^H A of a (subspace) non-Cartesian SENSE problem as one Toeplitz operator on the grid of twice the image size, shape
        (N K, N K) (see operators.ToeplitzNormal; the kernel comes from indigo_amd.toeplitz.psf_kernel); .H is itself"""
        return op.ToeplitzNormal(self, dims, maps, kern, K, **kwargs)

    def supports_padded_fft(self, grid, ncoils=None):
        """whether `fft_padded` / `ifft_cropped[_sum]` exist for this oversampled grid (and, if given, this many coils)"""
        return False

    def ccsrmm(self, y, A_shape, A_indx, A_ptr, A_vals, x, alpha=1, beta=0, adjoint=False, exwrite=False):
        raise NotImplementedError()

    def cdiamm(self, y, shape, offsets, data, x, alpha=1.0, beta=0.0, adjoint=True):
        """y = beta*y + alpha * op(A) * x for a DIA-stored A (op = ^H when adjoint)"""
        raise NotImplementedError()

    def onemm(self, y, x, alpha=1, beta=0):
        """y = beta*y + alpha * ones * x"""
        raise NotImplementedError()

    def cgemm(self, y, M, x, alpha, beta, forward):
        """y = beta*y + alpha * op(M) * x for a dense M"""
        raise NotImplementedError()

    def csymm(self, y, M, x, alpha, beta, left=True):
        """dense product with a real symmetric M, from the left or from the right"""
        raise NotImplementedError()

    def max(self, val, arr):
        raise NotImplementedError()

    def inspect(self, csr):
        """(nonzero rows, nonzero cols, exwrite) of a scipy CSR matrix; exwrite = every column has <= 1 nonzero."""
        counts = np.bincount(csr.indices, minlength=csr.shape[1])
        nzrow = int(np.count_nonzero(np.diff(csr.indptr)))
        return nzrow, int(np.count_nonzero(counts)), bool(counts.max(initial=0) <= 1)

    # ---------------------------------------------------------------------------
    # device CSR matrix
    # ---------------------------------------------------------------------------
    class csr_matrix(object):
        _index_base = 0

        def __init__(self, backend, A, name='mat'):
            if not spp.isspmatrix_csr(A):
                A = A.tocsr()
            A = self._type_correct(A)
            assert A.nnz < 2 ** 31 and max(A.shape) < 2 ** 31, "int32 CSR indices"
            self._backend = backend
            self._name = name
            self.shape = tuple(int(s) for s in A.shape)
            self.dtype = A.dtype
            self.rowPtrs = backend.copy_array(A.indptr.astype(np.int32) + self._index_base, name=name + ".rowPtrs")
            self.colInds = backend.copy_array(A.indices.astype(np.int32) + self._index_base, name=name + ".colInds")
            self.values = backend.copy_array(A.data, name=name + ".data")
            nzrow, nzcol, self._exwrite = backend.inspect(A)
            self._row_frac = nzrow / A.shape[0] if A.shape[0] else 1.0
            self._col_frac = nzcol / A.shape[1] if A.shape[1] else 1.0
            self._grid_il = False       # set_grid_interleaved

        @staticmethod
        def _check_panels(y, x, vals):
            assert x.dtype == _C64, "Bad dtype: expected complex64, got %s" % x.dtype
            assert y.dtype == _C64, "Bad dtype: expected complex64, got %s" % y.dtype
            assert vals.dtype == _C64

        def forward(self, y, x, alpha=1, beta=0):
            """y = alpha * A * x + beta * y"""
            self._check_panels(y, x, self.values)
            il = {'x_il': True} if self._grid_il else {}
            self._backend.ccsrmm(y, self.shape, self.colInds, self.rowPtrs, self.values,
                                 x, alpha=alpha, beta=beta, adjoint=False, exwrite=True, **il)

        def adjoint(self, y, x, alpha=1, beta=0):
            """y = alpha * A^H * x + beta * y"""
            self._check_panels(y, x, self.values)
            il = {'y_il': True} if self._grid_il else {}
            self._backend.ccsrmm(y, self.shape, self.colInds, self.rowPtrs, self.values,
                                 x, alpha=alpha, beta=beta, adjoint=True, exwrite=self._exwrite, **il)

        def set_grid_interleaved(self, flag=True):
            """The panel on the COLUMN side of this matrix (x of a forward product, y of an adjoint one) is stored
            row-major -- the values of one grid point for all panel columns (coils) contiguous -- instead of
            column-major.  This is the memory order of the fused transform's grid layout 2; the products are the
            same numbers in a different order."""
            self._grid_il = bool(flag)

        def set_grid_support(self, table, n0, nm, zw=16):
            """Hint: the columns of this matrix index a 3-D grid and only the tabulated support is ever
            non-zero / read in an adjoint product.  Backends may ignore it (the result inside the support
            is the same either way)."""
            pass

        def set_grid_bricks(self, n0, nm, ns, ncols=8, bm=2, bs=2, chunk=4096, run=4096):
            """Hint: the columns index an n0 x nm x ns grid (col = kx + n0*(km + nm*ks)); the adjoint product may bin the rows
            by grid bricks and scatter race-free.  Backends may ignore it."""
            pass

        def set_row_order(self, perm):
            """Hint: processing the rows in the order `perm` improves locality.  Backends may ignore it."""
            pass

        @property
        def nbytes(self):
            return self.rowPtrs.nbytes + self.colInds.nbytes + self.values.nbytes

        @property
        def nnz(self):
            return self.values.size

        def _type_correct(self, A):
            return A.astype(_C64)

    class dia_matrix(object):
        """Device-resident sparse matrix in diagonal (DIA) storage (reference backend.py:599-635): `data` is scipy's
        dia_matrix.data transposed -- one column per stored diagonal -- and `offsets` the diagonals' offsets."""

        def __init__(self, backend, A, name='mat'):
            assert isinstance(A, spp.dia_matrix)
            A = A.astype(_C64)
            self._backend = backend
            self.data = backend.copy_array(np.asfortranarray(A.data.T), name=name + ".data")
            self.offsets = backend.copy_array(A.offsets.astype(np.int32), name=name + ".offsets")
            self.shape = tuple(int(s) for s in A.shape)
            self.dtype = A.dtype
            self._row_frac = 1
            self._col_frac = 1
            self._exwrite = False

        def forward(self, y, x, alpha=1, beta=0):
            self._backend.cdiamm(y, self.shape, self.offsets, self.data, x, alpha=alpha, beta=beta, adjoint=False)

        def adjoint(self, y, x, alpha=1, beta=0):
            self._backend.cdiamm(y, self.shape, self.offsets, self.data, x, alpha=alpha, beta=beta, adjoint=True)

        @property
        def nbytes(self):
            return self.offsets.nbytes + self.data.nbytes

        @property
        def nnz(self):
            return self.data.size

    # ---------------------------------------------------------------------------
    # solvers
    # ---------------------------------------------------------------------------
    def cg(self, A, b_h, x_h, lamda=0.0, tol=1e-10, maxiter=100, team=None):
        """Conjugate gradients on (A + lamda I) x = b, host-scalar form: x_h is the start and receives the result; returns the
        relative residuals ||r_k|| / ||r_0||, one per iteration, stopping at the first below `tol`.

        The contract is the reference's (indigo/backends/backend.py:639-689: same start, same stopping rule, one operator
        evaluation per iteration, the two reductions through pdot / pnorm2 so that a `team` all-reduces them).  b_h / x_h may be
        device arrays of this backend: x is then updated in place and only the two scalars per iteration cross the host boundary.
        (HipBackend.cg overrides this with device-resident scalars and three fused vector passes per iteration.)"""
        in_place = isinstance(x_h, self.dndarray)
        x = x_h if in_place else self.copy_array(x_h, name='x')
        resid = b_h.copy(name='b') if isinstance(b_h, self.dndarray) else self.copy_array(b_h, name='b')
        q = x.copy()                                   # q = (A + lamda I) d for the current direction d

        def shifted(dst, src):
            A.eval(dst, src)
            if lamda:
                self.axpby(1, dst, lamda, src)

        shifted(q, x)
        self.axpby(1, resid, -1, q)                    # resid = b - (A + lamda I) x
        d = resid.copy(name='p')
        rho = rho0 = self.pnorm2(resid, team)
        trail = []
        for it in range(maxiter):
            shifted(q, d)
            step = rho / self.pdot(d, q, team)
            self.axpby(1, x, step, d)
            self.axpby(1, resid, -step, q)
            rho, rho_old = self.pnorm2(resid, team), rho
            self.axpby(rho / rho_old, d, 1, resid)     # d = resid + (rho / rho_old) d in one pass
            trail.append(float(np.sqrt(rho / rho0)))
            log.info("iter %d, residual %g", it, trail[-1])
            if trail[-1] < tol:
                log.info("cg reached tolerance")
                break
        else:
            log.info("cg reached maxiter")
        if not in_place:
            x.copy_to(x_h)
        return trail

    def fista(self, gradf, proxg, alpha, x_h, maxiter=100, callback=None):
        """FISTA (Beck and Teboulle 2009) for min f + g with a fixed step `alpha`:

            x_{k+1} = prox_{alpha g}(z_k - alpha grad f(z_k)),   t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2,   t_0 = 1,
            z_{k+1} = x_{k+1} + m_k (x_{k+1} - x_k),             m_k = (t_k - 1) / t_{k+1},                z_0 = x_0.

        gradf(g, z) writes grad f(z) into g; proxg(v, alpha) replaces v by prox_{alpha g}(v).  x_h is the start and receives the
        result (a host array, or a device array of this backend, updated in place).  callback(k, x), when given, runs after
        iteration k (from 0) with the iterate x_{k+1}.  Three vectors; besides gradf and proxg an iteration is two axpby passes
        (the gradient step into g's buffer, the extrapolation into x_k's buffer, then the three buffers change roles), so on a
        device backend it enqueues work and never waits for the device.  Unlike `apgd`, whose momentum is the reference's
        constant 0, this one advances t_k."""
        in_place = isinstance(x_h, self.dndarray)
        x = x_h if in_place else self.copy_array(x_h, name='x')
        x_out = x
        z, g = x.copy(name='z'), x.copy(name='g')
        t = 1.0
        for k in range(int(maxiter)):
            gradf(g, z)
            self.axpby(-alpha, g, 1, z)                # g <- z - alpha grad f(z)
            proxg(g, alpha)                            # g <- x_{k+1}
            t_next = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
            m = (t - 1.0) / t_next
            self.axpby(-m, x, 1 + m, g)                # x_k's buffer <- z_{k+1}
            x, z, g = g, x, z
            t = t_next
            if callback is not None:
                callback(k, x)
        if x is not x_out:
            x_out.copy(x)
        if not in_place:
            x_out.copy_to(x_h)

    def primal_dual(self, gradf, proxg, KH, dual_step, tau, x_h, u, maxiter=100, callback=None):
        """The Condat-Vu primal-dual iteration with an explicit gradient step, for min_x f(x) + g(x) + h(K x) with f smooth:

            x_{k+1} = prox_{tau g}( x_k - tau (grad f(x_k) + K^H u_k) ),
            u_{k+1} = dual_step(u_k, x_{k+1}, x_k)          # = prox_{sigma h*}(u_k + sigma K (2 x_{k+1} - x_k))

        gradf(g, x) writes grad f(x) into g; KH(g, u) adds K^H u onto g; proxg(v, tau) replaces v by prox_{tau g}(v), or is None
        (g = 0); dual_step(u, xn, xo) updates the dual variable u in place.  It converges for 1/tau - sigma ||K||^2 >= L/2, L the
        Lipschitz constant of grad f (Condat 2013, Vu 2013).  x_h is the start and receives the result (a host array, or a device
        array of this backend, updated in place); u is a device array, the dual start, updated in place.  callback(k, x), when
        given, runs after iteration k (from 0) with the iterate x_{k+1}.  Two primal vectors: the gradient is built in g's
        buffer, one axpby turns it into x_{k+1} there, and after the dual step x_k's buffer is free to be the next g -- the
        two change roles as in `fista`.  On a device backend an iteration enqueues work and never waits for the device."""
        in_place = isinstance(x_h, self.dndarray)
        x = x_h if in_place else self.copy_array(x_h, name='x')
        x_out = x
        g = x.copy(name='g')
        for k in range(int(maxiter)):
            gradf(g, x)
            KH(g, u)
            self.axpby(-tau, g, 1, x)                  # g <- x_k - tau (grad f(x_k) + K^H u_k)
            if proxg is not None:
                proxg(g, tau)                          # g <- x_{k+1}
            dual_step(u, g, x)
            x, g = g, x
            if callback is not None:
                callback(k, x)
        if x is not x_out:
            x_out.copy(x)
        if not in_place:
            x_out.copy_to(x_h)

    def apgd(self, gradf, proxg, alpha, x_h, maxiter=100, team=None):
        """Proximal gradient iteration for min f + g:  x <- prox_g(x - alpha grad f(y)),  y <- x + m (x - x_before).

        The reference (indigo/backends/backend.py:691-732) writes the accelerated (FISTA) momentum m = (t_k - 1) / t_{k+1} but never
        advances t_k from 1, so its m is 0 in every iteration and its iterates are those of the plain proximal gradient method --
        which the golden vectors captured from it pin (tests/golden/leaf_misc.npz).  `momentum` below is that sequence; the loop
        itself is written for any m.  The gradient step starts from x, not from y, as in the reference."""
        def momentum(k):
            t = 1.0                                    # (the reference's t_k: constant)
            return (t - 1.0) / (0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t)))

        x = self.copy_array(x_h)
        y, x_before, g = x.copy(), x.copy(), x.copy()
        for k in range(maxiter):
            gradf(g, y)
            self.axpby(1, x, -alpha, g)
            proxg(x, alpha)
            m = momentum(k)
            self.axpby(0, y, 1 + m, x)
            if m:
                self.axpby(1, y, -m, x_before)
            x_before.copy(x)
        x.copy_to(x_h)
