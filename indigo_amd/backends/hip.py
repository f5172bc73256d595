"""`HipBackend`: the MI355X backend.  Every leaf kernel is one ctypes call into
``libindigo_hip.so`` (hand-written HIP for gfx950, C ABI in include/indigo_hip.h).

Plays the role `CudaBackend` plays in the reference (indigo/backends/cuda.py:
device pointers in `dndarray._arr`, pitch copies, plan cache, one call per leaf)
but is not derived from it: there are no vendor BLAS/FFT/sparse libraries
underneath, no per-leaf device synchronisation, sizes are 64-bit, and the
adjoint SpMM uses a cached transposed CSR (gather) instead of a scatter.

There is no CPU fallback.  Constructing the backend without a usable GPU or
without the built library raises RuntimeError.
"""
import ctypes
import logging
import os

import numpy as np

from indigo_amd import _lib
from indigo_amd._lib import cplx as _cplx
from indigo_amd.backends.backend import WAVELET_IDS, Backend
from indigo_amd.grid_formats import brick_tasks, weights_are_real       # noqa: F401  (their home; imported from here by tools and tests)

log = logging.getLogger(__name__)
_C64 = np.dtype('complex64')


class HipBackend(Backend):

    def __init__(self, device_id=0, stream=None):
        """`stream`: optional raw hipStream_t (int) to adopt, e.g. a torch stream's `.cuda_stream`."""
        super().__init__(device_id)
        self._L = _lib.lib()
        ctx = ctypes.c_void_p()
        if stream is None:
            rc = self._L.ig_init(int(device_id), ctypes.byref(ctx))
        else:
            rc = self._L.ig_init_on_stream(int(device_id), ctypes.c_void_p(stream), ctypes.byref(ctx))
        _lib.check(rc, None, "ig_init")
        self._ctx = ctx
        self.device_id = int(device_id)
        self._plans = dict()
        # 'transpose': adjoint of a non-exwrite matrix gathers through a cached CSR of A^T (deterministic)
        # 'atomic'   : adjoint scatters with float atomics straight from A's CSR (no extra memory)
        self.adjoint_policy = 'transpose'
        # Format choices of this backend's matrices and fused trees (defaults = the measured best; tests switch routes off to
        # reach the fallback kernels):
        #   bricks        coil counts whose interleaved adjoint gridding is the brick-binned scatter (others: gather over G'^T)
        #   support_tile  kx points per entry of the fine k-space support table of coil-interleaved trees, by coil count (16: one table only)
        #   brick_shape   per coil count: (grid lines, slabs, heavy-brick piece, entries per run) of the binned format.  Four coils
        #                 pad a sample's share of a brick to 16 entries: bricks of 16 x 2 x 4 cells waste less than 16 x 2 x 2 (0.61
        #                 against 0.68 ms; profiles/r03_brick_shape_sweep.txt)
        #   xrows         wide panels (16..64 columns): repack only the panel rows the matrix touches (forward)
        #   wide_bricks   64-column column-major panels: brick scatter through LDS (adjoint)
        #   slots         coil counts whose adjoint gridding is the slot-format scatter (ig_ccsrmm_t_slots): the ranks of a coil-sharded
        #                 run with one or two coils
        #   placement_candidates / placement_min_bytes   arrays of at least that many bytes (scratch arenas, grids) are allocated that many
        #                 times, probed (ig_probe_placement) and the best-placed candidate kept; 1 = plain allocation
        #   cg_graph      HipBackend.cg replays a block of iterations as one HIP graph launch (ig_graph_*).  Off: measured on the headline
        #                 problem the replay saves 0.03 ms of a 6.89 ms iteration and recording costs 5 ms per solve (profiles/r05_cg_graph_ab.log)
        #   placement_window_gb   (round 6) a large array is a window of ONE allocation that many GB larger, placed at the best-probing 1 GB step
        #   separable / sep_gather / sep_scatter   the gridding matrix in separable form (one record per sample) and the kernels that compute
        #                 their taps from it: forward on every even grid; adjoint (shares) for `shares` coil counts from `shares_min_tw` taps
        #                 per axis on (kernel half-width > 2: below that the stored-tap bricks are faster)
        #   share_shape   per coil count: (grid lines, slabs, heavy-brick piece, shares per run).  The PIECE bounds how many samples a wave sums
        #                 into one float32 image before it adds it to the grid: pieces of 1024 shares put the evaluation 2.1e-5 from the float64
        #                 one on an ill-conditioned problem (oversampling 1.25, half-width 3: the k-space centre's sum leaks to the image's edge,
        #                 where the roll-off correction is large); 128: 4.7 ... 6.1e-6 over four runs, the stored-tap scatter 4.8 ... 7.6e-6 (the
        #                 order of the float atomics differs from run to run), 0.95 against 0.98 ms (profiles/r06_share_pieces.txt)
        self._placement_log = []          # (bytes, candidate probe times in ms, chosen) of every array placed by probing
        self.tuning = dict(placement_candidates=3, placement_min_bytes=1 << 31, placement_window_gb=24, placement_window_allocs=3, fold_odd_axes=True, real_gridding=True, gather_order=True, cg_graph=False, bricks=(4, 8), slots=(1, 2), slot_shape=(4, 4, 256, 64), support_tile={8: 4, 4: 8}, brick_shape={8: (2, 2, 4096, 4096), 4: (2, 4, 4096, 4096)}, xrows=True, runs=True, wide_bricks=True,
                           wide_brick_shape=(2, 2), wide_task_shape=(8192, 2048),
                           # round 6: gridding from the separable form of the matrix (one record per sample, taps computed)
                           separable=True, sep_gather=True, sep_scatter=True, shares=(4, 8), shares_min_tw=6, share_shape={8: (4, 4, 128, 1024), 4: (4, 4, 128, 1024)},
                           # samples per partial sum of coil_gram: a float32 chain of gram_slab / 8 = 2048 samples per wave (/ 4 beyond 32 coils), 1024 workgroups
                           # and 17 MB of partial sums at 2^24 samples x 64 coils
                           gram_slab=16384,
                           # samples from which a 16 x 8 x 8 tile of the Pipe-Menon spread sums in LDS before it touches the grid (ig_dcf_spread_r32;
                           # 0: every tile, 2^31: none; the same bits for every value: DESIGN.md §3.17)
                           # dcf_piece: samples per workgroup of a heavier tile (grid_formats.dcf_tiles)
                           dcf_lds_min=8, dcf_piece=2048)

    def __del__(self):
        try:
            for entry in getattr(self, '_plans', {}).values():
                self._L.ig_fft_destroy(entry[0])
            if getattr(self, '_ctx', None):
                self._L.ig_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            _lib.check(rc, self._ctx, what)

    # -- housekeeping ---------------------------------------------------------------
    def barrier(self):
        self._check(self._L.ig_sync(self._ctx), "ig_sync")

    @property
    def stream(self):
        """raw hipStream_t of this backend (int)"""
        return self._L.ig_stream(self._ctx) or 0

    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        self._check(self._L.ig_device_name(self._ctx, buf, 256), "ig_device_name")
        return buf.value.decode()

    def set_option(self, name, value):
        """plan options of the library (ig_set_option): 'fft.kernels' = 0 all kernels, 1 no A x B passes, 2 generic stages only;
        'fft.zc_intermediate' = 1 the fused SENSE leaf keeps what its y and z passes exchange z-contiguous per kx tile, 0 in the
        grid's own order (bit-identical results, same workspace); 'fft.xy_chunk_planes' = K > 0 the fused SENSE leaf (grid layout 2,
        256- / 512-point x and y axes) runs its x and y passes chunk by chunk over K image planes, so that what they exchange is
        re-read while it is still in the last-level cache, 0 one launch per pass, -1 (the default) as many planes as make 128 MiB
        of what they exchange (16 on the 512^3 x 8 grid; problems below that size keep one launch per pass); 'fft.xy_chunk_streams' = S in 1, 2, 3: chunk i
        runs on stream i mod S (default 2), joined back into the backend's stream before the call returns (bit-identical results either way;
        ignored while a graph is recorded); takes effect for plans made afterwards (cached plans are dropped)"""
        self._check(self._L.ig_set_option(self._ctx, name.encode(), int(value)), "ig_set_option(%s)" % name)
        for entry in self._plans.values():
            self._L.ig_fft_destroy(entry[0])
        self._plans = dict()

    def mem_usage(self):
        """bytes of device memory in use through this backend: the arrays it handed out (Backend.mem_usage, backend.py:249)
        plus what the library holds on its own (the SpMM kernels' repacked-panel buffer, work lists, reduction scratch)"""
        own = ctypes.c_size_t()
        self._check(self._L.ig_library_bytes(self._ctx, ctypes.byref(own)), "ig_library_bytes")
        return super().mem_usage() + own.value

    def mem_info(self):
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        self._check(self._L.ig_mem_info(self._ctx, ctypes.byref(free), ctypes.byref(total)), "ig_mem_info")
        return free.value, total.value

    # events: (start, stop) pairs on the backend's stream, no host sync until `elapsed_ms`
    def event(self):
        ev = ctypes.c_void_p()
        self._check(self._L.ig_event_create(self._ctx, ctypes.byref(ev)), "ig_event_create")
        return ev

    def record(self, ev):
        self._check(self._L.ig_event_record(ev), "ig_event_record")

    def elapsed_ms(self, start, stop):
        ms = ctypes.c_float()
        self._check(self._L.ig_event_elapsed_ms(start, stop, ctypes.byref(ms)), "ig_event_elapsed_ms")
        return ms.value

    def event_destroy(self, ev):
        self._L.ig_event_destroy(ev)

    def profile(self, on=True):
        """bracket every kernel launch with stream events (no host sync) until switched off"""
        self._check(self._L.ig_prof_enable(self._ctx, 1 if on else 0), "ig_prof_enable")
        self._prof_on = bool(on)

    def profile_report(self):
        """{kernel: dict(launches, total_ms, avg_ms, bytes)} since the last report; synchronises"""
        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self._L.ig_prof_report(self._ctx, buf, len(buf)), "ig_prof_report")
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms, nbytes = line.split()
            out[name] = dict(launches=int(n), total_ms=float(ms), avg_ms=float(ms) / max(int(n), 1), bytes=float(nbytes))
        return out

    # -- arrays -----------------------------------------------------------------------
    class dndarray(Backend.dndarray):
        """`_arr` is the device address (Python int)."""

        def _malloc(self, shape, dtype):
            b = self._backend
            if self.nbytes >= int(b.tuning.get('placement_min_bytes', 1 << 31)):
                slack = int(b.tuning.get('placement_window_gb', 0))
                if slack > 0:
                    ptr = self._malloc_window(slack)
                    if ptr is not None:
                        return ptr
                ncand = int(b.tuning.get('placement_candidates', 1))
                if ncand > 1:
                    return self._malloc_best_placed(ncand)
            ptr = ctypes.c_void_p()
            b._check(b._L.ig_malloc(b._ctx, self.nbytes, ctypes.byref(ptr)), "ig_malloc(%d bytes)" % self.nbytes)
            return ptr.value

        def _malloc_window(self, slack_gb):
            """A large array as the best-placed WINDOW of an allocation (round 6).  The passes that step megabytes per element run
            3 ... 6 % faster or slower with where their array lies -- from allocation to allocation (every other
            process or so gets a slow first one: 3.6 - 3.7 ms in the placement probe against 3.2), and inside ONE allocation the
            probe's time changes smoothly with the offset (profiles/r06_placement_offsets.txt, r06_placement_slack.txt): a slow level
            (3.7 ms for the headline's arena) over the first 0 ... 13 GB of an allocation, a ramp down over the next 7 - 8 GB, a fast
            plateau (2.9 ms) behind; what looked like two kinds of allocation in round 5 is where an allocation starts relative to that
            ramp.  So: an allocation of nbytes + slack_gb GB (24: the plateau has been inside it on every box so far), the probe
            (ig_probe_placement) on the window at every GB step, the fastest window kept.  An allocation without a ramp (all windows
            alike: all slow) is followed by another, up to `placement_window_allocs`; the losers are freed at the end.  slack_gb GB stay
            held beyond the array.  None (the caller falls back) when the device has no room for the slack."""
            b = self._backend
            GBs = 1 << 30
            nalloc = max(1, int(b.tuning.get('placement_window_allocs', 3)))
            worst = b.tuning.get('placement_pick') == 'worst'
            cands = []          # (best time, base, pick, times)
            try:
                for _ in range(nalloc):
                    free, total = ctypes.c_size_t(), ctypes.c_size_t()
                    # (a further allocation only while the device has room for it and as much again: another process on the same GPU
                    # must not fail because of a transient candidate)
                    need = (self.nbytes + (slack_gb + 4) * GBs) if not cands else 2 * (self.nbytes + slack_gb * GBs)
                    if b._L.ig_mem_info(b._ctx, ctypes.byref(free), ctypes.byref(total)) != 0 or free.value < need:
                        break
                    base = ctypes.c_void_p()
                    if b._L.ig_malloc(b._ctx, self.nbytes + slack_gb * GBs, ctypes.byref(base)) != 0:
                        break
                    cands.append([None, base.value, 0, []])
                    times = []
                    for off in range(slack_gb + 1):
                        ms = ctypes.c_double(0.0)
                        b._check(b._L.ig_probe_placement(b._ctx, ctypes.c_void_p(base.value + off * GBs), self.nbytes, ctypes.byref(ms)), "ig_probe_placement")
                        times.append(ms.value)
                    if len(cands) == 1:
                        # (the first window may have been timed while the clocks were still coming up: once more)
                        ms = ctypes.c_double(0.0)
                        b._check(b._L.ig_probe_placement(b._ctx, base, self.nbytes, ctypes.byref(ms)), "ig_probe_placement")
                        times[0] = min(times[0], ms.value)
                    pick = int(np.argmax(times)) if worst else int(np.argmin(times))
                    cands[-1] = [times[pick], base.value, pick, times]
                    # enough once a RAMP has been seen -- probes 8 % apart: the slow level (~3.7 ms on the headline's arena) and the fast one
                    # (2.9) or the way down between them -- the best window is then on the fast side.  An allocation whose windows all
                    # probe alike is all slow (a fast one always starts with a ramp): another one is tried, up to `placement_window_allocs`
                    # (the losers are held until the choice is made: freed at once, the next allocation of the same size would get their
                    # pages back)
                    allt = [v for c in cands for v in c[3]]
                    if min(allt) <= 0.92 * max(allt):
                        break
            except Exception:
                for c in cands:
                    if c[1] is not None:
                        b._L.ig_free(b._ctx, ctypes.c_void_p(c[1]))
                raise
            for c in cands:
                if c[0] is None:
                    b._L.ig_free(b._ctx, ctypes.c_void_p(c[1]))
            cands = [c for c in cands if c[0] is not None]
            if not cands:
                return None
            keep = (max if worst else min)(range(len(cands)), key=lambda i: cands[i][0])
            for i, c in enumerate(cands):
                if i != keep:
                    b._L.ig_free(b._ctx, ctypes.c_void_p(c[1]))
            t, base, pick, times = cands[keep]
            self._alloc_base = base
            b._placement_log.append((self.nbytes, [[round(v, 4) for v in c[3]] for c in cands], round(t, 4)))
            log.debug("placement: %d bytes, windows at +0 .. +%d GB of %d allocation(s) %s ms -> allocation %d, +%d GB", self.nbytes, slack_gb, len(cands),
                      [[round(v, 4) for v in c[3]] for c in cands], keep, pick)
            return base + pick * GBs

        def _malloc_best_placed(self, ncand):
            """A large array (a scratch arena, a grid): allocate up to `ncand` candidates, time the library's placement probe on each
            (ig_probe_placement: the write pattern of a pass that steps megabytes per element) and keep the fastest -- allocations of
            one size made by one process differ by 3 ... 6 % in such passes, repeatably.  Candidates that no longer
            fit are simply not tried; the losers are freed before this returns."""
            b = self._backend
            cands = []
            keep = None
            try:
                for _ in range(ncand):
                    if cands:
                        # a further candidate only while the device has room for it AND as much again: another process on the same
                        # GPU (ranks sharing a device in a rehearsal, another tenant) must not fail because of transient candidates
                        free, total = ctypes.c_size_t(), ctypes.c_size_t()
                        if b._L.ig_mem_info(b._ctx, ctypes.byref(free), ctypes.byref(total)) != 0 or free.value < 2 * self.nbytes:
                            break
                    ptr = ctypes.c_void_p()
                    rc = b._L.ig_malloc(b._ctx, self.nbytes, ctypes.byref(ptr))
                    if rc != 0:
                        if not cands:
                            b._check(rc, "ig_malloc(%d bytes)" % self.nbytes)
                        break
                    cands.append([None, ptr.value])
                    ms = ctypes.c_double(0.0)
                    b._check(b._L.ig_probe_placement(b._ctx, ptr, self.nbytes, ctypes.byref(ms)), "ig_probe_placement")
                    cands[-1][0] = ms.value
                if len(cands) > 1:
                    # the first candidate may have been timed while the clocks were still coming up (the probe is often the first work of
                    # a process): time it once more, now behind the others, and keep its better figure
                    ms = ctypes.c_double(0.0)
                    b._check(b._L.ig_probe_placement(b._ctx, ctypes.c_void_p(cands[0][1]), self.nbytes, ctypes.byref(ms)), "ig_probe_placement")
                    cands[0][0] = min(cands[0][0], ms.value)
                best = max(cands) if b.tuning.get('placement_pick') == 'worst' else min(cands)       # ('worst': lab, to see what the probe's spread is worth)
                keep = best[1]
            finally:
                # the losers -- all candidates if a probe failed -- are freed whatever happened
                for _, ptr in cands:
                    if ptr != keep:
                        b._L.ig_free(b._ctx, ctypes.c_void_p(ptr))
            b._placement_log.append((self.nbytes, [round(ms, 4) for ms, _ in cands], round(best[0], 4)))
            log.debug("placement: %d bytes, candidates %s ms -> %.4f", self.nbytes, [round(ms, 4) for ms, _ in cands], best[0])
            return best[1]

        def _free(self):
            b = self._backend
            if getattr(b, '_ctx', None):
                b._L.ig_free(b._ctx, ctypes.c_void_p(getattr(self, '_alloc_base', None) or self._arr))

        def _zero(self):
            b = self._backend
            if self.ndim == 2 and not self.contiguous:
                # strided view: clear column by column through a scale by zero
                b.scale(self, 0)
            else:
                b._check(b._L.ig_memset0(b._ctx, ctypes.c_void_p(self._arr), self.nbytes), "ig_memset0")

        def _pitched(self, host_rows):
            """(device pitch, host pitch, row bytes, count) for a 2-d column-major transfer"""
            return (self._leading_dim * self.itemsize, host_rows * self.itemsize,
                    self.shape[0] * self.itemsize, self.shape[1])

        def _copy_from(self, arr):
            assert arr.flags['F_CONTIGUOUS']
            b = self._backend
            src = ctypes.c_void_p(arr.ctypes.data)
            dst = ctypes.c_void_p(self._arr)
            if self.size == 0:
                return
            if self.ndim == 2 and not self.contiguous:
                dpitch, spitch, width, height = self._pitched(self.shape[0])
                rc = b._L.ig_copy2d(b._ctx, dst, dpitch, src, spitch, width, height, _lib.IG_H2D)
            else:
                assert self.contiguous
                rc = b._L.ig_copy2d(b._ctx, dst, self.nbytes, src, self.nbytes, self.nbytes, 1, _lib.IG_H2D)
            b._check(rc, "ig_copy2d(H2D)")

        def _copy_to(self, arr):
            b = self._backend
            if self.size == 0:
                return
            out = arr if arr.flags['F_CONTIGUOUS'] else np.empty(self.shape, self.dtype, order='F')
            dst = ctypes.c_void_p(out.ctypes.data)
            src = ctypes.c_void_p(self._arr)
            if self.ndim == 2 and not self.contiguous:
                spitch, dpitch, width, height = self._pitched(self.shape[0])
                rc = b._L.ig_copy2d(b._ctx, dst, dpitch, src, spitch, width, height, _lib.IG_D2H)
            else:
                assert self.contiguous
                rc = b._L.ig_copy2d(b._ctx, dst, self.nbytes, src, self.nbytes, self.nbytes, 1, _lib.IG_D2H)
            b._check(rc, "ig_copy2d(D2H)")
            if out is not arr:
                arr[...] = out.reshape(arr.shape, order='F')

        def _copy(self, d_arr):
            """device -> device: self <- d_arr"""
            b = self._backend
            assert self.size == d_arr.size
            if self.size == 0:
                return
            dst, src = ctypes.c_void_p(self._arr), ctypes.c_void_p(d_arr._arr)
            if self.ndim == 2 and d_arr.ndim == 2 and not (self.contiguous and d_arr.contiguous):
                assert self.shape == d_arr.shape
                rc = b._L.ig_copy2d(b._ctx, dst, self._leading_dim * self.itemsize,
                                    src, d_arr._leading_dim * d_arr.itemsize,
                                    self.shape[0] * self.itemsize, self.shape[1], _lib.IG_D2D)
            else:
                assert self.contiguous and d_arr.contiguous
                rc = b._L.ig_copy2d(b._ctx, dst, self.nbytes, src, self.nbytes, self.nbytes, 1, _lib.IG_D2D)
            b._check(rc, "ig_copy2d(D2D)")

        def __getitem__(self, slc):
            """Contiguous-box slicing; returns a view (pointer + F-order offset, same leading dim)."""
            if not isinstance(slc, tuple):
                slc = (slc,)
            slc = slc + (slice(None),) * (self.ndim - len(slc))
            start, shape = [], []
            for s, n in zip(slc, self.shape):
                if isinstance(s, (int, np.integer)):
                    s = slice(int(s), int(s) + 1)
                assert s.step in (None, 1), "strided slices are not supported"
                b, e, _ = s.indices(n)
                if e < b:
                    e = b
                start.append(b)
                shape.append(e - b)
            if self.ndim == 1:
                offset = start[0]
            else:
                # element (i0, i1, ...) lives at i0 + ld*(i1 + shape[1]*(i2 + ...))
                offset, stride = start[0], self._leading_dim
                for d in range(1, self.ndim):
                    offset += start[d] * stride
                    stride *= self.shape[d]
            ptr = self._arr + offset * self.itemsize
            ld = shape[0] if self.ndim == 1 else self._leading_dim
            return self._view(tuple(shape), ld, ptr)

    # -- BLAS-1 ---------------------------------------------------------------------------
    def _flat(self, a):
        assert a.contiguous or a.ndim == 2, "unsupported layout"
        return a.contiguous

    def axpby(self, beta, y, alpha, x):
        """y = beta*y + alpha*x  (one fused pass; the CUDA reference takes two, cuda.py:239-248)"""
        assert isinstance(x, self.dndarray) and isinstance(y, self.dndarray)
        assert x.dtype == _C64 and y.dtype == _C64, "only complex64 is supported"
        assert x.size == y.size
        br, bi = _cplx(beta)
        ar, ai = _cplx(alpha)
        if self._flat(y) and self._flat(x):
            self._check(self._L.ig_caxpby(self._ctx, y.size, br, bi, ctypes.c_void_p(y._arr),
                                          ar, ai, ctypes.c_void_p(x._arr)), "ig_caxpby")
        else:
            x2 = x if x.ndim == 2 else x.reshape(y.shape)
            assert x2.shape == y.shape
            for j in range(y.shape[1]):
                yp = y._arr + j * y._leading_dim * 8
                xp = x2._arr + j * x2._leading_dim * 8
                self._check(self._L.ig_caxpby(self._ctx, y.shape[0], br, bi, ctypes.c_void_p(yp),
                                              ar, ai, ctypes.c_void_p(xp)), "ig_caxpby")

    def scale(self, x, alpha):
        assert isinstance(x, self.dndarray) and x.dtype == _C64
        ar, ai = _cplx(alpha)
        if self._flat(x):
            self._check(self._L.ig_cscal(self._ctx, x.size, ar, ai, ctypes.c_void_p(x._arr)), "ig_cscal")
        else:
            for j in range(x.shape[1]):
                xp = x._arr + j * x._leading_dim * 8
                self._check(self._L.ig_cscal(self._ctx, x.shape[0], ar, ai, ctypes.c_void_p(xp)), "ig_cscal")

    def dot(self, x, y):
        """Re(x^H y) as a Python float (device -> host sync point)"""
        assert x.dtype == _C64 and y.dtype == _C64 and x.size == y.size
        assert x.contiguous and y.contiguous
        out = (ctypes.c_double * 2)()
        self._check(self._L.ig_cdotc(self._ctx, x.size, ctypes.c_void_p(x._arr), ctypes.c_void_p(y._arr), out), "ig_cdotc")
        return out[0]

    def cdot(self, x, y):
        """full complex x^H y"""
        out = (ctypes.c_double * 2)()
        self._check(self._L.ig_cdotc(self._ctx, x.size, ctypes.c_void_p(x._arr), ctypes.c_void_p(y._arr), out), "ig_cdotc")
        return complex(out[0], out[1])

    def norm2(self, x):
        """||x||^2"""
        assert x.dtype == _C64 and x.contiguous
        out = ctypes.c_double()
        self._check(self._L.ig_scnrm2sq(self._ctx, x.size, ctypes.c_void_p(x._arr), ctypes.byref(out)), "ig_scnrm2sq")
        return out.value

    # -- CG with device-resident scalars --------------------------------------------------------
    def _slots(self):
        if getattr(self, '_scal', None) is None:
            ptr, n = ctypes.c_void_p(), ctypes.c_int()
            self._check(self._L.ig_scalars(self._ctx, ctypes.byref(ptr), ctypes.byref(n)), "ig_scalars")
            self._scal = (ptr.value, n.value)
        return self._scal

    def cg(self, A, b_h, x_h, lamda=0.0, tol=1e-10, maxiter=100, team=None, check_every=10):
        """Conjugate gradients with the iteration's scalars kept on the device (same update sequence and the same
        numbers as Backend.cg / the reference's backend.py:651-689), an iteration's vector work in three fused passes
        (ig_cg_dot, ig_cg_step_r, ig_cg_step_xp: 7 reads + 3 writes of a vector instead of 9 + 3, three launches instead of
        twelve): alpha = rr/<p,Ap> and beta = r2/rr are computed inside the update kernels from the block partials of the
        reductions, so an iteration enqueues without a host synchronisation.  The relative residuals are recorded on the device for
        EVERY iteration and fetched every `check_every` iterations (the only syncs).  The reference leaves its loop the
        moment resid < tol (backend.py:683-685); here up to check_every-1 further iterations are already enqueued by
        then, so the step length is gated on the device: once rr/r0 < tol^2 (or <p,Ap> == 0: an exactly converged
        system) alpha is 0 and those iterations leave x and r alone.  The returned history ends at the first residual
        below tol, like the reference's.  A `team` (host-scalar all-reduces per iteration, backend.py:469-479) uses the
        base implementation."""
        if team is not None or not (hasattr(A, 'eval')):
            return super().cg(A, b_h, x_h, lamda=lamda, tol=tol, maxiter=maxiter, team=team)
        A_in, lamda_in = A, lamda
        A, lamda = self._split_identity(A, lamda)
        if np.imag(lamda) != 0:
            # the fused passes carry a REAL regularisation weight; a complex one (which the reference's loop accepts,
            # backend.py:651-689) takes the base implementation with the caller's own operator -- decided before anything is allocated
            return super().cg(A_in, b_h, x_h, lamda=lamda_in, tol=tol, maxiter=maxiter, team=team)
        base, nslots = self._slots()
        S = lambda i: ctypes.c_void_p(base + 8 * i)          # slot i (a device double)
        RRA, R0, RRB, ALPHA, HIST = 0, 1, 2, 4, 8            # rr lives in two slots used in turn (ig_cg_step_xp writes the other one)
        cap = nslots - HIST                                  # history slots: a ring, fetched before it wraps
        L, ctx = self._L, self._ctx
        P = lambda a: ctypes.c_void_p(a._arr)
        x_dev = isinstance(x_h, self.dndarray)
        x = x_h if x_dev else self.copy_array(x_h, name='x')
        b = b_h.copy(name='b') if isinstance(b_h, self.dndarray) else self.copy_array(b_h, name='b')
        assert x.dtype == _C64 and b.dtype == _C64 and x.contiguous and b.contiguous
        n = x.size
        Ap = x.copy()
        r = b
        A.eval(Ap, x)
        self.axpby(1, r, -1, Ap)
        self.axpby(1, r, -lamda, x)
        p = r.copy(name='p')
        self._check(L.ig_scnrm2sq_dev(ctx, n, P(r), S(RRA)), "ig_scnrm2sq_dev")
        self._check(L.ig_scalar_copy(ctx, S(R0), S(RRA), 1), "ig_scalar_copy")
        history = []
        fetched = 0
        every = max(1, min(int(check_every), cap))
        host = (ctypes.c_double * every)()
        tol2 = float(tol) ** 2
        lam = ctypes.c_float(float(np.real(lamda)))
        it = 0
        done = False

        def iteration(i):
            rr, rr_next = (RRA, RRB) if i % 2 == 0 else (RRB, RRA)
            A.eval(Ap, p)
            # three fused passes (ig_blas.hip): Ap += lamda p and <p, Ap>;  alpha = rr / <p, Ap> (zero once rr / r0 < tol^2: the
            # reference has left its loop by then), r -= alpha Ap, ||r||^2;  beta = r2 / rr, x += alpha p, p = r + beta p,
            # rr <- r2, history[i] = r2 / r0
            self._check(L.ig_cg_dot(ctx, n, P(p), P(Ap), lam), "ig_cg_dot")
            self._check(L.ig_cg_step_r(ctx, n, P(r), P(Ap), S(rr), S(R0), tol2, S(ALPHA)), "ig_cg_step_r")
            self._check(L.ig_cg_step_xp(ctx, n, P(x), P(p), P(r), S(ALPHA), S(rr), S(rr_next), S(R0), S(HIST + i % every)), "ig_cg_step_xp")

        # A block of `every` iterations issues the same launches on the same buffers every time (an even `every` keeps the two
        # rr slots in step): the SECOND block is recorded as a HIP graph (the first ran plain: formats built, attributes set,
        # the library's buffers sized) and every later full block is one graph launch -- the gaps between ~25 dependent launches
        # per iteration shrink from the host's launch path to the device's own.  Needs the scratch arena (the evaluation's
        # temporaries must sit where they sat when recorded); anything that cannot be recorded falls back to plain launches.
        graph = None
        use_graph = (self.tuning.get('cg_graph', False) and getattr(self, '_scratch', None) is not None and every % 2 == 0
                     and maxiter >= 3 * every and getattr(self, 'trace', None) is None and not getattr(self, '_prof_on', False))
        try:
            while it < maxiter and not done:
                nblk = min(every, maxiter - it)
                if use_graph and nblk == every and it % every == 0 and it >= every:
                    if graph is None:
                        try:
                            self._check(L.ig_graph_begin(ctx), "ig_graph_begin")
                            for j in range(every):
                                iteration(it + j)
                            g = ctypes.c_void_p()
                            self._check(L.ig_graph_end(ctx, ctypes.byref(g)), "ig_graph_end")
                            graph = g
                        except Exception as e:          # noqa: BLE001 -- e.g. a leaf that synchronises: this solve runs on plain launches
                            L.ig_graph_abort(ctx)
                            log.info("cg: the iteration cannot be recorded as a graph (%s); plain launches", e)
                            use_graph = False
                            continue
                    self._check(L.ig_graph_launch(graph), "ig_graph_launch")
                else:
                    for j in range(nblk):
                        iteration(it + j)
                it += nblk
                self._check(L.ig_scalar_read(ctx, S(HIST), it - fetched, host), "ig_scalar_read")       # (the block's only synchronisation)
                for j in range(it - fetched):
                    history.append(float(np.sqrt(host[j])))
                    log.info("iter %d, residual %g", fetched + j, history[-1])
                    if history[-1] < tol:
                        log.info("cg reached tolerance")
                        done = True
                        break
                fetched = it
        finally:
            if graph is not None:
                self.barrier()
                L.ig_graph_destroy(graph)
        if not done:
            log.info("cg reached maxiter")
        if not x_dev:
            x.copy_to(x_h)
        return history

    @staticmethod
    def _split_identity(A, lamda):
        """(A', lamda') with A + lamda I = A' + lamda' I: examples/pics.py:195 puts the Tikhonov term INTO the operator
        ((A.H * A) + lamda * Eye), which costs an axpby per evaluation; a real multiple of Eye at the root of the tree is
        moved into cg's own lamda instead, where ig_cg_dot adds it on the pass that reads p and Ap anyway."""
        from indigo_amd.operators import Sum, Scale, Eye
        if isinstance(A, Sum):
            for k in (0, 1):
                c = A._children[k]
                if isinstance(c, Scale) and isinstance(c.child, Eye) and np.imag(c._val) == 0:
                    return A._children[1 - k], lamda + float(np.real(c._val))
        return A, lamda

    def max(self, val, arr):
        """elementwise max on the real and imaginary parts independently"""
        assert arr.dtype == _C64 and arr.contiguous
        self._check(self._L.ig_cmax(self._ctx, arr.size * 2, ctypes.c_float(val), ctypes.c_void_p(arr._arr)), "ig_cmax")

    # -- FFT --------------------------------------------------------------------------------
    def _get_or_create_plan(self, x_shape):
        x_shape = tuple(int(s) for s in x_shape)
        if x_shape not in self._plans:
            dims = x_shape[:-1]
            assert 1 <= len(dims) <= 3, "FFT rank must be 1, 2 or 3"
            c_dims = (ctypes.c_int64 * len(dims))(*dims)
            plan, ws = ctypes.c_void_p(), ctypes.c_size_t()
            self._check(self._L.ig_fft_plan(self._ctx, len(dims), c_dims, x_shape[-1],
                                            ctypes.byref(plan), ctypes.byref(ws)), "ig_fft_plan%s" % (x_shape,))
            ws_in = ctypes.c_size_t()
            self._check(self._L.ig_fft_inplace_workspace(plan, ctypes.byref(ws_in)), "ig_fft_inplace_workspace")
            self._plans[x_shape] = (plan, ws.value, ws_in.value)
        return self._plans[x_shape]

    def _fft_workspace_size(self, x_shape):
        """bytes of scratch an UnscaledFFT of this shape may take (operators.UnscaledFFT._mem_usage / ScratchUsage): the
        in-place figure, so that a tree sized by it never allocates inside an evaluation"""
        return self._get_or_create_plan(x_shape)[2]

    def fft_describe(self, x_shape):
        plan = self._get_or_create_plan(x_shape)[0]
        buf = ctypes.create_string_buffer(1024)
        self._check(self._L.ig_fft_describe(plan, buf, 1024), "ig_fft_describe")
        return buf.value.decode()

    def _fft(self, y, x, direction):
        assert x.dtype == _C64 and y.dtype == _C64, "only complex64 is supported"
        assert x.shape == y.shape and x.contiguous and y.contiguous
        plan, ws, ws_inplace = self._get_or_create_plan(x.shape)
        if x._arr == y._arr:
            ws = ws_inplace
        if ws and getattr(self, '_scratch', None) is None:
            # no arena reserved (a bare fftn / ifftn call, not an operator tree): a grow-only workspace kept by the backend --
            # allocating, zeroing and freeing 9 GB per call (the chirp-z columns of a 640 x 277 x 410 x 8 transform) cost 50x
            # the transform.  The kernels write every element of it before they read it.
            tmp = getattr(self, '_fft_ws', None)
            if tmp is None or tmp.nbytes < ws:
                self._fft_ws = None
                tmp = self._fft_ws = self.empty_array((int(ws) // 8,), _C64, name='fft workspace')
            rc = self._L.ig_fft_exec(plan, ctypes.c_void_p(x._arr), ctypes.c_void_p(y._arr), direction, ctypes.c_void_p(tmp._arr))
        elif ws:
            with self.scratch(nbytes=ws) as tmp:
                rc = self._L.ig_fft_exec(plan, ctypes.c_void_p(x._arr), ctypes.c_void_p(y._arr), direction,
                                         ctypes.c_void_p(tmp._arr))
        else:
            rc = self._L.ig_fft_exec(plan, ctypes.c_void_p(x._arr), ctypes.c_void_p(y._arr), direction, None)
        self._check(rc, "ig_fft_exec")

    # fused zero-pad / crop transforms (operators.ZpadFFT)
    PADDED_AXES_POW2 = (256, 512)

    def support_words(self, n):
        """(zw_in, zw_out) of an axis the library has a zero-pad-aware z pass for (ig_fft_support_words: 256 and 512 through the
        power-of-two kernel, every length 128 ... 640 with factors 2, 3, 5, 7 that splits as A x B, A, B <= 32, through the A x B
        kernel, lengths with a larger prime factor through the chirp-z kernel over an A x B length), else None."""
        if not self.tuning.get('support_chirp', True) and self.padded_axis_kind(n) == 5:
            return None          # (lab switch: a chirp-z grid without its table, as in round 4)
        zi, zo = ctypes.c_int(), ctypes.c_int()
        if self._L.ig_fft_support_words(int(n), ctypes.byref(zi), ctypes.byref(zo)) != 0:
            return None
        return zi.value, zo.value

    def padded_axis_kind(self, n):
        """3 = power-of-two kernel, 4 = A x B kernel, 5 = chirp-z over an A x B length, 0 = no zero-pad-aware pass (ig_fft_padded_axis_kind)"""
        k = ctypes.c_int(0)
        self._check(self._L.ig_fft_padded_axis_kind(int(n), ctypes.byref(k)), "ig_fft_padded_axis_kind")
        return k.value

    def supports_padded_fft(self, grid, ncoils=None):
        """256- and 512-point axes in every grid layout; the reference driver's own oversampled grids (320 ... 640,
        examples/pics.py:87-90), every other smooth length from 128 to 640 and chirp-z y / z axes in the coil-interleaved layout --
        for ANY coil count: indigo_amd.fused.plan_chunks cuts it into interleaved chunks of 8, 4 and 2 coils, the last one
        padded with zero-weight coils where the count does not divide"""
        if len(grid) != 3:
            return False
        if all(int(n) in self.PADDED_AXES_POW2 for n in grid):
            return True
        kinds = [self.padded_axis_kind(n) for n in grid]
        # (5 = chirp-z: lengths with a prime factor above 7 -- 277, 410: int(N * osf) of the reference's driver -- on the y and z axes)
        return kinds[0] in (3, 4) and all(k in (3, 4, 5) for k in kinds[1:])

    def fold_axis_shifts(self, grid, phases):
        """Which axes' modulation the zero-padded / cropped transform of `grid` can carry itself (round 6).  `phases`: per-axis arrays
        ph with the k-space modulation exp(2 pi i (ph_x[kx] + ph_y[ky] + ph_z[kz])) that the gridding matrix would otherwise hold
        (Backend.fftc_mod, indigo/backends/backend.py:352-366).  On an ODD y or z axis that is linear in k with slope c / n, c = n // 2:
        a circular shift by c on the image side, which a chirp-z axis takes into its tables for nothing (ig_fft_set_axis_shift).
        Returns (shifts, phases') -- the shift per axis and the phases with those axes' terms replaced by their constant, so that
        the matrix built from phases' has real weights times one complex constant -- or (None, None) when no axis qualifies."""
        if not self.tuning.get('fold_odd_axes', True) or phases is None or len(grid) != 3:
            return None, None
        shifts, out = [0, 0, 0], [np.asarray(ph, dtype=np.float64) for ph in phases]
        for a in (1, 2):
            n = int(grid[a])
            ph = out[a]
            kind = ctypes.c_int(0)
            if n % 2 == 0 or ph.size != n or self._L.ig_fft_padded_axis_kind(n, ctypes.byref(kind)) != 0 or kind.value != 5:
                continue
            slope = (ph[1:] - ph[:-1]) * n                    # c for a linear phase (any constant offset)
            c = int(round(float(slope[0]))) % n
            lin = ph[0] + np.arange(n) * (c / n)
            d = (ph - lin)
            if c == 0 or np.abs(d - np.round(d)).max() > 1e-9:          # (whole turns do not matter)
                continue
            shifts[a] = c
            out[a] = np.full(n, ph[0])
        return (tuple(shifts), out) if any(shifts) else (None, None)

    def split_gridding_constant(self, phases):
        """(g, phases') with exp(2 pi i sum phases) = g * exp(2 pi i sum phases'), |g| = 1, and exp(2 pi i phases'_d[k]) = +-1 on every
        axis -- when the modulation is a sign per axis times a constant (every even axis of a centred transform: the constant is 1 for
        lengths divisible by four, -+i otherwise; a folded odd axis: its constant phase), and the constant is not 1.  The fused leaf then
        builds its gridding matrix from phases' -- REAL weights: 8-byte entries, 4-byte gather values, records with gconst = 1 -- and
        multiplies g into the per-voxel weights of the transform to its right, which are complex anyway.  (1, None) otherwise."""
        from indigo_amd.interp import _axis_signs
        if not self.tuning.get('real_gridding', True) or phases is None:
            return 1.0, None
        g, out = 1.0 + 0.0j, []
        for ph in phases:
            gs = _axis_signs(ph)
            if gs is None:
                return 1.0, None
            g *= gs[0]
            ph = np.asarray(ph, dtype=np.float64)
            out.append(ph - ph[0])
        if abs(g - 1.0) < 1e-12:
            return 1.0, None
        return complex(g), out

    def supports_single_coil_layout(self, grid):
        """the per-coil grid layouts (one coil per panel column: a left-over single coil runs without a padding coil) exist for
        power-of-two grids only"""
        return len(grid) == 3 and all(int(n) in self.PADDED_AXES_POW2 for n in grid)

    supports_support_tile = True          # ZpadFFT / the brick scatter take support tables of 8 or 4 kx points per entry

    def _padded_plan(self, grid, box_lo, box_dims, batch, layout=0, support_tile=16, kshift=None):
        kshift = tuple(int(v) for v in kshift) if kshift is not None else (0, 0, 0)
        key = ('padded', tuple(grid), tuple(box_lo), tuple(box_dims), int(batch), int(layout), int(support_tile), kshift)
        if key not in self._plans:
            a3 = ctypes.c_int64 * 3
            plan, ws = ctypes.c_void_p(), ctypes.c_size_t()
            self._check(self._L.ig_fft_plan_padded(self._ctx, a3(*grid), a3(*box_lo), a3(*box_dims), int(batch),
                                                   int(layout), ctypes.byref(plan), ctypes.byref(ws)),
                        "ig_fft_plan_padded%s" % (key,))
            try:
                if int(support_tile) != 16:
                    self._check(self._L.ig_fft_set_support_tile(plan, int(support_tile)), "ig_fft_set_support_tile")
                for axis, c in enumerate(kshift):          # (round 6) the centred transform's modulation of an odd chirp-z axis, carried by its passes
                    if c:
                        self._check(self._L.ig_fft_set_axis_shift(plan, axis, int(c)), "ig_fft_set_axis_shift(axis %d, %d)" % (axis, c))
            except Exception:
                self._L.ig_fft_destroy(plan)               # not in self._plans yet: nobody else would free it
                raise
            self._plans[key] = (plan, ws.value)
        return self._plans[key]

    def _fft_padded_workspace(self, grid, box_lo, box_dims, batch, layout=0):
        return self._padded_plan(grid, box_lo, box_dims, batch, layout)[1]

    @staticmethod
    def _slab(slab):
        """'z' or (z0, z1) -> the (phase, z0, z1) of the ig_fft_exec_cropped*_slab calls"""
        return (0, 0, 0) if slab == 'z' else (1, int(slab[0]), int(slab[1]))

    def fft_padded(self, y, x, w, grid, box_lo, box_dims, workspace=None, layout=0, support=None, support_tile=16, kshift=None):
        C = y.shape[1]
        assert y.dtype == _C64 and x.dtype == _C64 and y.contiguous and x.contiguous
        assert y.shape[0] == int(np.prod(grid)) and x.size == int(np.prod(box_dims))
        assert w is None or (w.contiguous and w.size == x.size * C)
        plan, ws = self._padded_plan(grid, box_lo, box_dims, C, layout, support_tile, kshift)
        assert layout == 0 or (workspace is not None and workspace.nbytes >= ws)
        self._check(self._L.ig_fft_exec_padded(plan, _ptr(x), 0, _ptr(w), _ptr(y), _ptr(workspace), _ptr(support)), "ig_fft_exec_padded")

    def ifft_cropped(self, xc, y, w, grid, box_lo, box_dims, workspace, layout=0, support=None, support_tile=16, slab=None, kshift=None):
        """xc[:, c] = conj(w[:, c]) * crop(IFFT(y[:, c])).  slab (grid layout 1 only): 'z' = only the z pass; (z0, z1) = the y and x
        passes of the image planes z0..z1-1 (after one 'z' call) -- the one-coil ranks of a coil-sharded run all-reduce finished
        slabs while later ones are transformed"""
        C = y.shape[1]
        assert y.dtype == _C64 and xc.dtype == _C64 and y.contiguous and xc.contiguous
        assert xc.shape == (int(np.prod(box_dims)), C) and (layout != 2 or xc.contiguous)
        plan, ws = self._padded_plan(grid, box_lo, box_dims, C, layout, support_tile, kshift)
        assert workspace.nbytes >= ws
        if slab is not None:
            assert layout == 1
            self._check(self._L.ig_fft_exec_cropped_slab(plan, _ptr(y), _ptr(w), _ptr(xc), xc.shape[0], _ptr(workspace), _ptr(support), *self._slab(slab)),
                        "ig_fft_exec_cropped_slab")
            return
        self._check(self._L.ig_fft_exec_cropped(plan, _ptr(y), _ptr(w), _ptr(xc), xc.shape[0], _ptr(workspace), _ptr(support)), "ig_fft_exec_cropped")

    def ifft_cropped_sum(self, x, y, w, grid, box_lo, box_dims, workspace, support=None, slab=None, support_tile=16, kshift=None):
        """x = sum_c conj(w[:, c]) * crop(IFFT(y[:, c])) for a coil-interleaved grid panel y (layout 2): the cropped
        transform with the coil combination folded into its last pass.
        slab: None = everything; 'z' = only the z pass; (z0, z1) = the y and x passes of the image planes z0..z1-1
        (after one 'z' call; lets a multi-GPU caller all-reduce finished slabs while later ones are transformed)"""
        C = y.shape[1]
        assert y.dtype == _C64 and x.dtype == _C64 and y.contiguous and x.contiguous and w is not None
        assert x.size == int(np.prod(box_dims))
        plan, ws = self._padded_plan(grid, box_lo, box_dims, C, 2, support_tile, kshift)
        assert workspace.nbytes >= ws
        if slab is None:
            self._check(self._L.ig_fft_exec_cropped_sum(plan, _ptr(y), _ptr(w), _ptr(x), _ptr(workspace), _ptr(support)), "ig_fft_exec_cropped_sum")
            return
        self._check(self._L.ig_fft_exec_cropped_sum_slab(plan, _ptr(y), _ptr(w), _ptr(x), _ptr(workspace), _ptr(support), *self._slab(slab)),
                    "ig_fft_exec_cropped_sum_slab")

    def sum_columns(self, y, X, alpha=1, beta=0, interleaved=False):
        assert y.dtype == _C64 and X.dtype == _C64 and y.contiguous and y.size == X.shape[0]
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        if interleaved:
            assert X.contiguous
            self._check(self._L.ig_csum_il(self._ctx, X.shape[0], X.shape[1], ctypes.c_void_p(X._arr),
                                           ar, ai, br, bi, ctypes.c_void_p(y._arr)), "ig_csum_il")
            return
        self._check(self._L.ig_csum_cols(self._ctx, X.shape[0], X.shape[1], ctypes.c_void_p(X._arr), X._leading_dim,
                                         ar, ai, br, bi, ctypes.c_void_p(y._arr)), "ig_csum_cols")

    def permute3(self, y, x, dims, perm, alpha=1, beta=0):
        """Backend.permute3 on the device (ig_permute3_c64): panels of any column count with their leading dimensions"""
        assert x.dtype == _C64 and y.dtype == _C64, "only complex64 is supported"
        n0, n1, n2 = (int(n) for n in dims)
        n = n0 * n1 * n2
        assert x.shape[0] == n and y.shape[0] == n and x.size == y.size, (x.shape, y.shape, dims)
        ncols = x.shape[1] if x.ndim == 2 else 1
        p = (ctypes.c_int * 3)(*(int(v) for v in perm))
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_permute3_c64(self._ctx, n0, n1, n2, p, ncols, ctypes.c_void_p(x._arr), x._leading_dim,
                                            ar, ai, br, bi, ctypes.c_void_p(y._arr), y._leading_dim), "ig_permute3_c64")

    def dwt3(self, y, x, dims, wavelet, levels, inverse=False, alpha=1, beta=0):
        """Backend.dwt3 on the device (ig_dwt3_c64): panels of any column count with their leading dimensions, or the columns
        stacked in one vector, as the host form takes them; y may be x"""
        assert x.dtype == _C64 and y.dtype == _C64, "only complex64 is supported"
        n0, n1, n2 = (int(n) for n in dims)
        n = n0 * n1 * n2
        assert n > 0 and x.size % n == 0 and x.size == y.size, (x.shape, y.shape, dims)
        ncols = x.size // n
        (xp, ldx), (yp, ldy) = self._frame_panel(x, n, ncols), self._frame_panel(y, n, ncols)
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_dwt3_c64(self._ctx, n0, n1, n2, WAVELET_IDS[wavelet], int(levels), int(bool(inverse)), ncols,
                                        xp, ldx, ar, ai, br, bi, yp, ldy), "ig_dwt3_c64")

    def soft_threshold(self, x, tau, dims, keep):
        """Backend.soft_threshold on the device (ig_csoft_c64), in place"""
        assert x.dtype == _C64, "only complex64 is supported"
        n0, n1, n2 = (int(n) for n in dims)
        assert x.shape[0] == n0 * n1 * n2, (x.shape, dims)
        ncols = x.shape[1] if x.ndim == 2 else 1
        c0, c1, c2 = (int(c) for c in keep)
        self._check(self._L.ig_csoft_c64(self._ctx, n0, n1, n2, c0, c1, c2, ncols, ctypes.c_float(float(tau)),
                                         ctypes.c_void_p(x._arr), x._leading_dim), "ig_csoft_c64")

    @staticmethod
    def _frame_panel(a, rows, frames):
        """(pointer, leading dimension) of `a` as a rows x frames panel: a is that panel, or the (rows * frames, 1) vector"""
        if a.shape == (rows, frames):
            return ctypes.c_void_p(a._arr), a._leading_dim
        assert a.shape in ((rows * frames, 1), (rows * frames,)), (a.shape, rows, frames)
        return ctypes.c_void_p(a._arr), rows

    def _grad(self, y, x, dims, comps, ncols, adjoint, alpha, beta):
        """ig_grad3[h]_c64 (comps = 3) and ig_grad4[h]_c64 (comps = 4) on x and y as panels of ncols columns"""
        assert x.dtype == _C64 and y.dtype == _C64, "only complex64 is supported"
        n0, n1, n2 = (int(n) for n in dims)
        n = n0 * n1 * n2
        rows_x, rows_y = (comps * n, n) if adjoint else (n, comps * n)
        (xp, ldx), (yp, ldy) = self._frame_panel(x, rows_x, ncols), self._frame_panel(y, rows_y, ncols)
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        name = "ig_grad%d%s_c64" % (comps, "h" if adjoint else "")
        self._check(getattr(self._L, name)(self._ctx, n0, n1, n2, ncols, xp, ldx, ar, ai, br, bi, yp, ldy), name)

    def _tv_dual(self, u, xn, xo, sigma, radii, dims, ncols):
        """ig_tv_dual_c64 (radii = (mu,)) and ig_tv4_dual_c64 (radii = (mu, mu_t)) on xn, xo and u as panels of ncols columns"""
        assert u.dtype == _C64 and xn.dtype == _C64 and xo.dtype == _C64, "only complex64 is supported"
        n0, n1, n2 = (int(n) for n in dims)
        n = n0 * n1 * n2
        (np_, ldn), (op_, ldo), (up, ldu) = (self._frame_panel(xn, n, ncols), self._frame_panel(xo, n, ncols),
                                             self._frame_panel(u, (2 + len(radii)) * n, ncols))
        name = "ig_tv_dual_c64" if len(radii) == 1 else "ig_tv4_dual_c64"
        self._check(getattr(self._L, name)(self._ctx, n0, n1, n2, ncols, np_, ldn, op_, ldo, ctypes.c_float(float(sigma)),
                                           *(ctypes.c_float(float(r)) for r in radii), up, ldu), name)

    def grad3(self, y, x, dims, adjoint=False, alpha=1, beta=0):
        """Backend.grad3 on the device (ig_grad3_c64 / ig_grad3h_c64): panels of any column count with their leading dimensions"""
        self._grad(y, x, dims, 3, x.shape[1] if x.ndim == 2 else 1, adjoint, alpha, beta)

    def tv_dual_step(self, u, xn, xo, sigma, mu, dims):
        """Backend.tv_dual_step on the device (ig_tv_dual_c64), in place on u"""
        self._tv_dual(u, xn, xo, sigma, (mu,), dims, xn.shape[1] if xn.ndim == 2 else 1)

    def grad4(self, y, x, dims, frames, adjoint=False, alpha=1, beta=0):
        """Backend.grad4 on the device (ig_grad4_c64 / ig_grad4h_c64): the frames are the columns of a panel with its leading
        dimension, or stacked in one column"""
        self._grad(y, x, dims, 4, int(frames), adjoint, alpha, beta)

    def tv4_dual_step(self, u, xn, xo, sigma, mu, mu_t, dims, frames):
        """Backend.tv4_dual_step on the device (ig_tv4_dual_c64), in place on u"""
        self._tv_dual(u, xn, xo, sigma, (mu, mu_t), dims, int(frames))

    def symgrad3(self, y, v, dims, adjoint=False, alpha=1, beta=0):
        """Backend.symgrad3 on the device (ig_symgrad3_c64 / ig_symgrad3h_c64): panels of any column count with their leading
        dimensions, or the columns stacked in one vector"""
        assert v.dtype == _C64 and y.dtype == _C64, "only complex64 is supported"
        n0, n1, n2 = (int(n) for n in dims)
        n = n0 * n1 * n2
        rows_v, rows_y = (6 * n, 3 * n) if adjoint else (3 * n, 6 * n)
        assert n > 0 and v.size % rows_v == 0 and v.size // rows_v * rows_y == y.size, (v.shape, y.shape, dims)
        ncols = v.size // rows_v
        (vp, ldv), (yp, ldy) = self._frame_panel(v, rows_v, ncols), self._frame_panel(y, rows_y, ncols)
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        name = "ig_symgrad3%s_c64" % ("h" if adjoint else "")
        self._check(getattr(self._L, name)(self._ctx, n0, n1, n2, ncols, vp, ldv, ar, ai, br, bi, yp, ldy), name)

    def _tgv_panels(self, dims, first, *rest):
        """(n0, n1, n2, ncols) and the (pointer, leading dimension) pairs of complex64 panels given as (array, rows / N): the column
        count is that of the first"""
        n0, n1, n2 = (int(n) for n in dims)
        n = n0 * n1 * n2
        assert n > 0 and first[0].size % (first[1] * n) == 0, (first[0].shape, dims)
        ncols = first[0].size // (first[1] * n)
        flat = []
        for a, comps in (first,) + rest:
            assert a.dtype == _C64, "only complex64 is supported"
            assert a.size == comps * n * ncols, (a.shape, comps, dims, ncols)
            flat.extend(self._frame_panel(a, comps * n, ncols))
        return (n0, n1, n2, ncols), flat

    def tgv_adjoint(self, gx, gv, p, q, dims):
        """Backend.tgv_adjoint on the device (ig_tgv_kh_c64): gx += D^H p and gv = E^H q - p in one pass"""
        head, panels = self._tgv_panels(dims, (p, 3), (q, 6), (gx, 1), (gv, 3))
        self._check(self._L.ig_tgv_kh_c64(self._ctx, *head, *panels), "ig_tgv_kh_c64")

    def tgv_dual_step(self, p, q, xn, xo, vn, vo, sigma, a1, a0, dims):
        """Backend.tgv_dual_step on the device (ig_tgv_dual_c64), in place on p and q"""
        head, ins = self._tgv_panels(dims, (xn, 1), (xo, 1), (vn, 3), (vo, 3))
        same, outs = self._tgv_panels(dims, (p, 3), (q, 6))
        assert same == head, (p.shape, xn.shape, dims)
        self._check(self._L.ig_tgv_dual_c64(self._ctx, *head, *ins, ctypes.c_float(float(sigma)), ctypes.c_float(float(a1)),
                                            ctypes.c_float(float(a0)), *outs), "ig_tgv_dual_c64")

    def _llr_args(self, x, dims, frames, block, shift):
        """the leading arguments of ig_llr_svt_c64 / ig_llr_nuc_c64, the panel pointer and its leading dimension, and nb"""
        assert x.dtype == _C64, "only complex64 is supported"
        dims = tuple(int(n) for n in dims)
        T = int(frames)
        xp, ldx = self._frame_panel(x, int(np.prod(dims)), T)
        block = tuple(int(b) for b in block)
        nb = int(np.prod([-(-n // max(1, min(b, n))) for n, b in zip(dims, block)]))
        return dims + (T,) + block + tuple(int(s) for s in shift), xp, ldx, nb

    def llr_threshold(self, x, tau, dims, frames, block, shift=(0, 0, 0)):
        """Backend.llr_threshold on the device (ig_llr_svt_c64), in place: the frames are the columns of a panel with its
        leading dimension, or stacked in one column"""
        head, xp, ldx, _ = self._llr_args(x, dims, frames, block, shift)
        self._check(self._L.ig_llr_svt_c64(self._ctx, *head, ctypes.c_float(float(tau)), xp, ldx), "ig_llr_svt_c64")

    def llr_norm(self, x, dims, frames, block, shift=(0, 0, 0)):
        """Backend.llr_norm on the device (ig_llr_nuc_c64): the blocks' nuclear norms as floats, summed on the host in float64"""
        return float(self.llr_block_norms(x, dims, frames, block, shift).astype(np.float64).sum())

    def llr_block_norms(self, x, dims, frames, block, shift=(0, 0, 0)):
        """the nuclear norm of every block's matrix (ig_llr_nuc_c64): nb float32 on the host, blocks numbered F-order"""
        head, xp, ldx, nb = self._llr_args(x, dims, frames, block, shift)
        nuc = self.zero_array((max(nb, 1), 1), np.dtype('float32'), name='llr.nuc')
        self._check(self._L.ig_llr_nuc_c64(self._ctx, *head, xp, ldx, ctypes.c_void_p(nuc._arr)), "ig_llr_nuc_c64")
        return nuc.to_host().ravel()[:nb]

    def frame_basis(self, y, x, phi, n, adjoint=False, alpha=1, beta=0):
        """Backend.frame_basis on the device (ig_basis_c64): the images and the frames are the columns of panels with their
        leading dimensions, or stacked in one column"""
        assert x.dtype == _C64 and y.dtype == _C64 and phi.dtype == _C64, "only complex64 is supported"
        assert phi.ndim == 2, phi.shape
        n, (T, K) = int(n), phi.shape
        cols_x, cols_y = (T, K) if adjoint else (K, T)
        (xp, ldx), (yp, ldy) = self._frame_panel(x, n, cols_x), self._frame_panel(y, n, cols_y)
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_basis_c64(self._ctx, n, K, T, ctypes.c_void_p(phi._arr), phi._leading_dim, int(bool(adjoint)),
                                         xp, ldx, ar, ai, br, bi, yp, ldy), "ig_basis_c64")

    def segment_phase(self, y, x, f, tau0, dtau, L, n, adjoint=False, alpha=1, beta=0):
        """Backend.segment_phase on the device (ig_fmap_phase_c64): the image and its segments are the columns of panels with their
        leading dimensions, or stacked in one column"""
        assert x.dtype == _C64 and y.dtype == _C64 and f.dtype == np.dtype('float32'), "complex64 panels and a float32 field map"
        n, L = int(n), int(L)
        assert f.size == n and f.contiguous, (f.shape, n)
        cols_x, cols_y = (L, 1) if adjoint else (1, L)
        (xp, ldx), (yp, ldy) = self._frame_panel(x, n, cols_x), self._frame_panel(y, n, cols_y)
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_fmap_phase_c64(self._ctx, n, L, ctypes.c_void_p(f._arr), ctypes.c_double(float(tau0)),
                                              ctypes.c_double(float(dtau)), int(bool(adjoint)), xp, ldx, ar, ai, br, bi, yp, ldy),
                    "ig_fmap_phase_c64")

    def segment_combine(self, y, x, b, period, n, adjoint=False, alpha=1, beta=0):
        """Backend.segment_combine on the device (ig_fmap_combine_c64): the samples and the segments' samples are the columns of
        panels with their leading dimensions, or stacked in one column"""
        assert x.dtype == _C64 and y.dtype == _C64 and b.dtype == _C64, "only complex64 is supported"
        assert b.ndim == 2 and b.shape[0] == int(period), (b.shape, period)
        n, (P, L) = int(n), b.shape
        cols_x, cols_y = (1, L) if adjoint else (L, 1)
        (xp, ldx), (yp, ldy) = self._frame_panel(x, n, cols_x), self._frame_panel(y, n, cols_y)
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_fmap_combine_c64(self._ctx, n, L, P, ctypes.c_void_p(b._arr), b._leading_dim, int(bool(adjoint)),
                                                xp, ldx, ar, ai, br, bi, yp, ldy), "ig_fmap_combine_c64")

    def fieldmap_init(self, f, y, dims, te):
        """Backend.fieldmap_init on the device (ig_fmapest_init_r32): the echo images are the columns of a panel with its leading
        dimension, or stacked in one column"""
        dims, n, E, te, _ = self.fieldmap_check("fieldmap_init", dims, y, te, (f,))
        yp, ldy = self._frame_panel(y, n, E)
        self._check(self._L.ig_fmapest_init_r32(self._ctx, *dims, yp, ldy, ctypes.c_double(te[0]), ctypes.c_double(te[1]),
                                                ctypes.c_void_p(f._arr)), "ig_fmapest_init_r32")

    def fieldmap_step(self, f_new, f_old, y, te, beta, dims, cost=False):
        """Backend.fieldmap_step on the device (ig_fmapest_step_r32).  cost=True: the same pass writes one double per workgroup,
        which come back and are added here in index order"""
        dims, n, E, te, beta = self.fieldmap_check("fieldmap_step", dims, y, te, (f_new, f_old), beta)
        return self._fieldmap_launch(f_new, f_old, y, te, beta, dims, n, E, cost)

    def fieldmap_cost(self, f, y, te, beta, dims):
        """Backend.fieldmap_cost on the device (ig_fmapest_step_r32 without f_new: the cost alone)"""
        dims, n, E, te, beta = self.fieldmap_check("fieldmap_cost", dims, y, te, (f,), beta)
        return self._fieldmap_launch(None, f, y, te, beta, dims, n, E, True)

    def _fieldmap_launch(self, f_new, f_old, y, te, beta, dims, n, E, cost):
        yp, ldy = self._frame_panel(y, n, E)
        parts, nparts = None, 0
        if cost:
            nparts = int(self._L.ig_fmapest_cost_parts(*dims))
            parts = getattr(self, '_fmapest_parts', None)
            if parts is None or parts.size < nparts:
                parts = self._fmapest_parts = self.empty_array((nparts,), np.dtype('float64'), name='fmapest.parts')
        self._check(self._L.ig_fmapest_step_r32(self._ctx, *dims, E, yp, ldy, ctypes.c_void_p(te.ctypes.data), ctypes.c_float(beta),
                                                ctypes.c_void_p(f_old._arr), ctypes.c_void_p(f_new._arr) if f_new is not None else None,
                                                ctypes.c_void_p(parts._arr) if cost else None, parts.size if cost else 0),
                    "ig_fmapest_step_r32")
        if not cost:
            return None
        total = 0.0
        for v in parts.to_host().reshape(-1)[:nparts].tolist():     # a fixed order: the same bits from call to call
            total += v
        return total

    def coil_maps(self, y, x, maps, n, ncoils, nmaps, adjoint=False, alpha=1, beta=0, interleaved=False, width=None):
        """Backend.coil_maps on the device (ig_coil_maps_c64): the images and the coil-major coil images are the columns of panels
        with their leading dimensions, or stacked in one column; interleaved coil images are one contiguous array"""
        assert x.dtype == _C64 and y.dtype == _C64 and maps.dtype == _C64, "only complex64 is supported"
        n, C, M = int(n), int(ncoils), int(nmaps)
        w = int(width) if (interleaved and width is not None) else C
        assert maps.contiguous and maps.size == n * w * M, (maps.shape, n, w, M)
        img, coil = (y, x) if adjoint else (x, y)
        ip, ldi = self._frame_panel(img, n, M)
        if interleaved:
            assert coil.contiguous and coil.size == n * w, (coil.shape, n, w)
            cp, sg, sc = ctypes.c_void_p(coil._arr), w, 1
        else:
            cp, sc = self._frame_panel(coil, n, C)
            sg = 1
        xp, yp = (cp, ip) if adjoint else (ip, cp)
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_coil_maps_c64(self._ctx, n, C, M, ctypes.c_void_p(maps._arr), int(bool(adjoint)), xp, ar, ai, br, bi,
                                             yp, ldi, sg, sc), "ig_coil_maps_c64")

    def nlinv_product(self, y, x, rho, coils, n, ncoils, adjoint=False, alpha=1, beta=0):
        """Backend.nlinv_product on the device (ig_nlinv_product_c64): the coils, x and y are the columns of panels with their
        leading dimensions, or stacked in one column"""
        assert x.dtype == _C64 and y.dtype == _C64 and rho.dtype == _C64 and coils.dtype == _C64, "only complex64 is supported"
        n, C = int(n), int(ncoils)
        assert rho.size == n and rho.contiguous, (rho.shape, n)
        cols_x, cols_y = (C, 1 + C) if adjoint else (1 + C, C)
        (cp, ldc), (xp, ldx), (yp, ldy) = self._frame_panel(coils, n, C), self._frame_panel(x, n, cols_x), self._frame_panel(y, n, cols_y)
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_nlinv_product_c64(self._ctx, n, C, ctypes.c_void_p(rho._arr), cp, ldc, int(bool(adjoint)), xp, ldx,
                                                 ar, ai, br, bi, yp, ldy), "ig_nlinv_product_c64")

    def sobolev_weight(self, y, x, dims, ncols, a, b, scale=1.0):
        """Backend.sobolev_weight on the device (ig_sobolev_weight_c64): the panels with their leading dimensions, or stacked in
        one column; y may be x"""
        assert x.dtype == _C64 and y.dtype == _C64, "only complex64 is supported"
        n0, n1, n2 = (int(n) for n in dims)
        n, ncols = n0 * n1 * n2, int(ncols)
        (xp, ldx), (yp, ldy) = self._frame_panel(x, n, ncols), self._frame_panel(y, n, ncols)
        self._check(self._L.ig_sobolev_weight_c64(self._ctx, n0, n1, n2, ncols, ctypes.c_double(float(a)), ctypes.c_double(float(b)),
                                                  ctypes.c_double(float(scale)), xp, ldx, yp, ldy), "ig_sobolev_weight_c64")

    def place_wrapped(self, vol, box, dims, box_dims):
        """Backend.place_wrapped on the device (ig_place_wrapped_c64): the volumes are the columns of a panel with its leading
        dimension, or stacked in one column; the boxes are one dense array"""
        assert vol.dtype == _C64 and box.dtype == _C64, "only complex64 is supported"
        dims, box_dims = tuple(int(n) for n in dims), tuple(int(b) for b in box_dims)
        N, nb = int(np.prod(dims)), int(np.prod(box_dims))
        ncols = box.size // max(nb, 1)
        assert box.contiguous and box.size == nb * ncols, (box.shape, box_dims)
        vp, ld = self._frame_panel(vol, N, ncols)
        self._check(self._L.ig_place_wrapped_c64(self._ctx, *dims, ncols, *box_dims, ctypes.c_void_p(box._arr), vp, ld), "ig_place_wrapped_c64")

    def espirit_eig(self, maps, evals, gram, n, ncoils, nmaps, iters=30, crop=0.8):
        """Backend.espirit_eig on the device (ig_espirit_eig_c64): the three panels with their leading dimensions, or stacked in one column"""
        assert gram.dtype == _C64 and maps.dtype == _C64 and evals.dtype == np.dtype('float32'), "complex64 panels and float32 eigenvalues"
        n, C, M = int(n), int(ncoils), int(nmaps)
        (gp, ldg), (mp, ldm), (ep, lde) = (self._frame_panel(gram, n, C * (C + 1) // 2), self._frame_panel(maps, n, C * M),
                                           self._frame_panel(evals, n, M))
        self._check(self._L.ig_espirit_eig_c64(self._ctx, n, C, M, int(iters), ctypes.c_float(float(crop)), gp, ldg, mp, ldm, ep, lde),
                    "ig_espirit_eig_c64")

    def coil_gram_parts(self, x, n, ncoils, slab=None):
        """the partial Gram matrices of ig_coil_gram_c64 on the host: ceil(n / slab) rows (row j: the samples [j slab, (j + 1) slab))
        of C (C + 1) / 2 complex64 columns, the row-wise upper triangle (`espirit_unpack`)"""
        assert x.dtype == _C64, "only complex64 is supported"
        n, C = int(n), int(ncoils)
        slab = self.tuning['gram_slab'] if slab is None else int(slab)
        xp, ldx = self._frame_panel(x, n, C)
        rows = max(1, -(-n // max(slab, 1)))
        parts = self.empty_array((rows, C * (C + 1) // 2), _C64, name='cc.parts')
        self._check(self._L.ig_coil_gram_c64(self._ctx, n, C, xp, ldx, slab, ctypes.c_void_p(parts._arr), parts._leading_dim), "ig_coil_gram_c64")
        return parts.to_host()

    def coil_gram(self, x, n, ncoils, slab=None):
        """Backend.coil_gram on the device (ig_coil_gram_c64): one partial sum per slab of `slab` samples (default
        tuning['gram_slab']), the rows added on the host in float64"""
        C = int(ncoils)
        parts = self.coil_gram_parts(x, n, C, slab)
        total = np.add.reduce(parts, axis=0, dtype=np.complex128)
        return self.espirit_unpack(total.reshape((1, -1)), 1, C)[0]

    def dict_match(self, x, atoms, n, chunk=None):
        """Backend.dict_match on the device (ig_dict_match_c64): the coefficient images are the columns of a panel with its leading
        dimension, or stacked in one column; one launch for all n voxels (`chunk` has no meaning here)"""
        assert x.dtype == _C64 and atoms.dtype == _C64, "only complex64 is supported"
        assert atoms.ndim == 2, atoms.shape
        n, (K, N) = int(n), atoms.shape
        xp, ldx = self._frame_panel(x, n, K)
        idx = self.empty_array((n, 1), np.dtype('int32'), name='dict.idx')
        ip = self.empty_array((n, 1), _C64, name='dict.ip')
        self._check(self._L.ig_dict_match_c64(self._ctx, n, K, N, xp, ldx, ctypes.c_void_p(atoms._arr), atoms._leading_dim,
                                              ctypes.c_void_p(idx._arr), ctypes.c_void_p(ip._arr)), "ig_dict_match_c64")
        return idx.to_host().ravel(), ip.to_host().ravel()

    def epg_signal(self, params, steps, flags, nstates, chunk=1 << 16):
        """Backend.epg_signal on the device (ig_epg_sim_c64): the parameters go up and the signals come down `chunk` atoms at a
        time; the program is handed over by host pointer with every call"""
        p, st, fl, K, nrec = self.epg_check(params, steps, flags, nstates)
        N, chunk = p.shape[0], max(1, int(chunk))
        out = np.empty((N, nrec), dtype=_C64)
        for i0 in range(0, N, chunk):
            n = min(chunk, N - i0)
            cols = [self.copy_array(np.asfortranarray(p[i0:i0 + n, c:c + 1]), name='epg.param') for c in range(3)]
            sig = self.empty_array((nrec, n), _C64, name='epg.signal')
            self._check(self._L.ig_epg_sim_c64(self._ctx, n, st.shape[0], K, *(ctypes.c_void_p(c._arr) for c in cols),
                                               ctypes.c_void_p(st.ctypes.data), ctypes.c_void_p(fl.ctypes.data),
                                               ctypes.c_void_p(sig._arr), sig._leading_dim), "ig_epg_sim_c64")
            out[i0:i0 + n] = sig.to_host().T
            del cols, sig
        return out

    def _dcf_args(self, what, w, records, sep, tiles):
        """(M, tw, records, stride, order) of the Pipe-Menon kernels' common arguments, checked"""
        f32, u32 = np.dtype('float32'), np.dtype('uint32')
        M, tw = int(w.size), int(sep['tw'])
        words = int(self._L.ig_interp3_sep_words(tw))
        stride = int(sep.get('stride') or words)
        assert w.dtype == f32 and w.contiguous, "%s: the weights are a contiguous float32 array" % what
        assert records.dtype == u32 and records.contiguous and records.size >= M * stride and stride >= words, (records.shape, M, stride)
        order = tiles['order']
        assert order.dtype == u32 and order.contiguous and order.size == M, (order.shape, M)
        return M, tw, ctypes.c_void_p(records._arr), stride, ctypes.c_void_p(order._arr)

    def dcf_spread(self, acc, w, records, sep, scale, tiles):
        """Backend.dcf_spread on the device (ig_dcf_spread_r32): one workgroup per non-empty tile of `tiles`; tiles of at least
        tuning['dcf_lds_min'] samples sum in LDS first, the others add straight to acc.  The same bits either way."""
        M, tw, rp, stride, op_ = self._dcf_args("dcf_spread", w, records, sep, tiles)
        dims = tuple(int(n) for n in sep['dims'])
        assert acc.dtype == np.dtype('int64') and acc.contiguous and acc.size == int(np.prod(dims)), (acc.shape, dims)
        ptr, ids = tiles['ptr'], tiles['ids']
        assert ptr.dtype == np.dtype('int64') and ids.dtype == np.dtype('int32') and ptr.contiguous and ids.contiguous, (ptr.dtype, ids.dtype)
        ntiles = int(ptr.size) - 1 if M else 0
        assert ids.size >= ntiles, (ids.shape, ptr.shape)
        lds_min = min(max(int(self.tuning['dcf_lds_min']), 0), 1 << 62)
        self._check(self._L.ig_dcf_spread_r32(self._ctx, M, tw, rp, stride, op_, ctypes.c_void_p(ptr._arr), ctypes.c_void_p(ids._arr), ntiles,
                                              ctypes.c_void_p(w._arr), ctypes.c_double(float(scale)), lds_min, ctypes.c_void_p(acc._arr), *dims),
                    "ig_dcf_spread_r32")

    def dcf_gather_div(self, w_out, acc, w, records, sep, scale, tiles, s_out=None):
        """Backend.dcf_gather_div on the device (ig_dcf_gather_div_r32): the two maxima come back as 8 bytes"""
        f32 = np.dtype('float32')
        M, tw, rp, stride, op_ = self._dcf_args("dcf_gather_div", w, records, sep, tiles)
        dims = tuple(int(n) for n in sep['dims'])
        assert acc.dtype == np.dtype('int64') and acc.contiguous and acc.size == int(np.prod(dims)), (acc.shape, dims)
        assert w_out.dtype == f32 and w_out.contiguous and w_out.size == M, (w_out.shape, M)
        assert s_out is None or (s_out.dtype == f32 and s_out.contiguous and s_out.size == M), (s_out.shape, M)
        if getattr(self, '_dcf_maxima', None) is None:
            self._dcf_maxima = self.zero_array((2,), f32, name='dcf.maxima')
        mx = self._dcf_maxima
        self._check(self._L.ig_dcf_gather_div_r32(self._ctx, M, tw, rp, stride, op_, ctypes.c_void_p(acc._arr), *dims, ctypes.c_double(float(scale)),
                                                  ctypes.c_void_p(w._arr), ctypes.c_void_p(w_out._arr),
                                                  ctypes.c_void_p(s_out._arr) if s_out is not None else None, ctypes.c_void_p(mx._arr)),
                    "ig_dcf_gather_div_r32")
        wmax, dev = mx.to_host()
        return float(wmax), float(dev)

    def row_scale(self, y, x, w, n, ncols):
        """Backend.row_scale on the device (ig_rowscale_r32_c64): the panels with their leading dimensions, or stacked in one
        column; y may be x"""
        assert x.dtype == _C64 and y.dtype == _C64 and w.dtype == np.dtype('float32'), "complex64 panels and float32 weights"
        n, C = int(n), int(ncols)
        assert w.size == n and w.contiguous, (w.shape, n)
        (xp, ldx), (yp, ldy) = self._frame_panel(x, n, C), self._frame_panel(y, n, C)
        self._check(self._L.ig_rowscale_r32_c64(self._ctx, n, C, ctypes.c_void_p(w._arr), xp, ldx, yp, ldy), "ig_rowscale_r32_c64")

    def psf_mix(self, y, x, kern, n, ncoils, interleaved=False, width=None):
        """Backend.psf_mix on the device (ig_psf_mix_c64): the K images are the columns of panels with their leading
        dimensions, or stacked in one column; y may be x"""
        assert x.dtype == _C64 and y.dtype == _C64 and kern.dtype == np.dtype('float32'), "complex64 panels and a float32 kernel array"
        n, C = int(n), int(ncoils)
        w = int(width) if (interleaved and width is not None) else C
        K = int(round(np.sqrt(kern.size // max(n, 1))))
        assert K * K * n == kern.size and kern.contiguous and w >= C, (kern.shape, n, C, w)
        rows = n * w
        (xp, ldx), (yp, ldy) = self._frame_panel(x, rows, K), self._frame_panel(y, rows, K)
        sg, sc = (w, 1) if interleaved else (1, n)
        self._check(self._L.ig_psf_mix_c64(self._ctx, n, C, K, ctypes.c_void_p(kern._arr), xp, ldx, yp, ldy, sg, sc), "ig_psf_mix_c64")

    def fftn(self, y, x):
        self._fft(y, x, -1)

    def ifftn(self, y, x):
        self._fft(y, x, +1)

    # -- SpMM -------------------------------------------------------------------------------
    def ccsrmm(self, y, A_shape, A_indx, A_ptr, A_vals, x, alpha=1, beta=0, adjoint=False, exwrite=False):
        m, k = A_shape
        n = x.shape[1]
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        rc = self._L.ig_ccsrmm(self._ctx, 1 if adjoint else 0, 1 if exwrite else 0, m, k, n, A_vals.size,
                               ar, ai, ctypes.c_void_p(A_vals._arr), ctypes.c_void_p(A_indx._arr),
                               ctypes.c_void_p(A_ptr._arr),
                               ctypes.c_void_p(x._arr), x._leading_dim, br, bi,
                               ctypes.c_void_p(y._arr), y._leading_dim)
        self._check(rc, "ig_ccsrmm")

    def ccsrmm_t(self, y, A_shape, At_indx, At_ptr, At_vals, x, alpha=1, beta=0, support=None, xperm=None):
        """y = alpha * A^H x + beta*y through the CSR of A^T (gather); `support` = (table, n0, nm) restricts
        the output rows to a grid support region (rows outside are left untouched)"""
        m, k = A_shape
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        if support is not None or xperm is not None:
            tab, n0, nm = support if support is not None else (None, 0, 0)
            rc = self._L.ig_ccsrmm_t_grid(self._ctx, m, k, x.shape[1], At_vals.size,
                                          ar, ai, ctypes.c_void_p(At_vals._arr), ctypes.c_void_p(At_indx._arr),
                                          ctypes.c_void_p(At_ptr._arr),
                                          ctypes.c_void_p(x._arr), x._leading_dim, br, bi,
                                          ctypes.c_void_p(y._arr), y._leading_dim,
                                          ctypes.c_void_p(tab._arr) if tab is not None else None, n0, nm,
                                          ctypes.c_void_p(xperm._arr) if xperm is not None else None)
            self._check(rc, "ig_ccsrmm_t_grid")
            return
        rc = self._L.ig_ccsrmm_t(self._ctx, m, k, x.shape[1], At_vals.size,
                                 ar, ai, ctypes.c_void_p(At_vals._arr), ctypes.c_void_p(At_indx._arr),
                                 ctypes.c_void_p(At_ptr._arr),
                                 ctypes.c_void_p(x._arr), x._leading_dim, br, bi,
                                 ctypes.c_void_p(y._arr), y._leading_dim)
        self._check(rc, "ig_ccsrmm_t")

    # -- ones / DIA / dense (outside the SENSE tree) ---------------------------------
    def onemm(self, y, x, alpha=1, beta=0):
        """y = beta*y + alpha * ones(M, K) * x"""
        assert x.dtype == _C64 and y.dtype == _C64 and x.shape[1] == y.shape[1]
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_conemm(self._ctx, y.shape[0], x.shape[0], x.shape[1], ar, ai, ctypes.c_void_p(x._arr), x._leading_dim,
                                      br, bi, ctypes.c_void_p(y._arr), y._leading_dim), "ig_conemm")

    def cdiamm(self, y, shape, offsets, data, x, alpha=1.0, beta=0.0, adjoint=True):
        assert x.dtype == _C64 and y.dtype == _C64 and data.dtype == _C64 and offsets.dtype == np.int32
        m, k = shape
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        self._check(self._L.ig_cdiamm(self._ctx, 1 if adjoint else 0, m, k, x.shape[1], offsets.size, ctypes.c_void_p(offsets._arr),
                                      ctypes.c_void_p(data._arr), data._leading_dim, ar, ai, ctypes.c_void_p(x._arr), x._leading_dim,
                                      br, bi, ctypes.c_void_p(y._arr), y._leading_dim), "ig_cdiamm")

    def cgemm(self, y, M, x, alpha=1, beta=0, forward=True, left=True):
        """y = beta*y + alpha * op(M) * x   (left)   or   beta*y + alpha * x * op(M)   (not left); op = identity / ^H"""
        assert x.dtype == _C64 and y.dtype == _C64 and M.dtype == _C64 and M.ndim == 2
        ar, ai = _cplx(alpha)
        br, bi = _cplx(beta)
        r, c = M.shape if forward else M.shape[::-1]
        if left:
            x2, y2 = x.reshape((c, -1)), y.reshape((r, -1))
            p = x2.shape[1]
        else:
            x2, y2 = x.reshape((-1, r)), y.reshape((-1, c))
            p = x2.shape[0]
        self._check(self._L.ig_cgemm(self._ctx, 0 if forward else 1, 0 if left else 1, M.shape[0], M.shape[1], p, ar, ai,
                                     ctypes.c_void_p(M._arr), M._leading_dim, ctypes.c_void_p(x2._arr), x2._leading_dim,
                                     br, bi, ctypes.c_void_p(y2._arr), y2._leading_dim), "ig_cgemm")

    def csymm(self, y, M, x, alpha, beta, left=True):
        """the same product for a real symmetric M (the reference's cublasCsymm call, cuda.py:362-392)"""
        self.cgemm(y, M, x, alpha, beta, forward=True, left=left)

    # -- gridding matrices from their description (indigo_amd.structured.InterpS): the library's native host builder ------------
    def _interp_matrix(self, npts, N, width, table, coord, dtype):
        """Backend.Interp's matrix through ig_interp3_count / _fill (bit-identical to the numpy formulation, tests/test_sense_cpu.py)"""
        import scipy.sparse as spp
        from indigo_amd.interp import interp_csr_arrays
        indptr, indices, data = interp_csr_arrays(npts, N, width, table, coord, dtype=np.float32)
        return spp.csr_matrix((data.astype(dtype), indices, indptr), shape=(npts, int(np.prod(N, dtype=np.int64))))

    def gridding_from_struct(self, s, grid_order=0, phases=None):
        """G' = interp * diag(exp(2 pi i separable phase)) * real constant (what `pics.py -O3` folds into the gridding matrix,
        examples/pics.py:104-177) in ONE native pass over the trajectory, columns numbered for the fused leaf's grid order
        (ig_interp3_fill_modulated) -- instead of a scipy product of a 5e7-nonzero matrix with two 1.3e8-entry diagonals and a
        renumbering sort.  None for any other column scaling: the caller takes the scipy route.  `phases`: per-axis phases to use instead of
        the description's (fold_axis_shifts: the leaf's transform carries the rest)."""
        import scipy.sparse as spp
        from indigo_amd.interp import interp_csr_arrays, interp_csr_modulated
        shape = (s.npts, int(np.prod(s.N, dtype=np.int64)))
        if s.colscale is None:
            indptr, indices, data = interp_csr_arrays(s.npts, s.N, s.width, s.table, s.coord, dtype=np.float32, grid_order=grid_order)
            return spp.csr_matrix((data.astype(_C64), indices, indptr), shape=shape)
        sep = s.colscale.separable()
        if sep is None or tuple(sep[0].shape) != tuple(s.N):
            return None
        indptr, indices, data = interp_csr_modulated(s.npts, s.N, s.width, s.table, s.coord, sep[0].phases if phases is None else phases, sep[1], grid_order=grid_order)
        return spp.csr_matrix((data, indices, indptr), shape=shape)

    def gridding_sep_from_struct(self, s, grid_order=0, phases=None):
        """the same G' in SEPARABLE form -- one record per sample (indigo_amd.interp.interp_sep_records) -- or None when the column
        scaling is no sign per axis times a real constant (an odd grid axis) or the kernel is wider than 8 taps"""
        from indigo_amd.interp import interp_sep_records
        if not self.tuning.get('separable', True):
            return None
        if s.colscale is None:
            return interp_sep_records(s.npts, s.N, s.width, s.table, s.coord, None, 1.0, grid_order=grid_order)
        sep = s.colscale.separable()
        if sep is None or tuple(sep[0].shape) != tuple(s.N):
            return None
        return interp_sep_records(s.npts, s.N, s.width, s.table, s.coord, sep[0].phases if phases is None else phases, sep[1], grid_order=grid_order)

    def inspect(self, csr):
        indptr = np.ascontiguousarray(csr.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
        nzrow, nzcol, exw = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        rc = self._L.ig_csr_inspect(ctypes.c_void_p(indptr.ctypes.data), ctypes.c_void_p(indices.ctypes.data),
                                    csr.shape[0], csr.shape[1], ctypes.byref(nzrow), ctypes.byref(nzcol),
                                    ctypes.byref(exw))
        _lib.check(rc, None, "ig_csr_inspect")
        return nzrow.value, nzcol.value, bool(exw.value)

    def csr_transpose(self, csr):
        """(indptr_t, indices_t, data_t) of csr^T via the library's native counting sort"""
        M, K = csr.shape
        indptr = np.ascontiguousarray(csr.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
        data = np.ascontiguousarray(csr.data, dtype=np.complex64)
        pt = np.empty(K + 1, dtype=np.int32)
        it = np.empty(csr.nnz, dtype=np.int32)
        dt = np.empty(csr.nnz, dtype=np.complex64)
        rc = self._L.ig_csr_transpose(M, K, csr.nnz, ctypes.c_void_p(indptr.ctypes.data),
                                      ctypes.c_void_p(indices.ctypes.data), ctypes.c_void_p(data.ctypes.data),
                                      ctypes.c_void_p(pt.ctypes.data), ctypes.c_void_p(it.ctypes.data),
                                      ctypes.c_void_p(dt.ctypes.data))
        _lib.check(rc, None, "ig_csr_transpose")
        return pt, it, dt


# the device CSR matrix and the formats of a gridding matrix: backends/hip_csr.py (it needs nothing of this module)
from indigo_amd.backends.hip_csr import _ptr, csr_matrix as _csr_matrix       # noqa: E402

HipBackend.csr_matrix = _csr_matrix
