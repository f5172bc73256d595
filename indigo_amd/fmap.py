"""The interpolator of the time-segmented off-resonance model (pics --fmap).  Host only, float64.

A spin at r with the field offset f(r) Hz carries the phase exp(-2 pi i f(r) t) at the sample time t.  Time segmentation (Noll;
Sutton, Noll and Fessler) replaces it by L phases at fixed times tau_l, mixed per sample,

    exp(-2 pi i f t_j)  ~  sum_{l < L} b_l(t_j) exp(-2 pi i f tau_l)

so that the forward model is L copies of the plain one between a per-voxel phase (operators.SegmentPhase) and a per-sample
mix (operators.SegmentCombine).  `segments` chooses the tau_l and computes the table b, the least-squares interpolator for the
histogram of the field map that is being corrected.
"""
import logging

import numpy as np

log = logging.getLogger(__name__)

MAXL = 16


def histogram(fmap, mask=None, bins=256):
    """centres f_h and counts w_h of the `bins`-bin histogram of the field map over `mask` (default: everywhere), empty bins left
    out; a constant field map is one centre, its value"""
    f = np.asarray(fmap, dtype=np.float64)
    f = f[np.asarray(mask, dtype=bool)] if mask is not None else f.reshape(-1)
    if f.size == 0:
        raise ValueError("fmap: the mask selects no voxel of the field map")
    lo, hi = float(f.min()), float(f.max())
    if lo == hi:
        return np.array([lo]), np.array([float(f.size)])
    counts, edges = np.histogram(f, bins=int(bins), range=(lo, hi))
    centres = 0.5 * (edges[:-1] + edges[1:])
    keep = counts > 0
    return centres[keep], counts[keep].astype(np.float64)


def interpolator(centres, counts, taus, t):
    """-> (b, err): b (len(t), L) minimises sum_h w_h |exp(-2 pi i f_h t) - sum_l b_l exp(-2 pi i f_h tau_l)|^2 for every t, by a
    minimum-norm least-squares solve (a constant field map makes the system rank one); one segment is b = 1.  err is the weighted
    RMS of the residual over the times given"""
    taus = np.asarray(taus, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    sw = np.sqrt(counts / counts.sum())
    E = np.exp(-2j * np.pi * np.outer(centres, taus))                          # (H, L)
    rhs = np.exp(-2j * np.pi * np.outer(centres, t))                           # (H, J)
    if taus.size == 1:
        b = np.ones((1, t.size), dtype=np.complex128)
    else:
        b = np.linalg.lstsq(sw[:, None] * E, sw[:, None] * rhs, rcond=None)[0]
    res = sw[:, None] * (rhs - E @ b)
    return b.T, float(np.sqrt((np.abs(res) ** 2).sum() / t.size))


def segment_times(times, L):
    """L times equispaced over [min t, max t]; one segment sits at the mid time"""
    lo, hi = float(np.min(times)), float(np.max(times))
    return np.array([0.5 * (lo + hi)]) if L == 1 else np.linspace(lo, hi, int(L))


def segments(fmap, times, L=None, mask=None, bins=256, tol=1e-3, maxL=MAXL):
    """-> (taus, b, period, err) of the time-segmented model for the real field map `fmap` (Hz) and the sample times `times`
    (seconds): (readout,) when the time depends on the readout index alone, or (readout, views), sample-major as the k-space is.

    taus    the L segment times, equispaced over [min t, max t] (L = 1: the mid time)
    b       the (period, L) complex128 table, row j the interpolator of sample j's time (`interpolator` on the `bins`-bin
            histogram of the field map over `mask`)
    period  the rows of the table: readout, or readout * views
    err     the weighted RMS of the model's residual over the histogram and all distinct times

    L None: the smallest L in 1..maxL with err < tol; a ValueError when maxL does not reach it."""
    fmap = np.asarray(fmap)
    if np.iscomplexobj(fmap):
        raise ValueError("fmap: the field map must be real (Hz); a complex one, R2* decay in its imaginary part, is not supported")
    times = np.asarray(times, dtype=np.float64)
    if times.ndim not in (1, 2) or times.size < 1 or not np.isfinite(times).all():
        raise ValueError("fmap: times must be a finite (readout,) or (readout, views) array, got shape %s" % (times.shape,))
    maxL = int(maxL)
    if not 1 <= maxL <= MAXL or (L is not None and not 1 <= int(L) <= maxL):
        raise ValueError("fmap: %s segments (at most %d), between 1 and %d are supported" % (L, maxL, MAXL))
    centres, counts = histogram(fmap, mask, bins)
    distinct, inverse = np.unique(times.reshape(-1, order='F'), return_inverse=True)
    span = float(np.abs(np.asarray(fmap, dtype=np.float64)).max() * (distinct[-1] - distinct[0]))
    for cand in ([int(L)] if L is not None else range(1, maxL + 1)):
        taus = segment_times(distinct, cand)
        b, err = interpolator(centres, counts, taus, distinct)
        if L is not None or err < tol:
            break
    else:
        raise ValueError("fmap: %d segments reach a model error of %.3e, not the tolerance %.3e: the field map spans %.1f cycles "
                         "over the readout (max|f| (max t - min t)); raise --fmap-tol or shorten the readout" % (maxL, err, tol, span))
    log.info("fmap: %d segments, field map span %.2f cycles, %d distinct times, model error %.3e", taus.size, span, distinct.size, err)
    return taus, b[inverse.reshape(-1)], int(times.size), err
