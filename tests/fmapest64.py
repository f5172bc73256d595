"""Float64 restatement of the regularised multi-echo field-map fit (Funai, Fessler, Yeo, Olafsson, Noll, IEEE TMI
27:1484, 2008), written from the definition -- the wrapped angle s itself, its cosine, sine and sin(s) / s -- and not the way the
backends compute it (the rotated product p exp(i k f)).  tests/test_fmapest_cpu.py checks it against closed forms: its gradient
against a finite difference of its own cost, monotone descent, the fixed point of noiseless data.

    y: (N, E) complex, the echo images on the F-ordered `dims` volume, y_l ~ m exp(-2 pi i f te_l);  f: (N,) real, in Hz
    pairs l < m in the order (0,1), (0,2), .., (0,E-1), (1,2), ..:   p = y_m conj(y_l), w = |p|, k = 2 pi (te_m - te_l),
    s = pv(angle(p) + k f) in [-pi, pi]
    Psi(f) = sum_j sum_pairs w (1 - cos s) + beta / 2 sum_edges (f_j - f_j')^2      edges: nearest neighbours along the three axes, no wrap
    g_j = sum_pairs w k sin s + beta sum_{j' ~ j} (f_j - f_j'),    d_j = sum_pairs w k^2 kappa(s) + 2 beta deg_j,   kappa = sin(s) / s
    step: f_j - g_j / d_j   (d_j = 0: f_j)
"""
import numpy as np

U = 2.0 ** -24                                           # the unit roundoff of float32


def pairs(E):
    return [(l, m) for l in range(E) for m in range(l + 1, E)]


def _pv(t):
    """the principal value of the angle t in [-pi, pi)"""
    return (t + np.pi) % (2.0 * np.pi) - np.pi


def _pair_terms(y, f, te):
    """for every pair: (w, k, s), each (N,) but the scalar k"""
    y = np.asarray(y, dtype=np.complex128)
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    te = np.asarray(te, dtype=np.float64)
    for l, m in pairs(te.size):
        p = y[:, m] * y[:, l].conj()
        k = 2.0 * np.pi * (te[m] - te[l])
        yield np.abs(p), k, _pv(np.angle(p) + k * f)


def _neighbours(f, dims):
    """(sum over the neighbours j' of f_j - f_j', the number of neighbours, sum over the forward edges of (f_j - f_j')^2), the first two (N,)"""
    v = np.asarray(f, dtype=np.float64).reshape(dims, order='F')
    diff, deg, edges = np.zeros(dims), np.zeros(dims), 0.0
    for a in range(3):
        if dims[a] < 2:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        e = v[lo] - v[hi]                                # f_j - f_j' over the edge (j, j' = j + e_a)
        diff[lo] += e
        diff[hi] -= e
        deg[lo] += 1
        deg[hi] += 1
        edges += float((e ** 2).sum())
    return diff.reshape(-1, order='F'), deg.reshape(-1, order='F'), edges


def cost(y, f, te, beta, dims):
    data = sum(float((w * (1.0 - np.cos(s))).sum()) for w, k, s in _pair_terms(y, f, te))
    return data + 0.5 * float(beta) * _neighbours(f, dims)[2]


def gradient(y, f, te, beta, dims):
    g = sum(w * k * np.sin(s) for w, k, s in _pair_terms(y, f, te))
    return g + float(beta) * _neighbours(f, dims)[0]


def curvature(y, f, te, beta, dims):
    d = sum(w * k * k * np.sinc(s / np.pi) for w, k, s in _pair_terms(y, f, te))          # np.sinc(x) = sin(pi x) / (pi x)
    return d + 2.0 * float(beta) * _neighbours(f, dims)[1]


def step(y, f, te, beta, dims):
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    g, d = gradient(y, f, te, beta, dims), curvature(y, f, te, beta, dims)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(d > 0, f - g / d, f)


def init(y, te):
    y = np.asarray(y, dtype=np.complex128)
    return -np.angle(y[:, 1] * y[:, 0].conj()) / (2.0 * np.pi * (float(te[1]) - float(te[0])))


def phantom(dims, te, noise=0.05, background=0.02, peak_hz=100.0, seed=0):
    """(y (N, E) complex128, the true field (N,) in Hz, the object's mask (N,)): a smooth field of up to about `peak_hz`, a bright
    ellipsoid of magnitude 1 over a background of `background`, complex noise of standard deviation `noise`"""
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in dims], indexing='ij')
    field = peak_hz * (0.6 * g[0] + 0.5 * g[1] ** 2 - 0.4 * g[2] * g[0] + 0.3 * np.sin(2.0 * g[2]) - 0.2)
    inside = (g[0] / 0.8) ** 2 + (g[1] / 0.7) ** 2 + (g[2] / 0.75) ** 2 < 1.0
    mag = np.where(inside, 1.0, background)
    rng = np.random.default_rng(seed)
    te = np.asarray(te, dtype=np.float64)
    y = mag[..., None] * np.exp(-2j * np.pi * field[..., None] * te)
    y = y + noise * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)) / np.sqrt(2.0)
    n = int(np.prod(dims))
    return y.reshape((n, te.size), order='F'), field.reshape(-1, order='F'), inside.reshape(-1, order='F')


def step_bound(y, f, te, beta, dims):
    """Per voxel, a bound on |float32 step - float64 step| for a kernel that forms p, the rotated product r = p exp(i k f) with the
    phase reduced in double, s = atan2(Im r, Re r), and accumulates g and d with fused multiply-adds, on the same float32 inputs.
    In units of U = 2^-24, with P pairs:
      p:  each component is a product and a fused multiply-add, 2 roundings of terms that sum to <= w         |dp| <= 2 sqrt(2) w   < 3 w
      phase: the reduced cycles rounded to float, <= U / 2 cycles = pi U rad; sincospi good to 2 ulp = 4 U per component
                                                                                                               |de| <= pi + 4 sqrt(2) < 9
      r = p e: 2 roundings per component again, plus the two above                                            |dr| <= (3 + 3 + 9) w = 15 w
      a term of g, k Im r: k rounded to float, 1; the fused multiply-add into the sum, 1                      <= 17 k w
      a term of d, k^2 Im r / s: h(r) = Im r / arg r = |r| kappa(arg r) is continuous across the wrap with |grad h| <= 1.1, so
        1.1 * 15 w < 17 w; atan2 good to 2 ulp = 4; the divide 1; k^2 two roundings and k itself twice, 4; the multiply-add 1   <= 27 k^2 w
      the penalty: f_j - f_j' 1, the sum of up to 6 of them 5, times beta 1, 2 beta deg 1                     <= 7 beta |f_j - f_j'|
      summing P terms: P more on every term.
    So |dg| <= (17 + P) U Ga with Ga = sum_pairs k w + beta sum |f_j - f_j'| (the magnitudes that enter g: Im r is a difference of
    products of size w, whatever sin s is), |dd| <= (27 + P) U Da with Da = sum_pairs k^2 w + 2 beta deg, and with |g| <= Ga
      |d(g / d)| <= |dg| / d + Ga / d * |dd| / d + U Ga / d  (the divide)  <= (27 + P) U (Ga / d) (1 + Da / d)
    (17 + P + 1 <= 27 + P), and the final subtraction rounds once more: U (|f| + Ga / d).  The float64 side's own rounding is
    2^-29 of that.  Where d = 0 both sides leave f alone and the bound is 0."""
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    P = len(pairs(len(te)))
    diff_abs = np.zeros(dims)
    v = f.reshape(dims, order='F')
    for a in range(3):
        if dims[a] < 2:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        e = np.abs(v[tuple(lo)] - v[tuple(hi)])
        diff_abs[tuple(lo)] += e
        diff_abs[tuple(hi)] += e
    deg = _neighbours(f, dims)[1]
    Ga = sum(k * w for w, k, s in _pair_terms(y, f, te)) + float(beta) * diff_abs.reshape(-1, order='F')
    Da = sum(k * k * w for w, k, s in _pair_terms(y, f, te)) + 2.0 * float(beta) * deg
    d = curvature(y, f, te, beta, dims)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(d > 0, Ga / d, 0.0)
        spread = np.where(d > 0, Da / d, 0.0)
    return np.where(d > 0, U * ((27 + P) * ratio * (1.0 + spread) + np.abs(f) + ratio), 0.0)


def init_bound(y, te):
    """|float32 init - float64 init| per voxel: p as above is off by <= 3 U w, so its angle by <= 3 U rad; atan2 good to 2 ulp = 4 U
    |angle|; 1 / k rounded to float and the product, 2 U |angle|:  (3 + 6 |angle|) U / k"""
    y = np.asarray(y, dtype=np.complex128)
    k = 2.0 * np.pi * (float(te[1]) - float(te[0]))
    return U * (3.0 + 6.0 * np.abs(np.angle(y[:, 1] * y[:, 0].conj()))) / k


def cost_bound(y, f, te, beta, dims):
    """|fused cost - float64 cost|: N P data terms w - Re r, each a float32 number converted to double and summed in double: w is a
    square root of a sum of two squares of p, <= (3 + 2) U w, Re r off by 15 U w as above, the subtraction 1:  21 U w per term.  A
    penalty term is the square in double of a float32 difference, 2 U of it, times beta given as float32, 1.  The double sums add
    N P 2^-53 of the total, nothing beside these."""
    data = sum(float(w.sum()) for w, k, s in _pair_terms(y, f, te))
    return U * (21.0 * data + 3.0 * 0.5 * float(beta) * _neighbours(f, dims)[2])
