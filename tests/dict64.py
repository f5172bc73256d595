"""A float64 restatement of dictionary matching (Backend.dict_match, ig_dict_match_c64, indigo_amd.dictmatch), for the tests, and the
generators of their cases: random panels, voxels built on known atoms, and a T2 phantom whose voxels sit on grid values."""
import numpy as np

C64 = np.dtype('complex64')


def products(d, x):
    """P[i, a] = d_a^H x_i in complex128: d is the K x N dictionary (atom a in column a), x the n x K panel"""
    return np.asarray(x, dtype=np.complex128) @ np.conj(np.asarray(d, dtype=np.complex128))


def scores(d, x):
    """s[i, a] = |d_a^H x_i|^2 in float64"""
    P = products(d, x)
    return P.real ** 2 + P.imag ** 2


def match(d, x):
    """-> (idx, ip, s): the lowest index of the largest score of every voxel, d_idx^H x there, and all scores"""
    P = products(d, x)
    s = P.real ** 2 + P.imag ** 2
    idx = np.argmax(s, axis=1)
    return idx.astype(np.int32), P[np.arange(P.shape[0]), idx], s


def random_case(n, K, N, seed):
    """-> (x, d): an n x K panel of voxels and a K x N dictionary of normalised atoms, complex64, entries centred on zero"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))).astype(C64)
    return np.asfortranarray(x), normalised_atoms(K, N, rng)


def normalised_atoms(K, N, rng):
    d = rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))
    return np.asfortranarray((d / np.linalg.norm(d, axis=0)[None, :]).astype(C64))


def planted_case(n, K, N, seed, noise=1e-3):
    """-> (x, d, m): voxel i is rho_i d_{m_i} + noise * (unit-variance complex noise), |rho_i| in [0.5, 2), m_i drawn from all N atoms"""
    rng = np.random.default_rng(seed)
    d = normalised_atoms(K, N, rng)
    m = rng.integers(0, N, size=n)
    m[:min(n, N)] = rng.permutation(N)[:min(n, N)]                                     # every atom once where n allows
    rho = (0.5 + 1.5 * rng.random(n)) * np.exp(2j * np.pi * rng.random(n))
    x = rho[:, None] * d.astype(np.complex128).T[m] + noise * (rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))) / np.sqrt(2)
    return np.asfortranarray(x.astype(C64)), d, m.astype(np.int32)


def largest_cross_score(d):
    """the largest |d_a^H d_b|^2 over a != b of a dictionary of unit atoms"""
    D = np.asarray(d, dtype=np.complex128)
    G = np.abs(D.conj().T @ D) ** 2
    np.fill_diagonal(G, 0)
    return float(G.max())


# ---- the T2 phantom -----------------------------------------------------------------------------------------------------------------

PHANTOM_DIMS = (12, 10, 8)
T2_ARGS = ["--model", "t2", "--te", "0.01", "--echoes", "16", "--t2", "0.02:0.3:32", "--rank", "4"]


def t2_phantom(atoms, phi, dims=PHANTOM_DIMS, seed=5):
    """a volume whose voxels carry atoms of the dictionary: -> (coeffs (X, Y, Z, 1, 1, 1, K) complex64, the coefficient images as
    pics --basis returns them; index (X, Y, Z) of the atom; rho (X, Y, Z) complex128; inside (X, Y, Z) bool).  Outside an ellipsoid
    the voxels are zero; inside, |rho| is between 0.5 and 1.5, so every voxel inside is far above a mask of 2 % of the largest."""
    rng = np.random.default_rng(seed)
    N = atoms.shape[0]
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in dims)]
    inside = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) < 0.8
    index = rng.integers(0, N, size=dims)
    first = np.flatnonzero(inside.ravel())[:N]
    index.ravel()[first] = np.arange(first.size)                                       # every atom, also the two ends of the grid
    rho = (0.5 + rng.random(dims)) * np.exp(2j * np.pi * rng.random(dims)) * inside
    c = rho[..., None] * (np.asarray(atoms, dtype=np.complex128) @ np.conj(np.asarray(phi, dtype=np.complex128)))[index]
    coeffs = c.reshape(dims + (1, 1, 1, phi.shape[1])).astype(C64)
    return coeffs, np.where(inside, index, 0).astype(np.int32), rho, inside
