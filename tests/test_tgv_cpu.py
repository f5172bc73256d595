"""pics --tgv on the CPU: the float64 restatement (tests/tgv64.py) against its definition voxel by voxel, the adjoint identities and norm
bounds of E and K, the host forms of Backend.symgrad3 / tgv_adjoint / tgv_dual_step and operators.SymGradient against it,
`tgv_solve` (the unchanged Backend.primal_dual on (x; v)) against a plain complex128 Condat-Vu loop iterate for iterate, and the
driver against the same loop on the dense matrix of its operator -- all on the numpy oracle backend."""
import logging
import os

import numpy as np
import pytest

import dwt64
import tgv64
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.solvers import ProxTerm, tgv_solve
from indigo_amd.util import rand64c

C64 = np.dtype('complex64')
SHAPES = [(17, 5, 3), (8, 1, 6), (1, 1, 9), (2, 2, 2), (6, 4, 1)]
R = 1.0 / np.sqrt(2.0)


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _c128(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _B_at(w, i, a):
    """(B_a w)[i] from the definition: (i_a < n_a - 1 ? w[i] : 0) - (i_a > 0 ? w[i - e_a] : 0)"""
    prev = tuple(i[b] - (b == a) for b in range(3))
    return (w[i] if i[a] < w.shape[a] - 1 else 0) - (w[prev] if i[a] > 0 else 0)


@pytest.mark.parametrize("dims", SHAPES)
def test_float64_symgrad_is_the_definition_and_has_its_adjoint(dims):
    rng = np.random.default_rng(1)
    n = int(np.prod(dims))
    x, v, p, q = _c128(rng, n, 2), _c128(rng, 3 * n, 2), _c128(rng, 3 * n, 2), _c128(rng, 6 * n, 2)
    # the definition, voxel by voxel, on the first column
    f = [v[a * n:(a + 1) * n, 0].reshape(dims, order='F') for a in range(3)]
    e = tgv64.symgrad(v[:, 0], dims).reshape(dims + (6,), order='F')
    for i in np.ndindex(*dims):
        for a in range(3):
            assert abs(e[i + (a,)] - _B_at(f[a], i, a)) < 1e-14
        for c, (a, b) in enumerate([(0, 1), (0, 2), (1, 2)]):
            assert abs(e[i + (3 + c,)] - (_B_at(f[a], i, b) + _B_at(f[b], i, a)) * R) < 1e-14
    # <E v, q> = <v, E^H q> and <K z, u> = <z, K^H u>
    lhs, rhs = np.vdot(q, tgv64.symgrad(v, dims)), np.vdot(tgv64.symgradh(q, dims), v)
    assert abs(lhs - rhs) < 1e-12 * np.linalg.norm(v) * np.linalg.norm(q)
    kp, kq = tgv64.k(x, v, dims)
    gx, gv = tgv64.kh(p, q, dims)
    lhs, rhs = np.vdot(p, kp) + np.vdot(q, kq), np.vdot(gx, x) + np.vdot(gv, v)
    assert abs(lhs - rhs) < 1e-12 * np.linalg.norm(np.r_[x, v]) * np.linalg.norm(np.r_[p, q])
    # the 6-component 2-norm is the Frobenius norm of the symmetric tensor
    t = tgv64.symgrad(v[:, 0], dims).reshape(dims + (6,), order='F')
    # (diagonal entries once, the off-diagonal entries (B_b v_a + B_a v_b) / 2 = t_ab / sqrt(2) twice)
    frob = (np.abs(t[..., :3]) ** 2).sum(axis=-1) + 2 * (np.abs(t[..., 3:] * R) ** 2).sum(axis=-1)
    np.testing.assert_allclose(tgv64.radius(tgv64.symgrad(v[:, 0], dims), dims, 6)[..., 0] ** 2, frob, rtol=1e-12)


def test_float64_symgrad_of_a_constant_field_vanishes_inside():
    dims = (7, 5, 4)
    n = int(np.prod(dims))
    v = np.repeat(np.array([2 - 3j, -1 + 0.5j, 0.25 + 4j]), n)
    e = tgv64.symgrad(v, dims).reshape(dims + (6,), order='F')
    assert np.array_equal(e[1:-1, 1:-1, 1:-1], np.zeros((5, 3, 2, 6)))
    assert np.abs(e[0]).max() > 0 and np.abs(e[-1]).max() > 0          # B_a is -D_a^H: the faces carry the boundary terms
    # and the xx component is zero away from the two x faces, whatever i_1 and i_2 are
    assert np.array_equal(e[1:-1, :, :, 0], np.zeros((5, 5, 4)))


def test_float64_norm_bounds():
    for dims in [(9, 8, 7), (17, 5, 3), (8, 1, 6), (1, 1, 9)]:
        assert tgv64.norm2_estimate(dims, 'E', iters=100) <= 12
        assert tgv64.norm2_estimate(dims, 'K', iters=100) <= 16
    lam_k, lam_e = tgv64.norm2_estimate((24, 20, 16), 'K'), tgv64.norm2_estimate((24, 20, 16), 'E')
    print("power-iteration estimates at 24 x 20 x 16: ||K||^2 %.3f, ||E||^2 %.3f" % (lam_k, lam_e))
    assert 14 < lam_k <= 16, lam_k                         # (the estimate is not trivially small)
    assert 10 < lam_e <= 12, lam_e


def test_float64_projection():
    dims = (5, 4, 3)
    rng = np.random.default_rng(2)
    for comps, rad in ((3, 2.4), (6, 3.4)):
        u = _c128(rng, comps * 60, 2)
        pr = tgv64.proj(u, rad, dims, comps)
        r, rp = tgv64.radius(u, dims, comps), tgv64.radius(pr, dims, comps)
        assert 0.1 < (r > rad).mean() < 0.9
        np.testing.assert_allclose(rp, np.minimum(r, rad), atol=1e-14)
        np.testing.assert_allclose(tgv64.proj(pr, rad, dims, comps), pr, atol=1e-14)
        assert np.array_equal(tgv64.proj(u, 0.0, dims, comps), np.zeros_like(u))
        assert np.array_equal(tgv64.proj(u, 1e6, dims, comps), u)


@pytest.mark.parametrize("dims", SHAPES)
def test_host_forms_match_the_float64_restatement(oracle_backend, dims):
    B = oracle_backend
    n = int(np.prod(dims))
    alpha, beta = 0.75 - 0.5j, -0.25 + 1.5j
    half = 0.5 + 0.5j
    x, xo = rand64c(n, 2, seed=1) - half, rand64c(n, 2, seed=4) - half
    v, vo = rand64c(3 * n, 2, seed=2) - half, rand64c(3 * n, 2, seed=5) - half
    p, q = rand64c(3 * n, 2, seed=6) - half, rand64c(6 * n, 2, seed=7) - half
    for adjoint, src, ref in ((False, v, tgv64.symgrad(v, dims)), (True, q, tgv64.symgradh(q, dims))):
        y0 = rand64c(ref.shape[0], 2, seed=3)
        y = B.copy_array(np.full(ref.shape, np.nan, dtype=C64, order='F'))
        B.symgrad3(y, B.copy_array(src), dims, adjoint=adjoint)
        np.testing.assert_allclose(y.to_host(), ref, atol=1e-6)
        y = B.copy_array(y0)
        B.symgrad3(y, B.copy_array(src), dims, adjoint=adjoint, alpha=alpha, beta=beta)
        np.testing.assert_allclose(y.to_host(), alpha * ref + beta * y0, atol=1e-6)
    # K^H: gx is added to, gv is written and not read
    gx0 = rand64c(n, 2, seed=8)
    gx, gv = B.copy_array(gx0), B.copy_array(np.full((3 * n, 2), np.nan, dtype=C64, order='F'))
    B.tgv_adjoint(gx, gv, B.copy_array(p), B.copy_array(q), dims)
    ref_x, ref_v = tgv64.kh(p, q, dims)
    np.testing.assert_allclose(gx.to_host(), gx0 + ref_x, atol=1e-6)
    np.testing.assert_allclose(gv.to_host(), ref_v, atol=1e-6)
    # the dual step, the columns stacked in one vector as the solver passes them
    sigma = 0.7
    stack = lambda a: np.asfortranarray(a.reshape((-1, 1), order='F'))         # noqa: E731
    tp, tq = tgv64.unprojected(p, q, x, xo, v, vo, sigma, dims)
    m1, m0 = float(np.median(tgv64.radius(tp, dims, 3))), float(np.median(tgv64.radius(tq, dims, 6)))    # about half of the voxels clip
    for a1, a0 in ((0.0, 0.0), (m1, m0), (1e3, 1e3), (m1, 0.0)):
        ref_p, ref_q = tgv64.dual_step(p, q, x, xo, v, vo, sigma, a1, a0, dims)
        p_d, q_d = B.copy_array(stack(p)), B.copy_array(stack(q))
        B.tgv_dual_step(p_d, q_d, *(B.copy_array(stack(a)) for a in (x, xo, v, vo)), sigma, a1, a0, dims)
        np.testing.assert_allclose(p_d.to_host(), stack(ref_p), atol=1e-6)
        np.testing.assert_allclose(q_d.to_host(), stack(ref_q), atol=1e-6)
    for share in ((tgv64.radius(tp, dims, 3) > m1).mean(), (tgv64.radius(tq, dims, 6) > m0).mean()):
        assert 0.2 <= share <= 0.8, share                  # the medians project some voxels and leave others


def test_symgradient_operator(oracle_backend):
    B = oracle_backend
    dims = (17, 5, 3)
    E = B.SymGradient(dims)
    n = 17 * 5 * 3
    assert E.shape == (6 * n, 3 * n) and E.H.shape == (3 * n, 6 * n)
    v = rand64c(3 * n, 2, seed=4) - (0.5 + 0.5j)
    q = rand64c(6 * n, 2, seed=5) - (0.5 + 0.5j)
    np.testing.assert_allclose(E * v, tgv64.symgrad(v, dims), atol=1e-6)
    np.testing.assert_allclose(E.H * q, tgv64.symgradh(q, dims), atol=1e-6)
    np.testing.assert_allclose((E.H * E) * v, tgv64.symgradh(tgv64.symgrad(v, dims), dims), atol=1e-5)
    for bad in [(17, 5), (17, 5, 0), (17, 5, 3, 1), (4, -1, 4)]:
        with pytest.raises(ValueError):
            B.SymGradient(bad)


@pytest.mark.parametrize("frames,with_prox", [(1, False), (2, False), (1, True)])
def test_tgv_solve_reproduces_a_numpy_loop(oracle_backend, frames, with_prox):
    """every iterate of tgv_solve, which runs Backend.primal_dual unchanged on (x; v), on a dense 24-voxel problem"""
    B = oracle_backend
    dims, a1, a0 = (6, 4, 1), 4.0, 3.0     # (chosen on the float64 loop below: both projections act on some voxels and not on others)
    N, iters = 24, 12
    rng = np.random.default_rng(2)
    Ms = [_c128(rng, 40, N).astype(C64) for _ in range(frames)]
    bs = [_c128(rng, 40, 1).astype(C64) for _ in range(frames)]
    H = np.zeros((N * frames, N * frames), dtype=np.complex128)
    for t, M in enumerate(Ms):
        H[t * N:(t + 1) * N, t * N:(t + 1) * N] = M.astype(np.complex128).conj().T @ M.astype(np.complex128)
    H = H.astype(C64)
    AHy = np.asfortranarray(np.concatenate([M.conj().T @ b for M, b in zip(Ms, bs)]).astype(C64))
    AHA = B.DenseMatrix(np.asfortranarray(H))
    Hd = H.astype(np.complex128)
    L = np.linalg.eigvalsh(Hd)[-1]
    tau, sigma = 0.9 / L, L / 32
    term = None
    if with_prox:                                         # prox of 0.3 ||x||_1 (complex soft threshold, no box kept)
        term = ProxTerm(lambda v, t: B.soft_threshold(v, t * 0.3, (N * frames, 1, 1), (0, 0, 0)),
                        lambda x: 0.3 * float(np.abs(x.to_host().astype(np.complex128)).sum()), "soft threshold 0.3")

    def soft(v, t):
        r = np.abs(v)
        return np.where(r <= t * 0.3, 0, v * (1 - t * 0.3 / np.maximum(r, 1e-300)))
    # the float64 loop treats the frames as the columns of its panels
    cols = lambda z: z.reshape((N, frames), order='F')                              # noqa: E731
    ref, (p_ref, q_ref) = tgv64.condat_vu(lambda z: cols(Hd @ z.reshape(-1, order='F') - AHy.astype(np.complex128)[:, 0]),
                                          soft if with_prox else None, tau, sigma, a1, a0, dims, np.zeros((N, frames)), iters)
    for rad, u, comps in ((a1, p_ref, 3), (a0, q_ref, 6)):
        on_ball = (tgv64.radius(u, dims, comps) >= rad * (1 - 1e-9)).mean()
        assert 0.1 < on_ball < 0.9, (comps, on_ball)
    for it in range(1, iters + 1):
        x, _ = tgv_solve(B, AHA, AHy, dims, it, a1, a0, step=tau, frames=frames, term=term)
        assert x.shape == (N * frames, 1)
        assert _rel(cols(x), ref[it - 1][0]) < 1e-5, it
    assert np.abs(ref[-1][1]).max() > 0.1 * np.abs(ref[-1][0]).max()   # v is a real part of the iteration, not a bystander


def test_pics_parses_and_rejects_the_tgv_options(oracle_backend):
    a = pics.parse(["--tgv", "0.01", "--tgv-ratio", "1.5", "--tgv-sigma", "2.5", "--l1", "0.02", "x.npz"])
    assert (a.tgv, a.tgv_ratio, a.tgv_sigma, a.l1, a.data) == (0.01, 1.5, 2.5, 0.02, "x.npz")
    a = pics.parse(["x.npz"])
    assert (a.tgv, a.tgv_ratio, a.tgv_sigma) == (0, 2.0, None)
    for bad in (["--tgv", "0.01", "--tv", "0.01"], ["--tgv", "0.01", "--tv-time", "0.01"], ["--tgv", "much"],
                ["--tgv", "0.01", "--tgv-ratio", "0"], ["--tgv", "0.01", "--l1", "0.1", "--llr", "0.1"]):
        with pytest.raises(SystemExit):
            pics.parse(bad + ["x.npz"])
    pics.parse(["--tgv", "0", "--tv", "0.01", "x.npz"])                 # --tgv 0 is off
    g = pics.Geometry((4, 4, 4), 64, 2, 1, 1, 1, (1, 8, 8), 64, (4, 4, 4, 1))
    for kw in (dict(tv=0.01), dict(tv_time=0.01)):
        with pytest.raises(ValueError, match="one analysis operator per run"):
            pics.check_options(g, tgv=0.02, **kw)
    assert pics.check_options(g, tgv=0.02, l1=0.1) is None


@pytest.fixture(scope="module")
def scan16(tmp_path_factory, oracle_backend):
    """a 16^3 two-coil radial scan, its k-space data and the dense matrix of its SENSE operator (built as test_tv_cpu's is)"""
    N, C, nro, nsp, osf = (16, 16, 16), 2, 16, 30, 1.5
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    img = (np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + g[2] ** 2)) * (1 + 0.3j)).astype(C64)
    img[(np.abs(g[0]) < 0.4) & (np.abs(g[1]) < 0.3)] += 0.5
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph)
                    for cx, cy, ph in [(-1, 0, 0.3), (1, 0.5, -0.4)]], axis=3).astype(C64)
    coord = radial_trajectory(nsp, nro, seed=2)
    traj = coord * np.array(N, dtype=np.float64)[:, None, None]
    B = oracle_backend
    B._scratch = None
    F1 = B.NUFFT((1, nro, nsp), N, coord, width=3, oversamp=(osf,) * 3, dtype=C64)
    A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
    ksp = (A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F')
    m = A.shape[0]
    AdH = np.concatenate([A.H * np.asfortranarray(np.eye(m, dtype=C64)[:, j:j + 480]) for j in range(0, m, 480)], axis=1)
    Ad = AdH.conj().T
    B._scratch = None
    path = os.path.join(str(tmp_path_factory.mktemp("scan16tgv")), "scan.npz")
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path, N, ksp, Ad.astype(np.complex128)


def _pics(B, argv):
    B._scratch = None
    out = pics.main(argv, backend=B)
    B._scratch = None
    return out


def test_pics_tgv_zero_is_the_cg_driver_and_tgv_is_not_tv(scan16, oracle_backend):
    path = scan16[0]
    args = ["-i", "4", "--osf", "1.5", "--lamda", "1e-3", "--debug", "40", path]
    a = _pics(oracle_backend, args)
    b = _pics(oracle_backend, ["--tgv", "0", "--tgv-ratio", "3"] + args)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    tgv = _pics(oracle_backend, ["--tgv", "0.02"] + args)
    tv = _pics(oracle_backend, ["--tv", "0.02"] + args)
    assert not np.array_equal(a.view(np.uint64), tgv.view(np.uint64)) and not np.array_equal(tv.view(np.uint64), tgv.view(np.uint64))
    with pytest.raises(SystemExit):
        _pics(oracle_backend, ["--tgv", "0.02", "--tv", "0.02"] + args)


# the weight test_tv_cpu uses for --tv, and a ratio below the default 2: v starts from 0 and grows slowly, so that in 10 iterations q
# reaches a ball of radius 2 a1 nowhere; with this one both projections act on a part of the voxels of the float64 reference below
TGV_A1, TGV_RATIO = 0.02, 0.25


@pytest.mark.parametrize("l1", [0.0, 0.05])
def test_pics_tgv_matches_a_float64_condat_vu(scan16, oracle_backend, caplog, l1):
    path, N, ksp, Ad = scan16
    lamda, a1, ratio, iters = 1e-3, TGV_A1, TGV_RATIO, 10
    a0 = ratio * a1
    y = ksp.reshape(-1, order='F').astype(np.complex128)
    AHy = Ad.conj().T @ y
    b = AHy / np.abs(AHy).max()
    AHA = Ad.conj().T @ Ad + lamda * np.eye(Ad.shape[1])
    L = np.linalg.eigvalsh(AHA)[-1]
    tau, sigma = 0.9 / L, L / 32
    keep = dwt64.coarse_box(N, 'db2', 3)

    def prox(v, t):
        return dwt64.dwt(dwt64.soft(dwt64.dwt(v, N, 'db2', 3), t * l1, N, keep), N, 'db2', 3, inverse=True)
    seen, (p, q) = tgv64.condat_vu(lambda z: AHA @ z - b, prox if l1 else None, tau, sigma, a1, a0, N, np.zeros_like(b), iters)
    x, v = seen[-1]
    shares = [(tgv64.radius(u, N, comps) >= rad * (1 - 1e-9)).mean() for rad, u, comps in ((a1, p, 3), (a0, q, 6))]
    print("share of dual vectors on the ball after %d iterations: p %.3f, q %.3f" % (iters, *shares))
    assert 0 < shares[0] < 1 and 0 < shares[1] < 1, shares              # the projections act, and not everywhere
    argv = ["-i", str(iters), "--osf", "1.5", "--lamda", str(lamda), "--tgv", str(a1), "--tgv-ratio", str(ratio), "--step", "%.12e" % tau, "--debug", "40", path]
    if l1:
        argv = ["--l1", str(l1)] + argv
    with caplog.at_level(logging.INFO, logger="pics"):
        out = _pics(oracle_backend, argv)
    assert out.shape == N + (1, 1)
    assert _rel(out.reshape(-1, order='F'), x) < 1e-4, _rel(out.reshape(-1, order='F'), x)
    # the steps that were logged are those of the rule, and the logged objective is the float64 one of the same iterate
    steps = [r.getMessage() for r in caplog.records if r.getMessage().startswith("tgv: tau")]
    assert len(steps) == 1
    got = dict(zip(("tau", "sigma", "a1", "a0"), (float(w.rstrip(",")) for w in steps[0].split()[2:9:2])))
    assert abs(got["tau"] - tau) < 1e-6 * tau and abs(got["sigma"] - sigma) < 1e-6 * sigma, (steps, tau, sigma)
    assert (got["a1"], got["a0"]) == (a1, a0), steps
    logged = [r.getMessage() for r in caplog.records if "objective" in r.getMessage()]
    assert logged and logged[-1].startswith("tgv iter %d, objective" % iters)
    obj = 0.5 * np.linalg.norm(Ad @ x - y / np.abs(AHy).max()) ** 2 + 0.5 * lamda * np.linalg.norm(x) ** 2 + tgv64.tgv(x, v, a1, a0, N)
    if l1:
        W = dwt64.dwt(x, N, 'db2', 3).reshape(N, order='F')
        inside = np.zeros(N, dtype=bool)
        inside[tuple(slice(0, c) for c in keep)] = True
        obj += l1 * np.abs(W[~inside]).sum()
    assert abs(float(logged[-1].split()[-1]) - obj) < 1e-4 * abs(obj), (logged[-1], obj)
