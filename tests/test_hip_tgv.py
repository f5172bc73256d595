"""The symmetrised gradient, its adjoint, the two fused passes of second-order total generalized variation and pics --tgv on the
MI355X: ig_symgrad3_c64 / ig_symgrad3h_c64 / ig_tgv_kh_c64 / ig_tgv_dual_c64 against the float64 restatement in tests/tgv64.py, and
the primal-dual driver against the same driver on the numpy oracle backend."""
import logging
import os
import re

import numpy as np
import pytest

import tgv64
from indigo_amd import pics
from indigo_amd.sense import radial_trajectory
from indigo_amd.util import rand64c

pytestmark = pytest.mark.gpu
C64 = np.dtype('complex64')
# the shapes of test_hip_tv: nothing a multiple of a wave or a line; several workgroups; unit axes; the smallest; 67 600 rows (more
# groups of rows than the kernels' grid holds, so they stride)
DIMS = [(17, 5, 3), (64, 48, 40), (8, 1, 6), (1, 1, 9), (2, 2, 2), (8, 260, 260)]
PAD = 37
HALF = 0.5 + 0.5j


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def _padded(hip, a, fill=0.0):
    """the panel a (rows x ncols) on the device with PAD extra rows of `fill` under every column, and the host copy"""
    p = np.full((a.shape[0] + PAD, a.shape[1]), fill, dtype=C64, order='F')
    p[:a.shape[0]] = a
    return hip.copy_array(p), p


def _back(d, host, rows):
    """the first `rows` rows of the padded device panel d, after checking that the rows below them are what `host` holds"""
    out = d.to_host()
    assert np.array_equal(out[rows:], host[rows:], equal_nan=True)      # the rows between columns are left alone
    return out[:rows]


@pytest.fixture(scope="module", params=DIMS, ids=lambda d: "x".join(map(str, d)))
def case(request):
    """two-column inputs of one volume shape and their float64 results, computed once"""
    dims = request.param
    n = int(np.prod(dims))
    c = dict(dims=dims, n=n, sigma=0.7)
    for seed, (name, comps) in enumerate((("x", 1), ("xo", 1), ("v", 3), ("vo", 3), ("p", 3), ("q", 6), ("gx0", 1)), start=1):
        c[name] = rand64c(comps * n, 2, seed=seed) - HALF
        c[name].setflags(write=False)
    c["Ev"], c["EHq"] = tgv64.symgrad(c["v"], dims), tgv64.symgradh(c["q"], dims)
    c["KHx"], c["KHv"] = tgv64.kh(c["p"], c["q"], dims)
    c["tp"], c["tq"] = tgv64.unprojected(c["p"], c["q"], c["x"], c["xo"], c["v"], c["vo"], c["sigma"], dims)
    return c


def _symgrad(hip, src, dims, adjoint=False, alpha=1, beta=0, y0=None):
    """symgrad3 of the panel src into a panel with PAD extra rows; y starts as y0 or NaN"""
    n = int(np.prod(dims))
    rows_y = 3 * n if adjoint else 6 * n
    s_d, _ = _padded(hip, src)
    y_d, yp = _padded(hip, np.full((rows_y, src.shape[1]), np.nan, dtype=C64) if y0 is None else y0, fill=np.nan)
    hip.symgrad3(y_d[:rows_y], s_d[:src.shape[0]], dims, adjoint=adjoint, alpha=alpha, beta=beta)
    return _back(y_d, yp, rows_y)


def test_symgrad3_matches_the_float64_operator(hip, case):
    dims, v, q = case["dims"], case["v"], case["q"]
    alpha, beta = 0.75 - 0.5j, -0.25 + 1.5j
    fwd = _symgrad(hip, v, dims)                                        # y starts as NaN: beta == 0 does not read it
    adj = _symgrad(hip, q, dims, adjoint=True)
    assert np.isfinite(fwd).all() and np.isfinite(adj).all()
    assert _rel(fwd, case["Ev"]) < 2e-6, _rel(fwd, case["Ev"])
    assert _rel(adj, case["EHq"]) < 2e-6, _rel(adj, case["EHq"])
    for adjoint, src, ref in ((False, v, case["Ev"]), (True, q, case["EHq"])):
        y0 = rand64c(ref.shape[0], 2, seed=9) - HALF
        out = _symgrad(hip, src, dims, adjoint=adjoint, alpha=alpha, beta=beta, y0=y0)
        assert _rel(out, alpha * ref + beta * y0) < 2e-6, (adjoint, _rel(out, alpha * ref + beta * y0))
    # adjoint identity <E v, q> = <v, E^H q> on the device results
    lhs, rhs = np.vdot(q.astype(np.complex128), fwd), np.vdot(adj.astype(np.complex128), v)
    assert abs(lhs - rhs) < 1e-6 * np.linalg.norm(v) * np.linalg.norm(q)


def test_tgv_adjoint_matches_the_float64_adjoint(hip, case):
    dims, n = case["dims"], case["n"]
    p_d, _ = _padded(hip, case["p"])
    q_d, _ = _padded(hip, case["q"])
    gx_d, gxp = _padded(hip, case["gx0"], fill=np.nan)                  # gx starts from random values and is added to
    gv_d, gvp = _padded(hip, np.full((3 * n, 2), np.nan, dtype=C64), fill=np.nan)     # gv starts from NaN and is not read
    hip.tgv_adjoint(gx_d[:n], gv_d[:3 * n], p_d[:3 * n], q_d[:6 * n], dims)
    gx, gv = _back(gx_d, gxp, n), _back(gv_d, gvp, 3 * n)
    ref_x = case["gx0"] + case["KHx"]
    assert _rel(gx, ref_x) < 2e-6, _rel(gx, ref_x)
    assert _rel(gv, case["KHv"]) < 2e-6, _rel(gv, case["KHv"])


def test_tgv_dual_step_matches_the_float64_step(hip, case):
    dims, n, sigma, tp, tq = (case[k] for k in ("dims", "n", "sigma", "tp", "tq"))
    r1, r0 = tgv64.radius(tp, dims, 3), tgv64.radius(tq, dims, 6)
    a1, a0 = float(np.float32(np.median(r1))), float(np.float32(np.median(r0)))      # the balls that clip about half of the voxels
    for clipped in ((r1 > a1).mean(), (r0 > a0).mean()):
        assert 0.2 <= clipped <= 0.8, clipped
    ref_p, ref_q = tgv64.proj(tp, a1, dims, 3), tgv64.proj(tq, a0, dims, 6)
    ins = [hip.copy_array(case[k]) for k in ("x", "xo", "v", "vo")]

    def step(a1_, a0_):
        p_d, pp = _padded(hip, case["p"], fill=np.nan)
        q_d, qp = _padded(hip, case["q"], fill=np.nan)
        hip.tgv_dual_step(p_d[:3 * n], q_d[:6 * n], *ins, sigma, a1_, a0_, dims)
        return _back(p_d, pp, 3 * n), _back(q_d, qp, 6 * n)
    p, q = step(a1, a0)
    assert _rel(p, ref_p) < 2e-6, _rel(p, ref_p)
    assert _rel(q, ref_q) < 2e-6, _rel(q, ref_q)
    assert tgv64.radius(p, dims, 3).max() <= a1 * (1 + 1e-6)
    assert tgv64.radius(q, dims, 6).max() <= a0 * (1 + 1e-6)
    p, q = step(0.0, 0.0)                                               # radius 0: exact zeros
    assert not p.any() and not q.any()
    p, q = step(1e6, 1e6)                                               # nothing clips: the unprojected step
    assert _rel(p, tp) < 2e-6, _rel(p, tp)
    assert _rel(q, tq) < 2e-6, _rel(q, tq)


def test_tgv_entries_refuse_overlap_and_negative_radii(hip):
    dims = (8, 4, 2)
    n = 64
    buf = hip.copy_array(rand64c(20 * n, 1, seed=1))
    before = buf.to_host()
    rows = lambda a, b: buf[a * n:b * n]                                # noqa: E731
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.symgrad3(rows(0, 6), rows(5, 8), dims)                      # y = rows [0, 6N) holds the top of v = rows [5N, 8N)
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.symgrad3(buf[6 * n - 1:9 * n - 1], rows(0, 6), dims, adjoint=True)
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tgv_adjoint(rows(8, 9), rows(9, 12), rows(0, 3), rows(3, 9), dims)          # gx inside q
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tgv_adjoint(rows(9, 10), rows(2, 5), rows(0, 3), rows(10, 16), dims)        # gv on p
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tgv_adjoint(rows(17, 18), rows(16, 19), rows(0, 3), rows(3, 9), dims)       # gx inside gv
    x, xo, v, vo = rows(9, 10), rows(10, 11), rows(11, 14), rows(14, 17)
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tgv_dual_step(rows(0, 3), rows(3, 9), x, xo, v, rows(1, 4), 1.0, 1.0, 1.0, dims)        # vo on p
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tgv_dual_step(rows(0, 3), rows(3, 9), rows(8, 9), xo, v, vo, 1.0, 1.0, 1.0, dims)      # xn inside q
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.tgv_dual_step(rows(0, 3), rows(2, 8), x, xo, v, vo, 1.0, 1.0, 1.0, dims)               # q on p
    for a1, a0 in ((-1.0, 1.0), (1.0, -1e-3)):
        with pytest.raises(RuntimeError, match="negative radius"):
            hip.tgv_dual_step(rows(0, 3), rows(3, 9), x, xo, v, vo, 1.0, a1, a0, dims)
    assert np.array_equal(buf.to_host(), before)
    hip.symgrad3(rows(0, 6), rows(6, 9), dims)                          # adjacent, not overlapping: fine
    np.testing.assert_allclose(buf.to_host()[:6 * n], tgv64.symgrad(before[6 * n:9 * n], dims), atol=1e-6)


def test_symgradient_in_an_operator_product(hip):
    dims = (17, 5, 3)
    E = hip.SymGradient(dims)
    v = rand64c(E.shape[1], 2, seed=6) - HALF
    ref = tgv64.symgradh(tgv64.symgrad(v, dims), dims)
    out = (E.H * E) * v
    assert _rel(out, ref) < 2e-6, _rel(out, ref)


def _scan(tmpdir, B, N, C, nro, nsp, osf, width=2):
    """the synthetic radial scan of test_hip_tv"""
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    img = (np.exp(-4 * (g[0] ** 2 + 1.5 * g[1] ** 2 + 0.7 * g[2] ** 2)) * (1 + 0.3j)).astype(np.complex64)
    img[(np.abs(g[0]) < 0.3) & (np.abs(g[1]) < 0.2)] += 0.5                 # an edge for the differences to see
    centres = [(-1, 0, 0.3), (1, 0.5, -0.4)][:C]
    mps = np.stack([np.exp(-((g[0] - cx) ** 2 + (g[1] - cy) ** 2)) * np.exp(1j * ph) for cx, cy, ph in centres],
                   axis=3).astype(np.complex64)
    coord = radial_trajectory(nsp, nro, seed=2)
    traj = coord * np.array(N, dtype=np.float64)[:, None, None]
    F1 = B.NUFFT((1, nro, nsp), N, coord, width=width, oversamp=(osf, osf, osf), dtype=C64)
    A = B.KronI(C, F1) * B.VStack([B.Diag(mps[:, :, :, c:c + 1]) for c in range(C)])
    ksp = (A * np.asfortranarray(img.reshape(-1, 1, order='F'))).reshape((1, nro, nsp, C), order='F')
    path = os.path.join(str(tmpdir), "scan.npz")
    np.savez(path, data=ksp.reshape(ksp.shape + (1,)).T, maps=mps.reshape(mps.shape + (1,)).T, traj=traj.T)
    return path


def _logged(caplog, pattern):
    return [float(m.group(1)) for r in caplog.records for m in [re.search(pattern, r.getMessage())] if m]


def test_pics_tgv_on_the_gpu_matches_the_oracle_backend(tmp_path, hip, oracle_backend, caplog):
    N = (64, 64, 64)
    path = _scan(tmp_path, hip, N, 2, nro=128, nsp=200, osf=2.0)
    args = ["--osf", "2.0", "--width", "2", "--lamda", "1e-3", "--tgv", "0.02", "--debug", "40", path]
    # the two power iterations' estimates of the largest eigenvalue of A^H A + lamda I
    est = {}
    for name, B in (("hip", hip), ("oracle", oracle_backend)):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="pics"):
            pics.main(["-i", "0", "--power-iters", "6"] + args, backend=B)
        oracle_backend._scratch = None
        est[name] = _logged(caplog, r"largest eigenvalue of A\^H A \+ lamda I (\S+)")[0]
    assert abs(est["hip"] - est["oracle"]) < 1e-4 * est["oracle"], est
    step = ["--step", "%.8e" % (0.9 / est["oracle"])]
    for extra, iters, tol in (([], "1", 1e-5), ([], "10", 1e-4), (["--l1", "0.02"], "10", 1e-4)):
        out = pics.main(extra + ["-i", iters] + step + args, backend=hip)
        ref = pics.main(extra + ["-i", iters, "--no-fuse"] + step + args, backend=oracle_backend)
        oracle_backend._scratch = None
        print("pics --tgv %s, %s iterations: relative difference %.3e" % (extra, iters, _rel(out, ref)))
        assert _rel(out, ref) < tol, (extra, iters, _rel(out, ref))
    # the objective falls
    obj = {}
    for iters in ("5", "30"):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="pics"):
            pics.main(["-i", iters] + args, backend=hip)
        obj[iters] = _logged(caplog, r"tgv iter \d+, objective (\S+)")[-1]
    assert obj["30"] < obj["5"], obj
