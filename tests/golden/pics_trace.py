#!/usr/bin/env python3
"""Records what the pics driver BUILDS for a list of flag combinations: the operator trees it logs, the scratch arenas it reserves
and the arrays it allocates, in order.  tests/test_pics_trace.py compares a fresh recording with the fixtures written here.

    python tests/golden/pics_trace.py oracle          # -> tests/golden/pics_trace_oracle.json  (numpy oracle backend, no GPU)
    python tests/golden/pics_trace.py hip             # -> tests/golden/pics_trace_hip.json     (on the MI355X)

The recorder only calls `pics.main(argv, backend=B)` on scans it writes itself from seeded generators, so the same file records
any revision of the driver.  Per case it keeps

    trees     every "tree:" dump of logger `pics`
    scratch   the sizes passed to `reserve_scratch`
    arrays    [method, name, shape, dtype] of every `copy_array`, `zero_array` and `empty_array` call (outermost calls only: the
              `empty_array` inside `zero_array` is not listed, the arena that `reserve_scratch` allocates is)
    shape     the shape of the result
"""
import contextlib
import json
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# image, coils, readout x views, and the gridding options of every run of the group
GROUPS = {
    "cpu": ((12, 10, 8), 3, 16, 40, ["--osf", "1.5"]),
    "gpu": ((32, 32, 32), 2, 64, 100, ["--osf", "2.0", "--width", "2"]),
    "gpu64": ((64, 64, 64), 3, 128, 150, ["--osf", "2.0", "--width", "2"]),         # where the fused leaf takes the maps
}
COMMON = ["--power-iters", "2", "--lamda", "1e-3"]
FMAP = ["--fmap", "{fmap}", "--dwell", "4e-6", "--fmap-segments", "3"]
# name, scan (one frame | three frames of which the first and the last share a trajectory | one frame, two sets of maps), flags
CASES = [
    ("plain", "one", []),
    ("O0", "one", ["-O", "0"]),
    ("no-fuse", "one", ["--no-fuse"]),
    ("frames", "frames", []),
    ("l1", "one", ["--l1", "0.01"]),
    ("tv-l1", "one", ["--tv", "0.01", "--l1", "0.01"]),
    ("tvtime-llr", "frames", ["--tv-time", "0.01", "--llr", "0.02"]),
    ("llr-shifts", "frames", ["--llr", "0.02", "--llr-shifts"]),
    ("basis", "frames", ["--basis", "{basis}"]),
    ("basis-toeplitz-l1", "frames", ["--basis", "{basis}", "--toeplitz", "--l1", "0.01"]),
    ("toeplitz-frames", "frames", ["--toeplitz"]),
    ("maps2", "maps2", []),
    ("maps2-tv", "maps2", ["--tv", "0.01"]),
    ("fmap", "one", FMAP),
    ("fmap-toeplitz-dcf", "one", FMAP + ["--toeplitz", "--dcf", "auto", "--dcf-iters", "3"]),
    ("dcf-frames", "frames", ["--dcf", "auto"]),
]
GROUP_CASES = {"cpu": [c[0] for c in CASES], "gpu": [c[0] for c in CASES], "gpu64": ["maps2", "maps2-tv"]}
BACKEND_GROUPS = {"oracle": ["cpu"], "hip": ["gpu", "gpu64"]}


def write_scans(dirpath, group):
    """the scans of a group, seeded: random k-space and maps, radial trajectories, a smooth real field map, a 3 x 2 basis
    -> {name: path}"""
    from indigo_amd.sense import radial_trajectory
    from indigo_amd.util import rand64c
    N, C, nro, nsp, _ = GROUPS[group]
    pix = np.array(N, dtype=np.float64)[:, None, None]
    trajs = [radial_trajectory(nsp, nro, seed=s) * pix for s in (2, 3, 2)]
    ksps = [rand64c(nro * nsp * C, 1, seed=10 + t).reshape((1, nro, nsp, C), order='F') for t in range(3)]
    maps = rand64c(int(np.prod(N)) * C, 2, seed=20).reshape(N + (C, 2), order='F')
    paths = {k: os.path.join(str(dirpath), "%s_%s" % (group, k)) for k in ("one.npz", "frames.npz", "maps2.npz", "basis.npy", "fmap.npy")}
    np.savez(paths["one.npz"], data=ksps[0].reshape(ksps[0].shape + (1,)).T, maps=maps[..., :1].T, traj=trajs[0].T)
    np.savez(paths["maps2.npz"], data=ksps[0].reshape(ksps[0].shape + (1,)).T, maps=maps.T, traj=trajs[0].T)
    np.savez(paths["frames.npz"], data=np.stack(ksps, axis=-1).reshape(ksps[0].shape + (1,) * 6 + (3,)).T, maps=maps[..., :1].T,
             traj=np.stack(trajs, axis=-1).reshape(trajs[0].shape + (1,) * 7 + (3,)).T)
    g = np.mgrid[tuple(slice(-1, 1, n * 1j) for n in N)]
    np.save(paths["fmap.npy"], (100 * g[0] + 50 * g[1] * g[2]).astype(np.float32).T)
    np.save(paths["basis.npy"], np.array([[1, 1], [1, 0], [1, -1]], dtype=np.float32) / np.sqrt([3, 2]).astype(np.float32))
    return {k.split(".")[0]: p for k, p in paths.items()}


def argv_of(case, group, paths, iters=1):
    _, scan, flags = next(c for c in CASES if c[0] == case)
    return ["-i", str(iters)] + COMMON + GROUPS[group][4] + [f.format(**paths) for f in flags] + [paths[scan]]


@contextlib.contextmanager
def recording(B, trace):
    """wraps B's allocation methods (on the instance) and listens to logger `pics` for the block; fills `trace`"""
    depth = [0]

    def wrap(method, entry, nests):
        inner = getattr(B, method)

        def outer(*a, **kw):
            if not (nests and depth[0]):
                entry(*a, **kw)
            depth[0] += nests
            try:
                return inner(*a, **kw)
            finally:
                depth[0] -= nests
        setattr(B, method, outer)

    def alloc(method):
        def entry(shape, dtype, name=''):
            trace["arrays"].append([method, name, [int(n) for n in np.atleast_1d(shape)], str(np.dtype(dtype))])
        return entry

    class Trees(logging.Handler):
        def emit(self, record):
            text = record.getMessage()
            if text.startswith("tree:"):
                trace["trees"].append(text)

    wrap("reserve_scratch", lambda nelems: trace["scratch"].append(int(nelems)), 0)
    wrap("copy_array", lambda arr, name='': trace["arrays"].append(["copy_array", name, [int(n) for n in arr.shape], str(arr.dtype)]), 1)
    wrap("zero_array", alloc("zero_array"), 1)
    wrap("empty_array", alloc("empty_array"), 1)
    plog, handler = logging.getLogger("pics"), Trees(level=logging.INFO)
    level = plog.level
    plog.addHandler(handler)
    plog.setLevel(logging.INFO)
    try:
        yield trace
    finally:
        plog.removeHandler(handler)
        plog.setLevel(level)
        for method in ("reserve_scratch", "copy_array", "zero_array", "empty_array"):
            delattr(B, method)


def record_case(B, case, group, paths, iters=1):
    """-> (trace, result) of one case on backend B.  The case runs twice and the second run is recorded: what a backend allocates at
    first use and keeps for its lifetime (a slot for results, a grow-only workspace) is no part of what the driver builds, and whether
    it is still to come depends on what the backend has served before"""
    from indigo_amd import pics
    trace = {"trees": [], "scratch": [], "arrays": [], "shape": None}
    argv = argv_of(case, group, paths, iters)
    B._scratch = None
    try:
        pics.main(argv, backend=B)
        B._scratch = None
        with recording(B, trace):
            out = pics.main(argv, backend=B)
    finally:
        B._scratch = None
    trace["shape"] = [int(n) for n in out.shape]
    return trace, out


def fixture_path(backend):
    return os.path.join(HERE, "pics_trace_%s.json" % backend)


def main(argv):
    import tempfile
    backend = argv[0]
    if backend == "oracle":
        from oracle.np_backend import NumpyBackend
        B = NumpyBackend()
    else:
        from indigo_amd.backends import get_backend
        B = get_backend("hip")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for group in BACKEND_GROUPS[backend]:
            paths = write_scans(tmp, group)
            out[group] = {case: record_case(B, case, group, paths)[0] for case in GROUP_CASES[group]}
    with open(argv[1] if len(argv) > 1 else fixture_path(backend), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
