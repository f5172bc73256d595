"""The reference-side binding (integration/hip_backend_for_indigo.py = INTEGRATION.md section 2 as a file) is EXECUTABLE:

  * its ctypes prototype table equals indigo_amd/_lib.py:PROTOTYPES -- which tests/test_abi.py keeps equal to include/indigo_hip.h
    and to the exports of the built library -- so a stub that drifts from the header fails here;
  * the host-only shim of the ABI (tests/abi_shim/ig_shim.c: the same ig_* symbols as CPU loops, test infrastructure) compiles
    against the real header: a changed prototype is a compile error;
  * the binding RUNS on top of the shim, as a subclass of the restated Backend base class (indigo_amd/backends/backend.py, which
    stands in for the reference's `indigo.backends.backend`), and reproduces the vectors captured from the reference
    (tests/golden): dndarray semantics, BLAS-1, FFT, csr / exwrite csr, dia, onemm, cgemm / csymm, apgd, composites, the SENSE
    tree and cg.  (tests/abi_shim/run_reference_tests.py runs the reference's own backend tests on it where a reference tree is
    at hand.)
No GPU, nothing outside the repository."""
import ast
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "integration", "hip_backend_for_indigo.py")
SHIM_SRC = os.path.join(ROOT, "tests", "abi_shim", "ig_shim.c")


def _stub_prototypes():
    """the stub's PROTOTYPES table, evaluated without importing the stub (it imports the reference's Backend)"""
    tree = ast.parse(open(STUB).read())
    env = {"C": ctypes}
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, (ast.Name, ast.Tuple)) for t in node.targets):
            names = [n.id for t in node.targets for n in ast.walk(t) if isinstance(n, ast.Name)]
            if "PROTOTYPES" in names or "c_f" in names:
                exec(compile(ast.Module([node], []), STUB, "exec"), env)
    return env["PROTOTYPES"]


def test_stub_prototypes_equal_the_abi():
    from indigo_amd import _lib
    protos = _stub_prototypes()
    assert len(protos) >= 20
    for name, (res, args) in protos.items():
        assert name in _lib.PROTOTYPES, name
        r2, a2 = _lib.PROTOTYPES[name]
        assert res == r2, (name, res, r2)
        assert len(args) == len(a2), (name, len(args), len(a2))
        for i, (u, v) in enumerate(zip(args, a2)):
            # (a POINTER(T) parameter may be declared as a bare void pointer on either side: same ABI)
            same = u == v or {u, v} <= {ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)} and ctypes.c_void_p in (u, v)
            assert same, (name, i, u, v)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("abi_shim") / "libig_shim.so")
    r = subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror=implicit-function-declaration", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                        SHIM_SRC, "-o", out, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, "the shim no longer compiles against include/indigo_hip.h (a prototype drifted?):\n" + r.stderr
    return out


def test_shim_defines_every_symbol_the_stub_binds(shim):
    L = ctypes.CDLL(shim)
    for name in _stub_prototypes():
        assert hasattr(L, name), name
    assert L.ig_abi_version() == 1


@pytest.fixture
def binding(shim, monkeypatch):
    """the binding's HipBackend on the shim; `indigo.backends.backend` resolves to the restated Backend for this test only"""
    import importlib.util
    import types
    from indigo_amd.backends import backend as restated
    monkeypatch.setenv("INDIGO_HIP_LIB", shim)
    for name in ("indigo", "indigo.backends"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        monkeypatch.setitem(sys.modules, name, pkg)
    monkeypatch.setitem(sys.modules, "indigo.backends.backend", restated)
    spec = importlib.util.spec_from_file_location("indigo.backends.hip", STUB)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HipBackend()


def test_binding_on_the_shim_reproduces_the_reference_goldens(binding):
    import numpy as np
    import test_oracle                  # the golden checks of the oracle, run here on the binding instead
    from conftest import check_misc_leaves, golden, rel_err
    from indigo_amd.sense import SenseProblem
    B = binding
    # dndarray semantics: round trip, 2-D views, device copy, reshape
    a = np.asfortranarray((np.arange(60).reshape(6, 10) * (1 + 2j)).astype(np.complex64))
    d = B.copy_array(a)
    np.testing.assert_array_equal(d.to_host(), a)
    np.testing.assert_array_equal(d[1:4, 2:7].to_host(), a[1:4, 2:7])
    np.testing.assert_array_equal(d[:, 3:5].to_host(), a[:, 3:5])
    np.testing.assert_array_equal(d.copy().to_host(), a)
    np.testing.assert_array_equal(d.reshape((60, 1)).to_host(), a.reshape(60, 1, order='F'))
    assert B.mem_usage() >= a.nbytes
    # the leaves and composites, against what the reference computed from the same inputs
    test_oracle.test_blas_leaves(B)
    test_oracle.test_fft_leaves(B)
    test_oracle.test_csrmm_leaves(B, "numpy")
    check_misc_leaves(B, test_oracle.TOL)
    test_oracle.test_composites(B)
    # the SENSE tree (reference leaves, level 0) and cg on its normal equations
    g = golden("sense")
    C, width, ntab, osf, ro, tr = g["params"]
    p = SenseProblem(tuple(int(n) for n in g["N"]), g["coord"], np.asfortranarray(g["maps"]), width=int(width), ntable=int(ntab),
                     oversamp=float(osf))
    A = p.build_tree(B, level=0)
    assert rel_err(A * g["sense_x"], g["sense_Ax"]) < 1e-5
    assert rel_err(A.H * g["sense_k"], g["sense_AHk"]) < 1e-5
    AHA = A.H * A + float(g["lamda"]) * B.Eye(A.shape[1])
    for it in (1, 2, 3):
        x0 = np.zeros((A.shape[1], 1), dtype=np.complex64, order='F')
        B.cg(AHA, g["cg_b"].copy(order='F'), x0, maxiter=it)
        assert rel_err(x0, g["cg_it%d" % it]) < 1e-4
