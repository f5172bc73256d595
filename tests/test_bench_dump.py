"""`bench.py --dump-outputs DIR` writes what the timed path computed in its last step (bench.py:dump_outputs): float32 (re, im)
pairs, a seeded sample of rows when an output exceeds its share of the budget, the same sample in every column and on every run."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(tmp_path, oracle_backend, monkeypatch):
    from indigo_amd.util import rand64c
    bench = _bench()
    B = oracle_backend
    small = rand64c(10, 3, seed=1)
    big = rand64c(40, 6, 5, seed=2)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * 8 * 5 * 25)           # the big array keeps 25 of its 240 rows
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("small", B.copy_array(small)), ("big", B.copy_array(big))])
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (10, 3, 2)
    np.testing.assert_array_equal(s[..., 0] + 1j * s[..., 1], small)
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (25, 5, 2)
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(240, 25, replace=False))
    np.testing.assert_array_equal(b[..., 0] + 1j * b[..., 1], big.reshape(240, 5, order='F')[rows])
    for name in ("small", "big"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy")))


def test_dump_outputs_stay_within_the_budget(tmp_path, oracle_backend):
    from indigo_amd.util import rand64c
    bench = _bench()
    B = oracle_backend
    arrays = [("x%d" % i, B.copy_array(rand64c(1 << 20, 2, seed=i))) for i in range(3)]        # 48 MiB of (re, im) pairs
    bench.dump_outputs(str(tmp_path), arrays)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert len(os.listdir(tmp_path)) == 3 and total <= 64 * 10 ** 6


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "1", "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout == ""


@pytest.mark.gpu
def test_config1_dumps_its_last_step_and_times_exactly_the_steps_asked_for(tmp_path):
    import scipy.sparse as spp
    from indigo_amd.util import rand64c
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout)
    assert line["steps"] == 3
    assert line["kernels"] and all(float(k["launches_per_step"]).is_integer() for k in line["kernels"].values()), line["kernels"]
    y = np.load(tmp_path / "spmm_y.npy")
    assert y.dtype == np.float32 and y.shape == (10000, 8, 2)
    A = spp.random(10000, 10000, density=0.01, format='csr', random_state=np.random.default_rng(1), dtype=np.float32).astype(np.complex64)
    assert rel_err(y[..., 0] + 1j * y[..., 1], A @ rand64c(10000, 8, seed=1)) < 1e-5
