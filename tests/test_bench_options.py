"""A plain `bench.py` run does only what its headline needs; `--full` adds the CPU baselines, the parity checks and, on the
default config, the extra measurements of other configurations (bench.py:parse)."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return mod.parse()


def test_plain_run_skips_every_extra(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full
    assert a.no_cpu_baseline and a.no_config5 and a.no_leaf_configs and a.no_dense
    assert (a.gpus, a.steps, a.warmup, a.config, a.standard, a.dump_outputs) == (1, 7, 2, 4, True, "")


def test_full_run_keeps_every_extra(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--full")
    assert a.full
    assert not (a.no_cpu_baseline or a.no_config5 or a.no_leaf_configs or a.no_dense)
    assert (a.steps, a.warmup, a.config, a.standard) == (7, 2, 4, True)


def test_full_run_parts_can_still_be_switched_off(monkeypatch):
    a = _parse(monkeypatch, "--full", "--no-extras")
    assert a.no_config5 and a.no_leaf_configs and a.no_dense and not a.no_cpu_baseline
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--no-dense")
    assert a.no_cpu_baseline and a.no_dense and not (a.no_config5 or a.no_leaf_configs)


@pytest.mark.gpu
def test_config1_checks_against_the_oracle_only_with_full():
    lines = {}
    for extra in ([], ["--full"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "1", "--steps", "3", "--warmup", "1"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[bool(extra)] = json.loads(r.stdout)
    plain, full = lines[False], lines[True]
    assert plain["cpu_baseline"] is None and plain["parity_rel_err"] is None
    assert full["cpu_baseline"]["value"] > 0 and full["parity_rel_err"] < 1e-5
    for line in (plain, full):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["unit"] == "products/s" and line["higher_is_better"] is True
