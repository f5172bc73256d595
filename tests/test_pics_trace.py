"""What the pics driver BUILDS, pinned: for the flag combinations of tests/golden/pics_trace.py the operator trees it logs, the sizes
of the scratch arenas it reserves, every array it allocates (method, name, shape, dtype, in order) and the shape of its result equal
the recordings in tests/golden/pics_trace_oracle.json (numpy oracle backend) and tests/golden/pics_trace_hip.json (MI355X; that
backend fuses differently).  The kernels' numbers have their own float64 tests; this is the wiring between them."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("pics_trace", os.path.join(GOLDEN, "pics_trace.py"))
pics_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pics_trace)


@pytest.fixture(scope="module")
def recorded():
    """{backend: the fixture}, {group: the scans' paths}: both read or written once"""
    return {}, {}


def _check(B, backend, group, case, recorded, tmp_path_factory):
    fixtures, scans = recorded
    if backend not in fixtures:
        with open(pics_trace.fixture_path(backend)) as f:
            fixtures[backend] = json.load(f)
    if group not in scans:
        scans[group] = pics_trace.write_scans(tmp_path_factory.mktemp("trace_" + group), group)
    want = fixtures[backend][group][case]
    got = json.loads(json.dumps(pics_trace.record_case(B, case, group, scans[group])[0]))
    for key in ("shape", "trees", "scratch", "arrays"):
        if got[key] != want[key]:
            pairs = list(zip(got[key], want[key]))
            i = next((i for i, (a, b) in enumerate(pairs) if a != b), len(pairs))
            pytest.fail("%s/%s: %s differs at entry %d of %d recorded (%d now):\nnow      %s\nrecorded %s" % (
                group, case, key, i, len(want[key]), len(got[key]), (got[key] + [None])[i], (want[key] + [None])[i]))


@pytest.mark.parametrize("case", pics_trace.GROUP_CASES["cpu"])
def test_the_driver_builds_what_was_recorded_on_the_oracle_backend(case, oracle_backend, recorded, tmp_path_factory):
    _check(oracle_backend, "oracle", "cpu", case, recorded, tmp_path_factory)


@pytest.mark.gpu
@pytest.mark.parametrize("group,case", [(g, c) for g in pics_trace.BACKEND_GROUPS["hip"] for c in pics_trace.GROUP_CASES[g]])
def test_the_driver_builds_what_was_recorded_on_the_gpu(group, case, hip, recorded, tmp_path_factory):
    _check(hip, "hip", group, case, recorded, tmp_path_factory)
