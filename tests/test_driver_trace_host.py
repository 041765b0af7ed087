"""The drivers' call traces against tests/golden/driver_traces.json (tests/_driver_trace.py: the fake engine, the
configurations and how the fixture was recorded — on the drivers as they were with three loops each).

Every configuration must ask the same things of the fits and of the engine, in the same order, and leave the same
samples, hypervolume trace, ``np.random`` state and counters behind.  Structure, names, integers (seeds among them)
and booleans are compared exactly; floats at rtol 1e-12, the bar of tests/test_host_surface.py for host goldens
(nothing here goes through BLAS or a device).
"""
import json

import numpy as np
import pytest

import _driver_trace as dt


@pytest.fixture(scope="module")
def golden():
    with open(dt.FIXTURE) as fh:
        return json.load(fh)


def assert_same(got, want, where):
    if isinstance(want, float) and isinstance(got, float):
        assert got == want or abs(got - want) <= 1e-12 * abs(want), (where, got, want)
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (where, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, f"{where}[{i}]")
    elif isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), (where, got, want)
        for k in want:
            assert_same(got[k], want[k], f"{where}.{k}")
    else:
        assert type(got) is type(want) and got == want, (where, got, want)


def test_the_fixture_is_not_degenerate(golden):
    dt.check_fixture(golden)


@pytest.mark.parametrize("name", sorted(dt.CONFIGS))
def test_solve_makes_the_recorded_calls(golden, name):
    got = json.loads(json.dumps(dt.run(name)))          # through JSON, as the fixture went
    want = golden[name]
    assert [r[0] for r in got] == [r[0] for r in want], name
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"{name}: record {i} ({w[0]})")

