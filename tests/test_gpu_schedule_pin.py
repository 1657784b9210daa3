"""The planner and the step scheduler against the build before they moved into units of their own and the environment knobs into
one table (tests/golden/schedule_pin/schedule_pin_parent.json, written on that build by tests/golden/make_schedule_pin.py).
Every pinned value is compared exactly: a host refactor that changes a launch count, a byte of device memory or a bit of the
factors has changed behaviour."""
import importlib
import json

import pytest

from schedule_pin_cases import CASES, run_case
from stmmqr_testlib import GOLDEN

pytestmark = pytest.mark.gpu
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    assert p.device_count() >= 1, "no GPU visible"
    return p


@pytest.fixture(scope="module")
def parent():
    return json.loads((GOLDEN / "schedule_pin" / "schedule_pin_parent.json").read_text())


@pytest.mark.parametrize("fixture,setting", CASES)
def test_schedule_and_factors_as_the_parent(pkg, parent, fixture, setting):
    want = parent[f"{fixture}/{setting}"]
    got = run_case(pkg, fixture, setting)
    for which, (a, b) in enumerate(zip(got, want)):
        diff = {k: (a[k], b[k]) for k in b if a[k] != b[k]}
        print(fixture, setting, "factorization", which + 1, a)
        assert not diff and a.keys() == b.keys(), f"factorization {which + 1}: (got, parent) {diff}"
    assert len(got) == len(want) == 2
