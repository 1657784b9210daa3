"""The PROCESS rows of csrc/stmmqr_knobs.h on the GPU: STMMQR_RSPW, STMMQR_RSPW_W, STMMQR_B0_ONE (how the riders of the passenger
launches are cut between workgroups and which kernel hosts T + block 0), STMMQR_PART_GRAIN / STMMQR_PART_CAP (the parts of the
assembly and C-pack launches) and STMMQR_RHS_BATCH (right-hand sides per pass of the resident-factor operations).  They are read once
per process, so this process sees one value of each; every setting gets a child process of its own (tests/process_knob_child.py)
that runs a battery of small cases (tests/process_knob_cases.py has the table and what each case pins) and reports digests.

The chain: the default child's factors pass the CPU oracle with the project's bounds (integers and flops exact, Tau and the packed
factors within 1e-11 of their 2-norms; the fixtures by parity.compare_numeric) -- every child checks that itself, and for every rider
case that options.lookahead = 0 (k_upd_w + k_upd_c, which read none of these knobs) gives the bits of lookahead = 2 in the same
process -- and every knob child's digests equal the default child's bit for bit.  That a forced value arrived, and what the launcher
chose where none was forced: under STMMQR_DBG = 131072 the host launchers print one line per launch with riders; every case must
report the launches process_knob_cases.rider_launches derives from the shapes (never none) with the slabs per rider and slab groups of
process_knob_cases.expected_report.

Two cases run in this process with no knob set: fronts tall and wide enough for the launchers' own rule to take two slabs per rider
(more than 240 rider tiles in a launch), on k_panel_pc and on k_panel_ca_pc.

Children run one after the other with a safety limit of 300 s (it asserts nothing about speed).  A child that ends by a signal, by
exit code 134 / 139 or at the limit fails its test, and every later test of the module fails at once without starting a child."""
import importlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import pytest

import process_knob_cases as pk

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CHILD = ROOT / "tests" / "process_knob_child.py"
LIMIT = 300
_STATE = {"dead": None, "default": {}}


def run_child(battery, knobs, tmp):
    if _STATE["dead"]:
        pytest.fail(f"no child started: an earlier one ended abnormally ({_STATE['dead']})")
    out = tmp / f"{battery}_{pk.setting_id(knobs).replace(',', '_').replace('=', '')}.json"
    env = dict(os.environ, **knobs)
    t0 = time.monotonic()
    try:
        r = subprocess.run([sys.executable, str(CHILD), battery, str(out)], capture_output=True, text=True, env=env, timeout=LIMIT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _STATE["dead"] = f"{battery} {pk.setting_id(knobs)}: still running after {LIMIT} s"
        pytest.fail(_STATE["dead"])
    if r.returncode < 0 or r.returncode in (134, 139):
        _STATE["dead"] = f"{battery} {pk.setting_id(knobs)}: exit code {r.returncode}"
        pytest.fail(_STATE["dead"] + "\n" + r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads(out.read_text())
    print(f"child {battery} [{pk.setting_id(knobs)}]: {time.monotonic() - t0:.1f} s in all, {d['wall']:.1f} s in its battery")
    return d


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("process_knobs")


@pytest.fixture(scope="module")
def default(tmp):
    """battery -> the child's report with no knob set (run once per battery, at its first use)"""
    def get(battery):
        if battery not in _STATE["default"]:
            _STATE["default"][battery] = run_child(battery, {}, tmp)
        return _STATE["default"][battery]
    return get


def check_rider_reports(d, knobs):
    assert sorted(d["reports"]) == sorted(c.name for c in pk.RIDER_CASES)
    for case in pk.RIDER_CASES:
        reports = d["reports"][case.name]
        print(f"  {case.name}: {len(reports)} rider launches, {d['seconds'][case.name]} s")
        assert len(reports) > 0, case.name
        pk.check_reports(case, knobs, reports)


def same_digests(d, ref):
    assert sorted(d["digests"]) == sorted(ref["digests"])
    differ = [k for k in ref["digests"] if d["digests"][k] != ref["digests"][k]]
    assert not differ, f"other bits than the default process in {differ}"


def test_rider_battery_default(default):
    d = default("rider")
    assert len(d["digests"]) == len(pk.RIDER_CASES)
    check_rider_reports(d, {})


@pytest.mark.parametrize("knobs", pk.RIDER_SETTINGS, ids=pk.setting_id)
def test_rider_battery_under_a_knob(default, tmp, knobs):
    ref = default("rider")
    d = run_child("rider", knobs, tmp)
    check_rider_reports(d, knobs)
    same_digests(d, ref)


@pytest.mark.parametrize("knobs", pk.PARTS_SETTINGS, ids=pk.setting_id)
def test_parts_battery_under_a_knob(default, tmp, knobs):
    ref = default("parts")
    assert len(ref["digests"]) == len(pk.PARTS_FIXTURES) + 1
    same_digests(run_child("parts", knobs, tmp), ref)


@pytest.mark.parametrize("knobs", pk.BATCH_SETTINGS, ids=pk.setting_id)
def test_batch_battery_under_a_knob(default, tmp, knobs):
    ref = default("batch")
    assert len(ref["digests"]) == 11 * len(pk.BATCH_FIXTURES)
    same_digests(run_child("batch", knobs, tmp), ref)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


@pytest.mark.parametrize("case", pk.ORGANIC_CASES, ids=lambda c: c.name)
def test_the_launchers_own_rule_takes_two_slabs(pkg, oracle, case):
    """no knob set: more than 240 rider tiles in a launch, so the rule of stm_launch_panel_pc / stm_launch_panel_ca_pc groups two slabs
    per rider; lookahead = 0 gives the same bits and the oracle its bounds (process_knob_cases.run_rider_case)"""
    if _STATE["dead"]:
        pytest.fail(f"not run: a child ended abnormally ({_STATE['dead']})")
    assert not any(k in os.environ for s in pk.RIDER_SETTINGS for k in s)
    t0 = time.monotonic()
    _, reports = pk.run_rider_case(pkg, oracle, case)
    print(f"{case.name}: {len(reports)} rider launches, {time.monotonic() - t0:.2f} s")
    pk.check_reports(case, {}, reports)
    grouped = [r for r in reports if r[0].startswith("k_panel") and r[1] * r[2] * r[3] > 240]
    print(f"  launches above 240 tiles: {grouped}")
    assert grouped and all(r[4] == 2 for r in grouped)
    if case.name == "4090x545":
        assert grouped == [["k_panel_pc", 1, 16, 16, 2, 8]]
    else:
        assert grouped == [["k_panel_ca_pc", 1, 16, 17, 2, 9], ["k_panel_ca_pc", 1, 15, 17, 2, 9]]
