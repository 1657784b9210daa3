"""The column step of the panel pipeline (dev_tall_group / dev_wave_panel, csrc/stmmqr_panel.hip) on fronts one row into each
register class of a column group and at its top: against the CPU oracle, and bit for bit against the results of the build before
the step lost its memory waits and the row masks of its rows r >= 1 (tests/golden/column_step/column_step_parent.npz, written by
tests/golden/make_column_step_golden.py).  Every panel runs as a pipeline of column groups (big_front_cols = 8,
tall_min_rows = 0, panel_algo = 1): rows <= 512 one row per thread (or the wave panel), <= 1024 two, <= 2048 four,
<= 4096 eight in 4-column groups, <= 8192 sixteen in 2-column groups."""
import importlib
from pathlib import Path

import numpy as np
import pytest

from column_step_cases import (DEAD_AT, GOLDEN, NO_WAVE_PANEL, golden_case, in_staircase, make_dead_front, make_front,
                               pin, run_front)

pytestmark = pytest.mark.gpu
GOLDEN_FILE = Path(__file__).resolve().parent / "golden" / "column_step" / "column_step_parent.npz"


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


def check_against_oracle(pkg, oracle, monkeypatch, F0, St0, npiv, tol, ntol, dbg=None):
    """As test_qr_front: rank, Stair, Rdead and flops exact, Tau and F within the project's 1e-11 (relative, 2-norm)."""
    if dbg is not None:
        monkeypatch.setenv("STMMQR_DBG", str(dbg))
    try:
        rg, Tg, Dg, flg, Fg, Sg = run_front(pkg, F0, St0, npiv, tol, ntol)
    finally:
        if dbg is not None:
            monkeypatch.delenv("STMMQR_DBG")
    Fo, So = F0.copy(order="F"), St0.copy()
    ro, To, Do, flo = oracle.front(Fo, So, npiv, tol, ntol)
    assert rg == ro
    np.testing.assert_array_equal(Sg, So)
    np.testing.assert_array_equal(Dg, Do)
    assert flg == flo
    dT, dF = np.linalg.norm(Tg - To), np.linalg.norm(Fg - Fo)
    print(f"|dTau| {dT:.3e} / {max(np.linalg.norm(To), 1):.3e}   |dF| {dF:.3e} / {np.linalg.norm(Fo):.3e}")
    assert dT <= 1e-11 * max(np.linalg.norm(To), 1)
    assert dF <= 1e-11 * np.linalg.norm(Fo)
    return rg, Dg, Fg, Sg


@pytest.mark.parametrize("stair", ["full", "steps", "tail", "diag12"])
@pytest.mark.parametrize("m", [300, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192])
def test_register_classes(pkg, oracle, monkeypatch, m, stair):
    """n = npiv = 37: one full panel and a 5-column one (a group with fewer columns than its width).  m = 300 with the wave
    panel switched off: the group with one row per thread.  ("steps" stays short whatever m is -- the wave panel; "tail" is
    the same staircase ending at row m, so that the irregular steps reach every class.)"""
    F0, St0 = make_front(m, 37, 1234 + m, stair)
    _, _, Fg, Sg = check_against_oracle(pkg, oracle, monkeypatch, F0, St0, 37, -1.0, 37, NO_WAVE_PANEL if m == 300 else None)
    assert not Fg[~in_staircase(St0, Sg, m)].any()             # (what the unmasked rows rely on, on the way out)


@pytest.mark.parametrize("m", [1025, 2049])
def test_dead_columns(pkg, oracle, monkeypatch, m):
    """tol = 1e-9 on every pivot: a duplicate column in the middle, first and last of a group, and a zero column."""
    F0, St0 = make_dead_front(m)
    rg, Dg, _, Sg = check_against_oracle(pkg, oracle, monkeypatch, F0, St0, 37, 1e-9, 37)
    assert rg == 37 - len(DEAD_AT)
    assert all(Dg[k] == 1 and Sg[k] == 0 for k in DEAD_AT) and Dg.sum() == len(DEAD_AT)


@pytest.mark.parametrize("m,n,npiv", [(520, 600, 560), (1030, 1100, 1100)])
def test_rows_run_out_inside_a_group(pkg, oracle, monkeypatch, m, n, npiv):
    F0, St0 = make_front(m, n, 4321, "steps")
    check_against_oracle(pkg, oracle, monkeypatch, F0, St0, npiv, -1.0, n)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN_FILE)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_same_bits_as_the_parent(pkg, golden, monkeypatch, name):
    (F0, St0), npiv, tol, ntol, dbg = golden_case(name)
    if dbg is not None:
        monkeypatch.setenv("STMMQR_DBG", str(dbg))
    try:
        r, Tau, Rdead, fl, F, St = run_front(pkg, F0, St0, npiv, tol, ntol)
    finally:
        if dbg is not None:
            monkeypatch.delenv("STMMQR_DBG")
    head, dig = pin(F, St0, St)
    assert r == int(golden[name + "_rank"]) and fl == float(golden[name + "_flops"])
    assert np.array_equal(St, golden[name + "_Stair"])
    assert np.array_equal(Rdead, golden[name + "_Rdead"])
    assert np.array_equal(Tau, golden[name + "_Tau"])
    assert np.array_equal(head, golden[name + "_head"])
    assert np.array_equal(dig, golden[name + "_digest"])
