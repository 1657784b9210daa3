"""The case list of tests/test_gpu_sweeps.py reaches the edges it was chosen for -- asserted from the shape arithmetic of
tests/sweep_cases.py (pair_geom / quad_geom, stm_pair_spw / stm_quad_spw, stm_pair_slots / stm_quad_slots and stm_upd_ncb of
csrc/stmmqr_sweep.hip and csrc/stmmqr_device.h restated in Python), not from anyone's reading of the table.  No GPU: the symbolic
phase, the arithmetic and the long-double reference run on the host."""
import importlib

import numpy as np
import pytest

import sweep_cases as sc
from adversarial_fronts import ref_front


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")


def test_the_arithmetic_on_shapes_worked_by_hand():
    """600 x 300, dense: ten panels.  Pairs after panels 1, 3, 5, 7 (9: no column behind the front's last panel); quads after 3 and 7."""
    pair, quad = sc.sweeps(600, 300, None, 2), sc.sweeps(600, 300, None, 4)
    assert [(s.p, s.g1, s.mp, s.nsl, s.ncbp, s.last_width) for s in pair] == [
        (1, 0, 600, 3, 7, 12), (3, 64, 536, 3, 5, 12), (5, 128, 472, 2, 3, 12), (7, 192, 408, 2, 1, 12), (9, 256, 344, 2, -1, 0)]
    assert [(s.p, s.g1, s.mp, s.nsl, s.ncbp, s.last_width) for s in quad] == [(3, 0, 600, 3, 5, 12), (7, 128, 472, 2, 1, 12)]
    assert all(s.spw == 1 and s.ngrp == s.nsl and s.slots == 3 for s in pair + quad)
    assert pair[-1].nb == (32, 12) and not pair[-1].work
    # the front of test_one_front_plan_adversarial (n = 160): the quad sweep has no column, the pair sweep has two once
    assert [(s.p, s.ncbp) for s in sc.sweeps(700, 160, None, 4)] == [(3, 0)]
    assert [(s.p, s.ncbp) for s in sc.sweeps(700, 160, None, 2)] == [(1, 2), (3, 0)]
    # rows run out in panel 2 (70 rows): the quad has V_0, V_1 of 70 and 70 rows, V_2 of 6 columns' worth of rows, no V_3
    s = sc.sweeps(70, 400, None, 4)[0]
    assert (s.nb, s.mpi, s.mp, s.ngrp, s.ncbp) == ((32, 32, 32, 0), (70, 70, 70, 0), 70, 1, 8)
    # slabs per workgroup and the slot stride of the partial sums: stm_pair_spw / stm_quad_spw against stm_*_slots
    assert [sc.pair_spw(n) for n in (15, 16, 31, 32, 63, 64)] == [1, 2, 2, 4, 4, 4]
    assert [sc.quad_spw(n) for n in (15, 16, 31, 32, 63, 64)] == [1, 2, 2, 4, 4, 8]
    assert [sc.pair_slots(n) for n in (3, 15, 16, 64, 65, 203)] == [3, 15, 16, 16, 17, 51]
    assert [sc.quad_slots(n) for n in (3, 15, 16, 64, 128, 129, 203)] == [3, 15, 16, 16, 16, 17, 26]
    # tiles of the applying kernels, 600 x 300, first quad: slab 0 is interior from row 128 on (4 super tiles, one per wave: no whole
    # trip), slab 1 is interior throughout (8 super tiles: one trip per wave, nothing left), slab 2 has 88 rows (2 super tiles, a tail)
    assert sc.tile_forms(quad[0]) == {"head", "tail", "pipeline", ("left", 0), ("left", 1)}
    assert sc.tile_forms(sc.sweeps(230, 400, None, 4)[1]) == {"head", "none"}          # rows ran out: no panel 7, every tile general
    # small or short fronts take no sweep at all
    assert sc.sweeps(600, 96, None, 4) == [] and sc.sweeps(60, 400, None, 2) == []


def test_slots_hold_every_group_count():
    """the host-sizing invariant for ANY rows a sweep may have inside a front of nslf slabs: ngrp <= slots"""
    for nslf in range(1, 300):
        for nsl in range(0, nslf + 1):
            assert (nsl + sc.pair_spw(nsl) - 1) // sc.pair_spw(nsl) <= sc.pair_slots(nslf), (nslf, nsl)
            assert (nsl + sc.quad_spw(nsl) - 1) // sc.quad_spw(nsl) <= sc.quad_slots(nslf), (nslf, nsl)


@pytest.mark.parametrize("w", [2, 4])
def test_case_list_covers_the_edges(w):
    cov = sc.coverage(w)
    print(f"\ncoverage of the sweeps of {w} panels (cases outside the `dead` group, sweeps with rows and columns):")
    for k, v in cov.items():
        print(f"  {k:20s} {sorted(v, key=str) if isinstance(v, set) else v}")
    print(f"  {'case':18s} {'front':>10s} {'kind':7s} sweeps: (p, g1, mp, nsl, spw, ngrp/slots, ncbp, last, nb)")
    for c in sc.CASES:
        for fr in c.fronts:
            rows = [(s.p, s.g1, s.mp, s.nsl, s.spw, f"{s.ngrp}/{s.slots}", s.ncbp, s.last_width, s.nb) for s in sc.front_sweeps(fr, w)]
            print(f"  {c.name:18s} {sc.front_rows(fr):5d}x{fr.fn:<4d} {fr.kind:7s} {rows}")
    assert cov["spw"] == ({1, 2, 4} if w == 2 else {1, 2, 4, 8})
    # both sides of every threshold in consecutive sweeps of one front
    assert cov["spw_pairs"] == ({(16, 15), (32, 31)} if w == 2 else {(16, 15), (32, 31), (64, 63)})
    assert cov["ngrp1"] and cov["partial_group"] and cov["one_row_slab"]
    assert cov["ncbp1"] and cov["ncbp_many"]
    assert {1, 31, 32} <= cov["last_width"]
    # a narrow last panel (1 and 12 columns).  It is never one of the V panels of a sweep with columns: behind panel p of such a sweep
    # lie block 0 and at least one column more, so every panel up to p is 32 wide -- or did nothing (0: its rows ran out)
    assert {1, 12} <= cov["narrow_last_panel"] and cov["v_panel_widths"] == {0, sc.NB}
    assert cov["end_pos"] == set(range(w))
    assert cov["runout_pos"] == set(range(w)) and cov["first_panel_empty"]
    assert cov["unequal_rows"] and cov["chunk_ends"]
    assert cov["launch_above_front"]
    # k_upd_c2 / k_upd_cq in full column blocks: the pipelined interior, every count of interior tiles a wave is left with after
    # its last whole trip (pair: 0 .. 3 tiles; quad: 0 / 1 super tile), general tiles above and below, groups without interior
    assert cov["tile_forms"] == {"head", "tail", "none", "pipeline"} | {("left", k) for k in range(4 if w == 2 else 2)}
    assert cov["slots_ok"]


@pytest.mark.parametrize("w", [2, 4])
def test_every_case_sweeps(w):
    """every case launches a sweep with columns, and outside the cases whose point is a front without rows also one with rows"""
    for c in sc.CASES:
        if w == 4 and c.name in sc.NO_QUAD_COLUMNS:          # five panels: the quad's launch has no column, as at n = 160 elsewhere
            assert not sc.case_launches(c, w), c.name
            continue
        assert sc.case_launches(c, w), c.name
        assert any(s.work for fr in c.fronts for s in sc.front_sweeps(fr, w)), c.name
        for fr in c.fronts:
            for s in sc.front_sweeps(fr, w):
                assert s.ngrp <= s.slots, (c.name, s)
    # the whole-panel dead cases: the panel is one of the first quad / of the pairs 0 and 1
    assert set(sc.DEAD["panel0"]) == set(range(0, 32)) and set(sc.DEAD["panel2"]) == set(range(64, 96))


def test_inputs_are_one_front_each_and_seeded(pkg):
    for c in sc.CASES:
        if max(fr.m for fr in c.fronts) > 4100:
            continue                                       # (the same pattern, taller: seconds of symbolic analysis)
        fronts = [sc.make_front(fr) for fr in c.fronts]
        sym, S, Ap, Ai, Ax = sc.analyzed(pkg, fronts)
        assert [int(x) for x in sym["Fm"][:len(fronts)]] == [sc.front_rows(fr) for fr in c.fronts], c.name
        again = [sc.make_front(fr) for fr in c.fronts]
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(fronts, again))


@pytest.mark.parametrize("name", ["dead_edges", "dead_panel0", "dead_panel2"])
def test_dead_cases_die_where_they_should(name):
    """long double: exactly the columns of sweep_cases.DEAD are dead under tol = 1e-9, and the long-double front of
    sweep_cases.ld_front takes the decisions of adversarial_fronts.ref_front"""
    fr = sc.BY_NAME[name].fronts[0]
    F, St = sc.make_front(fr)
    rank, St_ref, Rdead, _ = ref_front(F, St, fr.fn, sc.TOL_DEAD, fr.fn)
    assert rank == sc.expected_rank(fr)
    assert sorted(np.flatnonzero(Rdead).tolist()) == sorted(sc.DEAD[fr.dead])
    _, St_ld, Rdead_ld = sc.ld_front(F, St, sc.TOL_DEAD)
    assert np.array_equal(St_ld, St_ref) and np.array_equal(Rdead_ld, Rdead)
