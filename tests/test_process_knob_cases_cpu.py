"""What the case table of tests/process_knob_cases.py covers, computed from the table and the mirrors of the host rules alone (no GPU):
the mirrors against hand-computed values, the edges of the riders' slab groups that some (case, setting) must reach, and that every
(STMMQR_PART_GRAIN, STMMQR_PART_CAP) pair of the parts battery cuts some front of its fixtures in a non-trivial way."""
import itertools

import pytest

import process_knob_cases as pk


def test_rider_rspw_by_hand():
    # 16 x 16 = 256 tiles: k = 1 two rounds of 6, k = 2 one round (128 workgroups) of 7, k = 4 one of 9
    assert pk.rider_rspw(1, 16, 16) == 2
    # 15 x 16 = 240 tiles: one round of 6 with one slab per rider
    assert pk.rider_rspw(1, 15, 16) == 1
    # 16 x 17 = 272 tiles: k = 1 two rounds (12), k = 2 16 x 9 = 144 workgroups, one round of 7
    assert pk.rider_rspw(1, 16, 17) == 2
    # the boundary itself, with two fronts and through the number of slabs: 240 tiles one slab per rider, 241 .. two
    assert pk.rider_rspw(2, 12, 10) == 1 and pk.rider_rspw(1, 1, 240) == 1 and pk.rider_rspw(1, 1, 241) == 2
    assert pk.rider_rspw(2, 11, 11) == 2                       # 242 tiles: 2 x 11 x 6 = 132 workgroups
    # two rounds whatever the grouping up to 4: 4 x 30 x 16 = 1920 tiles -> k = 8 is the first with one round (240 workgroups, 13)
    assert pk.rider_rspw(4, 30, 16) == 8
    # the knob overrides, 0 and negative values do not
    assert pk.rider_rspw(1, 16, 16, 3) == 3 and pk.rider_rspw(1, 2, 3, 16) == 16 and pk.rider_rspw(1, 16, 16, 0) == 2
    # every test-size launch of the battery is far below 240 tiles: one slab per rider unless forced
    assert all(pk.rider_rspw(unfr, uncb, sl) == 1 for unfr in (1, 2) for uncb in (1, 2) for sl in (3, 6))


def test_work_parts_by_hand():
    assert pk.work_parts(600 * 97) == 29                       # 58200 / 2048 = 28.4
    assert pk.work_parts(1) == 1 and pk.work_parts(0) == 1
    assert pk.work_parts(2048) == 1 and pk.work_parts(2049) == 2
    assert pk.work_parts(8_388_608) == 4096 and pk.work_parts(8_388_609) == 4096 and pk.work_parts(8_386_561) == 4096
    assert pk.work_parts(8_386_560) == 4095
    assert pk.work_parts(58200, 1 << 40, 4096) == 1 and pk.work_parts(58200, 64, 4096) == 910
    assert pk.work_parts(58200, 1, 3) == 3 and pk.work_parts(58200, 1, 4096) == 4096 and pk.work_parts(58200, 2048, 1) == 1


def test_rider_launches_by_hand():
    # 600 x 97: steps 0 and 1 ride (65 and 33 trailing columns), the riders of step t behind the panels of step t + 1
    assert pk.rider_launches([(600, 97)]) == [(0, "k_upd_b0w", 1, 2, 3), (1, "k_panel_pc", 1, 2, 3), (1, "k_upd_b0w", 1, 1, 3),
                                               (2, "k_panel_pc", 1, 1, 3)]
    assert [x[1] for x in pk.rider_launches([(600, 97)], panel_algo=2, b0_one=0)] == ["k_upd_fw", "k_panel_ca_pc"] * 2
    assert pk.rider_launches([(300, 95), (600, 97)]) == [(0, "k_upd_b0w", 2, 2, 3), (1, "k_panel_pc", 2, 2, 3), (1, "k_upd_b0w", 2, 1, 3),
                                                          (2, "k_panel_pc", 2, 1, 3)]
    assert pk.rider_launches([(500, 97)]) == []                # two slabs: the one-workgroup update, nothing rides
    assert pk.rider_launches([(600, 64)]) == []                # no second column block behind block 0
    # the organic cases: 16 rider blocks x 16 slabs on k_panel_pc; 17 slabs, panels 1 .. 3 Gram-based (4200 - 32 p > 4096)
    a = pk.rider_launches(pk.case_dims(pk.ORGANIC_CASES[0]))
    assert a[1] == (1, "k_panel_pc", 1, 16, 16) and all(x[1] != "k_panel_ca_pc" for x in a)
    b = [x for x in pk.rider_launches(pk.case_dims(pk.ORGANIC_CASES[1])) if x[1].startswith("k_panel")]
    assert b[:4] == [(1, "k_panel_ca_pc", 1, 16, 17), (2, "k_panel_ca_pc", 1, 15, 17), (3, "k_panel_ca_pc", 1, 14, 17),
                     (4, "k_panel_pc", 1, 13, 17)]
    assert [pk.expected_report(x, {}) for x in b[:3]] == [(2, 9), (2, 9), (1, 17)]


def all_groups():
    return [g for case, env in itertools.product(pk.RIDER_CASES, [{}] + pk.RIDER_SETTINGS) for g in pk.rider_groups(case, env)]


def test_rider_coverage():
    G = all_groups()
    assert G

    def some(pred):
        return any(pred(g) for g in G)
    # slab groups of a launch: one, two, three or more
    assert some(lambda g: g["uy"] == 1) and some(lambda g: g["uy"] == 2) and some(lambda g: g["uy"] >= 3)
    # a rider that owns several slabs with rows in more than one of them
    assert some(lambda g: g["rspw"] > 1 and max(g["rows"]) > pk.SLAB)
    # the last group shorter than the others: by the launch's slabs, and by the rows (a group of one row, of a partial slab, empty)
    assert some(lambda g: g["uy"] >= 2 and g["umaxsl"] % g["rspw"] != 0)
    assert some(lambda g: g["uy"] == 2 and g["rows"][1] == 1)
    assert some(lambda g: g["uy"] == 2 and g["rows"][1] == 0 and g["rows"][0] == g["rspw"] * pk.SLAB)
    assert some(lambda g: g["uy"] == 2 and g["rows"][1] % pk.SLAB not in (0, 1) and g["rspw"] > 1)
    # a group longer than the front's rows (power of two and not)
    assert some(lambda g: g["rspw"] * pk.SLAB > g["nsl"] * pk.SLAB and g["uy"] == 1)
    assert some(lambda g: g["rspw"] == 3 and g["uy"] == 2)
    # the panel's rows end on a slab boundary inside a group, one row past such a boundary, and in a partial chunk
    inside = lambda g, mp: g["rspw"] > 1 and mp % pk.SLAB == 0 and (mp // pk.SLAB) % g["rspw"] != 0
    assert some(lambda g: inside(g, g["mp"]))
    assert some(lambda g: inside(g, g["mp"] - 1))
    assert some(lambda g: g["rspw"] > 1 and g["mp"] % pk.RB != 0 and g["mp"] > pk.SLAB)
    # ... and exactly at the end of a group
    assert some(lambda g: g["rspw"] > 1 and g["uy"] > 1 and g["mp"] == g["rspw"] * pk.SLAB)
    # a front with fewer slabs than the launch
    assert some(lambda g: g["nsl"] < g["umaxsl"] and g["rspw"] > 1)
    # rider column blocks of 1, 31 and 32 columns
    for nc in (1, 31, 32):
        assert some(lambda g: nc in g["cols"] and g["rspw"] > 1), nc
    # the two-ahead reload of dev_upd_c_h2 (r0 + 4 chunks < end of the group's rows): half 0 from 257 rows on, half 1 from 321 --
    # both, one half only, many trips, odd and even chunk counts per half
    chunks = lambda rows: -(-rows // pk.RB)
    assert some(lambda g: any(r > 5 * pk.RB for r in g["rows"]))
    assert some(lambda g: any(4 * pk.RB < r <= 5 * pk.RB for r in g["rows"]))
    assert some(lambda g: any(r >= 16 * pk.RB for r in g["rows"]))
    assert some(lambda g: any(chunks(r) > 8 and chunks(r) % 4 == 1 for r in g["rows"]))
    assert some(lambda g: any(chunks(r) > 8 and chunks(r) % 4 == 2 for r in g["rows"]))
    # both hosts
    assert {g["host"] for g in G} == {"k_panel_pc", "k_panel_ca_pc"}
    # with one slab per rider none of the reload trips exist: that is what the default process runs at these sizes
    D = [g for case in pk.RIDER_CASES for g in pk.rider_groups(case, {})]
    assert D and all(g["rspw"] == 1 and max(g["rows"]) <= pk.SLAB for g in D)


def test_organic_cases_group_by_the_rule():
    for case, host, tiles in ((pk.ORGANIC_CASES[0], "k_panel_pc", [256]), (pk.ORGANIC_CASES[1], "k_panel_ca_pc", [272, 255])):
        G = [g for g in pk.rider_groups(case, {}) if g["umaxsl"] * len(g["cols"]) > 240]
        assert [g["umaxsl"] * len(g["cols"]) for g in G] == tiles
        assert all(g["host"] == host and g["rspw"] == 2 for g in G)
    g = [g for g in pk.rider_groups(pk.ORGANIC_CASES[1], {}) if g["rspw"] == 2][0]
    assert g["uy"] == 9 and g["rows"][-1] == 4200 - 4096      # the last group: one partial slab


@pytest.mark.parametrize("knobs", pk.PARTS_SETTINGS, ids=pk.setting_id)
def test_parts_coverage(knobs):
    grain, cap = int(knobs["STMMQR_PART_GRAIN"]), int(knobs["STMMQR_PART_CAP"])
    cuts = [wp for name in pk.PARTS_FIXTURES for wp in pk.parts_of_fixture(name, grain, cap)]
    cuts.append((pk.M * pk.FN, pk.work_parts(pk.M * pk.FN, grain, cap)))
    big = [(w, p) for w, p in cuts if w > 2048]                  # fronts that the default grain cuts into several parts
    one = any(p == 1 for w, p in big)
    at_cap = any(p == cap and pk.ceil_div(w, grain) > cap for w, p in cuts)
    empty = any(p > pk.ceil_div(w, 256) for w, p in big)       # part q takes every p-th slab of 256 entries
    assert one or at_cap or empty
    # ... and what each pair is there for
    want = {(1 << 40, 4096): one and not at_cap and not empty,                  # one part for everything
            (64, 4096): all(p > pk.work_parts(w) for w, p in big) and at_cap,    # many parts (a grain below a slab: three in four empty)
            (1, 3): at_cap and not one and any(pk.ceil_div(w, 256) % 3 for w, p in big),       # the cap with an uneven cut
            (1, 4096): at_cap and empty and not one,                            # more parts than slabs
            (2048, 1): one and at_cap and not empty}                            # capped at one part
    assert want[(grain, cap)]
