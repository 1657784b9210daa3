"""The numpy model of the packed factors and of the download's window edges (tests/pack_window_cases.py), without a GPU:

* the model's Post-order block offsets, fed with the REAL reference's HStair / Hm, are the reference's Rblock offsets on every fixture;
* classify_edges equals a brute-force classifier that labels every position of the stack, on the small fixtures, for every window
  of window_list and every kept set of 0, 1 or 3 fronts;
* every aimed window produces an edge of the class it aims at;
* the windows tests/test_gpu_download_windows.py downloads with reach every class the layouts have, whichever fronts the planner
  keeps -- except what UNREACHABLE records, each entry of which is reached on another fixture."""
import itertools

import numpy as np
import pytest

from pack_window_cases import (CLASSES, EXACT, INNER, MAX_WINDOWS, aimed_windows, classify_edges, classify_edges_per_front, packed_layout,
                               window_edges, window_list)
from stmmqr_testlib import GOLDEN, Symbolic, load_golden

I64 = np.int64
WITH_FACTORS = sorted(p.stem for p in GOLDEN.glob("*.npz")
                      if {"num_HStair", "num_Hm", "num_Rblock_off"} <= set(np.load(p).files))
SMALL = [n for n in WITH_FACTORS if n.startswith("syn_")]
# the fixtures of tests/test_gpu_download_windows.py::test_windows_equal_one_copy
GPU_FIXTURES = ["syn_dense6x4", "syn_wide5x8", "syn_dupcol", "syn_rankdef_grid", "syn_grid3d", "dwt_992", "lns_3937", "bayer10"]
SINGLES_ONLY = ("lns_3937", "bayer10")          # too many fronts to enumerate the subsets of three: every single front as the kept one
_cache = {}


def layout_of(name, keep_h):
    """the layout of a fixture from the reference's own HStair / Hm (computed once, never changed)"""
    if (name, keep_h) not in _cache:
        g = load_golden(name)
        _cache[(name, keep_h)] = (g, packed_layout(Symbolic(g), g["num_HStair"], g["num_Hm"], keep_h))
    return _cache[(name, keep_h)]


def kept_sets(nf, sizes=(0, 1, 2, 3)):
    for q in sizes:
        if q <= nf:
            yield from itertools.combinations(range(nf), q)


# ---- 1: the model against the reference ----
@pytest.mark.parametrize("name", WITH_FACTORS)
def test_block_offsets_are_the_reference_s(name):
    g, L = layout_of(name, True)
    nf = L["nf"]
    assert np.array_equal(L["block_off"][:nf], np.asarray(g["num_Rblock_off"], I64)[:nf])
    if "num_rh_size" in g and g["num_rh_size"].size == nf:
        assert np.array_equal(L["block_size"][:nf], np.asarray(g["num_rh_size"], I64))
    if g["num_Stack"].size > 1:
        last = L["post"][-1]
        assert int(L["block_off"][last] + L["block_size"][last]) == g["num_Stack"].size == L["rh_total"]
    # without H every column keeps its R rows only: a prefix of the column with H
    L0 = layout_of(name, False)[1]
    for F1, F0 in zip(L["fronts"], L0["fronts"]):
        assert np.array_equal(F0["rlen"], F1["rlen"]) and not F0["hlen"].any()
        assert np.array_equal(np.diff(F0["off"]), F1["rlen"])


# ---- 2: the classifier against brute force ----
_labels, _brute = {}, {}


def labels_of(name, L):
    """every position of the stack labelled, one by one, with the front, the column and the row of the column it lies in, and
    whether it lies inside or at either end of a dead pivot column of its own block"""
    key = (name, L["keep_h"])
    if key not in _labels:
        total = L["rh_total"]
        front = np.full(total + 1, -1, I64); col = np.full(total + 1, -1, I64); rel = np.zeros(total + 1, I64)
        for f in L["post"]:
            F, b0 = L["fronts"][f], int(L["block_off"][f])
            for k in range(F["fn"]):
                for i in range(int(F["off"][k]), int(F["off"][k + 1])):
                    front[b0 + i], col[b0 + i], rel[b0 + i] = f, k, i - int(F["off"][k])
        in_dead = np.zeros(total + 1, bool)
        for f in L["post"]:
            F, b0 = L["fronts"][f], int(L["block_off"][f])
            for k in range(F["fn"]):
                if F["dead"][k]:
                    for p in range(b0 + int(F["off"][k]), b0 + int(F["off"][k + 1]) + 1):
                        in_dead[p] |= front[p] == f
        _labels[key] = (front, col, rel, in_dead)
    return _labels[key]


def brute_force_per_front(name, L, win):
    """{front: {class: count}}: the edges read off the labels one by one"""
    key = (name, L["keep_h"], win)
    if key in _brute:
        return _brute[key]
    front, col, rel, in_dead = labels_of(name, L)
    total = L["rh_total"]
    out = {f: {c: 0 for c in CLASSES} for f in range(L["nf"])}
    edges = [p for p in range(1, total) if p % win == 0]
    per_col = {}
    for p in edges:
        f, k, r = int(front[p]), int(col[p]), int(rel[p])
        assert f >= 0
        F, w = L["fronts"][f], out[f]
        rl, hl = int(F["rlen"][k]), int(F["hlen"][k])
        if k < F["fp"]:
            w["A"] += r > 0
        else:
            w["B"] += 0 < r < rl
            if L["keep_h"]:
                w["C"] += r == rl and hl > 0
                w["D"] += r > rl
        at_block = p == int(L["block_off"][f])
        w["F"] += at_block
        w["E"] += r == 0 and not at_block
        w["I"] += bool(in_dead[p])
        if r > 0:
            per_col[(f, k)] = per_col.get((f, k), 0) + 1
    for (f, k), cnt in per_col.items():
        out[f]["G"] += cnt >= 2
    inside = np.zeros(total + 1, bool)
    inside[edges] = True
    for f in L["post"]:
        b0, b1 = int(L["block_off"][f]), int(L["block_off"][f] + L["block_size"][f])
        if b1 > b0:
            out[f]["H"] += not inside[b0 + 1:b1].any()
    _brute[key] = out
    return out


def brute_force(name, L, kept, win):
    per = brute_force_per_front(name, L, win)
    out = {who: {c: 0 for c in CLASSES} for who in ("kept", "staged")}
    for f, d in per.items():
        for c, v in d.items():
            out["kept" if f in kept else "staged"][c] += int(v)
    return out


@pytest.mark.parametrize("keep_h", [True, False])
@pytest.mark.parametrize("name", SMALL)
def test_classifier_equals_brute_force(name, keep_h):
    g, L = layout_of(name, keep_h)
    if g["num_Stack"].size > 1 and keep_h:
        assert L["rh_total"] == g["num_Stack"].size
    ncases = 0
    for kept in kept_sets(L["nf"], (0, 1, 3)):
        for win in window_list(L, kept):
            assert classify_edges(L, kept, win) == brute_force(name, L, set(kept), win), (name, keep_h, kept, win)
            assert window_edges(L, win).size + 1 == max(1, -(-L["rh_total"] // win)) <= MAX_WINDOWS
            ncases += 1
    assert ncases >= 9


# ---- 3: the aimed windows ----
@pytest.mark.parametrize("keep_h", [True, False])
@pytest.mark.parametrize("name", GPU_FIXTURES + ["syn_grid2d", "reorientation_8"])
def test_aimed_windows_hit_their_class(name, keep_h):
    _, L = layout_of(name, keep_h)
    nf = L["nf"]
    by_size = sorted(range(nf), key=lambda f: -int(L["block_size"][f]))
    aimed_any = 0
    for kept in [(), tuple(by_size[:1]), tuple(by_size[:3]), tuple(L["post"][:2])]:
        aims = aimed_windows(L, kept)
        for (who, cl), win in aims.items():
            assert cl in EXACT + INNER + "G" and 2 <= -(-L["rh_total"] // win) <= MAX_WINDOWS, (name, kept, who, cl, win)
            assert classify_edges(L, kept, win)[who][cl] >= 1, (name, kept, who, cl, win)
        aimed_any += len(aims)
        if not keep_h:
            assert not any(cl == "C" for _, cl in aims)
    assert aimed_any or nf == 1


# ---- 4: what the GPU test's windows reach ----
# (fixture, keepH, who) -> the classes the windows of window_list cannot produce there although the layout has columns of that
# kind, and why.  test_every_class_is_reached_on_some_fixture asserts that each class is reached on a fixture of the list.
UNREACHABLE = {}


def exists_per_front(L):
    """bool[nf, classes]: what a front offers with at most MAX_WINDOWS windows per download.  An edge can be put on any position
    p >= rh_total / MAX_WINDOWS (the window p itself), so a per-edge class exists where such a position of it does; G (two edges
    inside one column) where a column is longer than two of the shortest windows.  Worked out from the layout alone."""
    total = L["rh_total"]
    least = max(1, -(-total // MAX_WINDOWS))
    has = np.zeros((max(L["nf"], 1), len(CLASSES)), bool)
    put = lambda f, cl, v: has.__setitem__((f, CLASSES.index(cl)), bool(v))
    inner = lambda a, b: np.any(np.maximum(a + 1, least) < b) if a.size else False        # a position p >= least with a < p < b
    for f in L["post"]:
        if L["block_size"][f] <= 0:
            continue
        F, b0 = L["fronts"][f], int(L["block_off"][f])
        clen = F["rlen"] + F["hlen"]
        piv = np.arange(F["fn"]) < F["fp"]
        start = b0 + F["off"][:-1]
        put(f, "A", inner(start[piv], (start + clen)[piv]))
        put(f, "B", inner(start[~piv], (start + F["rlen"])[~piv]))
        if L["keep_h"]:
            seam = (start + F["rlen"])[~piv & (F["hlen"] > 0)]
            put(f, "C", np.any(seam >= least))
            put(f, "D", inner((start + F["rlen"])[~piv], (start + clen)[~piv]))
        put(f, "E", np.any(start[(clen > 0) & (start > b0)] >= least))
        put(f, "F", b0 >= least and b0 > 0)
        put(f, "G", np.any(clen >= 2 * least + 1))
        put(f, "H", True)
        if F["dead"].any():
            d0, d1 = start[F["dead"]], (start + clen)[F["dead"]]
            put(f, "I", np.any(np.maximum(np.maximum(d0, 1), least) <= np.minimum(d1, min(total, b0 + int(L["block_size"][f])) - 1)))
    return has


_hits = {}


def hits_per_front(name, L, win):
    """bool[nf, classes]: the classes the windows of `win` doubles hit in every front (computed once per fixture and window)"""
    key = (name, L["keep_h"], win)
    if key not in _hits:
        _hits[key] = classify_edges_per_front(L, win) > 0
    return _hits[key]


def lacking(name, L, kept, has):
    """{who: classes} that exist for the kept / staged fronts but that no window of window_list(L, kept) hits"""
    hit = np.zeros_like(has)
    for win in window_list(L, kept):
        hit |= hits_per_front(name, L, win)
    km = np.zeros(has.shape[0], bool)
    km[list(kept)] = True
    out = {}
    for who, m in (("kept", km), ("staged", ~km)):
        lack = has[m].any(axis=0) & ~hit[m].any(axis=0)
        lack_s = {c for i, c in enumerate(CLASSES) if lack[i]} - set(UNREACHABLE.get((name, L["keep_h"], who), ""))
        if lack_s:
            out[who] = "".join(sorted(lack_s))
    return out, hit


def coverage_kept_sets(name, L):
    return kept_sets(L["nf"], (0, 1) if name in SINGLES_ONLY else (0, 1, 2, 3))


@pytest.mark.parametrize("keep_h", [True, False])
@pytest.mark.parametrize("name", GPU_FIXTURES)
def test_gpu_windows_reach_every_class(name, keep_h):
    """whichever fronts the planner keeps: every class the layout has for the kept and for the staged fronts is hit by some window
    of window_list, UNREACHABLE excepted"""
    _, L = layout_of(name, keep_h)
    has = exists_per_front(L)
    missing = {}
    for kept in coverage_kept_sets(name, L):
        lack, _ = lacking(name, L, kept, has)
        if lack:
            missing[kept] = lack
    assert not missing, (name, keep_h, len(missing), dict(list(missing.items())[:12]))


def forced_kept_sets(L):
    """STMMQR_KEEP_FRONTS = 0, 1, 3 takes the fronts with the largest slabs; the model does not know the slabs, so every choice of
    1 and of 3 among the five largest blocks stands in for them"""
    big = sorted(range(L["nf"]), key=lambda f: -int(L["block_size"][f]))[:5]
    yield ()
    for q in (1, 3):
        if q <= L["nf"]:
            yield from itertools.combinations(big, min(q, len(big)))


def test_every_class_is_reached_on_some_fixture():
    """every class is reached for kept and for staged fronts, with and without H, on EACH of the kept sets the GPU test may meet
    on at least one fixture of the list -- so test_every_edge_class_was_hit may ask for all of them, and nothing UNREACHABLE
    records is dropped"""
    for keep_h in (True, False):
        want = set(CLASSES) - (set() if keep_h else set("CD"))
        worst = {who: set() for who in ("kept", "staged")}            # reached on some fixture under its WORST kept set
        for name in GPU_FIXTURES:
            _, L = layout_of(name, keep_h)
            sure = {who: set(CLASSES) for who in worst}
            for kept in forced_kept_sets(L):
                _, hit = lacking(name, L, kept, exists_per_front(L))
                km = np.zeros(hit.shape[0], bool)
                km[list(kept)] = True
                if kept:                                              # (the kept classes come from the runs that keep a front)
                    sure["kept"] &= {c for i, c in enumerate(CLASSES) if hit[km][:, i].any()}
                if (~km).any():
                    sure["staged"] &= {c for i, c in enumerate(CLASSES) if hit[~km][:, i].any()}
            for who in worst:
                worst[who] |= sure[who]
        for who in worst:
            assert worst[who] >= want, (keep_h, who, "never reached: " + "".join(sorted(want - worst[who])))
