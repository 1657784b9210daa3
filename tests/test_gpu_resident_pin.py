"""The operations on the resident factors compute the bits they computed before their host layer was split into units of its own
(csrc/stmmqr_rfactor.cpp, stmmqr_rcond.cpp, stmmqr_rcov.cpp, stmmqr_seminormal.cpp, the state in stmmqr_resident.h): every case of
tests/resident_pin_cases.py against tests/golden/resident_pin/resident_pin_parent.npz, written by tests/golden/make_resident_pin.py on
the build before the split.  And: a plan whose schedule was rebuilt (stmmqr_plan_set_groups) computes the bits of a fresh plan -- the
tables of the resident operations follow the schedule generation."""
import importlib
from pathlib import Path

import numpy as np
import pytest

from resident_pin_cases import CASES, pack, rhs, run_case, unpack
from stmmqr_testlib import Symbolic, load_golden, scalar

pytestmark = pytest.mark.gpu
GOLDEN_FILE = Path(__file__).resolve().parent / "golden" / "resident_pin" / "resident_pin_parent.npz"


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN_FILE)


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_as_the_parent(pkg, golden, name):
    want = unpack(golden, name)
    got = unpack(pack(name, run_case(pkg, name)), name)
    assert sorted(got) == sorted(want)
    bad = [k for k in want if not np.array_equal(got[k], want[k])]
    for k in bad:
        if not k.endswith("/sha"):
            print(f"{name}/{k}: max |got - parent| = {np.max(np.abs(got[k] - want[k])):.3e} (|parent| <= {np.max(np.abs(want[k])):.3e})")
        else:
            cols = np.flatnonzero((got[k].reshape(-1, 32) != want[k].reshape(-1, 32)).any(axis=1))
            print(f"{name}/{k}: columns {cols.tolist()} differ")
    assert not bad, bad


# ---- a rebuilt schedule: against a fresh plan in the same process ----
FIXTURE = "syn_rankdef_grid"


def make_plan(pkg, g):
    S = Symbolic(g)
    return S, pkg.HipQR({**S.sc, **{k: v for k, v in S.arr.items() if v is not None}})


def factorize(plan, g):
    plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])


def operations(plan, S):
    Bm, Bn = rhs(S.m, 3, 71), rhs(S.n, 3, 72)
    return [plan.qmult(0, Bm), plan.solve(Bm), plan.rsolve(3, Bn), plan.rmult(Bm, trans=1)]


@pytest.fixture(scope="module")
def fresh(pkg):
    g = load_golden(FIXTURE)
    S, plan = make_plan(pkg, g)
    try:
        factorize(plan, g)
        return operations(plan, S)
    finally:
        plan.close()


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def test_same_grouping_set_again(pkg, fresh):
    """set_groups(zeros) keeps the grouping and moves the schedule generation: tables and maps are made again, the bits stay"""
    g = load_golden(FIXTURE)
    S, plan = make_plan(pkg, g)
    try:
        factorize(plan, g)
        assert same(operations(plan, S), fresh)
        plan.set_groups(np.zeros(S.nf, np.int32))
        factorize(plan, g)
        assert same(operations(plan, S), fresh)
    finally:
        plan.close()


def test_grouping_away_and_back(pkg, fresh):
    """half of the fronts elsewhere (the upper half and whatever lies above it: no front here waits for a block from there), so the
    operations are refused; back to one group, the tables follow the new schedule instead of the one in between"""
    g = load_golden(FIXTURE)
    S, plan = make_plan(pkg, g)
    try:
        factorize(plan, g)
        assert same(operations(plan, S), fresh)
        group = np.zeros(S.nf, np.int32)
        group[S.nf // 2:] = -1
        for _ in range(S.nf):                                    # ... closed towards the root
            for f in range(S.nf):
                if any(group[c] < 0 for c in S.arr["Child"][S.arr["Childp"][f]:S.arr["Childp"][f + 1]]):
                    group[f] = -1
        assert 0 < np.count_nonzero(group < 0) < S.nf
        plan.set_groups(group)
        plan.begin(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        plan.run_group(0)
        plan.finish()
        with pytest.raises(pkg.StmmqrError, match="every front on this device"):
            plan.qmult(0, rhs(S.m, 1, 73))
        plan.set_groups(np.zeros(S.nf, np.int32))
        factorize(plan, g)
        assert same(operations(plan, S), fresh)
    finally:
        plan.close()
