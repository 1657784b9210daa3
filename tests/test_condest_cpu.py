"""The yardstick of tests/test_gpu_condest.py, checked without a GPU: tests/condest_reference.py on the R_live of factors the CPU
oracle made.  Asserted, because it can be derived: an estimate of a norm of the inverse is |T^-1 x| / |x| of some x, so it never
exceeds the exact norm by more than the rounding of the solves, solve_tol(cond); Hager's estimate only grows, so it is never below
its first-round value; on a diagonal and on a 1 x 1 matrix it is exact; the returned v has |T v|_1 est = |v|_1 = 1.  Printed, not
asserted: estimate / exact per fixture, the rounds, and the smallest relative gap between the two largest |z_j| of a round -- what
decides whether a float64 run elsewhere picks the same e_j (tests/test_gpu_condest.py compares round by round only where the gap is
far above eps * cond_1)."""
import numpy as np
import pytest

import condest_reference as cr
from resident_reference import LD, Factors
from stmmqr_testlib import EPS, Symbolic, load_golden, scalar, solve_tol


def rlive(oracle, name):
    g = load_golden(name)
    S = Symbolic(g)
    N = oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    return Factors(S, N).Rlive


@pytest.mark.parametrize("name", cr.NAMES)
def test_estimates_are_lower_bounds(oracle, name):
    TL = rlive(oracle, name)
    T = np.asarray(TL, float)
    r = T.shape[0]
    assert r >= 1
    ex = cr.exact(T)
    h = cr.hager(T)
    tol1, tol2 = solve_tol(ex["cond1"]), solve_tol(ex["cond2"])
    gap = min(h["gaps"]) if h["gaps"] else float("inf")
    print(f"\n[condest cpu] {name}: r {r}; kind 1: cond_1 {ex['cond1']:.2e}, estimate / exact {h['est'] / ex['inv1']:.3f} after {h['rounds']} rounds, "
          f"smallest arg-max gap {gap:.1e} (1e3 eps cond_1 = {1e3 * EPS * ex['cond1']:.1e})")
    assert h["est"] <= ex["inv1"] * (1.0 + tol1)
    assert h["est"] >= h["first"]
    assert 1 <= h["rounds"] <= cr.MAX_ROUNDS
    v = h["v"]
    assert abs(float(np.abs(v).sum()) - 1.0) <= 4 * r * EPS
    Tv = float(np.abs(TL @ np.asarray(v, LD)).sum())                        # |T v|_1 in long double
    assert abs(Tv * h["est"] - 1.0) <= tol1
    for iters in (8, 16):
        p = cr.power2(T, iters)
        print(f"  kind 2, {iters} steps: cond_2 {ex['cond2']:.2e}, estimate / exact {p['norm'] * p['inv'] / ex['cond2']:.3f} "
              f"(norm {p['norm'] / ex['norm2']:.3f}, inverse {p['inv'] / ex['inv2']:.3f})")
        assert p["norm"] <= ex["norm2"] * (1.0 + 8 * r * EPS)
        assert p["inv"] <= ex["inv2"] * (1.0 + tol2)
        assert abs(float(np.linalg.norm(p["v"])) - 1.0) <= 8 * EPS
        Tv2 = float(np.sqrt(((TL @ np.asarray(p["v"], LD)) ** 2).sum()))
        assert abs(Tv2 * p["inv"] - 1.0) <= tol2


def test_exact_on_a_diagonal_and_on_1x1():
    d = np.array([3.0, -0.25, 7.0, 1e-3, -40.0])
    T = np.diag(d)
    h = cr.hager(T)
    assert h["est"] == 1.0 / 1e-3 == cr.exact(T)["inv1"]
    assert cr.norm1(T) == 40.0
    assert np.array_equal(np.abs(h["v"]), np.eye(5)[3])
    h1 = cr.hager(np.array([[-0.125]]))
    assert h1["est"] == 8.0 and h1["rounds"] == 1 and np.array_equal(h1["v"], [-1.0])
    p = cr.power2(np.array([[-0.125]]), 8)
    assert p["norm"] == 0.125 and p["inv"] == 8.0


def test_signs_of_zero_and_ties():
    """The two small matrices tests/test_gpu_condest.py runs on the device: on SIGNED_ZEROS the rule for the zeros of y decides the
    result (counting the zeros behind a negative diagonal entry as -1, as the sign bit of 0 / T_ii would, gives another estimate), on
    TIED the tie of the two largest |z_j| goes to the lower index and v says which one was taken."""
    T = cr.SIGNED_ZEROS
    good, bad = cr.hager(T), cr.hager(T, zero_sign=np.where(np.diag(T) < 0, -1.0, 1.0))
    assert (good["est"], good["rounds"]) == (5.25, 2) and (bad["est"], bad["rounds"]) == (7.125, 3)
    assert min(good["gaps"]) > 1e-3                                           # no tie decides anything on this one
    h = cr.hager(cr.TIED)
    assert h["est"] == 2.0 and h["rounds"] == 2 and np.array_equal(h["v"], [0.0, 1.0, 0.0, 0.0])
    h = cr.hager(np.eye(4))                                                   # every |z_j| equal: the first one wins and nothing moves
    assert h["est"] == 1.0 and h["rounds"] == 1
    s = cr.safeguard(5)
    assert np.array_equal(s, [1.0, -1.25, 1.5, -1.75, 2.0]) and np.array_equal(cr.safeguard(1), [1.0])


@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_dupcol", "syn_rankdef_grid"])
def test_r_only_reader(oracle, name):
    """rlive_from_r_only, which tests/test_gpu_condest.py uses on the plan of a LeastSquares object (it keeps no H), reads the same
    R_live out of the R-only layout as Factors does out of R+H: the R-only blocks here are qr_rhpack's keepH = 0 loop restated
    (r_only_blocks of tests/test_gpu_qless.py) applied to the oracle's factors."""
    from types import SimpleNamespace
    from test_gpu_qless import r_only_blocks
    g = load_golden(name)
    S = Symbolic(g)
    N = oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    Fa = Factors(S, N)
    blocks = r_only_blocks(S, N)
    off, run = np.zeros(S.nf, np.int64), 0
    for f, b in zip(S.Post[:S.nf], blocks):
        off[int(f)] = run
        run += b.size
    N0 = SimpleNamespace(Stack=np.concatenate(blocks) if blocks else np.zeros(0), Rblock_off=off, HStair=N.HStair, Hm=N.Hm)
    T, cols = cr.rlive_from_r_only(S, N0)
    assert np.array_equal(cols, Fa.pivot_col)
    assert np.array_equal(np.asarray(T, float), np.asarray(Fa.Rlive, float))
    k = int(cols[Fa.rank // 2])                                               # a view that ends at column k: the leading block
    T1, c1 = cr.rlive_from_r_only(S, N0, ncol=k)
    assert np.array_equal(c1, cols[cols < k]) and np.array_equal(T1, T[:c1.size, :c1.size])
