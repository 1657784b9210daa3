"""The condition estimate on the resident factors (stmmqr_plan_condest, stmmqr_ls_condest).

Yardstick: tests/condest_reference.py on the dense R_live = Factors.Rlive rebuilt from the plan's own downloaded factors -- the exact
norms, and the same two algorithms in float64 (validated without a GPU in tests/test_condest_cpu.py).  kappa below is the exact
condition of the kind, and solve_tol(kappa) what two correct float64 solves through these factors may differ by.

Path-independent checks (every fixture, both kinds): the norm of R_live (kind 1: exact, within (rank + 2) eps; kind 2: the power
iteration's value is a lower bound of it and equals the yardstick's own run), the inverse's estimate never above the exact norm,
out[0] = out[1] out[2], v zero on dead columns and of unit norm, |R_live v| out[2] = 1 in long double.
Against the yardstick's own run: kind 2 everywhere (the iteration has no branch); kind 1 where the measured relative gap between the
two largest |z_j| of every round (>= 5e-3, printed by tests/test_condest_cpu.py) is far above eps cond_1, so both runs choose the same
e_j: every fixture but lns_3937 (cond_1 1.9e13)."""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import condest_reference as cr
from minnorm_reference import SMALL, dense_of, qfill_of
from resident_reference import LD, Factors, make_front, stair_csc, symbolic_of
from stmmqr_testlib import EPS, Symbolic, load_golden, numeric_from_gpu, scalar, solve_tol

pytestmark = pytest.mark.gpu
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
NAMES = SMALL + ["bcsstk14", "lns_3937"]
SAME_PATH = SMALL + ["bcsstk14"]                 # kind 1 is compared round by round here (SMALL holds dwt_992)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    assert p.device_count() >= 1
    return p


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module(PKG + ".capi")


@pytest.fixture
def env():
    saved = {}

    def put(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = str(v)
    yield put
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def golden_plan(pkg, name, keep_h=True, zero=False):
    g = load_golden(name)
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}
    plan = pkg.HipQR(sym)
    plan.factorize(g["in_Ax"] * (0.0 if zero else 1.0), scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    return g, S, plan


_REF = {}


def reference(key, S, plan):
    """(Factors, exact values, the yardstick's runs of both kinds) of a factorization, computed once and shared by the kinds"""
    if key not in _REF:
        Fa = Factors(S, numeric_from_gpu(S, plan.download()))
        T = np.asarray(Fa.Rlive, float)
        _REF[key] = (Fa, cr.exact(T), cr.hager(T), cr.power2(T, 8))
    return _REF[key]


def check_estimate(c, kind, Fa, ex, q, label, same_path, yard):
    """the path-independent checks of one result dict c; then, same_path, against the yardstick's run `yard`"""
    r, n = Fa.rank, Fa.n
    kappa = ex["cond1"] if kind == 1 else ex["cond2"]
    norm, inv = (ex["norm1"], ex["inv1"]) if kind == 1 else (ex["norm2"], ex["inv2"])
    tol = solve_tol(kappa)
    print(f"\n[condest] {label} kind {kind}: r {c['r']}, cond {c['cond']:.4e} = {c['cond'] / kappa:.3f} of the exact {kappa:.3e}; norm {c['norm'] / norm:.4f}, "
          f"inverse {c['inv_norm'] / inv:.4f} of exact after {c['rounds']} rounds (allowed {tol:.1e})")
    assert c["r"] == r and c["kind"] == kind
    if kind == 1:
        assert abs(c["norm"] - norm) <= (r + 2) * EPS * norm                 # exact: column sums
    else:
        assert c["norm"] <= norm * (1.0 + 4 * (r + 2) * EPS)                 # the power iteration's value: a lower bound (two products of
                                                                             #  (r + 2) eps each, a norm and a root) ...
        assert abs(c["norm"] - yard["norm"]) <= tol * yard["norm"]           # ... and the yardstick's own, no branch in it
    assert c["inv_norm"] <= inv * (1.0 + tol)
    assert abs(c["cond"] - c["norm"] * c["inv_norm"]) <= 4 * EPS * c["cond"]
    v = c["v"]
    assert v.shape == (n,)
    live = np.asarray(q)[Fa.pivot_col]
    dead = np.setdiff1d(np.arange(n), live)
    assert np.all(v[dead] == 0.0)
    vl = np.asarray(v[live], LD)
    Rv = Fa.Rlive @ vl
    if kind == 1:
        assert abs(float(np.abs(vl).sum()) - 1.0) <= (r + 2) * EPS
        back = float(np.abs(Rv).sum())
    else:
        assert abs(float(np.sqrt((vl ** 2).sum())) - 1.0) <= (r + 2) * EPS
        back = float(np.sqrt((Rv ** 2).sum()))
    print(f"  |R_live v| * inverse estimate - 1 = {back * c['inv_norm'] - 1.0:.2e}")
    assert abs(back * c["inv_norm"] - 1.0) <= tol
    if same_path:
        want, rounds = (yard["est"], yard["rounds"]) if kind == 1 else (yard["inv"], 8)
        print(f"  vs the yardstick's run: {c['inv_norm'] / want - 1.0:.2e}, rounds {c['rounds']} / {rounds}")
        assert abs(c["inv_norm"] - want) <= tol * want
        assert c["rounds"] == rounds


@pytest.mark.parametrize("name", NAMES)
def test_fixtures(pkg, name):
    g, S, plan = golden_plan(pkg, name)
    _, _, plan0 = golden_plan(pkg, name, keep_h=False)
    try:
        Fa, ex, h, p = reference(name, S, plan)
        for kind in (1, 2):
            c = plan.condest(kind, with_vector=True)
            check_estimate(c, kind, Fa, ex, qfill_of(S), name, kind == 2 or name in SAME_PATH, h if kind == 1 else p)
            c0 = plan0.condest(kind)                                         # reads R only: the plan without H gives the same numbers
            assert c0["cond"] == c["cond"] and c0["rounds"] == c["rounds"]
            assert plan.condest(kind)["cond"] == c["cond"]                   # and a second call the same bits
    finally:
        plan.close(); plan0.close()


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "dwt_992"])
def test_every_front_split(pkg, env, name):
    """STMMQR_RTBIG_MIN=1: the R' solves split every front's columns over workgroups"""
    g, S, p0 = golden_plan(pkg, name)
    try:
        Fa, ex, _, _ = reference(name, S, p0)
        base = {k: p0.condest(k) for k in (1, 2)}
    finally:
        p0.close()
    env(STMMQR_RTBIG_MIN=1)
    g, S, plan = golden_plan(pkg, name)
    try:
        for kind in (1, 2):
            c = plan.condest(kind)
            tol = solve_tol(ex["cond1"] if kind == 1 else ex["cond2"])
            assert abs(c["cond"] - base[kind]["cond"]) <= tol * base[kind]["cond"]
            assert c["rounds"] == base[kind]["rounds"]
    finally:
        plan.close()


def test_carried_view(pkg):
    """A LeastSquares object holds the R of [A B]: its estimate is that of A alone.  The plain plan of syn_rand60x40 has the same
    column order (asserted), so its R is R11 up to the signs of rows; R'R is then the same matrix and kind 2 follows the same
    iterates.  Kind 1 starts from x = 1/r, which the row signs do change, so it cannot be held against the plain plan; it is held
    against the yardstick's own run on R11 itself, read from the carried plan's downloaded (R-only) factors, with the round count
    and the certificate |R11 E'v|_1 out[2] = 1, exactly as the fixtures are."""
    g, S, plan = golden_plan(pkg, "syn_rand60x40")
    m, n = S.m, S.n
    A = dense_of(m, n, g["in_Ap"], g["in_Ai"], g["in_Ax"])
    ls = pkg.LeastSquares(m, n, g["in_Ap"], g["in_Ai"], g["in_Ax"], nrhs=3)
    try:
        with pytest.raises(pkg.StmmqrError, match="no solve yet"):
            ls.condest()
        ls.solve(np.random.default_rng(2).standard_normal((m, 3)))
        assert np.array_equal(np.asarray(ls.symbolic()["Qfill"][:n]), qfill_of(S))
        Fa, ex, _, _ = reference("syn_rand60x40", S, plan)
        assert Fa.rank == n
        for kind in (1, 2):
            a, b = plan.condest(kind, with_vector=True), ls.condest(kind, with_vector=True)
            kappa = ex["cond1"] if kind == 1 else ex["cond2"]
            tol = solve_tol(kappa)
            print(f"\n[condest] carried kind {kind}: plain {a['cond']:.6e}, carried {b['cond']:.6e}, exact {kappa:.6e}")
            assert b["r"] == n and b["v"].shape == (n,)
            assert abs(a["norm"] - b["norm"]) <= max(tol, (n + 2) * EPS) * a["norm"]
            assert b["inv_norm"] <= (ex["inv1"] if kind == 1 else ex["inv2"]) * (1.0 + tol)
            if kind == 2:
                assert abs(a["cond"] - b["cond"]) <= tol * a["cond"]
                assert b["rounds"] == a["rounds"] == 8
                Av = np.asarray(A, LD) @ np.asarray(b["v"], LD)              # |A v|_2 = |R11 E'v|_2
                assert abs(float(np.sqrt((Av ** 2).sum())) * b["inv_norm"] - 1.0) <= tol
        # the plan of [A B] itself: ncol = n is the view, every column is refused (ntol = n, not n + 3)
        pab = ls.plan()
        # kind 1 against the yardstick on R11: every check of the fixtures (check_estimate), path and round count included
        Sab = symbolic_of(ls.symbolic())
        R11, cols = cr.rlive_from_r_only(Sab, pab.download(), ncol=n)
        assert R11.shape == (n, n) and np.array_equal(cols, np.arange(n))
        T11 = np.asarray(R11, float)
        view = SimpleNamespace(rank=n, n=n, Rlive=R11, pivot_col=cols)
        check_estimate(ls.condest(1, with_vector=True), 1, view, cr.exact(T11), qfill_of(S), "carried view", True, cr.hager(T11))
        check_estimate(ls.condest(2, with_vector=True), 2, view, cr.exact(T11), qfill_of(S), "carried view", True, cr.power2(T11, 8))
        assert pab.condest(2, ncol=n)["cond"] == ls.condest(2)["cond"]
        with pytest.raises(pkg.StmmqrError, match="carried solve"):
            plan.condest(1, ncol=n - 1)
    finally:
        ls.close(); plan.close()


def test_front_too_wide_for_the_one_workgroup_solve(pkg):
    """48 x 10921: stmmqr_plan_rsolve systems 2-3 refuse this front; the estimate's R' solves split it"""
    m, n = 48, 10921
    F, St = make_front(m, n)
    Ap, Ai, Ax = stair_csc(F, St)
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    plan = pkg.HipQR(sym)
    try:
        plan.factorize(Ax, 1e-10, n, Ap, Ai)
        with pytest.raises(pkg.StmmqrError, match="too wide"):
            plan.rsolve(3, np.ones(n))
        S = symbolic_of(sym)
        Fa, ex, h, p = reference("48x10921", S, plan)
        assert Fa.rank == m
        for kind in (1, 2):
            check_estimate(plan.condest(kind, with_vector=True), kind, Fa, ex, np.arange(n), "dense 48x10921", True, h if kind == 1 else p)
    finally:
        plan.close()


def triangular_plan(pkg, T):
    """a plan whose R is the upper triangular T itself: no pivot column has anything below its diagonal, so no reflector acts"""
    r = T.shape[0]
    A = sp.csc_matrix(T)
    A.eliminate_zeros()
    A.sort_indices()
    Ap, Ai, Ax = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)
    sym = pkg.analyze(r, r, Ap, Ai, Qfill=np.arange(r, dtype=np.int64))
    plan = pkg.HipQR(sym)
    plan.factorize(Ax, 1e-10, r, Ap, Ai)
    return sym, plan


def test_zeros_of_either_sign_and_ties(pkg):
    """k_ce_map's sign rule and k_ce_reduce's tie rule, directly.  SIGNED_ZEROS: R \\ e_j leaves -0.0 behind j wherever the diagonal is
    negative; counting those as -1 gives 7.125 after 3 rounds (tests/test_condest_cpu.py), the rule gives 5.25 after 2 -- every
    operation on this matrix is exact, so the device must return exactly that.  TIED: z = (1, 2, 2, 1), the lower index wins, and
    v = e_1 says so."""
    for T, est, rounds in ((cr.SIGNED_ZEROS, 5.25, 2), (cr.TIED, 2.0, 2)):
        sym, plan = triangular_plan(pkg, T)
        try:
            Fa = Factors(symbolic_of(sym), numeric_from_gpu(symbolic_of(sym), plan.download()))
            q = np.asarray(sym["Qfill"][:T.shape[0]])
            assert np.array_equal(np.asarray(Fa.Rlive, float), T[:, q[Fa.pivot_col]])      # R is the matrix itself
            c = plan.condest(1, with_vector=True)
        finally:
            plan.close()
        h = cr.hager(np.asarray(Fa.Rlive, float))
        assert (h["est"], h["rounds"]) == (est, rounds)
        assert (c["inv_norm"], c["rounds"]) == (est, rounds)
        assert c["norm"] == cr.norm1(T) and c["cond"] == est * cr.norm1(T)
        assert np.array_equal(c["v"][q[Fa.pivot_col]], h["v"])
    assert np.array_equal(h["v"], [0.0, 1.0, 0.0, 0.0])


def test_rank_zero(pkg):
    g, S, plan = golden_plan(pkg, "syn_grid2d", zero=True)
    try:
        for kind in (1, 2):
            c = plan.condest(kind, with_vector=True)
            assert (c["cond"], c["norm"], c["inv_norm"], c["rounds"], c["r"], c["kind"]) == (1.0, 0.0, 0.0, 0, 0, kind)
            assert np.all(c["v"] == 0.0) and c["v"].shape == (S.n,)
    finally:
        plan.close()


def test_refusals_and_device_output(pkg, capi):
    lib = capi.lib
    g = load_golden("syn_grid2d")
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    fresh = pkg.HipQR(sym)
    out = np.full(8, 7.0)
    try:
        with pytest.raises(pkg.StmmqrError) as e:
            fresh.condest()
        assert e.value.code == -4 and "no factorization" in str(e.value)
        fresh.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        y0 = fresh.rsolve(0, np.ones(S.m))
        call = lambda ncol, kind, o: lib.stmmqr_plan_condest(fresh._h, ncol, kind, 0, o, None, 0)
        assert call(S.n + 1, 1, out.ctypes.data) == -4 and "ncol" in capi.last_error()
        assert call(-1, 1, out.ctypes.data) == -4 and "ncol" in capi.last_error()
        assert call(S.n, 0, out.ctypes.data) == -4 and "kind" in capi.last_error()
        assert call(S.n, 3, out.ctypes.data) == -4 and "kind" in capi.last_error()
        assert call(S.n, 1, None) == -4 and "out" in capi.last_error()
        assert call(S.n - 1, 1, out.ctypes.data) == -4 and "carried solve" in capi.last_error()
        assert lib.stmmqr_plan_condest(None, S.n, 1, 0, out.ctypes.data, None, 0) == -4
        assert np.all(out == 7.0)                                            # no refusal wrote anything
        assert np.array_equal(fresh.rsolve(0, np.ones(S.m)), y0)             # the plan stays usable
        want = fresh.condest(1, with_vector=True)
        dout, dv = pkg.device_alloc(64), pkg.device_alloc(8 * S.n)           # device pointers: the same bits
        try:
            assert lib.stmmqr_plan_condest(fresh._h, S.n, 1, 0, dout, dv, 1) == 0
            v = np.zeros(S.n)
            pkg.device_copy(out.ctypes.data, dout, 64)
            pkg.device_copy(v.ctypes.data, dv, 8 * S.n)
        finally:
            pkg.device_free(dout); pkg.device_free(dv)
        assert out[0] == want["cond"] and out[4] == want["r"] and np.array_equal(v, want["v"])
    finally:
        fresh.close()
    # groups set: not a whole-tree plan (the construction of tests/test_gpu_selinv.py)
    parent = np.full(S.nf, -1)
    for f in range(S.nf):
        for q in range(int(S.Childp[f]), int(S.Childp[f + 1])):
            parent[int(S.Child[q])] = f
    group = np.zeros(S.nf, np.int32)
    f = int(parent[0])
    while f >= 0:
        group[f] = 1
        f = int(parent[f])
    assert group.any() and not group.all()
    plan = pkg.HipQR(sym)
    try:
        plan.set_groups(group)
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        with pytest.raises(pkg.StmmqrError, match="whole tree") as e:
            plan.condest()
        assert e.value.code == -4
        assert plan.result_sizes()[1] == S.n                                 # the plan stays usable
    finally:
        plan.close()
