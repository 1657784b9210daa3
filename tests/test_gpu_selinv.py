"""diag((A'A)^-1) by selected inversion of R'R on the resident factors (stmmqr_plan_covariance_diag, csrc/stmmqr_selinv.hip).

References: (a) |R^-T e_j|^2 in long double from the factors the plan returns (resident_reference.Factors; selinv_reference.SparseR is
the same substitution without the dense R for the three large fixtures), (b) for dense fronts with m >= n, the R of np.linalg.qr of A
-- independent of the factors, (c) the library's own R' solve, |plan.rsolve(3, e_j)|^2.

Tolerance (derived, not measured): two correct evaluations of z = R^-T e_j differ normwise by at most solve_tol(kappa), kappa =
cond_probe of the factor (tests/stmmqr_testlib.py), so |var_j - ref_j| <= 3 * solve_tol(kappa) * ref_j for every live j.  Every test
prints its largest |var - ref| / ref next to what is allowed; DESIGN.md records them.

The kernels choose no variant by size; the shapes sit on both sides of every block size they work in (STM_SI_NB 32, STM_SI_TILE 64,
STM_SI_KC 16, 256 threads of the list / diagonal kernels)."""
import importlib

import numpy as np
import pytest

from resident_reference import LD, Factors, make_front, stair_csc, symbolic_of
from selinv_reference import SparseR, backsub, to_caller_order
from stmmqr_testlib import EPS, I64, TOL_C, Symbolic, cond_probe, load_golden, numeric_from_gpu, scalar, solve_tol

pytestmark = pytest.mark.gpu
TOL = 1e-10
# The recurrence forms entries of (R'R)^-1, a matrix of condition cond(R)^2: an entry is determined to about eps * cond(R)^2 of the
# largest one, whatever its own size.  That every live variance comes out positive is therefore asserted only where
# TOL_C * eps * cond_probe^2 < 1 (of the fixtures: everywhere but lns_3937, cond_probe 1e11).
POSITIVE_C = TOL_C * EPS


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


def factor_reference(oracle, S, G):
    """(ref in the caller's column order, live mask there, cond_probe) from the downloaded factors"""
    N = numeric_from_gpu(S, G)
    Fa = Factors(S, N)
    Z = Fa.rtsolve(np.eye(S.n))
    ref = np.zeros(S.n, LD)
    ref[Fa.pivot_col] = (Z ** 2).sum(axis=0)[Fa.pivot_col]
    live = np.zeros(S.n, bool)
    live[Fa.pivot_col] = True
    assert np.array_equal(live, np.asarray(G.Rdead[:S.n]) == 0)
    return to_caller_order(S, ref), to_caller_order(S, live), cond_probe(oracle, S, N)


def dense_reference(A):
    """diag((A'A)^-1) of a dense full-column-rank A from np.linalg.qr's R, the substitution in long double"""
    R = np.linalg.qr(A, mode="r")
    Z = backsub(np.asarray(R, LD), np.eye(R.shape[0], dtype=LD))              # R^-1; row sums of squares = diag(R^-1 R^-T)
    return (Z ** 2).sum(axis=1)


def judge(var, ref, live, kappa, label):
    assert var.shape == ref.shape
    assert not np.any(var[~live]), f"{label}: a dead column is not exactly 0"
    allowed = 3 * solve_tol(kappa)
    ratio = float(np.max(np.abs(np.asarray(var, LD)[live] - ref[live]) / ref[live], initial=0.0))
    print(f"\n[selinv] {label}: live {int(live.sum())}/{live.size} cond_probe {kappa:.2e} max |var - ref| / ref {ratio:.2e} (allowed {allowed:.2e})")
    assert np.all(np.isfinite(var))
    if POSITIVE_C * kappa * kappa < 1:
        assert np.all(var[live] > 0)
    assert ratio <= allowed
    return ratio


def run_plan(pkg, oracle, A, Ap, Ai, Ax, label, min_nf=1, want_cn=0, exact_nf=None):
    """analyse (natural order), factorize, variances, download; judged against the factors' own R"""
    m, n = A.shape
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    nf = int(sym["nf"])
    assert nf >= min_nf and (exact_nf is None or nf == exact_nf)
    cn = [int(sym["Rp"][f + 1] - sym["Rp"][f]) - int(sym["Super"][f + 1] - sym["Super"][f]) for f in range(nf)]
    assert max(cn) >= want_cn, "the fixture degenerated: no front with that many non-pivotal columns"
    S = symbolic_of(sym)
    plan = pkg.HipQR(sym)
    try:
        st = plan.factorize(Ax, TOL, n, Ap, Ai)
        var = plan.covariance_diag()
        G = plan.download()
    finally:
        plan.close()
    assert st["retries"] == 0
    ref, live, kappa = factor_reference(oracle, S, G)
    judge(var, ref, live, kappa, f"{label} nf {nf} max cn {max(cn)}")
    return var, live, G


# ---- 1 + 4: one dense front ----
DENSE = [(1, 1), (5, 3), (40, 15), (40, 16), (40, 17), (40, 31), (40, 32), (40, 33), (80, 63), (80, 64), (80, 65), (200, 128), (200, 129),
         (200, 130), (300, 256), (300, 257), (700, 600)]


@pytest.mark.parametrize("m,n,kind", [(m, n, "full") for m, n in DENSE] + [(200, 130, "ramp")])
def test_one_dense_front(pkg, oracle, m, n, kind):
    F, St = make_front(m, n, kind)
    Ap, Ai, Ax = stair_csc(F, St)
    var, live, G = run_plan(pkg, oracle, F, Ap, Ai, Ax, f"dense {m}x{n} {kind}", exact_nf=1)
    assert G.rank == n and live.all()
    # independent of the factors: the R of numpy's QR of A
    ref = dense_reference(F)
    kappa = float(np.linalg.cond(F))
    ratio = float(np.max(np.abs(np.asarray(var, LD) - ref) / ref))
    print(f"[selinv] dense {m}x{n} {kind} vs np.linalg.qr: cond {kappa:.2e} max rel diff {ratio:.2e} (allowed {3 * solve_tol(kappa):.2e})")
    assert ratio <= 3 * solve_tol(kappa)


def test_wide_front_dead_columns_are_zero(pkg, oracle):
    F, St = make_front(48, 100)
    Ap, Ai, Ax = stair_csc(F, St)
    var, live, G = run_plan(pkg, oracle, F, Ap, Ai, Ax, "wide 48x100", exact_nf=1)
    assert G.rank == 48 and int(live.sum()) == 48 and live[:48].all()
    assert not np.any(var[48:])
    ref = dense_reference(F[:, :48])
    assert float(np.max(np.abs(np.asarray(var[:48], LD) - ref) / ref)) <= 3 * solve_tol(float(np.linalg.cond(F[:, :48])))


# ---- 2: block-arrow matrices ----
def csc_of(A):
    m, n = A.shape
    Ap, Ai, Ax = [0], [], []
    for j in range(n):
        r = np.flatnonzero(A[:, j])
        Ai.append(r.astype(I64)); Ax.append(A[r, j]); Ap.append(Ap[-1] + r.size)
    return np.array(Ap, I64), np.concatenate(Ai), np.concatenate(Ax)


def block_arrow(k, nb, nc, seed=0):
    """k dense diagonal blocks of mb x nb, then nc dense coupling columns over all rows"""
    mb = nb + (nc + k - 1) // k + 3
    rng = np.random.default_rng(1000 * nb + 10 * nc + k + seed)
    A = np.zeros((k * mb, k * nb + nc), order="F")
    for b in range(k):
        A[b * mb:(b + 1) * mb, b * nb:(b + 1) * nb] = rng.standard_normal((mb, nb)) / np.sqrt(mb)
    A[:, k * nb:] = rng.standard_normal((k * mb, nc)) / np.sqrt(k * mb)
    return A


@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("nc", [1, 17, 40, 67])
@pytest.mark.parametrize("nb", [31, 33, 70])
def test_block_arrow(pkg, oracle, nb, nc, k):
    A = block_arrow(k, nb, nc)
    var, live, G = run_plan(pkg, oracle, A, *csc_of(A), f"arrow k {k} nb {nb} nc {nc}", min_nf=2, want_cn=nc)
    assert live.all()
    ref = dense_reference(A)
    assert float(np.max(np.abs(np.asarray(var, LD) - ref) / ref)) <= 3 * solve_tol(float(np.linalg.cond(A)))


def test_three_level_arrow(pkg, oracle):
    """two pairs of blocks, each pair with its own coupling columns, and coupling columns over everything"""
    nb, n1, n2, mb = 33, 17, 40, 70
    rng = np.random.default_rng(99)
    m, n = 4 * mb, 4 * nb + 2 * n1 + n2
    A = np.zeros((m, n), order="F")
    c = 0
    for pair in range(2):
        for b in range(2):
            r0 = (2 * pair + b) * mb
            A[r0:r0 + mb, c:c + nb] = rng.standard_normal((mb, nb)) / np.sqrt(mb)
            c += nb
        A[2 * pair * mb:2 * (pair + 1) * mb, c:c + n1] = rng.standard_normal((2 * mb, n1)) / np.sqrt(2 * mb)
        c += n1
    A[:, c:] = rng.standard_normal((m, n2)) / np.sqrt(m)
    sym = pkg.analyze(m, n, *csc_of(A)[:2], Qfill=None)
    nf = int(sym["nf"])
    parent = np.full(nf, -1)
    for f in range(nf):
        for q in range(int(sym["Childp"][f]), int(sym["Childp"][f + 1])):
            parent[int(sym["Child"][q])] = f
    depth = 0
    for f in range(nf):
        d, p = 0, int(parent[f])
        while p >= 0:
            d, p = d + 1, int(parent[p])
        depth = max(depth, d)
    assert depth >= 2, "no front with a grandparent"
    var, live, G = run_plan(pkg, oracle, A, *csc_of(A), "three-level arrow", min_nf=3, want_cn=n1 + n2)
    assert live.all()
    ref = dense_reference(A)
    assert float(np.max(np.abs(np.asarray(var, LD) - ref) / ref)) <= 3 * solve_tol(float(np.linalg.cond(A)))


# ---- 3: golden fixtures ----
def plan_for(pkg, g, keep_h=True):
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}
    plan = pkg.HipQR(sym)
    plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    return S, plan


SMALL = ["syn_chain", "syn_star", "syn_grid2d", "syn_grid3d", "syn_rand60x40", "syn_wide5x8", "syn_dupcol", "syn_emptycol", "syn_rankdef_grid",
         "dwt_992"]


@pytest.mark.parametrize("name", SMALL)
def test_golden_against_the_dense_reference(pkg, oracle, name):
    g = load_golden(name)
    S, plan = plan_for(pkg, g)
    try:
        var = plan.covariance_diag()
        G = plan.download()
    finally:
        plan.close()
    ref, live, kappa = factor_reference(oracle, S, G)
    judge(var, ref, live, kappa, name)


@pytest.mark.parametrize("name", ["bcsstk14", "lns_3937", "epb1"])
def test_golden_against_the_rt_solve(pkg, oracle, name):
    g = load_golden(name)
    S, plan = plan_for(pkg, g)
    n = S.n
    try:
        var = plan.covariance_diag()
        G = plan.download()
        q = np.asarray(S.Qfill if S.Qfill is not None else np.arange(n))
        livec = np.sort(q[np.asarray(G.Rdead[:n]) == 0])                       # live columns, the caller's numbering
        pick = np.sort(np.random.default_rng(20240611).choice(livec, 32, replace=False))
        E = np.zeros((n, 32), order="F")
        E[pick, np.arange(32)] = 1.0
        Zg = plan.rsolve(3, E)                                                # R' \ (E' e_j)
    finally:
        plan.close()
    N = numeric_from_gpu(S, G)
    kappa = cond_probe(oracle, S, N)
    allowed = 3 * solve_tol(kappa)
    live = np.zeros(n, bool)
    live[livec] = True
    assert not np.any(var[~live]) and np.all(np.isfinite(var))
    if POSITIVE_C * kappa * kappa < 1:
        assert np.all(var[live] > 0)
    ref = (np.asarray(Zg, LD) ** 2).sum(axis=0)
    r1 = float(np.max(np.abs(np.asarray(var[pick], LD) - ref) / ref))
    # four of them through the long-double substitution on the downloaded R
    Sr = SparseR(S, N)
    qinv = np.empty(n, I64)
    qinv[q] = np.arange(n)
    B = np.zeros((n, 4))
    B[qinv[pick[::8]], np.arange(4)] = 1.0
    ref4 = (Sr.rtsolve(B) ** 2).sum(axis=0)
    r2 = float(np.max(np.abs(np.asarray(var[pick[::8]], LD) - ref4) / ref4))
    print(f"\n[selinv] {name}: n {n} rank {livec.size} cond_probe {kappa:.2e} vs rsolve(3) {r1:.2e} vs long double {r2:.2e} (allowed {allowed:.2e})")
    assert r1 <= allowed and r2 <= allowed


# ---- 5: bit identity ----
@pytest.mark.parametrize("name", ["syn_grid3d", "syn_rankdef_grid", "dwt_992", "lns_3937"])
def test_bit_identity(pkg, name):
    g = load_golden(name)
    S, plan = plan_for(pkg, g, keep_h=True)
    n = S.n
    try:
        v1 = plan.covariance_diag()
        v2 = plan.covariance_diag()
        d = pkg.device_alloc(8 * n)
        try:
            assert plan.covariance_diag(dev_ptr=d) is None
            v3 = np.zeros(n)
            pkg.device_copy(v3.ctypes.data, d, 8 * n)
        finally:
            pkg.device_free(d)
    finally:
        plan.close()
    S0, p0 = plan_for(pkg, g, keep_h=False)
    try:
        assert not p0.keep_h
        v0 = p0.covariance_diag()
    finally:
        p0.close()
    assert np.array_equal(v1, v2), "two calls on the same factorization differ"
    assert np.array_equal(v1, v3), "host and device results differ"
    assert np.array_equal(v1, v0), "plans with and without H differ"


# ---- 6: no side effects ----
@pytest.mark.parametrize("name", ["syn_grid3d", "lns_3937"])
def test_no_side_effects(pkg, oracle, name):
    g = load_golden(name)
    S, plan = plan_for(pkg, g)
    rng = np.random.default_rng(3)
    B = np.asfortranarray(rng.standard_normal((S.m, 2)))
    try:
        before = (plan.solve(B), plan.rsolve(0, B), plan.qmult(0, B))
        bytes0 = plan.device_bytes()
        var = plan.covariance_diag()
        assert plan.device_bytes() == bytes0
        after = (plan.solve(B), plan.rsolve(0, B), plan.qmult(0, B))
        for a, b, what in zip(before, after, ("solve", "rsolve(0)", "qmult(0)")):
            assert np.array_equal(a, b), f"{what} changed its bits after covariance_diag"
        # new values: A scaled by 1/2 column by column is the same problem with var * 4
        plan.factorize(0.5 * g["in_Ax"], 0.5 * scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
        var2 = plan.covariance_diag()
        G = plan.download()
    finally:
        plan.close()
    N = numeric_from_gpu(S, G)
    kappa = cond_probe(oracle, S, N)
    live = var > 0
    assert np.array_equal(live, var2 > 0)
    ratio = float(np.max(np.abs(var2[live] / var[live] - 4.0) / 4.0))
    print(f"\n[selinv] {name}: refactorized with A / 2: max |var2 / var - 4| / 4 = {ratio:.2e}")
    assert ratio <= 3 * solve_tol(kappa)


# ---- 7: LeastSquares ----
@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_grid3d", "syn_rankdef_grid", "dwt_992"])
def test_least_squares_variances_and_standard_errors(pkg, name, nrhs):
    import scipy.sparse as sp
    g = load_golden(name)
    m, n = int(scalar(g, "in_m")), int(scalar(g, "in_n"))
    Ap, Ai, Ax, tol = g["in_Ap"], g["in_Ai"], g["in_Ax"], float(scalar(g, "in_tol"))
    B = np.asfortranarray(np.random.default_rng(8).standard_normal((m, nrhs)))
    L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs, tol=tol)
    try:
        with pytest.raises(pkg.StmmqrError) as e:                            # before any solve
            L.variances()
        assert e.value.code == -4
        X, resid = L.solve(B)
        var = L.variances()
        se = L.std_errors()
        rank = int(L.info["rank"])
        live = var > 0
        d = pkg.device_alloc(8 * n)
        try:
            assert L.variances(dev_ptr=d) is None
            vd = np.zeros(n)
            pkg.device_copy(vd.ctypes.data, d, 8 * n)
        finally:
            pkg.device_free(d)
    finally:
        L.close()
    assert np.array_equal(var, vd)
    assert int(live.sum()) == rank
    assert not np.any(X[~live]), "a column with variance 0 is a dead column: x = 0"
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n)).toarray()[:, live]
    ref = dense_reference(A)
    kappa = float(np.linalg.cond(A))
    ratio = float(np.max(np.abs(np.asarray(var[live], LD) - ref) / ref))
    print(f"\n[selinv] LeastSquares {name} nrhs {nrhs}: rank {rank}/{n} cond {kappa:.2e} max rel diff {ratio:.2e} (allowed {3 * solve_tol(kappa):.2e})")
    assert ratio <= 3 * solve_tol(kappa)
    assert se.shape == (n, nrhs)
    if m > rank:
        want = np.sqrt(var[:, None] * (resid[None, :] ** 2 / (m - rank)))
        assert np.array_equal(se, want)
    else:
        assert np.all(np.isinf(se))


def test_std_errors_are_inf_without_degrees_of_freedom(pkg):
    F, St = make_front(12, 12)
    Ap, Ai, Ax = stair_csc(F, St)
    L = pkg.LeastSquares(12, 12, Ap, Ai, Ax, nrhs=1, tol=TOL)
    try:
        L.solve(np.ones(12))
        assert int(L.info["rank"]) == 12
        assert np.all(np.isinf(L.std_errors()))
        assert np.all(L.variances() > 0)
    finally:
        L.close()


# ---- 8: refusals ----
def test_refusals_leave_the_plan_usable(pkg):
    g = load_golden("syn_grid3d")
    S = Symbolic(g)
    n = S.n
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    fn = pkg.lib.stmmqr_plan_covariance_diag
    var = np.zeros(n)

    def refused(plan, ncol, ptr, word):
        rc = fn(plan._h, ncol, ptr, 0)
        msg = pkg.lib.stmmqr_last_error().decode()
        assert rc == -4 and msg and word in msg, (rc, msg)

    plan = pkg.HipQR(sym)
    try:
        refused(plan, n, var.ctypes.data, "no factorization")               # nothing factorized
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        good = plan.covariance_diag()
        refused(plan, n, None, "NULL")
        refused(plan, -1, var.ctypes.data, "ncol")
        refused(plan, n + 1, var.ctypes.data, "ncol")
        refused(plan, n - 2, var.ctypes.data, "ntol")                        # ncol < n on a plan that holds no [A B]
        assert np.array_equal(plan.covariance_diag(), good)                  # still usable, same bits
        assert np.all(np.isfinite(plan.rsolve(0, np.ones(S.m))))
    finally:
        plan.close()
    # groups set: not a whole-tree plan
    nf = S.nf
    parent = np.full(nf, -1)
    for f in range(nf):
        for q in range(int(S.Childp[f]), int(S.Childp[f + 1])):
            parent[int(S.Child[q])] = f
    group = np.zeros(nf, np.int32)
    f = int(parent[0])
    while f >= 0:
        group[f] = 1
        f = int(parent[f])
    assert group.any() and not group.all()
    plan = pkg.HipQR(sym)
    try:
        plan.set_groups(group)
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        refused(plan, n, var.ctypes.data, "whole tree")
        assert plan.result_sizes()[1] == n                                   # the plan stays usable
    finally:
        plan.close()
    # a permuted B column: the plan holds [A b] with ntol = n - 1, but its last column is not the caller's last
    q = np.roll(np.arange(n), 1)
    assert q[n - 1] != n - 1
    symq = pkg.analyze(S.m, n, g["in_Ap"], g["in_Ai"], Qfill=q)
    plan = pkg.HipQR(symq)
    try:
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), n - 1, g["in_Ap"], g["in_Ai"])
        refused(plan, n - 1, var.ctypes.data, "permuted")
        assert plan.covariance_diag().shape == (n,)
    finally:
        plan.close()
