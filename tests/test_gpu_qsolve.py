"""SURVEY.md 8 (f1) on the GPU: Q-apply and least-squares solve on the factors that stay resident in HBM
(stmmqr_plan_qmult / stmmqr_plan_solve; reference QR_qmult / QR_solve, STMMQR/include/SparseQR.h:403-417), checked
against the CPU oracle working on the downloaded factors of the SAME factorization, and through the residual the
reference's driver prints (qrtest.c:11-53)."""
import importlib

import numpy as np
import pytest

from stmmqr_testlib import cond_probe, solve_tol
from stmmqr_testlib import Symbolic, csc_matvec, golden_names, load_golden, numeric_from_gpu, scalar

pytestmark = pytest.mark.gpu
NAMES = golden_names()


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


def factorized_plan(pkg, g, bigcols=64):
    S = Symbolic(g)
    pkg.set_options(big_front_cols=bigcols)
    try:
        plan = pkg.HipQR({**S.sc, **{k: v for k, v in S.arr.items() if v is not None}})
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    finally:
        pkg.set_options(big_front_cols=64)
    return S, plan


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("bigcols", [64, 16])
def test_qmult_against_oracle(pkg, oracle, name, bigcols):
    g = load_golden(name)
    S, plan = factorized_plan(pkg, g, bigcols)
    try:
        N = numeric_from_gpu(S, plan.download())
        rng = np.random.default_rng(11)
        X = rng.standard_normal((S.m, 3))
        QtX = plan.qmult(0, X)
        for j in range(3):
            ref = oracle.qmult(0, S, N, X[:, j])
            assert np.linalg.norm(QtX[:, j] - ref) <= 1e-12 * max(np.linalg.norm(ref), 1e-300)
        # Q (Q' X) = X, and ||Q' x|| = ||x||
        back = plan.qmult(1, QtX)
        assert np.linalg.norm(back - X) <= 1e-12 * np.linalg.norm(X)
        assert abs(np.linalg.norm(QtX) - np.linalg.norm(X)) <= 1e-12 * np.linalg.norm(X)
        QX = plan.qmult(1, X[:, 0])
        ref = oracle.qmult(1, S, N, X[:, 0])
        assert np.linalg.norm(QX - ref) <= 1e-12 * np.linalg.norm(ref)
    finally:
        plan.close()


@pytest.mark.parametrize("name", NAMES)
def test_solve_residual_and_oracle(pkg, oracle, name):
    g = load_golden(name)
    S, plan = factorized_plan(pkg, g)
    try:
        G = plan.download()
        N = numeric_from_gpu(S, G)
        rng = np.random.default_rng(5)
        q = S.Qfill if S.Qfill is not None else np.arange(S.n)
        if G.rank != S.n:
            # rank deficient: the reference's basic solution (dead columns exactly 0), against the oracle's qr_rsolve
            # restatement, which tests/test_oracle_golden.py pins to the real reference's QR_solve output
            b = csc_matvec(S.m, g["in_Ap"], g["in_Ai"], g["in_Ax"], np.arange(S.n, dtype=float))
            x = plan.solve(b)
            xo = np.zeros(S.n)
            xo[q] = oracle.rsolve(S, N, oracle.qmult(0, S, N, b))
            # the dead columns are exactly 0 in both; elsewhere an exact 0 is rounding luck (x_true[0] = 0 here: 0.0 in one
            # implementation, 1e-17 in the other), so the zero PATTERNS are compared on the dead columns and by their count
            dead = np.zeros(S.n, dtype=bool)
            dead[q[np.flatnonzero(np.asarray(G.Rdead[:S.n]) != 0)]] = True
            assert np.all(x[dead] == 0.0) and np.all(xo[dead] == 0.0)
            assert int(dead.sum()) == S.n - G.rank
            assert int(np.sum(x == 0.0)) >= S.n - G.rank
            # (the triangular solve amplifies the rounding differences of the two Q'b by cond(R))
            d = np.linalg.norm(x - xo) / max(np.linalg.norm(xo), 1.0)
            kappa = cond_probe(oracle, S, N)
            print(f"[solve diff] {name} {d:.3e} cond_probe {kappa:.2e} allowed {solve_tol(kappa):.1e}")
            assert d <= solve_tol(kappa)
            if "solve_x" in g and int(scalar(g, "n1rows")) == 0 and int(scalar(g, "n1cols")) == 0:
                ref = g["solve_x"][:S.n]
                assert np.linalg.norm(x - ref) <= 1e-8 * max(np.linalg.norm(ref), 1.0)
            return
        Ap, Ai, Ax = g["in_Ap"], g["in_Ai"], g["in_Ax"]
        xtrue = rng.standard_normal((S.n, 2))
        B = np.stack([csc_matvec(S.m, Ap, Ai, Ax, xtrue[:, j]) for j in range(2)], axis=1)
        B[:, 1] += 1e-3 * rng.standard_normal(S.m)            # an inconsistent right-hand side as well (m >= n)
        X = plan.solve(B)
        for j in range(2):
            y = oracle.qmult(0, S, N, B[:, j])[:S.n]
            xo = np.zeros(S.n)
            xo[q] = oracle.rsolve(S, N, y)
            d = np.linalg.norm(X[:, j] - xo) / max(np.linalg.norm(xo), 1e-300)
            kappa = cond_probe(oracle, S, N)
            print(f"[solve diff] {name} {d:.3e} cond_probe {kappa:.2e} allowed {solve_tol(kappa):.1e}")
            assert d <= solve_tol(kappa)
        # the driver's check (qrtest.c:11-53): res = ||A x - b|| / (||A|| ||x|| + ||b||) for a consistent system
        r = csc_matvec(S.m, Ap, Ai, Ax, X[:, 0]) - B[:, 0]
        res = np.linalg.norm(r) / (np.linalg.norm(Ax) * np.linalg.norm(X[:, 0]) + np.linalg.norm(B[:, 0]))
        assert res <= 1e-10
        # least squares: A'(A x - b) = 0 for the inconsistent one
        r1 = csc_matvec(S.m, Ap, Ai, Ax, X[:, 1]) - B[:, 1]
        cols = np.repeat(np.arange(S.n), np.diff(Ap))
        Atr = np.zeros(S.n)
        np.add.at(Atr, cols, Ax * r1[Ai])
        assert np.linalg.norm(Atr) <= 1e-8 * np.linalg.norm(Ax) * np.linalg.norm(B[:, 1])
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["grid20_standin", "epb1", "syn_rankdef_grid"])
def test_blocked_qapply_equals_reflector_by_reflector(pkg, name, monkeypatch):
    """k_qapply_t (per panel: w = V'x, y = T'w, x -= V y with the T factors kept by the factorization) against k_qapply
    (one reflector after the other, STMMQR_DBG bit 13) on the same resident factors."""
    if name not in NAMES:
        pytest.skip("fixture not present")
    g = load_golden(name)
    S, plan = factorized_plan(pkg, g, 16)
    try:
        X = np.random.default_rng(3).standard_normal((S.m, 2))
        a0, a1 = plan.qmult(0, X), plan.qmult(1, X)
        monkeypatch.setenv("STMMQR_DBG", "8192")
        b0, b1 = plan.qmult(0, X), plan.qmult(1, X)
        monkeypatch.delenv("STMMQR_DBG")
        assert np.linalg.norm(a0 - b0) <= 1e-12 * np.linalg.norm(X)
        assert np.linalg.norm(a1 - b1) <= 1e-12 * np.linalg.norm(X)
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["xenon1_standin", "c5mini_standin"])
def test_solve_full_size_standin(pkg, name):
    """BASELINE configs[2] size (and the configs[4] structure with a 7818-row top front: 2-column panel groups, T built
    by the row-parallel update): residual of the device solve, factors never leave HBM."""
    g = load_golden(name)
    S, plan = factorized_plan(pkg, g)
    try:
        Ap, Ai, Ax = g["in_Ap"], g["in_Ai"], g["in_Ax"]
        xtrue = np.random.default_rng(2).standard_normal(S.n)
        b = csc_matvec(S.m, Ap, Ai, Ax, xtrue)
        x = plan.solve(b)
        res = np.linalg.norm(csc_matvec(S.m, Ap, Ai, Ax, x) - b) / (np.linalg.norm(Ax) * np.linalg.norm(x) + np.linalg.norm(b))
        assert res <= 1e-12
        assert np.linalg.norm(x - xtrue) <= 1e-8 * np.linalg.norm(xtrue)
        y = plan.qmult(0, b)
        assert abs(np.linalg.norm(y) - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["bcsstk14", "syn_rankdef_grid", "grid20_standin", "lns_3937", "syn_dupcol", "bayer10"])
@pytest.mark.parametrize("qt4", ["1", "0"])
def test_split_qapply_on_small_fronts(pkg, oracle, monkeypatch, name, qt4):
    """STMMQR_QBIG_MIN = 1 (read when the plan is made) sends EVERY front through the split Q-apply of the large fronts
    (rows over workgroups, slab partials of V'x summed in slab order; STMMQR_QT4 = 1, the default: a launch per group of FOUR panels
    with the group's 128 x 128 T4 built at the first use, k_qt4_build / k_qbig_step4; 0: a launch per panel): same Q'X / Q X as the
    oracle applies from the downloaded factors, and as the one-workgroup kernel."""
    if name not in NAMES:
        pytest.skip("fixture not present")
    g = load_golden(name)
    monkeypatch.setenv("STMMQR_QT4", qt4)
    monkeypatch.setenv("STMMQR_QBIG_MIN", "1")
    S, plan = factorized_plan(pkg, g)
    monkeypatch.delenv("STMMQR_QBIG_MIN")
    S2, plan2 = factorized_plan(pkg, g)
    try:
        N = numeric_from_gpu(S, plan.download())
        X = np.random.default_rng(11).standard_normal((S.m, 2))
        for method in (0, 1):
            got = plan.qmult(method, X)
            one = plan2.qmult(method, X)
            for j in range(2):
                ref = oracle.qmult(method, S, N, X[:, j])
                assert np.linalg.norm(got[:, j] - ref) <= 1e-12 * np.linalg.norm(ref)
            assert np.linalg.norm(got - one) <= 1e-12 * np.linalg.norm(one)
        back = plan.qmult(1, plan.qmult(0, X))
        assert np.linalg.norm(back - X) <= 1e-12 * np.linalg.norm(X)
        # ... and through the split back substitution (k_rbig_*): same solution as the one-workgroup kernels, which the
        # other tests of this file pin to the oracle / the reference
        B = np.random.default_rng(12).standard_normal((S.m, 2))
        xs, x1 = plan.solve(B), plan2.solve(B)
        assert np.linalg.norm(xs - x1) <= solve_tol(cond_probe(oracle, S, N), floor=1e-10) * max(np.linalg.norm(x1), 1.0)
        assert np.array_equal(xs == 0.0, x1 == 0.0)             # dead columns: exactly zero in both
    finally:
        plan.close(); plan2.close()


@pytest.mark.parametrize("name", NAMES)
def test_all_qmult_methods_and_solve_systems(pkg, oracle, name):
    """The rest of QR_qmult / QR_solve (SparseQR.c:1591-1700, 2040-2216, 2522): X Q', X Q as the transposes of Q X, Q' X;
    R X = B and R E' X = B against the oracle's qr_rsolve; R' X = B and R' X = E' B through the adjoint identity
    x' (R z) = b' z on random z (R has full row rank, so that pins x), rows of X beyond the rank exactly zero."""
    g = load_golden(name)
    S, plan = factorized_plan(pkg, g)
    try:
        N = numeric_from_gpu(S, plan.download())
        kappa = cond_probe(oracle, S, N)
        rng = np.random.default_rng(23)
        m, n, rank = S.m, S.n, int(N.c.rank)
        # ---- X Q' and X Q ----
        X = rng.standard_normal((3, m))
        XQt = plan.qmult(2, X)
        XQ = plan.qmult(3, X)
        for r in range(3):
            ref = oracle.qmult(1, S, N, X[r])                      # (X Q')(r,:) = (Q X(r,:)')'
            assert np.linalg.norm(XQt[r] - ref) <= 1e-12 * max(np.linalg.norm(ref), 1e-300)
            ref = oracle.qmult(0, S, N, X[r])
            assert np.linalg.norm(XQ[r] - ref) <= 1e-12 * max(np.linalg.norm(ref), 1e-300)
        # ---- R X = B, R E' X = B ----
        Y = rng.standard_normal((m, 2))
        X0 = plan.rsolve(0, Y)
        X1 = plan.rsolve(1, Y)
        q = S.Qfill if S.Qfill is not None else np.arange(n)
        for j in range(2):
            xo = oracle.rsolve(S, N, Y[:, j])                       # qr_rsolve restated: R \\ y in R's column order, dead columns 0
            scale = max(np.linalg.norm(xo), 1e-300)
            tolr = solve_tol(kappa)
            assert np.linalg.norm(X0[:, j] - xo) <= tolr * scale
            assert np.linalg.norm(X1[q, j] - xo) <= tolr * scale     # with E: X(Qfill(j)) = x(j)
        # ---- R' X = B, R' X = E' B ----
        B = rng.standard_normal((n, 2))
        X2 = plan.rsolve(2, B)
        X3 = plan.rsolve(3, B)
        dead = np.asarray(N.Rdead[:n]) != 0
        for j in range(2):
            assert not np.any(X2[rank:, j]) and not np.any(X3[rank:, j])
            for _ in range(4):
                z = rng.standard_normal(n)
                z[dead] = 0.0                                       # (a dead column has no equation in the squeezed R)
                Rz = oracle.rmult(S, N, z)                          # rank rows, then zeros
                lhs2, lhs3 = float(X2[:rank, j] @ Rz[:rank]), float(X3[:rank, j] @ Rz[:rank])
                rhs2, rhs3 = float(B[:, j] @ z), float(B[q, j] @ z)
                sc = np.linalg.norm(B[:, j]) * np.linalg.norm(z) + abs(rhs2)
                tolt = solve_tol(kappa)
                assert abs(lhs2 - rhs2) <= tolt * max(sc, np.linalg.norm(X2[:, j]) * np.linalg.norm(Rz))
                assert abs(lhs3 - rhs3) <= tolt * max(sc, np.linalg.norm(X3[:, j]) * np.linalg.norm(Rz))
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["syn_grid2d", "syn_rankdef_grid"])
@pytest.mark.parametrize("nrhs", [3, 33])
def test_solve_equals_its_parts(pkg, name, nrhs):
    """solve is QR_qmult(QR_QTX) followed by QR_solve(QR_RETX_EQUALS_B) without the trip to the host in between: the same passes over
    the tree, so the same bits (33: a full batch of 32 plus one)"""
    g = load_golden(name)
    S, plan = factorized_plan(pkg, g)
    try:
        B = np.random.default_rng(29).standard_normal((S.m, nrhs))
        X = plan.solve(B)
        Xp = plan.rsolve(1, plan.qmult(0, B))
        assert np.array_equal(X.view(np.uint64), Xp.view(np.uint64))
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["grid20_standin", "lns_3937", "bcsstk14", "syn_rankdef_grid", "epb1"])
def test_batched_right_hand_sides(pkg, oracle, monkeypatch, name):
    """QR_qmult / QR_solve take BLOCKS of right-hand sides (qr_panel, SparseQR.c:1591-1706).  Here every launch of a pass over the tree
    carries a batch of them (RhsBatch: right-hand side = blockIdx.y / .z, per-vector buffers at strides; STMMQR_RHS_BATCH, default 32).
    37 right-hand sides (one full batch + a ragged one) through all four qmult methods and all four solve systems: column j of a
    batched call is bit for bit what a one-vector call gives (the same kernels do the same arithmetic per vector), and column 0
    matches the oracle."""
    g = load_golden(name)
    S, plan = factorized_plan(pkg, g)
    try:
        N = numeric_from_gpu(S, plan.download())
        rng = np.random.default_rng(41)
        m, n, k = S.m, S.n, 37
        X = rng.standard_normal((m, k))
        for method in (0, 1):
            Y = plan.qmult(method, X)
            for j in (0, 5, 31, 32, 36):
                assert np.array_equal(Y[:, j], plan.qmult(method, X[:, j].copy()).ravel()), (method, j)
            ref = oracle.qmult(method, S, N, X[:, 0])
            assert np.linalg.norm(Y[:, 0] - ref) <= 1e-12 * max(np.linalg.norm(ref), 1e-300)
        Xr = rng.standard_normal((k, m))
        for method in (2, 3):
            Y = plan.qmult(method, Xr)
            for j in (0, 33, 36):
                assert np.array_equal(Y[j], plan.qmult(method, Xr[j:j + 1].copy()).ravel()), (method, j)
        B = rng.standard_normal((m, k))
        Xs = plan.solve(B)
        for j in (0, 7, 32, 36):
            assert np.array_equal(Xs[:, j], plan.solve(B[:, j].copy()).ravel()), j
        for system in (0, 1):
            Z = plan.rsolve(system, B)
            for j in (0, 36):
                assert np.array_equal(Z[:, j], plan.rsolve(system, B[:, j].copy()).ravel()), (system, j)
        Bn = rng.standard_normal((n, k))
        for system in (2, 3):
            Z = plan.rsolve(system, Bn)
            for j in (0, 31, 36):
                assert np.array_equal(Z[:, j], plan.rsolve(system, Bn[:, j].copy()).ravel()), (system, j)
    finally:
        plan.close()


@pytest.mark.parametrize("split_all", [0, 1])
@pytest.mark.parametrize("k", [2, 3, 6])
def test_small_batches_take_the_shared_workgroups_too(pkg, monkeypatch, k, split_all):
    """batches of 2 (two vectors per workgroup), 3 (four per workgroup, one of them idle) and 6 (a full group + a ragged one) through
    Q'b, Q b and the least-squares solve; split_all: every front through the split kernels of the large fronts (STMMQR_QBIG_MIN = 1).
    Column j of a batched call is bit for bit the one-vector call."""
    if split_all:
        monkeypatch.setenv("STMMQR_QBIG_MIN", "1")
    g = load_golden("lns_3937")
    S, plan = factorized_plan(pkg, g)
    if split_all:
        monkeypatch.delenv("STMMQR_QBIG_MIN")
    try:
        rng = np.random.default_rng(43 + k)
        X = rng.standard_normal((S.m, k))
        for method in (0, 1):
            Y = plan.qmult(method, X)
            for j in range(k):
                assert np.array_equal(Y[:, j], plan.qmult(method, X[:, j].copy()).ravel()), (method, j)
        Xs = plan.solve(X)
        for j in range(k):
            assert np.array_equal(Xs[:, j], plan.solve(X[:, j].copy()).ravel()), j
    finally:
        plan.close()


def test_batch_of_32_costs_little_more_than_one(pkg):
    """32 right-hand sides in one pass over the tree against one (default workload).  The round-4 verdict asked for <= 3 x.  The batch
    alone (one set of workgroups per vector in every launch) reached 3.0-3.6 x -- one vector after the other was 32 x -- because
    every vector's workgroup streamed V for itself; with four vectors per workgroup (k_qbig_step4 / k_qapply_t / k_rbig_init /
    k_rsolve templates: V, its masks and T read once for the four) it is 2.4 x (Q'b) and 2.2 x (solve).  Gate: 3 x."""
    import time
    g = load_golden("xenon1_colamd_standin")
    S, plan = factorized_plan(pkg, g)
    try:
        rng = np.random.default_rng(3)
        B1, B32 = rng.standard_normal((S.m, 1)), rng.standard_normal((S.m, 32))
        plan.solve(B32); plan.qmult(0, B32.copy())            # (buffers of the batch, T4 of the grouped Q-apply: first use)
        def best(fn):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            return min(ts)
        q1, q32 = best(lambda: plan.qmult(0, B1.copy())), best(lambda: plan.qmult(0, B32.copy()))
        s1, s32 = best(lambda: plan.solve(B1)), best(lambda: plan.solve(B32))
        print(f"[rhs batch] Q'b: 1 rhs {q1 * 1e3:.1f} ms, 32 rhs {q32 * 1e3:.1f} ms; solve: 1 rhs {s1 * 1e3:.1f} ms, 32 rhs {s32 * 1e3:.1f} ms")
        assert q32 <= 3.0 * q1 and s32 <= 3.0 * s1
    finally:
        plan.close()
