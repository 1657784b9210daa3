"""Least squares with the right-hand sides carried through the factorization, on the GPU: LeastSquares (stmmqr_ls_*) and
stmmqr_plan_solve_carried against the Q-based solve of a plan that keeps H, the least-squares conditions of the original problem,
and themselves (reuse, batches, device pointers)."""
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

from stmmqr_testlib import Symbolic, cond_probe, load_golden, numeric_from_gpu, scalar, solve_tol
from test_carried_cpu import augmented, backward_error, problem, symbolic_of

pytestmark = pytest.mark.gpu

LARGE = "xenon1_colamd_standin"                      # the workload of tools/time_qless.py and tools/time_carried.py


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


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


def matrix(g, name):
    """(m, n, Ap, Ai, Ax, tol, Quser): the matrix the golden factorization was made of, in the golden column order -- except syn_star,
    taken WITH its column singleton (the caller's full matrix, default tolerance and ordering)"""
    if name == "syn_star":
        return int(g["A_m"][0]), int(g["A_n"][0]), g["A_p"], g["A_i"], g["A_x"], -2.0, None
    m, n, Ap, Ai, Ax, tol = problem(g)
    return m, n, Ap, Ai, Ax, tol, (g["sym_Qfill"] if g["sym_Qfill"].size else np.arange(n))


def least_squares(pkg, mat, nrhs, **kw):
    m, n, Ap, Ai, Ax, tol, Q = mat
    if Q is not None:
        kw = dict(ordering=3, Quser=Q, **kw)
    return pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs, tol=tol, **kw)


def plan_of_a(pkg, mat, order, keep_h=True):
    """a plan of A alone in the column order `order`, factorized with the tolerance the object uses -> (sym dict, HipQR)"""
    m, n, Ap, Ai, Ax, tol, _ = mat
    sym = {k: v for k, v in pkg.analyze(m, n, Ap, Ai, Qfill=order).items() if k != "info"}
    plan = pkg.HipQR({**sym, "keepH": 1 if keep_h else 0})
    return sym, plan


def spmat(mat):
    m, n, Ap, Ai, Ax = mat[:5]
    return sp.csc_matrix((Ax, Ai, Ap), shape=(m, n))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", ["syn_grid3d", "syn_star", "syn_rand60x40", "syn_emptycol", "bcsstk14", "t2d_q9", "epb1"])
def test_full_rank_against_q_based_solve(pkg, oracle, name):
    g = load_golden(name)
    mat = matrix(g, name)
    m, n, Ap, Ai, Ax = mat[:5]
    B = np.asfortranarray(np.random.default_rng(3).standard_normal((m, 2)))
    L = least_squares(pkg, mat, 2)
    try:
        X, resid = L.solve(B)
        info = L.info
        assert int(info["rank"]) == n and info["retries"] == 0
        sym, plan = plan_of_a(pkg, mat, L.symbolic()["Qfill"][:n])
        try:
            plan.factorize(Ax, info["tol"], n, Ap, Ai)
            Xq = plan.solve(B)
            S = symbolic_of(sym)
            kappa = cond_probe(oracle, S, numeric_from_gpu(S, plan.download()))
        finally:
            plan.close()
        d = np.linalg.norm(X - Xq, axis=0) / np.maximum(np.linalg.norm(Xq, axis=0), 1e-300)
        print(f"[carried vs Q] {name} diff {d.max():.2e} cond_probe {kappa:.2e} allowed {solve_tol(kappa):.1e} resid {resid}")
        assert np.all(d <= solve_tol(kappa))
    finally:
        L.close()


@pytest.mark.parametrize("name", ["ex18", "bayer10"])
def test_ill_conditioned_backward_error(pkg, name):
    """cond(A) ~ 1e12: the bar is the backward error of the Q-based plan.solve on the same A and B, with a factor 10 (both are a few
    roundoffs and come from different trees).  Measured (carried, Q-based, seminormal info): DESIGN.md 6g."""
    g = load_golden(name)
    mat = matrix(g, name)
    m, n, Ap, Ai, Ax, tol, Q = mat
    A = spmat(mat)
    B = np.asfortranarray(np.random.default_rng(5).standard_normal((m, 2)))
    L = least_squares(pkg, mat, 2)
    try:
        X, resid = L.solve(B)
        rank = int(L.info["rank"])
    finally:
        L.close()
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    out = {}
    for keep in (1, 0):
        plan = pkg.HipQR({**sym, "keepH": keep})
        try:
            plan.factorize(Ax, tol, n, Ap, Ai)
            if keep:
                out["q"] = backward_error(A, plan.solve(B), B)
            else:
                Xs, out["csne_info"] = plan.solve_seminormal(B, refine=1)
                out["csne"] = backward_error(A, Xs, B)
        finally:
            plan.close()
    be = backward_error(A, X, B)
    print(f"[carried ill-conditioned] {name} rank {rank}: backward error carried {be:.3e} Q-based {out['q']:.3e} seminormal {out['csne']:.3e} "
          f"(its info {out['csne_info']:.3e})")
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(resid))
    assert be <= 10.0 * out["q"]


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "syn_dupcol", "dwt_992", "lns_3937"])
def test_rank_deficient(pkg, name):
    g = load_golden(name)
    mat = matrix(g, name)
    m, n = mat[:2]
    B = np.asfortranarray(np.random.default_rng(6).standard_normal((m, 2)))
    L = least_squares(pkg, mat, 2)
    try:
        X, resid = L.solve(B)
        rank = int(L.info["rank"])
        assert rank == int(scalar(g, "num_rank1")) and rank < n
        N = L.plan().download()
        assert N.rank1 == rank
        q = L.symbolic()["Qfill"][:n]
        dead = q[np.flatnonzero(np.asarray(N.Rdead[:n]) != 0)]
        assert dead.size == n - rank
        assert np.all(np.isfinite(X)) and np.all(np.isfinite(resid))
        assert np.all(X[dead, :] == 0.0)
        A = spmat(mat)
        true = np.linalg.norm(B - A @ X, axis=0)
        print(f"[carried rank-deficient] {name} rank {rank} of {n}: backward error {backward_error(A, X, B):.2e} resid {resid} true {true}")
    finally:
        L.close()


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_star", "syn_emptycol", "syn_grid3d"])
def test_residual_norms(pkg, name, nrhs):
    """|resid[j] - |b_j - A x_j|| <= 1e-10 (|A|_F |x_j| + |b_j|): the project's relative bar on the scale of the rounding error of
    forming the residual; on square full-rank input no rows are left below C and resid is exactly 0"""
    g = load_golden(name)
    mat = matrix(g, name)
    m, n = mat[:2]
    A = spmat(mat)
    B = np.asfortranarray(np.random.default_rng(7).standard_normal((m, nrhs)))
    L = least_squares(pkg, mat, nrhs)
    try:
        X, resid = L.solve(B)
        assert int(L.info["rank"]) == n
    finally:
        L.close()
    af = np.linalg.norm(mat[4])
    for j in range(nrhs):
        true = np.linalg.norm(B[:, j] - A @ X[:, j])
        scale = af * np.linalg.norm(X[:, j]) + np.linalg.norm(B[:, j])
        print(f"[carried resid] {name} rhs {j}: device {resid[j]:.16e} host {true:.16e} diff / scale {abs(resid[j] - true) / scale:.2e}")
        assert abs(resid[j] - true) <= 1e-10 * scale
        if m == n:
            assert resid[j] == 0.0
        else:
            assert resid[j] > 0.0


@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_grid3d", "dwt_992", "bcsstk14"])
def test_degenerate_right_hand_sides(pkg, name):
    g = load_golden(name)
    mat = matrix(g, name)
    m, n = mat[:2]
    A = spmat(mat)
    L = least_squares(pkg, mat, 2)
    try:
        X, resid = L.solve(np.zeros((m, 2)))
        assert np.all(X == 0.0) and np.all(resid == 0.0)
        x0 = np.random.default_rng(8).standard_normal((n, 2))
        B = np.asfortranarray(A @ x0)                                  # exactly in range(A): nothing is left for the B pivots
        X, resid = L.solve(B)
        assert np.all(np.isfinite(X)) and np.all(np.isfinite(resid))
        be = backward_error(A, X, B)
        print(f"[carried b in range(A)] {name}: backward error {be:.2e} resid {resid} |b| {np.linalg.norm(B, axis=0)}")
        assert be <= 1e-13
        B[:, 1] = 0.0                                                  # one zero column beside a general one
        X, resid = L.solve(B)
        assert np.all(X[:, 1] == 0.0) and resid[1] == 0.0 and np.all(np.isfinite(X))
    finally:
        L.close()


@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_star", "lns_3937", "t2d_q9"])
def test_reuse(pkg, name):
    import torch
    g = load_golden(name)
    mat = matrix(g, name)
    m, n, Ap, Ai, Ax = mat[:5]
    rng = np.random.default_rng(9)
    B1 = np.asfortranarray(rng.standard_normal((m, 2)))
    B2 = np.asfortranarray(rng.standard_normal((m, 2)))
    Ax2 = Ax * (1.0 + 1e-3 * rng.standard_normal(Ax.size))
    L = least_squares(pkg, mat, 2)
    try:
        X1, r1 = L.solve(B1)
        X1b, r1b = L.solve(B1)
        assert np.array_equal(bits(X1), bits(X1b)) and np.array_equal(bits(r1), bits(r1b))          # the same call twice
        X2, r2 = L.solve(B2, Ax=Ax2)
        info = L.info
        assert info["analyses"] == 1 and info["plans"] == 1 and info["solves"] == 3
        F = least_squares(pkg, (m, n, Ap, Ai, Ax2) + mat[5:], 2)
        try:
            Xf, rf = F.solve(B2)
            assert F.info["tol"] == info["tol"]
        finally:
            F.close()
        assert np.array_equal(bits(X2), bits(Xf)) and np.array_equal(bits(r2), bits(rf))            # == a fresh object, bit for bit
        # device pointers: B, X, A's values
        dB = torch.from_numpy(np.ascontiguousarray(B2.T)).cuda()
        dA = torch.from_numpy(np.ascontiguousarray(Ax2)).cuda()
        dX = torch.zeros((2, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rd = L.solve_dev(dB.data_ptr(), dX.data_ptr(), ax_ptr=dA.data_ptr())
        torch.cuda.synchronize()
        Xd = np.asfortranarray(dX.cpu().numpy().T)
        assert np.array_equal(bits(Xd), bits(X2)) and np.array_equal(bits(rd), bits(r2))
        assert L.info["analyses"] == 1 and L.info["plans"] == 1
        X3, r3 = L.solve(B1)                                                                        # Ax = None: the values given at create
        assert np.array_equal(bits(X3), bits(X1)) and np.array_equal(bits(r3), bits(r1))
    finally:
        L.close()


@pytest.mark.parametrize("name", ["syn_rand60x40", "dwt_992", "t2d_q9"])
def test_batches_of_right_hand_sides(pkg, name):
    """40 right-hand sides: a batch of 32 and one of 8, each in one pass over the tree (STMMQR_RHS_BATCH)"""
    g = load_golden(name)
    mat = matrix(g, name)
    m, n = mat[:2]
    k = 40
    B = np.asfortranarray(np.random.default_rng(10).standard_normal((m, k)))
    L = least_squares(pkg, mat, k)
    try:
        X, resid = L.solve(B)
        X1, r1 = L.plan().solve_carried(k)
        assert np.array_equal(bits(X1), bits(X)) and np.array_equal(bits(r1), bits(resid))
    finally:
        L.close()
    A = spmat(mat)
    be = backward_error(A, X, B)
    true = np.linalg.norm(B - A @ X, axis=0)
    scale = np.linalg.norm(mat[4]) * np.linalg.norm(X, axis=0) + np.linalg.norm(B, axis=0)
    print(f"[carried 40 rhs] {name}: backward error {be:.2e} resid diff / scale {np.max(np.abs(resid - true) / scale):.2e}")
    assert be <= 1e-13
    assert np.all(np.abs(resid - true) <= 1e-10 * scale)


@pytest.mark.parametrize("recycle", ["0", "2"])
@pytest.mark.parametrize("cache", ["0", "1"])
@pytest.mark.parametrize("name", ["dwt_992", "t2d_q9"])
def test_slab_recycling_and_front_form_rebuild(pkg, env, name, recycle, cache):
    """recycled slabs: the fronts are put back into front form level by level (STMMQR_RESIDENT_CACHE=0) or all at once (1); the same bits
    as without recycling"""
    g = load_golden(name)
    mat = matrix(g, name)
    m = mat[0]
    B = np.asfortranarray(np.random.default_rng(12).standard_normal((m, 3)))
    env(STMMQR_RECYCLE="0")
    L = least_squares(pkg, mat, 3)
    try:
        X0, r0 = L.solve(B)
    finally:
        L.close()
    env(STMMQR_RECYCLE=recycle, STMMQR_RESIDENT_CACHE=cache)
    L = least_squares(pkg, mat, 3)
    try:
        X, r = L.solve(B)
        Xb, rb = L.solve(B)
    finally:
        L.close()
    assert np.array_equal(bits(X), bits(X0)) and np.array_equal(bits(r), bits(r0))
    assert np.array_equal(bits(Xb), bits(X0)) and np.array_equal(bits(rb), bits(r0))


@pytest.mark.parametrize("name", ["syn_rand60x40", "dwt_992", "t2d_q9"])
def test_plan_level(pkg, name):
    """stmmqr_plan_solve_carried on a HipQR built from capi.analyze of [A B] with the object's column order: the object's bits, also
    on a plan that keeps H; the refusals leave the plan usable"""
    g = load_golden(name)
    mat = matrix(g, name)
    m, n, Ap, Ai, Ax = mat[:5]
    k = 2
    B = np.asfortranarray(np.random.default_rng(13).standard_normal((m, k)))
    L = least_squares(pkg, mat, k)
    try:
        X, resid = L.solve(B)
        Q = L.symbolic()["Qfill"]
        tol = L.info["tol"]
    finally:
        L.close()
    Bp, Bi, Bx = augmented(m, n, Ap, Ai, Ax, B)
    sym = {kk: v for kk, v in pkg.analyze(m, n + k, Bp, Bi, Qfill=Q).items() if kk != "info"}
    for keep in (0, 1):
        plan = pkg.HipQR({**sym, "keepH": keep})
        try:
            with pytest.raises(pkg.StmmqrError) as e:                       # nothing factorized
                plan.solve_carried(k)
            assert e.value.code == -4
            plan.factorize(Bx, tol, n + k, Bp, Bi)                            # the B columns rank-tested: refused
            with pytest.raises(pkg.StmmqrError) as e:
                plan.solve_carried(k)
            assert e.value.code == -4 and "ntol" in str(e.value)
            plan.factorize(Bx, tol, n)
            for bad in (0, n + k + 1, k + 1):                                 # (k + 1: ntol does not belong to that many right-hand sides)
                with pytest.raises(pkg.StmmqrError) as e:
                    plan.solve_carried(bad)
                assert e.value.code == -4
            Xp, rp = plan.solve_carried(k)
            assert np.array_equal(bits(Xp), bits(X)) and np.array_equal(bits(rp), bits(resid))
            assert plan.keep_h == bool(keep)
            assert np.all(np.isfinite(plan.rsolve(3, np.ones(n + k))))        # the plan stays usable
        finally:
            plan.close()
    # a permuted B column is refused
    Qbad = Q.copy()
    Qbad[[n - 1, n]] = Qbad[[n, n - 1]]
    symb = {kk: v for kk, v in pkg.analyze(m, n + k, Bp, Bi, Qfill=Qbad).items() if kk != "info"}
    plan = pkg.HipQR({**symb, "keepH": 0})
    try:
        plan.factorize(Bx, tol, n, Bp, Bi)
        with pytest.raises(pkg.StmmqrError) as e:
            plan.solve_carried(k)
        assert e.value.code == -4 and "permuted" in str(e.value)
    finally:
        plan.close()


def test_large_fixture(pkg):
    """the workload tools/time_qless.py times, one right-hand side: no retries, less device memory than the plan of A that keeps H
    (DESIGN.md 6f measured 2.76 against 3.17 GB without the extra column), backward error within a factor 10 of the Q-based solve's"""
    g = load_golden(LARGE)
    mat = matrix(g, LARGE)
    m, n, Ap, Ai, Ax, tol, Q = mat
    A = spmat(mat)
    b = np.random.default_rng(14).standard_normal(m)
    L = least_squares(pkg, mat, 1)
    try:
        x, resid = L.solve(b)
        info = L.info
        ls_bytes = L.plan().device_bytes()                       # (after the solve: the front-form scratch of the resident operations included)
    finally:
        L.close()
    S = Symbolic(g)
    plan = pkg.HipQR({**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1})
    try:
        st = plan.factorize(Ax, tol, n, Ap, Ai)
        xq = plan.solve(b)
        h_bytes = plan.device_bytes()                            # (likewise after its solve)
    finally:
        plan.close()
    be, beq = backward_error(A, x[:, None], b[:, None]), backward_error(A, xq[:, None], b[:, None])
    print(f"[carried large] {LARGE}: retries {info['retries']} reschedules {info['reschedules']} device GB carried {ls_bytes / 1e9:.3f} "
          f"(after the factorization, with values {info['device_bytes'] / 1e9:.3f}) keepH=1 plan of A {h_bytes / 1e9:.3f} ({st['device_bytes'] / 1e9:.3f}); factorization ms {info['ms_factorize']:.2f} "
          f"(A with H {st['ms_total']:.2f}) solve ms {info['ms_solve']:.2f}; backward error carried {be:.3e} Q-based {beq:.3e} resid {resid}")
    assert info["retries"] == 0
    assert int(info["rank"]) == n
    # when the factorization finished (plan + the values [Ax | b]) against the plan of A with H at the same moment; and both after the solve
    assert info["device_bytes"] < st["device_bytes"]
    assert ls_bytes < h_bytes
    assert be <= 10.0 * beq
