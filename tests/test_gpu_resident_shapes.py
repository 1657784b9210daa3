"""Q-apply and back substitution on the resident factors at the fronts where their launchers change the kernel variant.

stm_launch_qapply_t / stm_launch_rsolve (csrc/stmmqr_resident.hip) run 4, 2 or 1 right-hand sides of a batch per workgroup by the
dynamic LDS one of them needs (stm_lds_qapply / stm_lds_rsolve, csrc/stmmqr_device.h), up to 128 KB; the planner sends a front that
needs more to the split kernels whatever its entry count.  The fixtures under tests/golden only ever reach the four-vector class
of the Q-apply, so here dense one-front plans sit on both sides of every threshold (tests/resident_reference.py SHAPES; the classes
are asserted from the analysis in tests/test_resident_reference_cpu.py): tall thin fronts for the Q-apply, short wide ones (every
column pivotal, 48 live) for the back substitution, batches of 1, 2, 3 and 5 so that the last workgroup of the two- and four-vector
kernels is ragged.

Checked at every shape: column j of a batched call is bit for bit the one-vector call; Q'X and Q X against the long-double
application of the reflectors rebuilt from the downloaded factors (1e-12, the project's bound); Q(Q'X) = X and |Q'x| = |x|;
R \\ Y, R' \\ B and the least-squares / basic solution against long double within solve_tol(cond_probe) -- the solution also
against a long-double Householder loop on A that never sees the factors; the driver's residual; exact zeros beyond the rank.

Measured on the MI355X (largest over the shapes of a class; bound 1e-12 / solve_tol >= 1e-9): DESIGN.md 6b."""
import importlib

import numpy as np
import pytest

import resident_reference as rr
from resident_reference import LD, Factors, householder_solve, make_front, rel, stair_csc, symbolic_of
from stmmqr_testlib import cond_probe, numeric_from_gpu, solve_tol

pytestmark = pytest.mark.gpu
TOL = 1e-10                     # far below the smallest pivot of these fronts (asserted)
ALL_BATCHES = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


def batched(call, X, batches, what):
    """call(X[:, :k]) for every batch size; every column must carry the bits of its one-vector call.  Returns the widest result."""
    kmax = max(batches)
    one = np.stack([np.asarray(call(X[:, j].copy())).ravel() for j in range(kmax)], axis=1)
    for k in batches:
        if k == 1:
            continue
        Y = call(X[:, :k].copy())
        for j in range(k):
            assert np.array_equal(Y[:, j], one[:, j]), f"{what}: column {j} of a batch of {k} differs from the one-vector call"
    return one


def check_plan(pkg, oracle, A, Ap, Ai, Ax, nf, batches=ALL_BATCHES, qmult23=False, label=""):
    """factorize A (dense blocks, no column permutation) under one plan, run every operation, close the plan, then judge"""
    m, n = A.shape
    kmax = max(batches)
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    assert sym["nf"] == nf
    np.testing.assert_array_equal(sym["PLinv"], np.arange(m))
    S = symbolic_of(sym)
    rng = np.random.default_rng(7 * m + n)
    X = np.asfortranarray(rng.standard_normal((m, kmax)))
    Y = np.asfortranarray(rng.standard_normal((m, kmax)))
    Bn = np.asfortranarray(rng.standard_normal((n, kmax)))
    xt = rng.standard_normal((n, kmax))
    if m < n:
        B = np.asfortranarray(rng.standard_normal((m, kmax)))            # full row rank: every b is consistent, x is the basic solution
    else:
        B = A @ xt
        B[:, 1::2] += 1e-3 * rng.standard_normal((m, len(range(1, kmax, 2))))     # consistent and inconsistent ones alternate
        B = np.asfortranarray(B)
    out = {"B": B}
    rt_ok = all(rr.rt_fits(int(sym["Fm"][f]), int(sym["Rp"][f + 1] - sym["Rp"][f])) for f in range(nf))
    plan = pkg.HipQR(sym)
    try:
        stats = plan.factorize(Ax, TOL, n, Ap, Ai)
        G = plan.download()
        out["qt"] = batched(lambda v: plan.qmult(0, v), X, batches, "Q'X")
        out["q"] = batched(lambda v: plan.qmult(1, v), X, batches, "Q X")
        out["back"] = plan.qmult(1, out["qt"])
        out["solve"] = batched(plan.solve, B, batches, "solve")
        out["r0"] = batched(lambda v: plan.rsolve(0, v), Y, batches, "R X = B")
        out["r1"] = batched(lambda v: plan.rsolve(1, v), Y, batches, "R E'X = B")
        if rt_ok:
            out["r2"] = batched(lambda v: plan.rsolve(2, v), Bn, batches, "R'X = B")
            out["r3"] = batched(lambda v: plan.rsolve(3, v), Bn, batches, "R'X = E'B")
        else:
            for system in (2, 3):                                         # the documented refusal, before any launch
                with pytest.raises(pkg.StmmqrError) as e:
                    plan.rsolve(system, Bn)
                assert e.value.code == -3 and "too wide for the one-workgroup R' solve" in str(e.value)
            assert np.array_equal(plan.rsolve(0, Y[:, 0].copy()), out["r0"][:, 0])          # (the plan stays usable)
        if qmult23:
            Xr = np.ascontiguousarray(X.T)                               # the vectors as rows: X Q' = (Q X')', X Q = (Q'X')'
            for method, same in ((2, "q"), (3, "qt")):
                Z = plan.qmult(method, Xr)
                assert np.array_equal(Z.T, out[same]), f"qmult {method} differs from the transposed qmult {3 - method}"
                assert np.array_equal(plan.qmult(method, Xr[:1].copy()).ravel(), out[same][:, 0])
    finally:
        plan.close()
    # ---- decisions: the long-double loop on A ----
    Xi, rank_i, dead_i, absb = householder_solve(A, B, TOL)
    assert stats["retries"] == 0
    assert G.rank == rank_i == min(m, n)
    np.testing.assert_array_equal(np.asarray(G.Rdead[:n]) != 0, dead_i)
    assert not dead_i[:min(m, n)].any()                                  # no column dies; beyond the last row nothing is left to pivot on
    assert float(absb[:rank_i].min()) > 1e6 * TOL
    # ---- Q ----
    N = numeric_from_gpu(S, G)
    Fa = Factors(S, N)
    assert Fa.rank == G.rank
    e_qt, e_q = rel(out["qt"], Fa.qtx(X)), rel(out["q"], Fa.qx(X))
    e_back = rel(out["back"], X)
    e_norm = float(np.abs(np.linalg.norm(out["qt"], axis=0) / np.linalg.norm(X, axis=0) - 1).max())
    # ---- R ----
    kappa = cond_probe(oracle, S, N)
    allowed = solve_tol(kappa)
    e_r0, e_r1 = rel(out["r0"], Fa.rsolve(Y)), rel(out["r1"], Fa.rsolve(Y))
    e_sf, e_si = rel(out["solve"], Fa.rsolve(Fa.qtx(B))), rel(out["solve"], Xi)
    e_rt = max(rel(out["r2"], Fa.rtsolve(Bn)), rel(out["r3"], Fa.rtsolve(Bn))) if rt_ok else float("nan")
    anorm = np.linalg.norm(Ax)
    res = float(max(np.linalg.norm(A @ out["solve"][:, j] - B[:, j]) / (anorm * np.linalg.norm(out["solve"][:, j]) + np.linalg.norm(B[:, j]))
                    for j in range(0, kmax, 2)))
    print(f"\n[resident shapes] {label or f'{m}x{n}'}: Q'X {e_qt:.2e} QX {e_q:.2e} Q(Q'X) {e_back:.2e} norm {e_norm:.2e} | cond_probe {kappa:.1e} "
          f"allowed {allowed:.1e}: R\\Y {e_r0:.2e} R'\\B {e_rt:.2e} solve vs factors {e_sf:.2e} vs A {e_si:.2e} residual {res:.2e}")
    assert e_qt <= 1e-12 and e_q <= 1e-12
    assert e_back <= 1e-12 and e_norm <= 1e-12
    assert e_r0 <= allowed and e_r1 <= allowed
    assert e_sf <= allowed and e_si <= allowed
    if rt_ok:
        assert e_rt <= allowed
        assert not np.any(out["r2"][G.rank:]) and not np.any(out["r3"][G.rank:])
    assert res <= 1e-10                                                   # the driver's check, consistent systems
    for key in ("solve", "r0", "r1"):
        assert not np.any(out[key][dead_i]), f"{key}: a dead column of the basic solution is not exactly 0"
    if m >= n:
        assert rel(out["solve"][:, 0::2], xt[:, 0::2]) <= allowed
    return Fa, out


def one_front(pkg, oracle, m, n, kind="full", **kw):
    F, St = make_front(m, n, kind)
    Ap, Ai, Ax = stair_csc(F, St)
    return check_plan(pkg, oracle, F, Ap, Ai, Ax, 1, label=f"{m}x{n} {kind}", **kw)


ONE_WORKGROUP = [s for s in rr.SHAPES if rr.SHAPES[s] != (0, 0)]
SPLIT = [s for s in rr.SHAPES if rr.SHAPES[s] == (0, 0)]


@pytest.mark.parametrize("shape", ONE_WORKGROUP, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_workgroup_kernels_on_both_sides_of_every_threshold(pkg, oracle, shape):
    """k_qapply_t<4 / 2 / 1> and k_rsolve<4 / 2 / 1> with full and ragged workgroups, dynamic LDS up to exactly 128 KB"""
    one_front(pkg, oracle, *shape, qmult23=(shape == (8171, 40)))


def test_five_panels_under_a_ramp_staircase(pkg, oracle):
    """4500 x 160, two vectors per workgroup: the reflectors of a panel start and end at different rows"""
    one_front(pkg, oracle, 4500, 160, "ramp")


@pytest.mark.parametrize("shape", SPLIT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fronts_beyond_the_lds_limit_take_the_split_kernels(pkg, oracle, shape):
    """One row / one column past what a workgroup holds in LDS, below 2^20 entries: such a front could be factorized but neither
    applied nor solved with (16363 x 40: refused; 48 x 10921: a launch asking for more LDS than configured) until the planner sent
    it to the split kernels.  Batches of 1 and 5."""
    assert shape[0] * shape[1] < 1 << 20
    one_front(pkg, oracle, *shape, batches=(1, 5))


def test_small_front_in_the_variant_its_sibling_forces(pkg, oracle):
    """diag(8171 x 40, 50 x 20): two fronts on one tree level, launched together with the LDS of the tall one -- the small front runs
    one vector per workgroup with 64 KB it does not use.  Each block against its own long-double solution."""
    A1, A2 = make_front(8171, 40)[0], make_front(50, 20)[0]
    A = np.zeros((8221, 60), order="F")
    A[:8171, :40], A[8171:, 40:] = A1, A2
    Ap = np.concatenate([np.arange(0, 8171 * 40 + 1, 8171), 8171 * 40 + np.arange(50, 50 * 20 + 1, 50)]).astype(np.int64)
    Ai = np.concatenate([np.tile(np.arange(8171, dtype=np.int64), 40), np.tile(8171 + np.arange(50, dtype=np.int64), 20)])
    Ax = np.concatenate([A1.T.ravel(), A2.T.ravel()])
    Fa, out = check_plan(pkg, oracle, A, Ap, Ai, Ax, 2, label="diag(8171x40, 50x20)")
    assert [len(r) for r in Fa.refl] in ([40, 20], [20, 40])
    B = out["B"]                                                         # (the blocks do not interact: each has its own solution)
    for blk, rows, cols in ((A1, slice(0, 8171), slice(0, 40)), (A2, slice(8171, 8221), slice(40, 60))):
        Xb, rank_b, dead_b, _ = householder_solve(blk, B[rows], TOL)
        assert rank_b == blk.shape[1] and not dead_b.any()
        d = rel(out["solve"][cols], Xb)
        print(f"  block {blk.shape[0]}x{blk.shape[1]}: solve vs its own long-double solution {d:.2e}")
        assert d <= solve_tol(float(np.linalg.cond(blk)))


def test_carried_right_hand_sides_on_a_tall_front(pkg):
    """LeastSquares (the right-hand sides carried through the factorization, R only) on the 8170 x 40 front with 3 right-hand sides:
    the long-double least-squares solution and its residual norms"""
    m, n, k = 8170, 40, 3
    F, St = make_front(m, n)
    Ap, Ai, Ax = stair_csc(F, St)
    rng = np.random.default_rng(m + n)
    B = F @ rng.standard_normal((n, k))
    B[:, 1:] += 1e-3 * rng.standard_normal((m, k - 1))
    B = np.asfortranarray(B)
    L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=k, tol=TOL, ordering=3, Quser=np.arange(n))
    try:
        X, resid = L.solve(B)
        info = L.info
    finally:
        L.close()
    assert int(info["rank"]) == n and info["retries"] == 0
    Xi, rank_i, dead_i, _ = householder_solve(F, B, TOL)
    assert rank_i == n and not dead_i.any()
    R = np.asarray(B, LD) - np.asarray(F, LD) @ Xi
    rn = np.sqrt((R * R).sum(axis=0)).astype(float)
    d = rel(X, Xi)
    allowed = solve_tol(float(np.linalg.cond(F)))
    dr = float(np.abs(resid - rn).max() / np.linalg.norm(B, axis=0).max())
    print(f"\n[resident shapes] carried 8170x40, 3 rhs: x {d:.2e} (allowed {allowed:.1e}) residual norms {dr:.2e} of |b|")
    assert d <= allowed
    assert dr <= 1e-12
