"""What tests/test_gpu_resident_shapes.py relies on, checked without a GPU: the long-double references of
tests/resident_reference.py agree with the CPU oracle's checkers on factors the oracle produced (dense one-front plans, tall,
staircase, wide, rank deficient, two fronts), the reference that never sees the factors agrees with the one built from them, and
every shape of the table falls into the class of right-hand sides per workgroup that the table lists -- computed from the
analysis of the very pattern the GPU test factorizes, so the table cannot drift off the launchers' thresholds unnoticed."""
import importlib

import numpy as np
import pytest

import resident_reference as rr
from resident_reference import LD, Factors, householder_solve, make_front, rel, stair_csc, symbolic_of
from stmmqr_testlib import EPS, I64, TOL_C

PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
TOL = 1e-10


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def block_diagonal(blocks):
    """CSC of diag(blocks) (dense blocks) and the dense matrix"""
    m, n = sum(b.shape[0] for b in blocks), sum(b.shape[1] for b in blocks)
    A = np.zeros((m, n), order="F")
    Ap, Ai, Ax, r0, c0 = [0], [], [], 0, 0
    for b in blocks:
        A[r0:r0 + b.shape[0], c0:c0 + b.shape[1]] = b
        for k in range(b.shape[1]):
            Ai.append(np.arange(r0, r0 + b.shape[0], dtype=I64))
            Ax.append(b[:, k])
            Ap.append(Ap[-1] + b.shape[0])
        r0 += b.shape[0]
        c0 += b.shape[1]
    return A, np.array(Ap, I64), np.concatenate(Ai), np.concatenate(Ax)


def small_case(name):
    """(A dense, Ap, Ai, Ax, fronts expected, dead columns expected)"""
    if name == "tall":
        F, St = make_front(300, 40)
    elif name == "ramp":
        F, St = make_front(300, 70, "ramp")
    elif name == "wide":
        F, St = make_front(20, 70)
    elif name == "dead":
        F, St = make_front(200, 40)
        F[:, 17] = F[:, 3] - 2 * F[:, 9]                    # a pivot of rounding size: dead at tol = 1e-10
        F[:, 39] = F[:, 0]
    else:
        assert name == "two"
        A, Ap, Ai, Ax = block_diagonal([make_front(120, 24)[0], make_front(30, 10)[0]])
        return A, Ap, Ai, Ax, 2, []
    Ap, Ai, Ax = stair_csc(F, St)
    dead = {"dead": [17, 39], "wide": list(range(20, 70))}.get(name, [])
    return F, Ap, Ai, Ax, 1, dead


@pytest.mark.parametrize("name", ["tall", "ramp", "wide", "dead", "two"])
def test_references_agree_with_the_oracle_and_with_each_other(pkg, oracle, name):
    A, Ap, Ai, Ax, nf, want_dead = small_case(name)
    m, n = A.shape
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    assert sym["nf"] == nf
    np.testing.assert_array_equal(sym["PLinv"], np.arange(m))
    S = symbolic_of(sym)
    N = oracle.factorize(S, Ap, Ai, Ax, TOL, n)
    assert np.flatnonzero(N.Rdead[:n]).tolist() == want_dead
    Fa = Factors(S, N)
    assert Fa.rank == int(N.c.rank) == n - len(want_dead)
    rng = np.random.default_rng(17)
    X = rng.standard_normal((m, 3))
    # ---- Q'X, Q X, R \ Y from the factors: the oracle's fp64 checkers on the same factors ----
    QtX, QX = Fa.qtx(X), Fa.qx(X)
    for j in range(3):
        assert rel(oracle.qmult(0, S, N, X[:, j]), QtX[:, j]) <= 1e-13
        assert rel(oracle.qmult(1, S, N, X[:, j]), QX[:, j]) <= 1e-13
        assert rel(oracle.rsolve(S, N, X[:, j]), Fa.rsolve(X[:, j])) <= 1e-13
    assert rel(Fa.qx(QtX), X) <= 1e-15 and abs(float(np.sqrt((QtX ** 2).sum() / (X ** 2).sum())) - 1) <= 1e-15      # (orthogonal to fp64 rounding of V, tau)
    # ---- R' \ B: the adjoint identity x'(R z) = b'z with the oracle's R z, z zero on the dead columns ----
    B = rng.standard_normal((n, 2))
    Xt = Fa.rtsolve(B)
    assert not np.any(Xt[Fa.rank:])
    dead = np.asarray(N.Rdead[:n]) != 0
    for j in range(2):
        for _ in range(3):
            z = rng.standard_normal(n)
            z[dead] = 0.0
            Rz = oracle.rmult(S, N, z)
            lhs, rhs = float(Xt[:, j] @ np.asarray(Rz, LD)), float(B[:, j] @ z)
            assert abs(lhs - rhs) <= 1e-13 * max(np.linalg.norm(B[:, j]) * np.linalg.norm(z), float(np.linalg.norm(Xt[:, j].astype(float))) * np.linalg.norm(Rz))
    # ---- the reference from A alone: same decisions, same solution as through the oracle's factors.  The factors carry the
    # rounding of an fp64 factorization: a relative backward error of a few eps, so the solution differs by eps * cond for a
    # consistent system and by eps * cond^2 at most for an inconsistent one (least-squares perturbation bound) ----
    live = np.flatnonzero(~dead)
    kappa = float(np.linalg.cond(A[:, live]))
    xt = rng.standard_normal(n)
    xt[dead] = 0.0
    Bs = np.stack([A @ xt, A @ xt + 1e-3 * rng.standard_normal(m)], axis=1)
    Xi, rank_i, dead_i, absb = householder_solve(A, Bs, TOL)
    assert rank_i == Fa.rank and np.array_equal(dead_i, dead)
    ratio = np.array(absb[:n][absb[:n] > 0], float) / TOL
    assert np.all((ratio < 1e-3) | (ratio > 1e3))                               # no decision anywhere near tol
    Xf = Fa.rsolve(Fa.qtx(Bs))
    d0, d1 = rel(Xf[:, 0], Xi[:, 0]), rel(Xf[:, 1], Xi[:, 1])
    print(f"\n{name}: cond {kappa:.1f}; independent vs factor-based solve: consistent {d0:.2e}, inconsistent {d1:.2e}")
    assert d0 <= TOL_C * EPS * kappa and d1 <= TOL_C * EPS * kappa * kappa
    assert not np.any(Xi[dead]) and not np.any(Xf[dead])
    if m >= n and not want_dead:
        assert rel(Xi[:, 0], xt) <= TOL_C * EPS * kappa


def dense_pattern(m, n):
    return np.arange(0, m * n + 1, m, dtype=I64), np.tile(np.arange(m, dtype=I64), n)


@pytest.mark.parametrize("shape", list(rr.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_shape_table_sits_on_the_thresholds(pkg, shape):
    m, n = shape
    sym = pkg.analyze(m, n, *dense_pattern(m, n), Qfill=None)
    assert sym["nf"] == 1                               # one front, tall or wide
    fp, fn, fm = int(sym["Super"][1] - sym["Super"][0]), int(sym["Rp"][1] - sym["Rp"][0]), int(sym["Fm"][0])
    assert (fp, fn, fm) == (n, n, m)
    assert m * n < 1 << 20                              # not split for its entry count
    qa, rs = rr.lds_qapply(fm, fn), rr.lds_rsolve(fp, fn)
    split = qa > rr.LDS_MAX or rs > rr.LDS_MAX
    got = (0, 0) if split else (rr.rhs_class(qa), rr.rhs_class(rs))
    assert got == rr.SHAPES[shape], (qa, rs)


def test_thresholds_are_met_exactly_and_neighbours_differ():
    assert rr.lds_qapply(2026, 40) == 16384 and rr.lds_qapply(8170, 40) == 65536 and rr.lds_qapply(16362, 40) == 131072
    assert rr.lds_rsolve(10920, 10920) == 131072
    assert 4 * rr.lds_rsolve(1362, 1362) <= 65536 < 4 * rr.lds_rsolve(1363, 1363)
    assert 2 * rr.lds_rsolve(5458, 5458) <= 131072 < 2 * rr.lds_rsolve(5459, 5459)
    for a, b in (((2026, 40), (2027, 40)), ((8170, 40), (8171, 40)), ((16362, 40), (16363, 40)), ((48, 1362), (48, 1363)),
                 ((48, 5458), (48, 5459)), ((48, 10920), (48, 10921))):
        assert rr.SHAPES[a] != rr.SHAPES[b]
    # the R' solve keeps its own limit: refused on the two widest fronts, taken everywhere else
    assert [s for s in rr.SHAPES if not rr.rt_fits(*s)] == [(48, 10920), (48, 10921)]


def test_ramp_and_block_diagonal_patterns_analyse_as_expected(pkg):
    F, St = make_front(4500, 160, "ramp")
    assert St[0] < 64 and St[-1] == 4500 and np.all(np.diff(St) >= 0)
    Ap, Ai, _ = stair_csc(F, St)
    sym = pkg.analyze(4500, 160, Ap, Ai, Qfill=None)
    assert sym["nf"] == 1 and int(sym["Fm"][0]) == 4500
    np.testing.assert_array_equal(sym["PLinv"], np.arange(4500))
    Ap = np.concatenate([np.arange(0, 8171 * 40 + 1, 8171), 8171 * 40 + np.arange(50, 50 * 20 + 1, 50)]).astype(I64)
    Ai = np.concatenate([np.tile(np.arange(8171, dtype=I64), 40), np.tile(8171 + np.arange(50, dtype=I64), 20)])
    sym = pkg.analyze(8221, 60, Ap, Ai, Qfill=None)
    assert sym["nf"] == 2
    assert sorted(int(x) for x in sym["Fm"][:2]) == [50, 8171]
    assert sym["Parent"][0] == sym["Parent"][1]         # neither is the other's child: one tree level
