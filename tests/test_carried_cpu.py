"""Least squares with the right-hand sides carried through the factorization, host half (no GPU): the symbolic analysis of
[A B] that LeastSquares builds, and the arithmetic of the method on the CPU oracle -- factorize [A B] with ntol = n, read
C = Q'B out of the last columns of R, back-substitute over the first n columns (a host restatement written here from the packed
blocks), compare against the least-squares conditions of the original problem."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

from stmmqr_testlib import Symbolic, front_R, load_golden, scalar

PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
NAMES = ["syn_grid3d", "syn_star", "syn_rand60x40", "syn_rankdef_grid", "syn_dupcol", "syn_emptycol", "syn_wide5x8", "dwt_992", "lns_3937",
         "bcsstk14", "ex18", "bayer10"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def problem(g):
    """the matrix the golden factorization was made of (m, n, Ap, Ai, Ax, tol)"""
    return int(scalar(g, "in_m")), int(scalar(g, "in_n")), g["in_Ap"], g["in_Ai"], g["in_Ax"], float(scalar(g, "in_tol"))


def rhs(m, k, seed=11):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((m, k)))


def augmented(m, n, Ap, Ai, Ax, B):
    """[A B] in compressed columns: the B columns dense, rows 0 .. m-1"""
    k = B.shape[1]
    Bp = np.concatenate([Ap, Ap[-1] + m * np.arange(1, k + 1)]).astype(np.int64)
    Bi = np.concatenate([Ai, np.tile(np.arange(m, dtype=np.int64), k)])
    Bx = np.concatenate([Ax, B.reshape(-1, order="F")])
    return Bp, Bi, Bx


def symbolic_of(sym: dict) -> Symbolic:
    return Symbolic({"sym_" + k: (v if isinstance(v, np.ndarray) else np.array([v])) for k, v in sym.items()})


def backward_error(A, X, B):
    af = sp.linalg.norm(A) if A.nnz else 0.0
    worst = 0.0
    for j in range(B.shape[1]):
        r = B[:, j] - A @ X[:, j]
        den = af * (af * np.linalg.norm(X[:, j]) + np.linalg.norm(B[:, j]))
        q = np.linalg.norm(A.T @ r)
        worst = max(worst, q / den if den > 0 else (np.inf if q > 0 else 0.0))
    return worst


def carried_solve_host(S: Symbolic, N, n, k):
    """x = E R11^-1 C and the residual norms from the packed blocks of a factorization of [A B] (ntol = n): fronts from the root
    down; in every front the rows of its live A pivots hold [R11 R12 | C]."""
    blocks = N.rh_blocks(S)
    x = np.zeros((S.n, k))                                  # R's column order; the B entries are never used
    resid2 = np.zeros(k)
    for f in reversed([int(f) for f in S.Post[:S.nf]]):
        fp = int(S.Super[f + 1] - S.Super[f])
        p1, fn = int(S.Rp[f]), int(S.Rp[f + 1] - S.Rp[f])
        fm = int(N.Hm[f])
        if fm <= 0 or fn <= 0:
            continue
        stair = N.HStair[p1:p1 + fn]
        cols = S.Rj[p1:p1 + fn]
        R = front_R(blocks[f], stair, fp, fn, fm)
        live, rm_of = [], {}
        q = 0
        for c in range(fp):
            if stair[c] != 0 and q < fm:
                live.append(c)
                q += 1
            rm_of[c] = q                                     # rows of R in pivotal column c
        la = [c for c in live if cols[c] < n]                # live A pivots: rows 0 .. ra-1
        ra = len(la)
        for c in range(fp):
            if cols[c] >= n:                                 # a B column that is pivotal here: below row ra, its part of the residual
                resid2[cols[c] - n] += float(np.sum(R[ra:rm_of[c], c] ** 2))
        if ra == 0:
            continue
        bcol = {int(cols[c]) - n: c for c in range(fn) if cols[c] >= n}
        others = [c for c in range(fn) if cols[c] < n and c not in la]
        T = R[:ra, la]
        for j in range(k):
            acc = R[:ra, bcol[j]] - R[:ra, others] @ x[cols[others], j]
            x[cols[la], j] = np.linalg.solve(T, acc) if ra else 0.0
    X = np.zeros((n, k))
    q = S.Qfill if S.Qfill is not None else np.arange(S.n)
    X[q[:n], :] = x[:n, :]
    return X, np.sqrt(resid2)


@pytest.mark.parametrize("nrhs", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_symbolic_of_augmented_problem(pkg, name, nrhs):
    g = load_golden(name)
    m, n, Ap, Ai, Ax, tol = problem(g)
    L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs, tol=tol, symbolic_only=True)
    try:
        sym = L.symbolic()
        assert sym["m"] == m and sym["n"] == n + nrhs
        assert sym["anz"] == int(Ap[-1]) + m * nrhs
        Q = sym["Qfill"]
        assert np.array_equal(np.sort(Q[:n]), np.arange(n))
        assert np.array_equal(Q[n:], np.arange(n, n + nrhs))
        info = L.info
        assert info["analyses"] == 1 and info["plans"] == 0 and info["nf"] == sym["nf"]
    finally:
        L.close()


@pytest.mark.parametrize("order", ["golden", "library"])
@pytest.mark.parametrize("nrhs", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_arithmetic_on_the_library_analysis(pkg, oracle, name, nrhs, order):
    """Backward error <= 1e-13 and the rank of A, on the analysis LeastSquares makes of [A B].

    The rank a thresholded Householder QR finds belongs to a matrix AND a column order: the golden num_rank1 is that of the golden
    Qfill.  The fixtures are the matrices handed to qr_factorize (already in the reference's fill-reducing order), so the library's
    default ordering permutes them once more and three ill-conditioned ones then have another rank -- with or without B:
    lns_3937 1801 (golden 1822), ex18 5665 (5666), bayer10 12099 (12101), measured with the CPU oracle; the factorization of A alone
    in the same order gives the same 1801 / 5665 / 12099.  So "golden": the golden column order (ordering GIVEN), rank1 == golden
    num_rank1; "library": the default ordering, rank1 == the rank1 of the oracle's factorization of A alone in that order -- carrying B
    must not change the rank of A.  Both: the backward error bar."""
    g = load_golden(name)
    m, n, Ap, Ai, Ax, tol = problem(g)
    gq = g["sym_Qfill"] if g["sym_Qfill"].size else np.arange(n)
    kw = dict(ordering=3, Quser=gq) if order == "golden" else {}
    L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs, tol=tol, symbolic_only=True, **kw)
    try:
        sym = L.symbolic()
    finally:
        L.close()
    S = symbolic_of(sym)
    if order == "golden":
        assert np.array_equal(sym["Qfill"][:n], gq)
        want = int(scalar(g, "num_rank1"))
    else:
        sa = pkg.analyze(m, n, Ap, Ai, Qfill=sym["Qfill"][:n])
        want = int(oracle.factorize(symbolic_of({k: v for k, v in sa.items() if k != "info"}), Ap, Ai, Ax, tol, n).c.rank1)
    B = rhs(m, nrhs)
    Bp, Bi, Bx = augmented(m, n, Ap, Ai, Ax, B)
    N = oracle.factorize(S, Bp, Bi, Bx, tol, n)
    X, resid = carried_solve_host(S, N, n, nrhs)
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n))
    be = backward_error(A, X, B)
    true = np.linalg.norm(B - A @ X, axis=0)
    print(f"[carried cpu] {name} nrhs {nrhs} {order} order: backward error {be:.2e} rank1 {int(N.c.rank1)} (expected {want}, golden "
          f"{int(scalar(g, 'num_rank1'))}) nf {S.nf} resid rel diff {np.max(np.abs(resid - true) / np.maximum(true, 1e-300)):.2e}")
    assert np.all(np.isfinite(X))
    assert be <= 1e-13
    assert int(N.c.rank1) == want


def test_argument_errors(pkg):
    g = load_golden("syn_rand60x40")
    m, n, Ap, Ai, Ax, tol = problem(g)
    for kw in (dict(nrhs=0), dict(nrhs=-3), dict(ordering=5), dict(ordering=10), dict(ordering=3, Quser=np.zeros(n, np.int64)),
               dict(ordering=3, Quser=np.arange(1, n + 1)), dict(nrhs=10 ** 6)):
        with pytest.raises(pkg.StmmqrError) as e:
            pkg.LeastSquares(m, n, Ap, Ai, Ax, symbolic_only=True, **kw)
        assert e.value.code == -4, kw
    with pytest.raises(pkg.StmmqrError) as e:
        pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=10 ** 6, symbolic_only=True)
    assert "limit" in str(e.value)
    L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=32, ordering=3, Quser=np.arange(n)[::-1].copy(), symbolic_only=True)    # (32 are supported)
    try:
        assert np.array_equal(L.symbolic()["Qfill"][:n], np.arange(n)[::-1])
        with pytest.raises(pkg.StmmqrError) as e:                                    # the host half alone does not solve
            L.solve(np.zeros((m, 32)))
        assert e.value.code == -4
    finally:
        L.close()
