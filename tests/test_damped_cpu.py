"""Damped, weighted least squares (DampedLeastSquares, stmmqr_ls_create_damped / stmmqr_ls_solve_damped), host half (no GPU):
the symbolic analysis of [A; I | B; 0], the refusals that need no device, and the yardstick of tests/test_gpu_damped.py -- the explicit
matrix [W A; D | W B; 0] factorized by the CPU oracle on the damped object's own analysis and solved with carried_solve_host --
validated against numpy.linalg.lstsq of the dense augmented matrix."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

from stmmqr_testlib import EPS, load_golden, solve_tol
from test_carried_cpu import augmented, carried_solve_host, problem, symbolic_of

PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
SMALL = ["syn_rand60x40", "syn_wide5x8", "syn_dupcol", "syn_rankdef_grid", "syn_emptycol", "syn_star", "syn_grid3d"]
REAL = ["bcsstk14", "epb1"]
RANKDEF = ["syn_wide5x8", "syn_dupcol", "syn_rankdef_grid", "syn_emptycol"]          # rank-deficient undamped, rank n damped


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def matrix_of(name):
    """(m, n, Ap, Ai, Ax) of a fixture.  The synthetic ones as the caller's full matrix A_* (as tests/test_gpu_carried.py takes
    syn_star): what they are here for -- the empty column of syn_emptycol, the column singleton of syn_star, m < n of syn_wide5x8 --
    is gone from the matrix the golden factorization was made of, which has the singletons removed.  The real ones: problem(g)."""
    g = load_golden(name)
    if name in SMALL:
        return int(g["A_m"][0]), int(g["A_n"][0]), g["A_p"].astype(np.int64), g["A_i"].astype(np.int64), g["A_x"].astype(np.float64)
    return problem(g)[:5]


def weights(m, seed=21):
    return np.random.default_rng(seed).uniform(0.5, 2.0, m)


def scales(n, seed=22):
    return np.random.default_rng(seed).uniform(0.5, 2.0, n)


def explicit(m, n, Ap, Ai, Ax, w, D):
    """[W A; D] in compressed columns, the layout of the damped object: column j = A's entries in their given order (each ONE product
    w[i] * a), then the entry of row m + j.  w None: all 1."""
    Ap = np.asarray(Ap, np.int64)
    cols = np.repeat(np.arange(n), np.diff(Ap))
    Cp = Ap + np.arange(n + 1)
    Ci = np.zeros(int(Ap[-1]) + n, np.int64)
    Cx = np.zeros(int(Ap[-1]) + n)
    pos = np.arange(int(Ap[-1])) + cols
    Ci[pos] = Ai
    Cx[pos] = Ax if w is None else np.asarray(w)[Ai] * Ax
    Ci[Ap[1:] + np.arange(n)] = m + np.arange(n)
    Cx[Ap[1:] + np.arange(n)] = D
    return Cp, Ci, Cx


def explicit_rhs(B, w, n):
    """[W B; 0], (m + n) x nrhs"""
    B = np.asarray(B, float).reshape(B.shape[0], -1)
    top = B if w is None else np.asarray(w)[:, None] * B
    return np.asfortranarray(np.vstack([top, np.zeros((n, B.shape[1]))]))


def dense_of(mm, n, Cp, Ci, Cx):
    return sp.csc_matrix((Cx, Ci, Cp), shape=(mm, n)).toarray()


def default_tol(mm, n, Cp, Cx):
    """the project's rule, 20 (rows + columns) eps max_j |C(:,j)|_2 (numpy's norms: not the library's bits, which no CPU test needs)"""
    norms = [np.linalg.norm(Cx[Cp[j]:Cp[j + 1]]) for j in range(n)]
    return 20.0 * (mm + n) * EPS * max(norms, default=0.0)


def damping_cases(m, n):
    """(label, w, D): Levenberg with weights, and given column scales without; every D_jj >= 0.05, far above any tolerance here"""
    return [("w, lam 1e-2", weights(m), np.full(n, np.sqrt(1e-2))), ("d, lam 0.3", None, np.sqrt(0.3) * scales(n))]


@pytest.mark.parametrize("nrhs", [1, 4])
@pytest.mark.parametrize("name", SMALL + REAL)
def test_symbolic_of_the_damped_problem(pkg, name, nrhs):
    m, n, Ap, Ai, Ax = matrix_of(name)
    perm = np.random.default_rng(5).permutation(n).astype(np.int64)
    for kw in ({}, dict(ordering=3, Quser=perm)):
        L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs, symbolic_only=True, **kw)
        P = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs, symbolic_only=True, **kw)
        try:
            sym, info = L.symbolic(), L.info
            assert sym["m"] == m + n and sym["n"] == n + nrhs
            assert sym["anz"] == int(Ap[-1]) + n + (m + n) * nrhs
            Q = sym["Qfill"]
            assert np.array_equal(Q[:n], P.symbolic()["Qfill"][:n]), "the columns of A alone are ordered as the plain object orders them"
            if kw:
                assert np.array_equal(Q[:n], perm)
            assert np.array_equal(Q[n:], np.arange(n, n + nrhs))
            assert info["analyses"] == 1 and info["plans"] == 0 and info["nf"] == sym["nf"]
            assert L.dims == {"m": m, "n": n, "nrhs": nrhs, "damped": True}
            assert P.dims == {"m": m, "n": n, "nrhs": nrhs, "damped": False}
        finally:
            L.close(); P.close()


@pytest.mark.parametrize("nrhs", [1, 4])
@pytest.mark.parametrize("name", SMALL)
def test_yardstick_against_the_dense_solution(pkg, oracle, name, nrhs):
    """The explicit [W A; D | W B; 0] on the damped object's analysis, CPU oracle + carried_solve_host, against numpy.linalg.lstsq of
    the dense augmented matrix: |x - x_ref| <= solve_tol(cond_2 of the dense matrix) |x_ref|, the residual of the augmented problem
    to the same bar, and rank n (every D_jj is above the tolerance) also where A alone is rank-deficient."""
    m, n, Ap, Ai, Ax = matrix_of(name)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs, symbolic_only=True)
    try:
        S = symbolic_of(L.symbolic())
    finally:
        L.close()
    B = np.asfortranarray(np.random.default_rng(11).standard_normal((m, nrhs)))
    for label, w, D in damping_cases(m, n):
        Cp, Ci, Cx = explicit(m, n, Ap, Ai, Ax, w, D)
        Be = explicit_rhs(B, w, n)
        tol = default_tol(m + n, n, Cp, Cx)
        assert D.min() > tol
        Fp, Fi, Fx = augmented(m + n, n, Cp, Ci, Cx, Be)
        N = oracle.factorize(S, Fp, Fi, Fx, tol, n)
        X, resid = carried_solve_host(S, N, n, nrhs)
        Cd = dense_of(m + n, n, Cp, Ci, Cx)
        Xr = np.linalg.lstsq(Cd, Be, rcond=None)[0]
        kappa = float(np.linalg.cond(Cd))
        bar = solve_tol(kappa)
        dx = np.linalg.norm(X - Xr, axis=0) / np.maximum(np.linalg.norm(Xr, axis=0), 1e-300)
        rr = np.linalg.norm(Be - Cd @ Xr, axis=0)
        print(f"[damped cpu] {name} nrhs {nrhs} {label}: cond {kappa:.2e} |x - lstsq| / |lstsq| {dx.max():.2e} (allowed {bar:.1e}) rank1 "
              f"{int(N.c.rank1)}/{n} resid rel diff {np.max(np.abs(resid - rr) / np.maximum(np.linalg.norm(Be, axis=0), 1e-300)):.2e}")
        assert int(N.c.rank1) == n, "every D_jj is above the tolerance: full column rank" + (" (A alone is not)" if name in RANKDEF else "")
        assert np.all(dx <= bar)
        assert np.all(np.abs(resid - rr) <= bar * np.linalg.norm(Be, axis=0))


def raw_solve_damped(pkg, L, dmp, m, n, nrhs):
    """stmmqr_ls_solve_damped with host arrays and the damping struct given as it is (None: a NULL pointer)"""
    capi = importlib.import_module(PKG + ".capi")
    B, X = np.zeros((max(m, 1), nrhs), order="F"), np.zeros((max(n, 1), nrhs), order="F")
    capi._check(pkg.lib.stmmqr_ls_solve_damped(L._h, None, 0, None if dmp is None else C.byref(dmp), B.ctypes.data, max(m, 1), X.ctypes.data,
                                               max(n, 1), None, 0), "stmmqr_ls_solve_damped")


def argument_refusals(pkg, L, P, m, n, nrhs, after=lambda: None):
    """every refusal of the two solve entry points that is decided before the device is looked at (shared with the GPU tests, where
    the objects are live and after() solves on them): each raises with the code -4 and names its cause"""
    capi = importlib.import_module(PKG + ".capi")
    B = np.zeros((m, nrhs))
    seen = []

    def refused(call, word):
        with pytest.raises(pkg.StmmqrError) as e:
            call()
        assert e.value.code == -4 and word in str(e.value), str(e.value)
        seen.append(word)
        after()

    refused(lambda: raw_solve_damped(pkg, P, capi.LsDamping(None, None, 1.0, 0, 1e-6, 1e32, None, None), m, n, nrhs), "plain object")
    refused(lambda: pkg.LeastSquares.solve(L, B), "damped object")
    refused(lambda: raw_solve_damped(pkg, L, None, m, n, nrhs), "null damping")
    for lam in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
        refused(lambda: L.solve(B, lam=lam), "lambda")
    for scale in (-1, 2, 7):
        refused(lambda: L.solve(B, lam=1.0, scale=scale), "scale must be 0 or 1")
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (1.0, np.nan)):
        refused(lambda: L.solve(B, lam=1.0, scale=1, scale_min=lo, scale_max=hi), "scale_min")
    return seen


def test_argument_refusals_on_the_host_half(pkg):
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=2, symbolic_only=True)
    P = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=2, symbolic_only=True)
    try:
        assert len(argument_refusals(pkg, L, P, m, n, 2)) == 16
        # both solve entry points with good arguments: the host half alone does not solve, and says so
        with pytest.raises(pkg.StmmqrError) as e:
            L.solve(np.zeros((m, 2)), lam=1.0, w=np.ones(m))
        assert e.value.code == -4 and "host half" in str(e.value)
        with pytest.raises(pkg.StmmqrError) as e:
            P.solve(np.zeros((m, 2)))
        assert e.value.code == -4 and "host half" in str(e.value)
        with pytest.raises(pkg.StmmqrError) as e:                                    # the diagnostics refuse as on the plain object
            L.leverages()
        assert e.value.code == -4
        assert L.info["solves"] == 0 and L.dims["damped"]
    finally:
        L.close(); P.close()


def test_create_refusals_are_the_plain_object_s(pkg):
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    for kw in (dict(nrhs=0), dict(nrhs=-3), dict(ordering=5), dict(ordering=10), dict(ordering=3, Quser=np.zeros(n, np.int64)),
               dict(ordering=3, Quser=np.arange(1, n + 1)), dict(nrhs=10 ** 6)):
        with pytest.raises(pkg.StmmqrError) as e:
            pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, symbolic_only=True, **kw)
        assert e.value.code == -4, kw
    with pytest.raises(pkg.StmmqrError) as e:
        pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=10 ** 6, symbolic_only=True)
    assert "limit" in str(e.value)
