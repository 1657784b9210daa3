"""The yardstick of tests/test_gpu_minnorm.py, checked without a GPU: on factors the CPU oracle made of the small fixtures, the
long-double reference Factors.qx(Factors.rtsolve(E'b)) is the minimum-2-norm solution of M(:, live)' x = b(live) that
np.linalg.lstsq returns, within solve_tol(cond(M(:, live))); it lies in the span of the first rank columns of Q, and the entries of
b at dead columns do not enter it."""
import numpy as np
import pytest

from minnorm_reference import SMALL, dense_of, live_columns, minnorm_from_factors, minnorm_lstsq, qfill_of
from resident_reference import Factors, rel
from stmmqr_testlib import Symbolic, load_golden, scalar, solve_tol


@pytest.mark.parametrize("name", SMALL)
def test_reference_is_the_minimum_norm_solution(oracle, name):
    g = load_golden(name)
    S = Symbolic(g)
    Ap, Ai, Ax = g["in_Ap"], g["in_Ai"], g["in_Ax"]
    N = oracle.factorize(S, Ap, Ai, Ax, scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    Fa = Factors(S, N)
    M = dense_of(S.m, S.n, Ap, Ai, Ax)
    q = qfill_of(S)
    live = live_columns(Fa, q)
    assert live.size == Fa.rank == int(N.c.rank)
    B = np.random.default_rng(5).standard_normal((S.n, 3))
    X = minnorm_from_factors(Fa, B, q)
    kappa = float(np.linalg.cond(M[:, live])) if live.size else 1.0
    ref = minnorm_lstsq(M, live, B)
    d = rel(X, ref) if live.size else float(np.abs(np.asarray(X, float)).max())
    # the equations themselves, and minimality: x has no component outside range(M(:, live))
    Xd = np.asarray(X, float)
    res = float(np.linalg.norm(M[:, live].T @ Xd - B[live]) / max(np.linalg.norm(M[:, live]) * np.linalg.norm(Xd) + np.linalg.norm(B[live]), 1e-300))
    print(f"\n[minnorm cpu] {name}: rank {Fa.rank} of {S.n}, cond {kappa:.2e}, vs lstsq {d:.2e} (allowed {solve_tol(kappa):.1e}), residual {res:.2e}")
    assert d <= solve_tol(kappa)
    assert res <= 1e-12
    # in the span of Q(:, :rank), as far as a Q made of fp64 reflectors is orthogonal: the project's bound for Q-applied quantities
    tail = np.asarray(Fa.qtx(X)[Fa.rank:], float)
    assert np.linalg.norm(tail) <= 1e-12 * max(np.linalg.norm(Xd), 1e-300)
    # dead columns have no equation
    dead = np.setdiff1d(np.arange(S.n), live)
    if dead.size:
        B2 = B.copy()
        B2[dead] += 10.0
        assert np.array_equal(np.asarray(minnorm_from_factors(Fa, B2, q)), np.asarray(X))
    # the permuted form takes b in R's column order
    assert np.array_equal(np.asarray(minnorm_from_factors(Fa, B[q], None)), np.asarray(X))
