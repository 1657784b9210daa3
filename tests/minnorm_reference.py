"""References of the minimum-norm solve on the resident factors, x = Q (R' \\ (E'b)) (TEST INFRASTRUCTURE, imports no GPU code).

With a factorization M E = Q R whose dead pivot columns are squeezed out of R, x is the minimum-2-norm solution of the equations
M(:, live)' x = b(live), live = the columns of M whose pivots did not die.  Two references:
* from the factors, in np.longdouble: Factors.qx(Factors.rtsolve(E'b)) of tests/resident_reference.py -- what the device must
  compute from the same factors, to rounding;
* from M alone, in float64: np.linalg.lstsq(M[:, live].T, b[live]), which returns the minimum-norm solution.
tests/test_minnorm_cpu.py holds the first against the second on factors the CPU oracle made."""
import numpy as np

from resident_reference import LD, Factors
from stmmqr_testlib import I64

SMALL = ["syn_chain", "syn_star", "syn_grid2d", "syn_grid3d", "syn_rand60x40", "syn_wide5x8", "syn_dupcol", "syn_emptycol",
         "syn_rankdef_grid", "dwt_992"]


def dense_of(m, n, Ap, Ai, Ax):
    M = np.zeros((m, n))
    for j in range(n):
        p, q = int(Ap[j]), int(Ap[j + 1])
        np.add.at(M[:, j], Ai[p:q], Ax[p:q])
    return M


def qfill_of(S):
    return np.arange(S.n, dtype=I64) if S.Qfill is None else np.asarray(S.Qfill[:S.n], I64)


def live_columns(Fa: Factors, qfill):
    """the columns of M (caller's numbering) whose pivots are live, in the order of the rows of R"""
    return np.asarray(qfill, I64)[Fa.pivot_col]


def minnorm_from_factors(Fa: Factors, B, qfill=None):
    """Q (R' \\ (E'B)) in long double, rows in the caller's order of M; qfill None: B is already in R's column order"""
    B = np.asarray(B, LD).reshape(Fa.n, -1)
    return Fa.qx(Fa.rtsolve(B if qfill is None else B[np.asarray(qfill, I64)]))


def minnorm_lstsq(M, live, B):
    """the minimum-norm solution of M(:, live)' x = B(live), float64"""
    B = np.asarray(B, float).reshape(M.shape[1], -1)
    return np.linalg.lstsq(M[:, live].T, B[live], rcond=None)[0]
