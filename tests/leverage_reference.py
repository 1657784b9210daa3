"""Extended-precision reference of the leverages and of single entries of (A_live' A_live)^-1 (csrc/stmmqr_leverage.hip), from the
blocks that selinv_reference.selinv_diag keeps (TEST INFRASTRUCTURE, imports no GPU code).

A row of A makes its columns a clique of A'A, so for two columns of one row the later one (R's order) is a column of the front
where the earlier one is pivotal, and
    h_i = sum_{a, b in row i} a_ia a_ib Z(col_a, col_b)
reads the held blocks only.  Every lookup asserts that the pair is found.  Independent of the factors: dense_leverages, the row sums
of Q1^2 of np.linalg.qr of the live columns."""
import numpy as np

from resident_reference import LD
from selinv_reference import selinv_diag
from stmmqr_testlib import EPS, I64, TOL_C, solve_tol


class Blocks:
    """The selected inverse as selinv_diag(..., keep_blocks=True) holds it: entry(k1, k2) for two columns in R's order"""

    def __init__(self, S, N, ncol=None):
        self.ncol = int(S.n) if ncol is None else int(ncol)
        self.var, self.held = selinv_diag(S, N, ncol=self.ncol, keep_blocks=True)
        self.Super = np.asarray(S.Super[:int(S.nf) + 1], I64)
        self._lut = {}

    def front_of(self, k):
        return int(np.searchsorted(self.Super, k, side="right")) - 1

    def lut(self, f):
        """position in front f's block by global column: >= 0, -1 dead, -2 not a column of the front"""
        if f not in self._lut:
            t = np.full(self.ncol, -2, I64)
            for c, p in self.held[f][1].items():
                if c < self.ncol:
                    t[c] = p
            self._lut[f] = t
        return self._lut[f]

    def entry(self, k1, k2):
        k1, k2 = (k1, k2) if k1 <= k2 else (k2, k1)
        f = self.front_of(k1)
        t = self.lut(f)
        assert t[k1] != -2 and t[k2] != -2, f"pair ({k1}, {k2}) is not in the block of front {f}"
        if t[k1] < 0 or t[k2] < 0:
            return LD(0)
        return self.held[f][0][t[k1], t[k2]]

    def row(self, cols, vals):
        """a' Z a for a row given by its columns (R's order, any order, duplicates allowed) and values"""
        o = np.argsort(cols, kind="stable")
        c, v = np.asarray(cols, I64)[o], np.asarray(vals, LD)[o]
        h = LD(0)
        for a in range(c.size):
            f = self.front_of(c[a])
            t = self.lut(f)
            pb = t[c[a:]]
            assert t[c[a]] != -2 and not np.any(pb == -2), f"a pair of the row is not in the block of front {f}"
            if t[c[a]] < 0:
                continue
            w = 2 * v[a:]
            w[0] = v[a]
            ok = pb >= 0
            h += v[a] * np.sum(w[ok] * self.held[f][0][t[c[a]], pb[ok]])
        return h


def rows_in_r_order(S, m, Ap, Ai, Ax, ncol=None):
    """per row of the caller's matrix: (columns in R's order, values), the caller's columns >= ncol left out"""
    n = len(Ap) - 1
    ncol = n if ncol is None else int(ncol)
    q = np.asarray(S.Qfill if S.Qfill is not None else np.arange(n), I64)
    qinv = np.empty(n, I64)
    qinv[q] = np.arange(n)
    col = np.repeat(np.arange(n, dtype=I64), np.diff(Ap))
    keep = col < ncol
    r, c, v = np.asarray(Ai, I64)[keep], qinv[col[keep]], np.asarray(Ax)[keep]
    assert np.all(c < ncol)
    o = np.argsort(r, kind="stable")
    r, c, v = r[o], c[o], v[o]
    cut = np.searchsorted(r, np.arange(m + 1))
    return [(c[cut[i]:cut[i + 1]], v[cut[i]:cut[i + 1]]) for i in range(m)]


def leverages(S, N, m, Ap, Ai, Ax, ncol=None, rows=None):
    """(lev [m] or [len(rows)] in long double, Blocks): the pair sums over the held blocks"""
    Z = Blocks(S, N, ncol)
    R = rows_in_r_order(S, m, Ap, Ai, Ax, ncol)
    pick = range(m) if rows is None else rows
    return np.array([Z.row(*R[i]) for i in pick], LD), Z


def dense_leverages(A, live):
    """row sums of Q1^2, Q1 from np.linalg.qr of the live columns of a dense A: independent of the factors"""
    if not np.any(live):
        return np.zeros(A.shape[0])
    Q1 = np.linalg.qr(np.asarray(A)[:, live], mode="reduced")[0]
    return (Q1 ** 2).sum(axis=1)


def allowed(ref, a1, max_var, kappa):
    """The bound on |h_i - ref_i| (derived, not measured): 3 solve_tol(kappa) ref_i, two correct evaluations of |R^-T a_i|^2, plus
    TOL_C eps kappa^2 |a_i|_1^2 max_j var_j: an entry of Z carries about u cond^2 times the largest entry, Z is positive
    definite, so that is its largest diagonal, and a row sees at most |a_i|_1^2 of it."""
    return 3 * solve_tol(kappa) * np.asarray(ref, float) + TOL_C * EPS * kappa * kappa * np.asarray(a1, float) ** 2 * float(max_var)
