"""Extended-precision reference of the selected inversion of R'R (csrc/stmmqr_selinv.hip), front by front from the packed blocks
(TEST INFRASTRUCTURE, imports no GPU code).

Per front, parents before children, with the live-pivot rule of the resident-factor kernels (HStair != 0 and a row left):
    R11 = R[0:rm, live pivots]      R12 = R[0:rm, non-pivotal columns]
    Z_NN  gathered from the parent's block through a position table (live pivot: compact index, non-pivotal: rm + cj, dead: -1 --
          a -1 zeroes the row and the column)
    [G | S] = R11^-1 [I | R12]      Z_PN = -S Z_NN      Z_PP = G G' - Z_PN S'
    var[column of live pivot i] = Z_PP[i, i], dead columns 0.
The child -> parent column map is rebuilt here from Rj (the global column of every local one), not taken from the library.
ncol < n: the plan holds [A B]; pivots and non-pivotal columns with Rj >= ncol take no part."""
import numpy as np

from resident_reference import LD
from stmmqr_testlib import I64, front_R


def backsub(T, B):
    """T^-1 B for an upper triangular T, in long double"""
    X = np.array(B, LD)
    for i in range(T.shape[0] - 1, -1, -1):
        X[i] = (X[i] - T[i, i + 1:] @ X[i + 1:]) / T[i, i]
    return X


def selinv_diag(S, N, ncol=None, keep_blocks=False):
    """diag((R_live' R_live)^-1) in R's column order (length ncol), by the front-wise recurrence"""
    n, nf = int(S.n), int(S.nf)
    ncol = n if ncol is None else int(ncol)
    blocks = N.rh_blocks(S)
    var = np.zeros(ncol, LD)
    held = {}                                             # front -> (Z block, {global column: position or -1})
    for f in reversed([int(f) for f in S.Post[:nf]]):
        fp = int(S.Super[f + 1] - S.Super[f])
        p1, fn, fm = int(S.Rp[f]), int(S.Rp[f + 1] - S.Rp[f]), int(N.Hm[f])
        stair = N.HStair[p1:p1 + fn]
        cols = [int(c) for c in S.Rj[p1:p1 + fn]]
        R = np.asarray(front_R(blocks[f], stair, fp, fn, fm), LD) if fm > 0 and fn > 0 else np.zeros((0, fn), LD)
        live, q = [], 0
        pos = {}
        for k in range(fp):
            if cols[k] >= ncol:
                break                                     # (the B pivots follow the A pivots)
            if stair[k] != 0 and q < fm:
                pos[cols[k]] = q
                live.append(k)
            else:
                pos[cols[k]] = -1
            q += int(stair[k] != 0)
        rm = len(live)
        others = [k for k in range(fp, fn) if cols[k] < ncol]
        assert others == list(range(fp, fp + len(others))), "the columns that are cut are not the last of the front's list"
        cn = len(others)
        for cj, k in enumerate(others):
            pos[cols[k]] = rm + cj
        Z = np.zeros((rm + cn, rm + cn), LD)
        par = int(S.Parent[f]) if f < len(S.Parent) else -1
        if cn:
            if 0 <= par < nf and par in held:
                Zp, ppos = held[par]
                pp = np.array([ppos.get(cols[k], -1) for k in others], I64)
                ok = pp >= 0
                Z[np.ix_(rm + np.flatnonzero(ok), rm + np.flatnonzero(ok))] = Zp[np.ix_(pp[ok], pp[ok])]
        if rm:
            R11 = R[:rm][:, live]
            assert not np.any(np.tril(R11, -1))
            GS = backsub(R11, np.concatenate([np.eye(rm, dtype=LD), R[:rm][:, others]], axis=1))
            G, Sm = GS[:, :rm], GS[:, rm:]
            Zpn = -Sm @ Z[rm:, rm:]
            Z[:rm, rm:] = Zpn
            Z[rm:, :rm] = Zpn.T
            Z[:rm, :rm] = G @ G.T - Zpn @ Sm.T
            for i, k in enumerate(live):
                var[cols[k]] = Z[i, i]
        held[f] = (Z, pos)
    return (var, held) if keep_blocks else var


def to_caller_order(S, var):
    """var in R's column order -> the caller's: out[Qfill[j]] = var[j]"""
    q = S.Qfill if S.Qfill is not None else np.arange(S.n)
    out = np.zeros(len(var), var.dtype)
    out[np.asarray(q[:len(var)], I64)] = var
    return out


class SparseR:
    """Factors.rtsolve without the dense rank x n array (epb1: 3.4 GB in long double): the same R, rebuilt from the same packed
    blocks with the same row numbering (front after front), kept by columns; the same forward substitution over the live pivot
    columns in long double."""

    def __init__(self, S, N):
        self.n, nf = int(S.n), int(S.nf)
        blocks = N.rh_blocks(S)
        rows, vals = {}, {}
        self.pivot_col = []
        row0 = 0
        for f in range(nf):
            fp = int(S.Super[f + 1] - S.Super[f])
            p1, fn, fm = int(S.Rp[f]), int(S.Rp[f + 1] - S.Rp[f]), int(N.Hm[f])
            if fm <= 0 or fn <= 0:
                continue
            stair = N.HStair[p1:p1 + fn]
            R = front_R(blocks[f], stair, fp, fn, fm)
            rm, q = R.shape[0], 0
            for k in range(fn):
                col = int(S.Rj[p1 + k])
                if k < fp and stair[k] != 0 and q < fm:
                    self.pivot_col.append(col)
                    q += 1
                if rm:
                    rows.setdefault(col, []).append(row0 + np.arange(rm))
                    vals.setdefault(col, []).append(np.asarray(R[:, k], LD))
            assert q == rm == int(N.Hr[f])
            row0 += rm
        self.rank = row0
        self.col = {c: (np.concatenate(rows[c]), np.concatenate(vals[c])) for c in self.pivot_col}

    def rtsolve(self, B):
        """the first `rank` rows of R' \\ B (B: n x k in R's column order)"""
        B = np.asarray(B, LD).reshape(self.n, -1)
        Z = np.zeros((self.rank, B.shape[1]), LD)
        for i, c in enumerate(self.pivot_col):
            r, v = self.col[c]
            up = r < i
            d = v[r == i]
            assert d.size == 1
            Z[i] = (B[c] - v[up] @ Z[r[up]]) / d[0]
        return Z
