"""Extended-precision references of the operations on the resident factors (Q'X, Q X, R \\ Y, R' \\ B, least squares), the
dense fronts on both sides of every threshold of their launchers, and the thresholds themselves restated
(TEST INFRASTRUCTURE, imports no GPU code).

Two references, both in np.longdouble:
* from the factors as they were returned (packed R+H in qr_rhpack order, HStair, HTau, Rdead, Hii, HPinv): the live reflectors and
  R are rebuilt and applied one by one -- what csrc/stmmqr_resident.hip must compute from the same factors, so Q'X and Q X are
  determined to rounding whatever cond(A) is;
* from A itself: a Householder column loop that carries the right-hand sides (householder_solve) -- independent of anything the
  factorization under test returned.

The launchers (stm_launch_qapply_t, stm_launch_rsolve) put 4, 2 or 1 vectors of a batch into a workgroup by the dynamic LDS one
vector needs (stm_lds_qapply, stm_lds_rsolve in csrc/stmmqr_device.h, restated here); a front that needs more than 128 KB takes the
split kernels.  SHAPES holds the smallest dense fronts on each side of each threshold."""
import numpy as np

from stmmqr_testlib import I64, Symbolic

LD = np.longdouble
# x87 extended precision (64-bit mantissa) or better: the reference must be more accurate than what it judges
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended-precision type on this platform"

LDS_MAX = 131072


def lds_qapply(fm, fn):
    return ((fm + 1) & ~1) * 8 + fn * 4 + 16


def lds_rsolve(fp, fn):
    return (((fp + 1) & ~1) + (fn - fp) + 2) * 8 + fp * 4 + 16


def rhs_class(need):
    """vectors of a batch of three or more that share a workgroup; 0: the front takes the split kernels"""
    if 4 * need <= 65536:
        return 4
    if 2 * need <= LDS_MAX:
        return 2
    return 1 if need <= LDS_MAX else 0


# (m, n): (class of the Q-apply, class of the back substitution).  A dense front has every column pivotal (fp = fn = n).
SHAPES = {
    (2026, 40): (4, 4),         # Q-apply: 4 * need is exactly 65536
    (2027, 40): (2, 4),
    (8170, 40): (2, 4),         # 2 * need is exactly 131072
    (8171, 40): (1, 4),
    (16362, 40): (1, 4),        # need is exactly 131072
    (16363, 40): (0, 0),        # one more row: split (a split front is split for both operations)
    (20000, 40): (0, 0),
    (4500, 160): (2, 4),        # five panels
    (48, 1362): (4, 4),         # back substitution: 4 * need = 65504, the last width within 65536
    (48, 1363): (4, 2),
    (48, 5458): (2, 2),         # 2 * need = 131056, the last width within 131072
    (48, 5459): (2, 1),
    (48, 10920): (2, 1),        # need is exactly 131072
    (48, 10921): (0, 0),        # one more column: split
}
TALL = [s for s in SHAPES if s[0] > s[1]]
WIDE = [s for s in SHAPES if s[0] < s[1]]


def rt_fits(m, n):
    """LevelTables::lds_rt of a dense one-front plan (restab::level_tables): the one-workgroup R' solve is refused beyond 128 KB"""
    return (((n + 1) & ~1) + ((min(n, max(m, 1)) + 2) & ~1)) * 8 + n * 4 + 32 <= LDS_MAX


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_front(m, n, kind="full", seed=None):
    """(F, Stair): seeded Gaussian columns of unit expected norm under a staircase; "full": dense, "ramp": column k ends at
    row (k + 1) m / n + 8 (tests/adversarial_fronts.py make_adversarial without the crafted columns)"""
    rng = np.random.default_rng(1000003 * m + n if seed is None else seed)
    if kind == "full":
        St = np.full(n, m, I64)
    else:
        assert kind == "ramp"
        St = np.minimum(m, (np.arange(1, n + 1) * m) // n + 8).astype(I64)
    F = np.zeros((m, n), order="F")
    for k in range(n):
        F[:St[k], k] = rng.standard_normal(St[k]) / np.sqrt(St[k])
    return F, St


def stair_csc(F, St):
    """CSC of a front whose column k holds the rows [0, St[k])"""
    m, n = F.shape
    Ap = np.zeros(n + 1, I64)
    Ap[1:] = np.cumsum(St)
    Ai = np.concatenate([np.arange(t, dtype=I64) for t in St])
    Ax = np.concatenate([F[:t, k] for k, t in enumerate(St)])
    return Ap, Ai, Ax


def symbolic_of(sym):
    """stmmqr_testlib.Symbolic of the dict that analyze() returns"""
    return Symbolic({"sym_" + k: (v if isinstance(v, np.ndarray) else np.array([v])) for k, v in sym.items() if k != "info"})


# ---------------------------------------------------------------------------------------------------------------------
# reference from the returned factors
# ---------------------------------------------------------------------------------------------------------------------
class Factors:
    """The live reflectors and R of a factorization (S: symbolic with nf, n, m, Super, Rp, Rj, Hip; N: Stack, Rblock_off, HStair,
    HTau, Hii, HPinv, Hm, Hr, Rdead, rank as downloaded), rebuilt front by front from the packed blocks -- column k of a front:
    a dead pivot holds the R rows so far; a live pivot the R rows up to its diagonal, then its reflector below the diagonal up to
    HStair[k]; a non-pivotal column the R rows of the front, then its reflector below its own diagonal row."""

    def __init__(self, S, N):
        self.m, self.n, self.nf = int(S.m), int(S.n), int(S.nf)
        self.HPinv = np.asarray(N.HPinv[:self.m], I64)
        self.refl = []                                # per front: [(rows in the permuted order, v, tau)] in column order
        self.rank = int(np.sum(np.asarray(N.Hr[:self.nf])))
        R = np.zeros((self.rank, self.n), LD)
        self.pivot_col = np.full(self.rank, -1, I64)  # the live pivot column (R's column order) of every row of R
        row0 = 0
        for f in range(self.nf):
            pr, fp = int(S.Rp[f]), int(S.Super[f + 1] - S.Super[f])
            fn, fm = int(S.Rp[f + 1]) - pr, int(N.Hm[f])
            St, Tau = N.HStair[pr:pr + fn], N.HTau[pr:pr + fn]
            Hi = np.asarray(N.Hii[int(S.Hip[f]):int(S.Hip[f]) + fm], I64)
            blk = N.Stack[int(N.Rblock_off[f]):]
            out, p, rm, h = [], 0, 0, 0
            for k in range(fn):
                t, col = int(St[k]), int(S.Rj[pr + k])
                if k < fp:
                    if t == 0:                        # dead pivot column
                        R[row0:row0 + rm, col] = blk[p:p + rm]
                        p += rm
                        continue
                    assert rm < fm, "a live pivot column without a row"
                    self.pivot_col[row0 + rm] = col
                    rm += 1
                    h = rm
                else:
                    if h >= fm:                       # the rows ran out: R only
                        R[row0:row0 + rm, col] = blk[p:p + rm]
                        p += rm + max(t - fm, 0)
                        continue
                    h += 1
                R[row0:row0 + rm, col] = blk[p:p + rm]
                ln = max(t - h, 0)
                v = np.ones(1 + ln, LD)
                v[1:] = blk[p + rm:p + rm + ln]
                out.append((Hi[h - 1:h + ln], v, LD(Tau[k])))
                p += rm + ln
            assert rm == int(N.Hr[f]), (f, rm, int(N.Hr[f]))
            self.refl.append(out)
            row0 += rm
        self.R = R
        dead = np.asarray(N.Rdead[:self.n]) != 0
        assert np.array_equal(np.sort(self.pivot_col), np.flatnonzero(~dead)), "live pivot columns and Rdead disagree"
        self.Rlive = R[:, self.pivot_col]             # rank x rank
        assert not np.any(np.tril(self.Rlive, -1)), "R over its live pivot columns is not upper triangular"

    def _apply(self, W, fronts, reverse):
        for f in fronts:
            for rows, v, tau in (reversed(self.refl[f]) if reverse else self.refl[f]):
                if tau != 0:
                    W[rows] -= np.outer(v, tau * (v @ W[rows]))

    def qtx(self, X):
        """Q'X in the permuted row order of the factorization (QR_QTX)"""
        X = np.asarray(X, LD).reshape(self.m, -1)
        W = np.zeros_like(X)
        W[self.HPinv] = X
        self._apply(W, range(self.nf), False)
        return W

    def qx(self, X):
        """Q X for X in the permuted row order (QR_QX)"""
        W = np.array(np.asarray(X, LD).reshape(self.m, -1))
        self._apply(W, range(self.nf - 1, -1, -1), True)
        return W[self.HPinv]

    def rsolve(self, Y):
        """R \\ Y over the live columns, dead columns 0 (R's column order; QR_RX_EQUALS_B)"""
        Y = np.asarray(Y, LD).reshape(self.m, -1)
        r, T = self.rank, self.Rlive
        Z = np.array(Y[:r])
        for i in range(r - 1, -1, -1):
            Z[i] = (Z[i] - T[i, i + 1:] @ Z[i + 1:]) / T[i, i]
        X = np.zeros((self.n, Y.shape[1]), LD)
        X[self.pivot_col] = Z
        return X

    def rtsolve(self, B):
        """R' \\ B: the equations of the live columns, forwards; rows beyond the rank 0 (QR_RTX_EQUALS_B)"""
        B = np.asarray(B, LD).reshape(self.n, -1)
        r, T = self.rank, self.Rlive
        Z = np.array(B[self.pivot_col])
        for i in range(r):
            Z[i] = (Z[i] - T[:i, i] @ Z[:i]) / T[i, i]
        X = np.zeros((self.m, B.shape[1]), LD)
        X[:r] = Z
        return X


# ---------------------------------------------------------------------------------------------------------------------
# reference from A alone
# ---------------------------------------------------------------------------------------------------------------------
def householder_solve(A, B, tol):
    """Householder column loop on A (m x n, dense) in long double with B (m x k) carried: a column whose pivot |beta| <= tol is dead
    and dropped, columns after the last row are dead (the rules of qr_front: tests/adversarial_fronts.py ref_front).  Returns
    (X, rank, dead, absbeta): X (n x k) = the least-squares solution over the live columns with x = 0 on the dead ones (the basic
    solution), absbeta[k] = |beta| of column k at its turn."""
    M = np.array(A, LD, order="F")
    m, n = M.shape
    C = np.array(np.asarray(B, LD).reshape(m, -1))
    dead = np.zeros(n, bool)
    absb = np.zeros(n, LD)
    live = []
    g = 0
    for k in range(n):
        if g >= m:
            dead[k:] = True
            break
        alpha = M[g, k]
        x = M[g + 1:, k]
        ss = x @ x if x.size else LD(0)
        beta = alpha if ss == 0 else -np.copysign(np.sqrt(alpha * alpha + ss), alpha)
        absb[k] = abs(beta)
        if absb[k] <= tol:
            dead[k] = True
            M[g:, k] = 0
            continue
        if ss != 0:
            tau = (beta - alpha) / beta
            v = np.ones(m - g, LD)
            v[1:] = x / (alpha - beta)
            if k + 1 < n:
                M[g:, k + 1:] -= np.outer(v, tau * (v @ M[g:, k + 1:]))
            C[g:] -= np.outer(v, tau * (v @ C[g:]))
            M[g + 1:, k] = 0
        M[g, k] = beta
        live.append(k)
        g += 1
    T = M[:g][:, live]
    Z = np.array(C[:g])
    for i in range(g - 1, -1, -1):
        Z[i] = (Z[i] - T[i, i + 1:] @ Z[i + 1:]) / T[i, i]
    X = np.zeros((n, C.shape[1]), LD)
    X[live] = Z
    return X, g, dead, absb


def rel(got, ref):
    """largest ||got - ref|| / ||ref|| over the columns, evaluated in long double"""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    got, ref = got.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
    d = np.sqrt(((got - ref) ** 2).sum(axis=0))
    return float((d / np.maximum(np.sqrt((ref ** 2).sum(axis=0)), LD(1e-300))).max())
