"""References of the null-space basis of R and of the minimum-norm projector (TEST INFRASTRUCTURE, imports no GPU code).

From Factors.R (tests/resident_reference.py: rank x n in np.longdouble, with pivot_col): with pc the live and jd the dead pivot columns
among the first ncol, R11 = R(:, pc), R12 = R(:, jd),
    W = R11^-1 R12 by back substitution,   N_ref = [-W on pc; I on jd]   (ncol x d, R's column order),
and the projection of x onto the complement of range(N): x - N y with y the least-squares solution of N y = x by householder_solve
(a Householder column loop on N itself -- no Gram matrix, no Cholesky factor: independent of the route under test).

Both are long double.  Where that would take ten seconds and more (r^2 d or ncol d^2 beyond BUDGET multiply-adds: lns_3937 alone
among the fixtures, d = 2086) the same two steps run in float64 (scipy's solve_triangular, numpy's lstsq); the float64 route's own
error there, eps cond(R11), lies far inside the tolerances of that fixture, which are made of cond(R11).  The one check that is NOT
made of cond(R11), |N_ref' x|, never needs N_ref itself: N_ref' x = x(jd) - R12' (R11' \\ x(pc)) is one forward substitution per
vector (nref_t_apply), long double on every fixture.  tests/test_nullspace_cpu.py holds the long double route against
numpy.linalg.lstsq on A itself."""
import numpy as np
import scipy.linalg as sla

from resident_reference import LD, householder_solve
from stmmqr_testlib import EPS, I64

BUDGET = 2.5e9                 # long double multiply-adds a reference may cost (about 4 ns each)


def split(Fa, ncol=None):
    """(pc, jd): the live pivot columns among the first ncol in the order of the rows of R, and the dead ones ascending"""
    ncol = Fa.n if ncol is None else int(ncol)
    pc = np.asarray(Fa.pivot_col[Fa.pivot_col < ncol], I64)
    assert np.all(np.diff(pc) > 0), "the rows of R are not in the order of their pivot columns"
    jd = np.setdiff1d(np.arange(ncol, dtype=I64), pc)
    return pc, jd


def blocks(Fa, ncol=None, cols=None):
    """(R11, R12 restricted to the dead columns jd[cols], pc, jd) in long double"""
    pc, jd = split(Fa, ncol)
    r = pc.size
    R11 = Fa.Rlive if r == Fa.rank else Fa.R[:r][:, pc]
    sel = jd if cols is None else jd[np.asarray(cols, I64)]
    return R11, Fa.R[:r][:, sel], pc, jd


def back_substitute(T, B):
    """T \\ B for upper triangular T, row by row in the precision of the operands"""
    Z = np.array(B)
    for i in range(T.shape[0] - 1, -1, -1):
        Z[i] = (Z[i] - T[i, i + 1:] @ Z[i + 1:]) / T[i, i]
    return Z


def is_heavy(r, d, ncol):
    return 0.5 * r * r * d > BUDGET or float(ncol) * d * d > BUDGET


def emulate_w(R11, R12):
    """W by the float64 emulation of the device's two steps: the column of R as it is, then one triangular solve"""
    if R12.shape[1] == 0 or R11.shape[0] == 0:
        return np.zeros(R12.shape)
    return sla.solve_triangular(np.asarray(R11, float), np.asarray(R12, float), lower=False)


def nullspace_ref(Fa, ncol=None, cols=None):
    """N_ref (ncol x d, or the columns `cols` of it) in R's column order; long double unless is_heavy"""
    ncol = Fa.n if ncol is None else int(ncol)
    R11, R12, pc, jd = blocks(Fa, ncol, cols)
    k = R12.shape[1]
    W = np.asarray(emulate_w(R11, R12), LD) if is_heavy(pc.size, k, ncol) else back_substitute(R11, R12)
    N = np.zeros((ncol, k), LD)
    N[pc] = -W
    sel = jd if cols is None else jd[np.asarray(cols, I64)]
    N[sel, np.arange(k)] = 1
    return N


_SPLIT = LD(2) ** 32 + 1          # Dekker's splitter for a 64-bit significand


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """p = fl(a b) and e with p + e = a b exactly (Dekker / Veltkamp in long double: no fma needed)"""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dot2_rows(M, Y):
    """sum_j M[j, :, None] * Y[j, None, :] (M: r x c, Y: r x k -> c x k) as an unevaluated pair (s, c): every product and every
    addition with its rounding error carried (Ogita / Rump / Oishi's Dot2, row after row): twice the working precision"""
    s = np.zeros((M.shape[1], Y.shape[1]), LD)
    c = np.zeros_like(s)
    for j in range(M.shape[0]):
        p, e = _two_prod(M[j][:, None], Y[j][None, :])
        s, e2 = _two_sum(s, p)
        c += e + e2
    return s, c


def nref_t_apply(R11, R12, pc, jd, X):
    """N_ref' X = X(jd) - R12' y, y = R11' \\ X(pc), for X (ncol x k) in R's column order, never N_ref itself.  The terms of R12' y are
    up to cond(R11) times the result, so long double alone would leave eps_LD cond(R11) there (2e-11 on lns_3937, above what the
    orthogonality bound allows): y is a pair y0 + dy -- the forward substitution row by row in long double, then one step of
    refinement on a residual whose products and sums carry their rounding errors (Dot2) -- and so is the product with R12."""
    X = np.asarray(X, LD).reshape(-1, 1) if np.ndim(X) == 1 else np.asarray(X, LD)
    T, B = np.asarray(R11, LD), X[pc]

    def forward(C):
        Y = np.array(C)
        for i in range(T.shape[0]):
            Y[i] = (Y[i] - T[:i, i] @ Y[:i]) / T[i, i]
        return Y
    y0 = forward(B)
    s, c = _dot2_rows(T, y0)                                 # (T' y0)_i = sum_j T[j, i] y0[j]: the zeros below the diagonal add nothing
    dy = forward((B - s) - c)
    R12 = np.asarray(R12, LD)
    s, c = _dot2_rows(R12, y0)
    return ((X[jd] - s) - c) - R12.T @ dy


def project_ref(N, X):
    """x - N y, y = argmin |N y - x|: Householder in long double (float64 lstsq where is_heavy)"""
    X = np.asarray(X, LD).reshape(N.shape[0], -1)
    if N.shape[1] == 0:
        return np.array(X)
    if is_heavy(0, N.shape[1], N.shape[0]):
        Y = np.linalg.lstsq(np.asarray(N, float), np.asarray(X, float), rcond=None)[0]
    else:
        Y, rank, _, _ = householder_solve(N, X, 0.0)
        assert rank == N.shape[1]
    return X - N @ np.asarray(Y, LD)


def rn_residual(R11, R12, Wneg_live):
    """per column |R N(:, k)|_2 = |R12(:, k) + R11 N(pc, k)|_2 in long double"""
    D = R12 + R11 @ np.asarray(Wneg_live, LD)
    return np.sqrt((D * D).sum(axis=0))


def rn_bound(R11, R12, N_live_norms):
    """what |R N(:, k)| may be, per column: 4 x the larger of what the float64 emulation of the two steps leaves and
    (r + 2) eps |R_live|_F |N(:, k)|_2 (the factor 4: another summation order in the blocked solves)"""
    r = R11.shape[0]
    emu = rn_residual(R11, R12, -emulate_w(R11, R12))
    fro = float(np.sqrt((np.asarray(R11, float) ** 2).sum()))
    return 4.0 * np.maximum(np.asarray(emu, float), (r + 2) * EPS * fro * np.asarray(N_live_norms, float)), np.asarray(emu, float)


def colnorm(M):
    M = np.asarray(M, LD)
    return np.sqrt((M * M).sum(axis=0))


def cond2(T):
    """cond_2 of a triangular matrix by its singular values; beyond 2000 rows, where those take minutes, the lower bound of 8 steps of
    the power iteration on T'T and on its inverse (tests/condest_reference.py power2: 0.9 .. 1 of the exact value -- a smaller
    condition makes every tolerance built on it tighter, never wider)"""
    T = np.asarray(T, float)
    if T.shape[0] == 0:
        return 1.0
    if T.shape[0] > 2000:
        import condest_reference as cr
        p = cr.power2(T, 8)
        return float(p["norm"] * p["inv"])
    s = np.linalg.svd(T, compute_uv=False)
    return float(s[0] / s[-1])


def norm2(M):
    M = np.asarray(M, float)
    return float(np.linalg.norm(M, 2)) if M.size else 0.0
