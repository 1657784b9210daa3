"""The yardstick of the condition estimate on the resident factors, stmmqr_plan_condest (TEST INFRASTRUCTURE, pure numpy / scipy,
imports no GPU code).  On a dense upper triangular T = R over its live pivot columns (Factors.Rlive of tests/resident_reference.py):

* the exact values: |T|_1, |T^-1|_1 = np.abs(inv).sum(0).max(), the singular values;
* the same two algorithms the device runs, in float64 with LAPACK's triangular solves:
  hager(T): Hager's one-norm estimate of |T^-1|_1 in Higham's form (the convention of dtrcon / dlacn2) -- from x = 1/r at most five
  rounds of y = T \\ x, xi = sign(y) (y >= 0, and -0.0, giving +1), z = T' \\ xi, x = e_j at the FIRST largest |z_j|; a round stops
  the iteration when its |y|_1 does not exceed the estimate so far, when |z|_inf <= z'x, or when the arg-max repeats; then the
  safeguard vector x_i = (-1)^i (1 + i / (r - 1)) with estimate 2 |T \\ x|_1 / (3 r); the larger of the two.  v = y / |y|_1 of the
  x that attained it.
  power2(T, iters): `iters` steps of x <- T'(T x) / |T'(T x)|_2 with |T|_2 ~ sqrt |T'(T x)|_2, and of x <- T \\ (T' \\ x) / |.|_2
  with |T^-1|_2 ~ 1 / |T v|_2 of the last iterate v; both from the safeguard vector, normalised.
Every estimate is |M x| / |x| of some x: a lower bound."""
import numpy as np
import scipy.linalg as sla

MAX_ROUNDS = 5
# the fixtures of tests/test_condest_cpu.py: those of the GPU tests and the smallest dense one.  (reorientation_8, r = 3079, and
# grid20_standin, r = 8000, were measured with the same functions -- DESIGN.md 6k -- but their dense SVDs take a minute and a half.)
NAMES = ["syn_chain", "syn_star", "syn_grid2d", "syn_grid3d", "syn_rand60x40", "syn_wide5x8", "syn_dupcol", "syn_emptycol",
         "syn_rankdef_grid", "syn_dense6x4", "dwt_992", "bcsstk14", "lns_3937"]


def safeguard(r):
    if r <= 1:
        return np.ones(r)
    i = np.arange(r)
    return np.where(i & 1, -1.0, 1.0) * (1.0 + i / float(r - 1))


def norm1(T):
    return float(np.abs(T).sum(axis=0).max()) if T.size else 0.0


def exact(T):
    """{"norm1", "inv1", "cond1", "norm2", "inv2", "cond2"} of a nonsingular upper triangular T (r >= 1)"""
    T = np.asarray(T, float)
    inv = sla.solve_triangular(T, np.eye(T.shape[0]))
    sv = np.linalg.svd(T, compute_uv=False)
    e = {"norm1": norm1(T), "inv1": float(np.abs(inv).sum(axis=0).max()), "norm2": float(sv[0]), "inv2": float(1.0 / sv[-1])}
    e["cond1"], e["cond2"] = e["norm1"] * e["inv1"], e["norm2"] * e["inv2"]
    return e


def hager(T, zero_sign=None):
    """-> {"est", "first", "rounds", "v", "gaps"}: the estimate of |T^-1|_1, its first-round value, the rounds entered, the unit
    one-norm vector with |T v|_1 est = 1, and per completed round the relative gap between the largest and second largest |z_j|.
    zero_sign (tests only): the sign given to the exact zeros of y, entry by entry, in place of +1 -- what a rule that read the
    sign bit of a zero would do."""
    T = np.asarray(T, float)
    r = T.shape[0]
    x = np.full(r, 1.0 / r)
    est, first, jprev, rounds, v, gaps = 0.0, None, -1, 0, None, []
    for rnd in range(1, MAX_ROUNDS + 1):
        rounds = rnd
        y = sla.solve_triangular(T, x)
        g = float(np.abs(y).sum())
        if first is None:
            first = g
        if rnd > 1 and not g > est:
            break
        est, v = g, y / g
        if rnd == MAX_ROUNDS:
            break
        xi = np.where(y >= 0.0, 1.0, -1.0)
        if zero_sign is not None:
            xi = np.where(y == 0.0, zero_sign, xi)
        z = sla.solve_triangular(T, xi, trans="T")
        az = np.abs(z)
        j = int(np.argmax(az))                       # the first index that attains the maximum
        if r > 1:
            top = np.sort(az)[-2:]
            gaps.append(float((top[1] - top[0]) / top[1]) if top[1] > 0 else 0.0)
        if az[j] <= float(z @ x) or j == jprev:
            break
        jprev = j
        x = np.zeros(r)
        x[j] = 1.0
    y = sla.solve_triangular(T, safeguard(r))
    g = float(np.abs(y).sum())
    if 2.0 * g / (3.0 * r) > est:
        est, v = 2.0 * g / (3.0 * r), y / g
    return {"est": est, "first": first, "rounds": rounds, "v": v, "gaps": gaps}


def power2(T, iters=8):
    """-> {"norm", "inv", "v"}: lower estimates of |T|_2 and |T^-1|_2 after `iters` steps, v the last iterate of the inverse iteration"""
    T = np.asarray(T, float)
    r = T.shape[0]
    s = safeguard(r)
    x = s / np.linalg.norm(s)
    lam = 0.0
    for _ in range(iters):
        w = T.T @ (T @ x)
        lam = float(np.linalg.norm(w))
        if not lam > 0:
            break
        x = w / lam
    v = s / np.linalg.norm(s)
    for _ in range(iters):
        w = sla.solve_triangular(T, sla.solve_triangular(T, v, trans="T"))
        mu = float(np.linalg.norm(w))
        if not (mu > 0 and np.isfinite(mu)):
            break
        v = w / mu
    return {"norm": float(np.sqrt(lam)), "inv": float(1.0 / np.linalg.norm(T @ v)), "v": v}


def rlive_from_r_only(S, N, ncol=None):
    """R over its live pivot columns among the first ncol, from the R-only factors of a plan without H (qr_rhpack's keepH = 0
    layout: column k of a front holds the R rows of the front's live pivots up to k, a non-pivotal column all of them), in long
    double.  S: Symbolic (nf, n, Super, Rp, Rj), N: the download (Stack, Rblock_off, HStair, Hm).  -> (R_live, its columns in R's
    column order); with ncol < n the rows and columns of the trailing columns' pivots are left out: R11 of a plan that holds [A B]."""
    n = int(S.n)
    ncol = n if ncol is None else int(ncol)
    cols = []
    row0 = 0
    per_front = []
    for f in range(int(S.nf)):
        pr, fp = int(S.Rp[f]), int(S.Super[f + 1] - S.Super[f])
        fn = int(S.Rp[f + 1]) - pr
        fm = int(N.Hm[f])
        blk = np.asarray(N.Stack[int(N.Rblock_off[f]):])
        rm, at, ent = 0, 0, []
        for k in range(fn):
            if k < fp and int(N.HStair[pr + k]) != 0 and rm < fm:
                rm += 1
                cols.append(int(S.Rj[pr + k]))
            ent.append((int(S.Rj[pr + k]), row0, blk[at:at + rm] if fm > 0 else blk[:0]))
            at += rm if fm > 0 else 0
        per_front.append(ent)
        row0 += rm
    R = np.zeros((row0, n), np.longdouble)
    for ent in per_front:
        for col, r0, v in ent:
            R[r0:r0 + v.size, col] = v
    cols = np.asarray(cols, np.int64)
    assert np.all(np.diff(cols) > 0)
    keep = np.flatnonzero(cols < ncol)
    assert keep.size == 0 or keep[-1] == keep.size - 1, "the pivots of the trailing columns do not come last"
    T = R[:keep.size][:, cols[keep]]
    assert not np.any(np.tril(T, -1))
    return T, cols[keep]


# A 6 x 6 upper triangular matrix with small integer entries (every operation on it is exact) and negative diagonal entries: the
# rows of y = T \\ e_j behind j are zeros that a division computes as 0 / T_ii = -0.0.  Counting them as -1 changes the path and
# the estimate (5.25 becomes 7.125, tests/test_condest_cpu.py), so a run on it pins the rule "zero, of either sign, counts as +1".
# A matrix that is upper triangular already is its own R: every pivot column has nothing below its diagonal, so no reflector acts.
SIGNED_ZEROS = np.array([[-2., -1., 2., 1., 1., -3.],
                         [0., -2., 3., 3., 2., -3.],
                         [0., 0., -1., -2., -2., 3.],
                         [0., 0., 0., 1., 1., -3.],
                         [0., 0., 0., 0., -1., -2.],
                         [0., 0., 0., 0., 0., -2.]])
# diag: |T^-1| has its two largest columns tied (2, 2): z = (1, 2, 2, 1) in the first round, the lower index wins, v = e_1
TIED = np.diag([1.0, 0.5, 0.5, 1.0])
