"""Inputs and helpers of tests/test_gpu_block0.py: dense / staircase fronts whose steps take the one-launch form of T + column
block 0 (k_upd_b0w, dev_k_upd_b0 in csrc/stmmqr_update.hip) with a chosen number of panel rows below the diagonal block.

What decides the launch (csrc/stmmqr_schedule.cpp, csrc/stmmqr_run.cpp `rides`): a front is large from 64 columns and 64 rows on;
a step's update is row-parallel when one of its fronts has three slabs of 256 rows (its row bound: the front's, not the panel's);
the step rides -- block 0 through k_upd_b0w -- when one of its fronts has a second column block of 32 behind block 0.  The rows of a
panel's update, mp, are those its staircase reaches below the first pivot row of the panel.

One front: m x fn with columns 0..31 ending at row `first` (or under a staircase of their own) and every other column full, so
panel 0 has mp = max staircase of its columns and panel 1 has mp = m - 32.  fn = 97: panel 0 is followed by 65 columns (three column
blocks), panel 1 by 33 (two), panel 2 by one -- two riding steps.  Two fronts: a block-diagonal matrix, two roots of the same
level, panel p of both in step p."""
import re

import numpy as np

from resident_reference import stair_csc, symbolic_of

I64 = np.int64
NB = 32           # panel width and column block of the update
SLAB = 256        # rows of an update workgroup
B0_TIMELINE = 32768          # STMMQR_DBG bit: slab 0 of every block-0 workgroup set stamps its phases; the host prints their means and
                             # the number of (launch, front) pairs that ran to the end of dev_k_upd_b0
DEAD_AT = (3, 8, 20)         # duplicates of columns 1 and 2, a zero column: all in panel 0


def panel0_staircase(kind, first, m, seed):
    if kind == "full":                     # a dense 32-column block of `first` rows
        return np.full(NB, first, I64)
    if kind == "steps":                    # 1..3 more rows per column from row 3 on: every end inside the first 64-row chunk or just beyond
        rng = np.random.default_rng(seed)
        return np.minimum(m, 2 + np.cumsum(rng.integers(1, 4, NB))).astype(I64)
    if kind == "boundary":                 # the ends ON chunk boundaries: 16 columns of 64 rows, 16 of 128
        return np.repeat(np.array([64, 128], I64), NB // 2)
    raise ValueError(kind)


def make_front(m, fn, first, kind="full", seed=0, dead=False):
    """(F, Stair): Gaussian entries under the staircase; dead: duplicates and a zero column at DEAD_AT"""
    St = np.full(fn, m, I64)
    St[:NB] = panel0_staircase(kind, first, m, seed + 17)
    rng = np.random.default_rng(seed + 1000 * m + fn)
    F = np.zeros((m, fn), order="F")
    for k in range(fn):
        F[:St[k], k] = rng.standard_normal(St[k])
    if dead:
        F[:, 3], F[:, 8], F[:, 20] = F[:, 1], F[:, 2], 0.0
    return F, St


def block_diag_csc(fronts):
    """CSC of diag(front 0, front 1, ...) from [(F, Stair), ...]"""
    Ap, Ai, Ax, r0 = [np.zeros(1, I64)], [], [], 0
    for F, St in fronts:
        p, i, x = stair_csc(F, St)
        Ap.append(p[1:] + Ap[-1][-1])
        Ai.append(i + r0)
        Ax.append(x)
        r0 += F.shape[0]
    return np.concatenate(Ap), np.concatenate(Ai), np.concatenate(Ax)


def riding_block0(dims):
    """[(front, panel, nc of block 0)] of every block-0 workgroup set the default schedule launches for fronts of dims = [(m, fn), ...]
    (m >= fn, full rank) that start in the same step; empty when no step rides"""
    out = []
    if max((m + SLAB - 1) // SLAB for m, _ in dims) < 3:
        return out
    for p in range(max((fn + NB - 1) // NB for _, fn in dims)):
        trail = [max(fn - NB * (p + 1), 0) for _, fn in dims]
        if max(trail) > NB:
            out += [(f, p, min(t, NB)) for f, t in enumerate(trail) if t > 0]
    return out


def block0_count(err):
    """the count at the end of the last `[block-0 launch, ...]` line of the library's stderr"""
    found = re.findall(r"\[block-0 launch[^\n]*\((\d+)\)", err)
    assert found, "no block-0 timeline line on stderr"
    return int(found[-1])


FIELDS = ("HTau", "HStair", "Rdead", "Rblock_off")


def factorize(pkg, sym, Ap, Ai, Ax, tol, ntol, **options):
    """one factorization on a plan of its own under `options`; (stats, downloaded factors); the options are restored"""
    saved = pkg.get_options()
    pkg.set_options(**options)
    try:
        plan = pkg.HipQR(sym)
        try:
            st = plan.factorize(Ax, tol, ntol, Ap, Ai)
            return st, plan.download()
        finally:
            plan.close()
    finally:
        pkg.set_options(**saved)


def assert_same_bits(A, B):
    """two downloads of one input's factors: the same bits in rank, rh_total, FIELDS and Stack[:rh_total]"""
    assert (B.rank, B.rh_total) == (A.rank, A.rh_total)
    for k in FIELDS:
        assert np.array_equal(getattr(B, k), getattr(A, k)), k
    assert np.array_equal(B.Stack[:B.rh_total], A.Stack[:A.rh_total])


def assert_oracle(oracle, S, Ap, Ai, Ax, tol, n, stats, B):
    """the factors B (with the stats of their factorization) against the CPU oracle, as test_gpu_column_step.py::check_against_oracle:
    rank, staircase, Rdead and flops exact; Tau and the packed factors within 1e-11 of their 2-norms"""
    No = oracle.factorize(S, Ap, Ai, Ax, tol, n)
    assert B.rank == No.c.rank and B.rh_total == No.c.rh_total
    np.testing.assert_array_equal(B.HStair[:S.rjsize], No.HStair[:S.rjsize])
    np.testing.assert_array_equal(B.Rdead[:n], No.Rdead[:n])
    assert stats["flops"] == No.c.flopcount
    To, Fo = No.HTau[:S.rjsize], No.Stack[:No.c.rh_total]
    dT, dF = np.linalg.norm(B.HTau[:S.rjsize] - To), np.linalg.norm(B.Stack[:B.rh_total] - Fo)
    print(f"|dTau| {dT:.3e} / {max(np.linalg.norm(To), 1):.3e}   |dF| {dF:.3e} / {np.linalg.norm(Fo):.3e}")
    assert dT <= 1e-11 * max(np.linalg.norm(To), 1)
    assert dF <= 1e-11 * np.linalg.norm(Fo)


def analyzed(pkg, fronts):
    """(sym, S, Ap, Ai, Ax) of diag(fronts) through the package's symbolic phase, columns in their given order: one front each"""
    Ap, Ai, Ax = block_diag_csc(fronts)
    m, n = sum(F.shape[0] for F, _ in fronts), sum(F.shape[1] for F, _ in fronts)
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    assert sym["nf"] == len(fronts)
    np.testing.assert_array_equal(sym["PLinv"], np.arange(m))
    return sym, symbolic_of(sym), Ap, Ai, Ax
