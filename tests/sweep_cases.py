"""Inputs, shape arithmetic and helpers of tests/test_gpu_sweeps.py and tests/test_sweep_cases_cpu.py: dense / staircase fronts whose
trailing update goes through the pair and quad sweeps of csrc/stmmqr_sweep.hip (k_upd_w2 / y2 / c2, k_upd_wq / yq / cq) under
options.pair_update = 1 / 4 with STMMQR_PAIR_MIN = 1, chosen for the edges of those kernels' indexing and masks.

What decides a sweep (restated here from the code, `sweeps` below):
  the planner (stmmqr_schedule.cpp is_pair): a large front (fn >= 64, fm >= 64) of at least 4 panels takes sweeps; every panel of
      such a front is a step (no early end), and after panel p = w - 1 (mod w), w = 2 / 4, ONE sweep launch applies the w panels
      p - w + 1 .. p to the column blocks beyond block 0 of panel p: ncbp = stm_upd_ncb(p) - 1 of them, from column 32 (p + 2) on;
  pair_geom / quad_geom: g1 = first pivot row of the sweep's first panel, mp_i = pt_i - g1 the rows V_i reaches (0: the panel did
      nothing, its rows ran out), mp = max mp_i; nb_i the panel's columns;
  stm_pair_spw / stm_quad_spw: slabs of 256 rows per workgroup from nsl = ceil(mp / 256): 1 / 2 / 4 from 16 / 32 slabs, the quad 8
      from 64; ngrp = ceil(nsl / spw) partial sums per column block, against a slot stride stm_pair_slots / stm_quad_slots of
      nslf = ceil(fm / 256), the FRONT's slabs (host sizing, stmmqr_schedule.cpp).
All of it for a full-rank front (every pivot live while rows last), whose panel p starts at pivot row min(32 p, m)."""
import re
from collections import namedtuple

import numpy as np

from block0_cases import block_diag_csc
from resident_reference import symbolic_of

I64 = np.int64
LD = np.longdouble
NB = 32           # panel width and column block of the update
SLAB = 256        # rows of a slab
BIG_COLS = 64     # options.big_front_cols (default): fronts from this many columns and 64 rows on are large
SWEEP_LINES = 65536          # STMMQR_DBG bit: the host prints one `[sweep launch]` line per front of every pair / quad sweep launch
TOL_DEAD = 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# 1. shape arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def pair_spw(nsl):
    return 4 if nsl >= 32 else 2 if nsl >= 16 else 1


def quad_spw(nsl):
    return 8 if nsl >= 64 else pair_spw(nsl)


def pair_slots(nslf):
    return nslf if nslf < 16 else max((nslf + 3) // 4, 16)


def quad_slots(nslf):
    return nslf if nslf < 16 else max((nslf + 7) // 8, 16)


def upd_ncb(fn, p):
    """stm_upd_ncb: column blocks of 32 behind panel p"""
    return (fn - min((p + 1) * NB, fn) + 31) // 32


def takes_sweeps(m, fn):
    """Planner::is_pair under STMMQR_PAIR_MIN = 1 and the default big_front_cols"""
    return fn >= BIG_COLS and m >= 64 and (fn + NB - 1) // NB >= 4


def panel_rows(m, fn, St):
    """[(g1, pt, nb)] of every panel of a full-rank m x fn front under the (non-decreasing) staircase St, as the panel kernels leave
    them in PanelDesc: a panel that starts without rows did nothing (nb = 0); otherwise nb = its columns, pt = min(m, max(St of its
    last column, g1 + nb))"""
    out = []
    for p in range((fn + NB - 1) // NB):
        k1, k2 = p * NB, min(fn, (p + 1) * NB)
        g1 = min(k1, m)
        out.append((g1, g1, 0) if g1 >= m else (g1, min(m, max(int(St[k2 - 1]), g1 + k2 - k1)), k2 - k1))
    return out


Sweep = namedtuple("Sweep", "w p g1 mp mpi nb nsl spw ngrp slots ncbp last_width work")


def sweeps(m, fn, staircase=None, sweep=4):
    """Every sweep launch of a full-rank m x fn front under pair_update = 1 (sweep = 2) / 4 (sweep = 4): one Sweep per panel
    p = sweep - 1 (mod sweep), whether or not it has a column (ncbp > 0) or rows (work).  staircase: None (dense) or St[fn]."""
    w = int(sweep)
    assert w in (2, 4)
    if not takes_sweeps(m, fn):
        return []
    St = np.full(fn, m, I64) if staircase is None else np.asarray(staircase, I64)
    assert St.shape == (fn,) and np.all(np.diff(St) >= 0)
    pan = panel_rows(m, fn, St)
    nslf = (m + SLAB - 1) // SLAB
    out = []
    for p in range(w - 1, len(pan), w):
        mine = pan[p - w + 1:p + 1]
        g1 = mine[0][0]
        nb = tuple(q[2] for q in mine)
        mpi = tuple(q[1] - g1 if q[2] > 0 else 0 for q in mine)
        mp = max(mpi) if nb[0] > 0 else 0
        nsl = (mp + SLAB - 1) // SLAB
        spw = (quad_spw if w == 4 else pair_spw)(nsl)
        ncbp = upd_ncb(fn, p) - 1
        out.append(Sweep(w=w, p=p, g1=g1, mp=mp, mpi=mpi, nb=nb, nsl=nsl, spw=spw, ngrp=(nsl + spw - 1) // spw,
                         slots=(quad_slots if w == 4 else pair_slots)(nslf), ncbp=ncbp,
                         last_width=(fn - NB * (p + 2) - NB * (ncbp - 1)) if ncbp > 0 else 0, work=(mp > 0 and ncbp > 0)))
    return out


NWAVES = 4        # waves of an update workgroup (NT / 64)


def tile_forms(s):
    """Which forms of a 16-row tile the applying kernel (k_upd_c2 / k_upd_cq) takes in a full column block of Sweep s with every
    reflector live, over all its slab groups and waves -- restated from the kernels: tiles [t_lo, t_hi) of a group are interior
    (below every unit diagonal, inside every panel's rows); the pair pipelines them four per trip and wave, the quad as super tiles
    of 32 rows two per trip and wave; everything else is the general (masked) tile.  Returns a set of
    "head" (general tiles above the interior), "tail" (below it), "pipeline", ("left", k) (k interior tiles / super tiles of a wave
    after its last whole trip, k = 0 included), "none" (a group without interior tile)."""
    out = set()
    if not s.work:
        return out
    dead = 0 in s.nb
    dmax = s.w * NB - 1                                        # last unit diagonal, relative to g1
    for sl in range(0, s.nsl, s.spw):
        rbeg, rend = sl * SLAB, min(s.mp, (sl + s.spw) * SLAB)
        ntile = (rend - rbeg + 15) >> 4
        rfull = min(min(s.mpi), rend)
        t_lo = ntile if dead else min(ntile, max(0, (dmax + 1 - rbeg + 15) >> 4))
        t_hi = max(t_lo, (rfull - rbeg) >> 4)
        if t_lo > 0:
            out.add("head")
        if t_hi == t_lo:
            out.add("none")
        for wid in range(NWAVES):
            if s.w == 2:
                tix = wid + NWAVES * max(0, (t_lo - wid + NWAVES - 1) // NWAVES)
                if tix < t_hi:
                    nint = (t_hi - 1 - tix) // NWAVES + 1
                    out.add(("left", nint - 4 * (nint >> 2)))
                    if nint >> 2:
                        out.add("pipeline")
            else:
                ns = (t_hi - t_lo) >> 1
                if ns > wid:
                    nmine = (ns - 1 - wid) // NWAVES + 1
                    out.add(("left", nmine - 2 * (nmine >> 1)))
                    if nmine >> 1:
                        out.add("pipeline")
        if ntile > (t_hi if s.w == 2 else t_lo + 2 * ((t_hi - t_lo) >> 1)):
            out.add("tail")
    return out


def launches(dims, sweep):
    """[(front, panel, ncbp)] of the sweep launches WITH a column that the library reports for fronts of dims = [(m, fn), ...]:
    symbolic (whether rows are left is the kernels' business), so it holds for rank-deficient fronts too"""
    return [(f, s.p, s.ncbp) for f, (m, fn) in enumerate(dims) for s in sweeps(m, fn, None, sweep) if s.ncbp > 0]


def reported_launches(err):
    """[(front, panel, ncbp)] with ncbp > 0 from the `[sweep launch]` lines of the library's stderr, and the panels per sweep they name"""
    found = re.findall(r"\[sweep launch\] w (\d+) step \d+ front (\d+) panel (\d+) ncbp (-?\d+)", err)
    return sorted((int(f), int(p), int(c)) for _, f, p, c in found if int(c) > 0), {int(w) for w, _, _, _ in found}


# ---------------------------------------------------------------------------------------------------------------------
# 2. cases
# ---------------------------------------------------------------------------------------------------------------------
def staircase(kind, m, fn, seed):
    if kind == "full":
        return np.full(fn, m, I64)
    if kind == "ramp":                     # column k ends at row (k + 1) m / fn + 8 (tests/test_gpu_seams.py make_front)
        return np.minimum(m, (np.arange(1, fn + 1) * m) // fn + 8).astype(I64)
    if kind == "steps":                    # 1..3 more rows per column (tests/test_gpu_seams.py make_front): the panels of a sweep end on different rows
        return np.minimum(m, 2 + np.cumsum(np.random.default_rng(seed).integers(1, 4, fn))).astype(I64)
    if kind == "chunks":                   # panel p ends at row 64 (p + 2): a multiple of 64 rows below the first pivot row 64 j / 128 j of its sweep
        return np.minimum(m, 64 * (np.arange(fn) // NB + 2)).astype(I64)
    raise ValueError(kind)


# name -> {column: source column or None (zero)}: dead columns under tol = TOL_DEAD of the 600 x 257 fronts
DEAD = {
    "edges": {3: 1, 8: 2, 20: None, 99: 97, 104: 98, 116: None},       # panels 0 and 3: first and last of quad 0, of the pairs (0, 1) and (2, 3)
    "panel0": {k: None for k in range(0, 32)},                          # a whole panel without a reflector: position 0 of the quad
    "panel2": {k: None for k in range(64, 96)},                         # ... position 2
}

Front = namedtuple("Front", "m fn kind seed dead", defaults=("full", 0, None))
Case = namedtuple("Case", "name fronts tol group")


def _cases():
    out = []
    for kind in ("full", "ramp"):
        for fn in (129, 160, 161, 191, 193, 224, 225, 257, 289, 300):
            out.append(Case(f"cols_{kind}_{fn}", (Front(600, fn, kind, fn),), -1.0, "columns"))
    for m in (70, 100, 128, 140, 170, 200, 230):
        out.append(Case(f"runout_{m}", (Front(m, 400, "full", m),), -1.0, "runout"))
    for m, fn in ((3900, 300), (4000, 300), (4097, 300), (8000, 300), (16200, 300), (4000, 420)):
        out.append(Case(f"slabs_{m}x{fn}", (Front(m, fn, "full", m),), -1.0, "slabs"))
    # (the `steps` staircase ends after ~2 fn rows: the rows of the matrix below it are empty and the FRONT has St[-1] rows, front_rows)
    out.append(Case("steps_600x257", (Front(600, 257, "steps", 11),), -1.0, "stairs"))
    out.append(Case("steps_4000x300", (Front(4000, 300, "steps", 12),), -1.0, "stairs"))
    out.append(Case("ramp_4000x300", (Front(4000, 300, "ramp", 14),), -1.0, "stairs"))     # unequal rows on a front of 16 slabs
    out.append(Case("chunks_600x257", (Front(600, 257, "chunks", 13),), -1.0, "stairs"))
    for name in DEAD:
        out.append(Case(f"dead_{name}", (Front(600, 257, "full", 21, name),), TOL_DEAD, "dead"))
    out.append(Case("two_fronts", (Front(600, 193, "full", 31), Front(900, 257, "full", 32)), -1.0, "two"))
    return out


CASES = _cases()
NO_QUAD_COLUMNS = {f"cols_{kind}_{fn}" for kind in ("full", "ramp") for fn in (129, 160)}     # meant for the pair sweep alone
BY_NAME = {c.name: c for c in CASES}


def stair_of(fr):
    return staircase(fr.kind, fr.m, fr.fn, fr.seed + 17)


def front_rows(fr):
    """rows of the front: those of the matrix that hold an entry (all of them except under the `steps` staircase)"""
    return int(stair_of(fr)[-1])


def make_front(fr):
    """(F, Stair) of a Front: Gaussian entries under the staircase, seeded; dead columns as DEAD says"""
    St = stair_of(fr)
    rng = np.random.default_rng(fr.seed + 1000 * fr.m + fr.fn)
    F = np.zeros((fr.m, fr.fn), order="F")
    for k in range(fr.fn):
        F[:St[k], k] = rng.standard_normal(St[k])
    for k, src in sorted((DEAD[fr.dead] if fr.dead else {}).items()):
        F[:, k] = 0.0 if src is None else F[:, src]
    return F, St


def expected_rank(fr):
    return min(front_rows(fr), fr.fn) - (len(DEAD[fr.dead]) if fr.dead else 0)


def front_sweeps(fr, w):
    """the Sweeps of a Front (full-rank arithmetic: an input of the `dead` group follows it only in its launches)"""
    return sweeps(front_rows(fr), fr.fn, np.minimum(stair_of(fr), front_rows(fr)), w)


def case_launches(case, w):
    return launches([(front_rows(fr), fr.fn) for fr in case.fronts], w)


def coverage(w):
    """what the case list reaches for sweeps of w panels, as sets / flags over all cases outside the `dead` group; only sweeps
    with rows and a column count (Sweep.work)"""
    cov = dict(spw=set(), spw_pairs=set(), ngrp1=False, partial_group=False, one_row_slab=False, ncbp1=False, ncbp_many=False,
               last_width=set(), narrow_last_panel=set(), v_panel_widths=set(), end_pos=set(), runout_pos=set(),
               first_panel_empty=False, unequal_rows=False, chunk_ends=False, slots_ok=True, launch_above_front=False,
               tile_forms=set())
    for c in CASES:
        if c.group == "dead":
            continue
        for fr in c.fronts:
            m, sw = front_rows(fr), front_sweeps(fr, w)
            live = [s for s in sw if s.work]
            if live:
                cov["end_pos"].add(((fr.fn + NB - 1) // NB) % w)
                if fr.fn % NB:
                    cov["narrow_last_panel"].add(fr.fn % NB)
            for a, b in zip(live, live[1:]):                     # consecutive sweeps of ONE front on both sides of a threshold
                if a.spw != b.spw:
                    cov["spw_pairs"].add((a.nsl, b.nsl))
            for s in sw:
                cov["slots_ok"] &= s.ngrp <= s.slots
            for s in live:
                cov["spw"].add(s.spw)
                cov["ngrp1"] |= s.ngrp == 1
                cov["partial_group"] |= s.nsl % s.spw != 0
                cov["one_row_slab"] |= s.mp % SLAB == 1
                cov["ncbp1"] |= s.ncbp == 1
                cov["ncbp_many"] |= s.ncbp > 1
                cov["last_width"].add(s.last_width)
                cov["v_panel_widths"] |= set(s.nb)
                if s.ncbp > 1 or s.last_width == NB:             # (a full column block: a ragged one takes general tiles alone)
                    cov["tile_forms"] |= tile_forms(s)
                live_mp = [r for r, n in zip(s.mpi, s.nb) if n > 0]
                cov["unequal_rows"] |= len(set(live_mp)) == len(live_mp) > 1
                cov["chunk_ends"] |= fr.kind == "chunks" and all(r % 64 == 0 for r in live_mp)
                if m < fr.fn and 0 in s.nb:                      # the rows run out inside this sweep: in its panel nb.index(0) - 1
                    cov["runout_pos"].add(s.nb.index(0) - 1)
                if m < fr.fn and 0 not in s.nb and s.g1 + w * NB >= m:
                    cov["runout_pos"].add(w - 1)                 # ... in its last panel
            cov["first_panel_empty"] |= any(s.ncbp > 0 and s.nb[0] == 0 for s in sw)
        if len(c.fronts) > 1:                                    # one launch for all: its grid is the largest front's
            per = [{s.p: s for s in front_sweeps(fr, w)} for fr in c.fronts]
            for p in set.intersection(*[set(d) for d in per]):
                cov["launch_above_front"] |= (len({d[p].ncbp for d in per}) > 1 and min(d[p].ncbp for d in per) > 0 and
                                              len({(front_rows(fr) + SLAB - 1) // SLAB for fr in c.fronts}) > 1)
    return cov


# ---------------------------------------------------------------------------------------------------------------------
# 3. helpers of the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def analyzed(pkg, fronts):
    """(sym, S, Ap, Ai, Ax) of diag(fronts) through the package's symbolic phase: one front each, rows in their given order"""
    Ap, Ai, Ax = block_diag_csc(fronts)
    m, n = sum(F.shape[0] for F, _ in fronts), sum(F.shape[1] for F, _ in fronts)
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    assert sym["nf"] == len(fronts)
    np.testing.assert_array_equal(sym["PLinv"], np.arange(m))
    return sym, symbolic_of(sym), Ap, Ai, Ax


def factorize(pkg, sym, Ap, Ai, Ax, tol, ntol, X=None, **options):
    """one factorization on a plan of its own under `options`: (stats, downloaded factors, Q'X or None); the options are restored"""
    saved = pkg.get_options()
    pkg.set_options(**options)
    try:
        plan = pkg.HipQR(sym)
        try:
            st = plan.factorize(Ax, tol, ntol, Ap, Ai)
            return st, plan.download(), (plan.qmult(0, X) if X is not None else None)
        finally:
            plan.close()
    finally:
        pkg.set_options(**saved)


def unpack_front(N, S, f):
    """(Fout, Stair_out, Tau): front f (every column pivotal) back in front form from its packed R+H block -- a dead pivot column holds
    the R rows so far, a live one its R rows, the diagonal and the reflector below it up to Stair (tests/oracle_plan.py front_rhoff)"""
    pr, fn, fm = int(S.Rp[f]), int(S.Rp[f + 1] - S.Rp[f]), int(N.Hm[f])
    assert int(S.Super[f + 1] - S.Super[f]) == fn
    St = np.asarray(N.HStair[pr:pr + fn], I64)
    off = int(N.Rblock_off[f])
    end = min([int(o) for o in N.Rblock_off[:int(S.nf)] if int(o) > off], default=int(N.rh_total))
    blk = N.Stack[off:end]
    F = np.zeros((fm, fn), order="F")
    p = rm = 0
    for k in range(fn):
        t = int(St[k])
        if t == 0:
            t = rm
        elif rm < fm:
            rm += 1
        F[:t, k] = blk[p:p + t]
        p += t
    assert p == blk.size, (p, blk.size)
    return F, St, np.asarray(N.HTau[pr:pr + fn])


def column_distances(A, B):
    """per column k: ||A[:, k] - B[:, k]|| / ||B[:, k]|| (0 where both are zero, inf where only B is)"""
    A, B = np.asarray(A), np.asarray(B)                    # (fp64 against fp64 stays fp64: the difference of two close doubles is exact)
    d, nb = np.sqrt(((A - B) ** 2).sum(axis=0)), np.sqrt((B ** 2).sum(axis=0))
    out = np.zeros(B.shape[1])
    nz = nb > 0
    out[nz] = (d[nz] / nb[nz]).astype(np.float64)
    out[~nz & (d > 0)] = np.inf
    return out


def ld_front(F, Stair, tol):
    """The unblocked column loop of the front factorization in long double (the rules of adversarial_fronts.ref_front, every column
    pivotal and under the tolerance), returning the factored front in front form: (Fout, Stair_out, Rdead)"""
    A = np.asfortranarray(F, dtype=LD)
    m, n = A.shape
    St = np.array(Stair, I64)
    Rdead = np.zeros(n, np.int8)
    g = 0
    for k in range(n):
        if g >= m:
            Rdead[k:] = 1
            St[k:] = 0
            break
        t = max(g + 1, int(St[k]))
        alpha = A[g, k]
        x = A[g + 1:t, k]
        ss = x @ x if x.size else LD(0)
        beta, tau = (alpha, LD(0)) if ss == 0 else (-np.copysign(np.sqrt(alpha * alpha + ss), alpha), None)
        if abs(beta) <= tol:
            A[g:, k] = 0
            St[k] = 0
            Rdead[k] = 1
            continue
        St[k] = t
        if tau is None:
            tau = (beta - alpha) / beta
            v = x / (alpha - beta)
            if k + 1 < n:
                w = tau * (A[g, k + 1:] + v @ A[g + 1:t, k + 1:])
                A[g, k + 1:] -= w
                A[g + 1:t, k + 1:] -= np.outer(v, w)
            A[g + 1:t, k] = v
        A[g, k] = beta
        g += 1
    return A, St, Rdead
