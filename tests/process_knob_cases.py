"""Inputs, mirrors, batteries and digests of tests/test_gpu_process_knobs.py (no GPU at import).

The PROCESS rows of csrc/stmmqr_knobs.h (STMMQR_RSPW, STMMQR_RSPW_W, STMMQR_B0_ONE, STMMQR_PART_GRAIN, STMMQR_PART_CAP,
STMMQR_RHS_BATCH) are read once per process (knobs::once<>), so one pytest process only ever sees one value of each.  A battery is a
list of small cases that tests/process_knob_child.py runs in a fresh process under whatever environment it was given; it reports one
sha256 digest per case, and for the rider battery the lines the host launchers print under STMMQR_DBG = RIDER_LAUNCH
(`[rider launch] host <kernel> unfr .. uncb .. umaxsl .. rspw .. uy ..`: csrc/stmmqr_kernels.h, stm_report_rider_launch).

Rider battery (dense / staircase fronts of block0_cases.make_front, options.lookahead = 2).  A front of m x 97 has four panels; steps
0 and 1 ride (65 and 33 trailing columns: rider column blocks of 32 + 1 columns in step 0, of 1 column in step 1).  The riders of step t
run in two launches: k_upd_w's tiles behind T + block 0 of step t (k_upd_b0w, STMMQR_RSPW_W slabs per workgroup; k_upd_fw under
STMMQR_B0_ONE = 0) and k_upd_c's tiles behind the panels of step t + 1 (k_panel_pc, or k_panel_ca_pc when every panel of that step is
Gram-based; STMMQR_RSPW slabs per workgroup, 0: the launcher's rule, rider_rspw).  Step 0 updates mp = `first` rows, step 1 m - 32.

  600 x 97 (three slabs), first in 33, 256, 257, 320, 512, 513: with two slabs per rider the groups are {0, 1}, {2}; the rows of step 0 end
      inside slab 0, at the end of group 0's first and second slab, or one row into the next; step 1 has 568 rows (a partial last slab)
  1400 x 97 (six slabs), first in 1024, 1025, 1100: with four per rider the groups are {0..3}, {4, 5} -- group 1 is empty, holds one row
      or a partial slab; three per rider: groups that are no power of two; sixteen: one group longer than the front
  diag(300 x 95, 600 x 97): two fronts in one launch, the launch's three slabs above A's own two, A's rider block 31 columns wide
  600 x 97 with duplicate / zero columns in panel 0 (tol 1e-9) under the `steps` and `boundary` staircases: dead reflectors
      (pdiag = STM_BIGROW) and staircase ends inside the grouped rows
  the first three again with options.panel_algo = 2: the riders' host is k_panel_ca_pc with its one-dimensional index decomposition

Parts battery: whole factorizations of four fixtures and the 600 x 97 front (k_assemble / k_cpack cut into work_parts parts).
Batch battery: qmult, the four triangular systems, solve and the two minimum-norm solves with seven right-hand sides on two fixtures."""
import contextlib
import hashlib
import os
import re
import tempfile
from collections import namedtuple

import numpy as np

from block0_cases import NB, SLAB, analyzed, assert_oracle, assert_same_bits, factorize, make_front

RIDER_LAUNCH = 131072        # STMMQR_DBG bit: one stderr line per launch that carries riders (host only)
RB = 64                      # rows of a chunk of dev_upd_c_h2: its two halves take alternate chunks of the workgroup's rows
CA_MIN_ROWS = 4096           # STM_CA_MIN_ROWS: a panel with more expected rows is Gram-based under options.panel_algo = 0
PASS_MAXWG = 384             # STMMQR_PASS_MAXWG: the most workgroups of T + block 0 of a riding step (two per slab of every front)
M, FN = 600, 97

# ---- the rider battery -----------------------------------------------------------------------------------------------------------
# fronts: (m, fn, first, kind, seed, dead) of block0_cases.make_front
RiderCase = namedtuple("RiderCase", "name fronts tol options")


def _one(m, first, **options):
    suffix = "_gram" if options else ""
    return RiderCase(f"{m}x{FN}_first{first}{suffix}", ((m, FN, first, "full", first, False),), -1.0, options)


def _two(**options):
    suffix = "_gram" if options else ""
    return RiderCase(f"diag_300x95_{M}x{FN}{suffix}", ((300, 95, 193, "full", 95, False), (M, FN, 257, "full", 96, False)), -1.0, options)


FIRST_600 = (33, 256, 257, 320, 512, 513)
FIRST_1400 = (1024, 1025, 1100)
RIDER_CASES = ([_one(M, f) for f in FIRST_600] + [_one(1400, f) for f in FIRST_1400] + [_two()] +
               [RiderCase(f"{M}x{FN}_dead_{kind}", ((M, FN, 0, kind, 5, True),), 1e-9, {}) for kind in ("steps", "boundary")] +
               [_one(M, f, panel_algo=2) for f in FIRST_600] + [_one(1400, f, panel_algo=2) for f in FIRST_1400] + [_two(panel_algo=2)])

# the two in-process cases of tests/test_gpu_process_knobs.py: no knob set, the launchers' own rule picks two slabs per rider
ORGANIC_CASES = (RiderCase("4090x545", ((4090, 545, 4090, "full", 1, False),), -1.0, {}),      # 16 slabs, never Gram-based: 256 tiles
                 RiderCase("4200x545", ((4200, 545, 4200, "full", 2, False),), -1.0, {}))      # 17 slabs, panels 0-3 Gram-based: 272, 255

RIDER_SETTINGS = ([{"STMMQR_RSPW": str(k)} for k in (1, 2, 3, 4, 16)] + [{"STMMQR_RSPW_W": str(k)} for k in (1, 3, 4, 16)] +
                  [{"STMMQR_RSPW": "4", "STMMQR_RSPW_W": "4"}, {"STMMQR_B0_ONE": "0"}])
PARTS_SETTINGS = [{"STMMQR_PART_GRAIN": str(g), "STMMQR_PART_CAP": str(c)} for g, c in
                  ((1 << 40, 4096), (64, 4096), (1, 3), (1, 4096), (2048, 1))]
BATCH_SETTINGS = [{"STMMQR_RHS_BATCH": str(k)} for k in (1, 3)]
PARTS_FIXTURES = ("syn_grid3d", "syn_rankdef_grid", "bcsstk14", "epb1")
PARTS_FRONT = _one(M, 320)
BATCH_FIXTURES = ("bcsstk14", "syn_rankdef_grid")
NRHS = 7


def setting_id(env):
    return ",".join(f"{k[len('STMMQR_'):]}={v}" for k, v in env.items()) or "default"


def case_fronts(case):
    return [make_front(m, fn, first, kind, seed=seed, dead=dead) for m, fn, first, kind, seed, dead in case.fronts]


def case_dims(case):
    return [(fr[0], fr[1]) for fr in case.fronts]


# ---- mirrors of the host rules ---------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def rider_rspw(unfr, uncb, umaxsl, force=0):
    """slabs per rider workgroup of stm_launch_panel_pc / stm_launch_panel_ca_pc: the first k of 1, 2, 4, 8, 16 with the least
    ceil(tiles of ceil(umaxsl / k) slab groups / 240) * (5 + k); STMMQR_RSPW > 0 overrides"""
    best, rspw = 1e30, 1
    for k in (1, 2, 4, 8, 16):
        t = ceil_div(unfr * uncb * ceil_div(umaxsl, k), 240) * (5.0 + k)
        if t < best:
            best, rspw = t, k
    return force if force > 0 else rspw


def work_parts(work, grain=2048, cap=4096):
    """workgroups a front gets in the assembly / C-pack launches for `work` entries (stmmqr_schedule.cpp)"""
    return min(cap, max(1, ceil_div(work, grain)))


def rider_launches(dims, panel_algo=0, b0_one=1):
    """[(step, host kernel, unfr, uncb, umaxsl)] of every launch with riders that the passenger schedule makes for dense full-row
    fronts of dims = [(m, fn), ...] (m >= fn) that start in one step, in launch order: step t rides when its update is row-parallel
    (a front of three slabs), a second column block follows block 0 and T + block 0 fits PASS_MAXWG workgroups; its k_upd_w riders
    sit behind T + block 0 of step t, its k_upd_c riders behind the panels of step t + 1"""
    out, pend = [], None
    nsl = [ceil_div(m, SLAB) for m, _ in dims]
    for p in range(max(ceil_div(fn, NB) for _, fn in dims)):
        act = [f for f, (_, fn) in enumerate(dims) if p < ceil_div(fn, NB)]
        if pend is not None:
            gram = all(panel_algo == 2 or (panel_algo == 0 and dims[f][0] - min(NB * p, dims[f][1]) > CA_MIN_ROWS) for f in act)
            out.append((p, "k_panel_ca_pc" if gram else "k_panel_pc") + pend)
            pend = None
        ncb = [ceil_div(dims[f][1] - min(dims[f][1], NB * (p + 1)), NB) for f in act]
        maxcb, maxsl = max(ncb), max(nsl[f] for f in act)
        if maxsl >= 3 and maxcb > 1 and 2 * sum(nsl[f] for f in act) <= PASS_MAXWG:
            pend = (len(act), maxcb - 1, maxsl)
            out.append((p, "k_upd_b0w" if b0_one else "k_upd_fw") + pend)
    return out


def expected_report(launch, env):
    """(rspw, uy) that the launcher of `launch` = (step, host, unfr, uncb, umaxsl) must report under the knobs of env"""
    _, host, unfr, uncb, umaxsl = launch
    if host == "k_upd_fw":
        return 1, umaxsl
    if host == "k_upd_b0w":
        w = int(env.get("STMMQR_RSPW_W", 2))
        rspw = w if w > 0 else 2
    else:
        rspw = rider_rspw(unfr, uncb, umaxsl, int(env.get("STMMQR_RSPW", 0)))
    return rspw, ceil_div(umaxsl, rspw)


def rider_groups(case, env):
    """what every k_upd_c rider launch of a case asks of dev_upd_c_h2 under env, from the case table alone: one dict per (launch,
    front of the riding step) with the launch's slab groups, and per group the rows it updates.  Dense full-rank fronts only (the
    rows of step 0 are `first`, of step p m - 32 p)."""
    out = []
    dims = case_dims(case)
    for step, host, unfr, uncb, umaxsl in rider_launches(dims, case.options.get("panel_algo", 0), int(env.get("STMMQR_B0_ONE", 1))):
        if not host.startswith("k_panel"):
            continue
        t = step - 1                                            # the step whose update rides
        rspw, uy = expected_report((step, host, unfr, uncb, umaxsl), env)
        for m, fn, first, kind, _, dead in case.fronts:
            if kind != "full" or dead or t >= ceil_div(fn, NB):
                continue
            mp = first if t == 0 else m - NB * t
            trail = fn - NB * (t + 1)
            rows = [max(0, min(mp, (g + 1) * rspw * SLAB) - g * rspw * SLAB) for g in range(uy)]
            out.append(dict(case=case.name, step=t, host=host, rspw=rspw, uy=uy, umaxsl=umaxsl, nsl=ceil_div(m, SLAB), mp=mp, rows=rows,
                            cols=[min(NB, trail - NB * cb) for cb in range(1, ceil_div(trail, NB))]))
    return out


# ---- running a case --------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def library_stderr(sink):
    """what the library prints on the process's stderr (C stdio) while the block runs, appended to the list `sink` as one string"""
    import sys
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            yield
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
            tmp.seek(0)
            sink.append(tmp.read().decode(errors="replace"))


REPORT = re.compile(r"\[rider launch\] host (\w+) unfr (\d+) uncb (\d+) umaxsl (\d+) rspw (\d+) uy (\d+)")


def parse_reports(err):
    """[[host, unfr, uncb, umaxsl, rspw, uy]] of the `[rider launch]` lines in the library's stderr"""
    return [[h] + [int(x) for x in rest] for h, *rest in REPORT.findall(err)]


def digest_factors(stats, N, rjsize):
    h = hashlib.sha256()
    h.update(np.array([N.rank, N.rh_total], np.int64).tobytes())
    h.update(np.array([stats["flops"]], np.float64).tobytes())
    for a in (N.HStair, N.Rdead, N.Rblock_off, N.HTau[:rjsize], N.Stack[:N.rh_total]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digest_array(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def with_dbg(bits):
    """context: STMMQR_DBG (read at every run of a schedule) set to `bits`, then restored"""
    @contextlib.contextmanager
    def cm():
        old = os.environ.get("STMMQR_DBG")
        os.environ["STMMQR_DBG"] = str(bits)
        try:
            yield
        finally:
            if old is None:
                del os.environ["STMMQR_DBG"]
            else:
                os.environ["STMMQR_DBG"] = old
    return cm()


def run_rider_case(pkg, oracle, case):
    """One rider case in this process: lookahead = 0 (k_upd_w + k_upd_c: they read no PROCESS knob) and lookahead = 2 must give the
    same bits, and the lookahead = 2 factors pass the oracle comparison of test_gpu_block0.check.  Returns (digest, reports)."""
    sym, S, Ap, Ai, Ax = analyzed(pkg, case_fronts(case))
    n = int(sym["n"])
    st0, A = factorize(pkg, sym, Ap, Ai, Ax, case.tol, n, lookahead=0, **case.options)
    err = []
    with with_dbg(RIDER_LAUNCH), library_stderr(err):
        st2, B = factorize(pkg, sym, Ap, Ai, Ax, case.tol, n, lookahead=2, **case.options)
    assert st0["retries"] == 0 and st2["retries"] == 0 and st0["reschedules"] == 0 and st2["reschedules"] == 0, case.name
    assert_same_bits(A, B)
    assert_oracle(oracle, S, Ap, Ai, Ax, case.tol, n, st2, B)
    return digest_factors(st2, B, int(S.rjsize)), parse_reports(err[0])


def check_reports(case, env, reports):
    """the launch list of a case is rider_launches' and every reported rspw / uy is the mirror's -- never an empty list"""
    want = rider_launches(case_dims(case), case.options.get("panel_algo", 0), int(env.get("STMMQR_B0_ONE", 1)))
    assert want and reports, (case.name, "no rider launch")
    assert [r[:4] for r in reports] == [list(w[1:]) for w in want], (case.name, reports, want)
    for r, w in zip(reports, want):
        assert tuple(r[4:]) == expected_report(w, env), (case.name, r, w, expected_report(w, env))


def fixture_plan(pkg, name):
    """(S, g, sym dict) of a golden fixture"""
    from stmmqr_testlib import Symbolic, load_golden
    g = load_golden(name)
    S = Symbolic(g)
    return S, g, {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}


def run_parts_battery(pkg, oracle):
    """{case: digest}: whole factorizations, each checked against the CPU oracle (parity.compare_numeric as __graft_entry__.smoke;
    the dense front as test_gpu_block0.check)"""
    from parity import compare_numeric
    from stmmqr_testlib import scalar
    out = {}
    for name in PARTS_FIXTURES:
        S, g, sym = fixture_plan(pkg, name)
        tol, ntol = scalar(g, "in_tol"), int(scalar(g, "in_ntol"))
        st, N = factorize(pkg, sym, g["in_Ap"], g["in_Ai"], g["in_Ax"], tol, ntol)
        No = oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], tol, ntol)
        compare_numeric(oracle, S, N, No, g, ftol=1e-10, name=name)
        out[name] = digest_factors(st, N, int(S.rjsize))
    case = PARTS_FRONT
    sym, S, Ap, Ai, Ax = analyzed(pkg, case_fronts(case))
    st, N = factorize(pkg, sym, Ap, Ai, Ax, case.tol, int(sym["n"]))
    assert_oracle(oracle, S, Ap, Ai, Ax, case.tol, int(sym["n"]), st, N)
    out[case.name] = digest_factors(st, N, int(S.rjsize))
    return out


def run_batch_battery(pkg):
    """{fixture/operation: digest of the output} with NRHS right-hand sides"""
    from stmmqr_testlib import scalar
    out = {}
    for name in BATCH_FIXTURES:
        S, g, sym = fixture_plan(pkg, name)
        plan = pkg.HipQR(sym)
        try:
            plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
            rng = np.random.default_rng(len(name))
            Xm, Xn = rng.standard_normal((S.m, NRHS)), rng.standard_normal((S.n, NRHS))
            Xr = rng.standard_normal((NRHS, S.m))
            ops = {"qmult0": lambda: plan.qmult(0, Xm), "qmult1": lambda: plan.qmult(1, Xm), "qmult2": lambda: plan.qmult(2, Xr),
                   "qmult3": lambda: plan.qmult(3, Xr), "rsolve0": lambda: plan.rsolve(0, Xm), "rsolve1": lambda: plan.rsolve(1, Xm),
                   "rsolve2": lambda: plan.rsolve(2, Xn), "rsolve3": lambda: plan.rsolve(3, Xn), "solve": lambda: plan.solve(Xm),
                   "solve_minnorm": lambda: plan.solve_minnorm(Xn), "solve_lsminnorm": lambda: plan.solve_lsminnorm(Xm)}
            for op, call in ops.items():
                Y = call()
                assert np.all(np.isfinite(Y)), (name, op)
                out[f"{name}/{op}"] = digest_array(Y)
        finally:
            plan.close()
    return out


def parts_of_fixture(name, grain, cap):
    """[(work, parts)] of the assembly and the C-pack cut of every front of a fixture (the work: fm_ub * fn, and cn * min(fm_ub, cn)
    with cn = fn - fp, as stmmqr_schedule.cpp; fm_ub is the analysis' Fm)"""
    from stmmqr_testlib import Symbolic, load_golden
    S = Symbolic(load_golden(name))
    out = []
    for f in range(S.nf):
        fn, fp, fm = int(S.Rp[f + 1] - S.Rp[f]), int(S.Super[f + 1] - S.Super[f]), int(S.Fm[f])
        cn = fn - fp
        out += [(w, work_parts(w, grain, cap)) for w in (fm * fn, cn * min(fm, cn))]
    return out
