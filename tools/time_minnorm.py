"""The minimum-norm solve on the resident factors (HipQR.solve_minnorm), timed next to what it is measured against:
  solve_minnorm          1 and 32 right-hand sides
  qmult(1, rsolve(3))    the composition it replaces (the m x nrhs block crosses PCIe twice more) -- "refused" where a front is too
                         wide for the one-workgroup R' solve
  rsolve(0), qmult(1)    the back substitution and the Q pass of the same plan: the split R' pass is the mirror of the first, and
                         solve_minnorm minus qmult(1) is what the R' pass costs
With --rtbig-min V a second plan is created under STMMQR_RTBIG_MIN=V (fronts of V entries or more take the split R' kernels) and
the two plans are timed alternately in the same process, with the largest difference between their results.
A warm plan; host arrays in and out; every call ends in the download of its result and is timed by the host wall clock: 3 calls
to warm up, then calls until 0.3 s and at least 10 of them have passed -- median (min) in ms.
usage: python tools/time_minnorm.py [--rtbig-min V] [fixture ...]"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stmmqr_testlib import Symbolic, load_golden, scalar  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")


def timed(calls, warm=3, least=10, window=0.3):
    """every call of `calls` in turn, round after round: -> [(median, min)] in ms"""
    for _ in range(warm):
        for f in calls:
            f()
    t = [[] for _ in calls]
    t_end = time.perf_counter() + window * len(calls)
    while len(t[0]) < least or time.perf_counter() < t_end:
        for i, f in enumerate(calls):
            t0 = time.perf_counter()
            f()
            t[i].append((time.perf_counter() - t0) * 1e3)
    return [(float(np.median(x)), float(min(x))) for x in t]


def make_plan(g, S):
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    plan = pkg.HipQR(sym)
    plan.set_pattern(g["in_Ap"], g["in_Ai"])
    for _ in range(2):
        st = plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    return plan, st


args = sys.argv[1:]
rtbig = None
if args[:1] == ["--rtbig-min"]:
    rtbig, args = int(args[1]), args[2:]
for name in (args or ["xenon1_colamd_standin", "sme3dc_standin", "c5mini_standin"]):
    g = load_golden(name)
    S = Symbolic(g)
    m, n = S.m, S.n
    rng = np.random.default_rng(1)
    B = {k: np.asfortranarray(rng.standard_normal((n, k))) for k in (1, 32)}
    Y = {k: np.asfortranarray(rng.standard_normal((m, k))) for k in (1, 32)}
    os.environ.pop("STMMQR_RTBIG_MIN", None)
    plan, st = make_plan(g, S)
    fmt = lambda mm: f"{mm[0]:.3f} ({mm[1]:.3f})"
    if rtbig is not None:
        os.environ["STMMQR_RTBIG_MIN"] = str(rtbig)
        plan2, _ = make_plan(g, S)
        os.environ.pop("STMMQR_RTBIG_MIN")
        nsplit = int(np.count_nonzero(np.asarray(S.Fm[:S.nf]) * np.diff(np.asarray(S.Rp[:S.nf + 1])) >= rtbig))
        out = [f"{name} m {m} n {n} nf {S.nf} fronts_of_{rtbig}_entries_or_more {nsplit}"]
        for k in (1, 32):
            a, b = timed([lambda: plan.solve_minnorm(B[k]), lambda: plan2.solve_minnorm(B[k])])
            d = np.linalg.norm(plan.solve_minnorm(B[k]) - plan2.solve_minnorm(B[k])) / np.linalg.norm(plan.solve_minnorm(B[k]))
            out.append(f"nrhs {k}: default {fmt(a)} ms, STMMQR_RTBIG_MIN={rtbig} {fmt(b)} ms, difference {d:.2e}")
        plan2.close()
    else:
        out = [f"{name} m {m} n {n} nf {S.nf} fact_ms {st['ms_total']:.1f}"]
        try:
            plan.rsolve(3, B[1])
            composed = True
        except pkg.StmmqrError as e:
            if e.code != -3:
                raise
            composed = False
        for k in (1, 32):
            calls = [lambda: plan.solve_minnorm(B[k]), lambda: plan.rsolve(0, Y[k]), lambda: plan.qmult(1, Y[k])]
            if composed:
                calls.append(lambda: plan.qmult(1, plan.rsolve(3, B[k])))
            r = timed(calls)
            out.append(f"nrhs {k}: solve_minnorm {fmt(r[0])} ms, rsolve(0) {fmt(r[1])} ms, qmult(1) {fmt(r[2])} ms, qmult(1, rsolve(3)) " +
                       (fmt(r[3]) + " ms" if composed else "refused"))
    plan.close()
    print(" | ".join(out), flush=True)
