"""The condition estimate and the products with R on the resident factors, timed next to what they are made of:
  condest(1)             Hager / Higham's one-norm estimate: `rounds` solve pairs (R \\ then R' \\) and one more R \\
  condest(2)             8 steps of the power iteration on R'R and on its inverse: 8 solve pairs and 17 products with R
  rsolve(0)              one back substitution of the same plan
  solve_minnorm          one R' \\ pass (the one that takes fronts of any width) plus the Q pass
  rmult(0), rmult(1)     R x and R'y with 1 and 32 vectors
A warm plan; host arrays in and out; every call ends in the download of its result and is timed by the host wall clock: 3 calls
to warm up, then calls until 0.3 s and at least 10 of them have passed -- median (min) in ms.
usage: python tools/time_condest.py [fixture ...]"""
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


for name in (sys.argv[1:] or ["xenon1_colamd_standin", "c5mini_standin"]):
    g = load_golden(name)
    S = Symbolic(g)
    m, n = S.m, S.n
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    plan = pkg.HipQR(sym)
    plan.set_pattern(g["in_Ap"], g["in_Ai"])
    for _ in range(2):
        st = plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    rng = np.random.default_rng(1)
    X = {k: np.asfortranarray(rng.standard_normal((n, k))) for k in (1, 32)}
    Y = {k: np.asfortranarray(rng.standard_normal((m, k))) for k in (1, 32)}
    c1, c2 = plan.condest(1), plan.condest(2)
    fmt = lambda mm: f"{mm[0]:.3f} ({mm[1]:.3f})"
    r = timed([lambda: plan.condest(1), lambda: plan.condest(2), lambda: plan.rsolve(0, Y[1]), lambda: plan.solve_minnorm(X[1]),
               lambda: plan.rmult(X[1], 0), lambda: plan.rmult(X[32], 0), lambda: plan.rmult(Y[1], 1), lambda: plan.rmult(Y[32], 1)])
    plan.close()
    print(f"{name} m {m} n {n} nf {S.nf} fact_ms {st['ms_total']:.1f} | cond_1 >= {c1['cond']:.3e} ({c1['rounds']} rounds), "
          f"cond_2 >= {c2['cond']:.3e} (8 steps) | condest(1) {fmt(r[0])} ms, condest(2) {fmt(r[1])} ms, rsolve(0) {fmt(r[2])} ms, "
          f"solve_minnorm {fmt(r[3])} ms | rmult(0) x1 {fmt(r[4])} ms, x32 {fmt(r[5])} ms; rmult(1) x1 {fmt(r[6])} ms, x32 {fmt(r[7])} ms", flush=True)
