"""keepH = 1 against keepH = 0 (R only) on one fixture, timed: factorization (device ms of the last of 3 calls), device memory the plan
holds, the cached drop-in seam (qr_factorize with the plan from its cache, download included; best of 3), rsolve system 1, the
seminormal solve (one correction step) and, with H, plan.solve.  Times are the best of 5 (ms, host wall clock incl. transfers).
usage: python tools/time_qless.py [fixture]"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stmmqr_testlib import Symbolic, csc_matvec, load_golden, scalar  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "xenon1_colamd_standin"
g = load_golden(name)
S = Symbolic(g)
tol, ntol = scalar(g, "in_tol"), int(scalar(g, "in_ntol"))
Ap, Ai, Ax = g["in_Ap"], g["in_Ai"], g["in_Ax"]
b = csc_matvec(S.m, Ap, Ai, Ax, np.arange(S.n, dtype=np.float64))


def best(f, k=5):
    t = []
    for _ in range(k):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


for keep in (1, 0):
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": keep}
    plan = pkg.HipQR(sym)
    plan.set_pattern(Ap, Ai)
    for _ in range(3):
        st = plan.factorize(Ax, tol, ntol)
    row = {"fact_ms": st["ms_total"], "device_GB": plan.device_bytes() / 1e9, "packed_M": plan.result_sizes()[0] / 1e6}
    y = plan.rsolve(3, b[:S.n] if S.m >= S.n else np.ones(S.n))
    plan.rsolve(1, y)
    row["rsolve1_ms"] = best(lambda: plan.rsolve(1, y))
    plan.solve_seminormal(b)
    row["csne_ms"] = best(lambda: plan.solve_seminormal(b, refine=1))
    x, info = plan.solve_seminormal(b, refine=1)
    row["csne_info"] = info
    if keep:
        plan.solve(b)
        row["solve_ms"] = best(lambda: plan.solve(b))
    plan.close()
    pkg.plan_cache_clear()
    pkg.qr_factorize_seam(sym, Ap, Ai, Ax, tol, ntol).close()          # (builds the plan the next calls take from the cache)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        N = pkg.qr_factorize_seam(sym, Ap, Ai, Ax, tol, ntol)
        t.append((time.perf_counter() - t0) * 1e3)
        N.close()
    row["seam_cached_ms"] = min(t)
    pkg.plan_cache_clear()
    print(f"{name} keepH={keep} " + " ".join(f"{k} {v:.4g}" for k, v in row.items()), flush=True)
