"""diag((A'A)^-1) by selected inversion (HipQR.covariance_diag) on a fixture, timed next to the two things it is measured against: the
factorization of the same plan (device ms of the last of 3 calls) and the only route that existed before, n / 32 batches of 32
unit vectors through rsolve(3, .) -- ONE batch is timed and multiplied; where that route refuses the fixture (a front too wide for
the one-workgroup R' solve) it prints "refused".  Also: the 32 variances of that batch against |R^-T e_j|^2.
The call is timed by the host wall clock (best of 3, allocation and release of its arena included).
usage: python tools/time_covariance.py [fixture ...]      default: the default workload of bench.py and c5mini_standin"""
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


def best(f, k=3):
    t = []
    for _ in range(k):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


for name in (sys.argv[1:] or ["xenon1_colamd_standin", "c5mini_standin"]):
    g = load_golden(name)
    S = Symbolic(g)
    tol, ntol = scalar(g, "in_tol"), int(scalar(g, "in_ntol"))
    n = S.n
    for keep in (1, 0):
        sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": keep}
        arena = sum((min(int(S.Super[f + 1] - S.Super[f]), int(S.Fm[f])) + int(S.Rp[f + 1] - S.Rp[f]) - int(S.Super[f + 1] - S.Super[f])) ** 2
                    for f in range(S.nf))
        plan = pkg.HipQR(sym)
        plan.set_pattern(g["in_Ap"], g["in_Ai"])
        for _ in range(3):
            st = plan.factorize(g["in_Ax"], tol, ntol)
        var = plan.covariance_diag()                 # (the first resident-factor operation of a plan creates the scratch they share)
        bytes0 = plan.device_bytes()
        t_cov = best(plan.covariance_diag)
        assert plan.device_bytes() == bytes0
        live = np.flatnonzero(var > 0)
        pick = np.sort(np.random.default_rng(1).choice(live, min(32, live.size), replace=False))
        E = np.zeros((n, pick.size), order="F")
        E[pick, np.arange(pick.size)] = 1.0
        row = {"n": n, "nf": S.nf, "rank": st["rank"] if "rank" in st else live.size, "fact_ms": st["ms_total"], "covariance_ms": t_cov,
               "cov_over_fact": t_cov / st["ms_total"], "arena_GB": 8e-9 * arena, "plan_GB": bytes0 / 1e9}
        try:
            Z = plan.rsolve(3, E)
            t_rs = best(lambda: plan.rsolve(3, E))
            ref = (Z ** 2).sum(axis=0)
            row.update({"rsolve3_batch_ms": t_rs, "rsolve3_all_ms": t_rs * n / 32, "speedup": t_rs * n / 32 / t_cov,
                        "max_rel_diff_32": float(np.max(np.abs(var[pick] - ref) / ref))})
            old = ""
        except pkg.StmmqrError as e:
            if e.code != -3:
                raise
            old = " rsolve3 refused"
        plan.close()
        print(f"{name} keepH={keep} " + " ".join(f"{a} {b:.4g}" for a, b in row.items()) + old, flush=True)
