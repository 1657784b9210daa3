"""Three ways to a least-squares solution on one fixture, timed for 1 and for 32 right-hand sides: (a) the plan of A that keeps H +
plan.solve, (b) the R-only plan of A + the seminormal solve (one correction step), (c) the R-only plan of [A B] + the carried solve
(LeastSquares).  Per row: factorization (device ms of the last of 3 calls), solve (best of 5, ms, host wall clock incl. transfers;
for (c) the device ms of the back substitution beside it), device GB the plan holds after the factorization, backward error
|A'r| / (|A|_F (|A|_F |x| + |b|)).  (c) factorizes at every solve: its solve column is the back substitution alone.
usage: python tools/time_carried.py [fixture]"""
import importlib
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stmmqr_testlib import Symbolic, load_golden, scalar  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "xenon1_colamd_standin"
g = load_golden(name)
S = Symbolic(g)
tol, ntol = scalar(g, "in_tol"), int(scalar(g, "in_ntol"))
Ap, Ai, Ax = g["in_Ap"], g["in_Ai"], g["in_Ax"]
m, n = S.m, S.n
A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n))
af = np.linalg.norm(Ax)
Q = S.Qfill if S.Qfill is not None else np.arange(n)


def best(f, k=5):
    t = []
    for _ in range(k):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


def berr(X, B):
    X, B = X.reshape(n, -1), B.reshape(m, -1)
    return max(np.linalg.norm(A.T @ (B[:, j] - A @ X[:, j])) / (af * (af * np.linalg.norm(X[:, j]) + np.linalg.norm(B[:, j])))
               for j in range(B.shape[1]))


def show(tag, k, row):
    print(f"{name} nrhs={k} {tag} " + " ".join(f"{a} {b:.4g}" for a, b in row.items()), flush=True)


for k in (1, 32):
    B = np.asfortranarray(np.random.default_rng(1).standard_normal((m, k)))
    for keep in (1, 0):
        sym = {**S.sc, **{kk: v for kk, v in S.arr.items() if v is not None}, "keepH": keep}
        plan = pkg.HipQR(sym)
        plan.set_pattern(Ap, Ai)
        for _ in range(3):
            st = plan.factorize(Ax, tol, ntol)
        row = {"fact_ms": st["ms_total"], "device_GB": plan.device_bytes() / 1e9, "flops": st["flops"]}
        if keep:
            X = plan.solve(B)
            row["solve_ms"] = best(lambda: plan.solve(B))
        else:
            X, _ = plan.solve_seminormal(B, refine=1)
            row["solve_ms"] = best(lambda: plan.solve_seminormal(B, refine=1))
        row["backward_err"] = berr(X, B)
        plan.close()
        show("(a) H + plan.solve" if keep else "(b) R only + seminormal", k, row)
    L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=k, ordering=3, Quser=Q, tol=tol)
    for _ in range(3):
        X, resid = L.solve(B)
    info = L.info
    p = L.plan()
    row = {"fact_ms": info["ms_factorize"], "device_GB": info["device_bytes"] / 1e9, "flops": info["flops"], "flop_bound": info["flop_bound"],
           "nf": info["nf"], "solve_ms": best(lambda: p.solve_carried(k)), "solve_device_ms": info["ms_solve"],
           "backward_err": berr(X, B), "retries": info["retries"]}
    L.close()
    show("(c) R only of [A B] + carried", k, row)
