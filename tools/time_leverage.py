"""Leverages from the resident blocks of the selected inverse (HipQR.leverage), timed next to what they are measured against:
  xenon1_colamd_standin   covariance_diag alone; leverage with var (ONE selected inversion serves both); the only route that existed
                          before, m / 32 batches of 32 rows through rsolve(3, .) -- ONE batch is timed and multiplied ("old route")
  c5mini_standin          the same, where the old route refuses (a front too wide for the one-workgroup R' solve): prints "refused"
Also: the 32 leverages of that batch against |R^-T a_i|^2, sum h against the rank, and the longest row (a row costs nnz(row)^2 lookups
on one wave).  A warm plan; every call is timed by the host wall clock, best of 3, allocation and release of its buffers included.
usage: python tools/time_leverage.py [fixture ...]"""
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
    m, n = S.m, S.n
    A = sp.csc_matrix((g["in_Ax"], g["in_Ai"], g["in_Ap"]), shape=(m, n)).tocsr()
    rownz = np.diff(A.indptr)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    plan = pkg.HipQR(sym)
    plan.set_pattern(g["in_Ap"], g["in_Ai"])
    for _ in range(3):
        st = plan.factorize(g["in_Ax"], tol, ntol)
    var = plan.covariance_diag()                     # (the first resident-factor operation of a plan creates the scratch they share)
    lev, var2 = plan.leverage(with_var=True)
    assert np.array_equal(var, var2)
    bytes0 = plan.device_bytes()
    t_cov = best(plan.covariance_diag)
    t_lev = best(lambda: plan.leverage(with_var=True))
    assert plan.device_bytes() == bytes0
    rank = int(np.count_nonzero(var > 0))
    row = {"m": m, "n": n, "nf": S.nf, "rank": rank, "nnz": int(A.nnz), "max_row_nnz": int(rownz.max()), "sum_row_nnz2": float((rownz.astype(float) ** 2).sum()),
           "fact_ms": st["ms_total"], "covariance_ms": t_cov, "leverage_with_var_ms": t_lev, "leverage_over_covariance": t_lev / t_cov,
           "sum_h_minus_rank": float(lev.sum()) - rank, "min_h": float(lev.min()), "max_h": float(lev.max())}
    pick = np.sort(np.random.default_rng(1).choice(m, min(32, m), replace=False))
    E = np.asfortranarray(A[pick].toarray().T)
    try:
        Z = plan.rsolve(3, E)
        t_rs = best(lambda: plan.rsolve(3, E))
        ref = (Z ** 2).sum(axis=0)
        row.update({"rsolve3_batch_ms": t_rs, "old_route_ms": t_rs * m / 32, "speedup": t_rs * m / 32 / t_lev,
                    "max_abs_diff_32": float(np.max(np.abs(lev[pick] - ref)))})
        old = ""
    except pkg.StmmqrError as e:
        if e.code != -3:
            raise
        old = " old route: refused"
    plan.close()
    print(f"{name} " + " ".join(f"{a} {b:.4g}" for a, b in row.items()) + old, flush=True)
