"""The minimum-norm least-squares path on rank-deficient factors, timed part by part:
  build                  device ms of the three parts of the first call after a factorization (events on the plan's stream): the basis
                         N (d unit vectors through R x and R \\ in batches), the Gram matrix N'N, its Cholesky factorization
  project x1, x32        (I - N G^-1 N')^2 X for 1 and 32 vectors with device pointers in and out on the basis held: the wall clock of
                         a call that ends in a synchronize
  solve                  one stmmqr_plan_solve of the same plan (host arrays), next to them
A warm plan; 3 calls to warm up, then calls until 0.3 s and at least 10 of them have passed -- median (min) in ms; the build is
repeated after a new factorization each time (5 times: median).
usage: python tools/time_lsminnorm.py [fixture ...]"""
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
capi = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd.capi")


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


for name in (sys.argv[1:] or ["cvxqp3", "lns_3937"]):
    g = load_golden(name)
    S = Symbolic(g)
    m, n = S.m, S.n
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    plan = pkg.HipQR(sym)
    plan.set_pattern(g["in_Ap"], g["in_Ai"])
    builds = []
    for _ in range(6):
        st = plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
        plan.project_minnorm(np.ones(n))                           # builds N, G and L
        builds.append(plan.nullspace_times())
    builds = builds[1:]
    med = {k: float(np.median([b[k] for b in builds])) for k in ("N", "gram", "cholesky")}
    _, info = plan.project_minnorm(np.ones(n), with_info=True)
    d = info["d"]
    rng = np.random.default_rng(1)
    B = np.asfortranarray(rng.standard_normal((m, 1)))
    dX = pkg.device_alloc(8 * n * 32)
    Xh = np.asfortranarray(rng.standard_normal((n, 32)))
    pkg.device_copy(dX, Xh.ctypes.data, 8 * n * 32)
    proj = lambda k: capi._check(capi.lib.stmmqr_plan_project_minnorm(plan._h, n, dX, n, k, 0, 1, None), "stmmqr_plan_project_minnorm")
    fmt = lambda mm: f"{mm[0]:.3f} ({mm[1]:.3f})"
    r = timed([lambda: proj(1), lambda: proj(32), lambda: plan.solve(B)])
    pkg.device_free(dX)
    held = plan.device_bytes()
    plan.close()
    print(f"{name} m {m} n {n} nf {S.nf} d {d} fact_ms {st['ms_total']:.1f} | build: N {med['N']:.3f} ms, Gram {med['gram']:.3f} ms, "
          f"Cholesky {med['cholesky']:.3f} ms (device) | project x1 {fmt(r[0])} ms, x32 {fmt(r[1])} ms | solve x1 {fmt(r[2])} ms | "
          f"|N|_F {info['norm_N']:.3e}, min diag L {info['min_diag_L']:.6f}, |N'x| / (|N| |x|) {info['orth']:.1e}, device bytes {held / 1e6:.1f} MB",
          flush=True)
