"""New values of the same pattern: a fresh SparseQR on them (before stmmqr_sparseqr_refactorize the only route: singletons, COLAMD,
analysis, plan, arenas and the factorization again) next to SparseQR.refactorize on the object that exists, from a host array and
from a device pointer.  Per fixture:
  fresh        ana_seconds and fac_seconds of a new object on the new values (stmmqr_sparseqr_info), median of `reps` objects
  refactorize  wall seconds of the call (refactor_info[3]), device ms of the value kernels ([1]) and of the factorization ([2]),
               median of `reps` calls after one to warm up (the first call allocates the staging buffer and uploads the maps)
The values alternate between Ax (1 + 0.25 cos(0.7 p + 0.3)) and Ax, so that every call has work to do.
usage: python tools/time_refactor.py [fixture ...]"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stmmqr_testlib import load_golden  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
REPS = 5


def matrix(name):
    g = load_golden(name)
    if "A_p" in g:
        return int(g["A_m"][0]), int(g["A_n"][0]), g["A_p"], g["A_i"], g["A_x"]
    return int(g["in_m"][0]), int(g["in_n"][0]), g["in_Ap"], g["in_Ai"], g["in_Ax"]


def med(rows):
    return np.median(np.array(rows), axis=0)


import torch  # noqa: E402

for name in (sys.argv[1:] or ["bcsstk14", "bayer10", "ex18", "xenon1_colamd_standin"]):
    m, n, Ap, Ai, Ax = matrix(name)
    Ax2 = Ax * (1.0 + 0.25 * np.cos(0.7 * np.arange(Ax.size) + 0.3))
    rx = pkg.relax_for_qr(n, int(Ap[-1]))
    fresh = []
    for _ in range(REPS):
        F = pkg.SparseQR(m, n, Ap, Ai, Ax2, relax=rx)
        i = F.info
        fresh.append((i["ana_seconds"], i["fac_seconds"], i["ms_device"]))
        n1 = int(i["n1cols"])
        F.close()
    Q = pkg.SparseQR(m, n, Ap, Ai, Ax, relax=rx)
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (Ax2, Ax)]
    torch.cuda.synchronize()
    host, devp = [], []
    for k in range(2 * (REPS + 1)):
        Q.refactorize((Ax2, Ax)[k % 2])
        r = Q.refactor_info
        if k >= 2:
            host.append((r[3], r[1], r[2]))
    for k in range(2 * (REPS + 1)):
        Q.refactorize(dev_ptr=dev[k % 2].data_ptr())
        r = Q.refactor_info
        if k >= 2:
            devp.append((r[3], r[1], r[2]))
    r = Q.refactor_info
    Q.close()
    f, h, d = med(fresh), med(host), med(devp)
    print(f"{name} m {m} n {n} nz {Ax.size} n1cols {n1} | fresh: ana {f[0] * 1e3:.1f} ms, fac {f[1] * 1e3:.1f} ms (device {f[2]:.1f} ms) | "
          f"refactorize(host): {h[0] * 1e3:.1f} ms (values {h[1]:.3f} ms, factorization {h[2]:.1f} ms on the device) | "
          f"refactorize(device pointer): {d[0] * 1e3:.1f} ms (values {d[1]:.3f} ms, factorization {d[2]:.1f} ms) | "
          f"refactorize / fresh fac: {h[0] / f[1]:.2f} (host), {d[0] / f[1]:.2f} (device pointer); beyond the plan {r[7] / 1e6:.2f} MB", flush=True)
