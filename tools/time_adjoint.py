"""The adjoint of the least-squares solve (stmmqr_ls_adjoint) next to the solve it belongs to, on one fixture with every argument
resident on the device: nrhs 1 and 32, refine 0 and 1, the plain object and the damped one (lambda = 1, row weights).
Per line, medians of 3 calls after one warm-up:
  solve       wall ms of solve_dev, device ms of its factorization and back substitution
  adjoint     wall ms of adjoint_dev with every output asked for; device ms of the call (info), of its two triangular passes alone
              (info), and of k_lsa_entries with the staging of its four vectors: the device ms of the call minus those of the same
              call with Axbar and Dbar not asked for (the library has no clock around that kernel alone)
usage: python tools/time_adjoint.py [fixture]"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stmmqr_testlib import Symbolic, load_golden  # noqa: E402

import torch  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "xenon1_colamd_standin"
g = load_golden(name)
S = Symbolic(g)
Ap, Ai, Ax = g["in_Ap"].astype(np.int64), g["in_Ai"].astype(np.int64), g["in_Ax"].astype(np.float64)
m, n = S.m, S.n
Q = S.Qfill if S.Qfill is not None else np.arange(n)
rng = np.random.default_rng(1)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median(f, reps=3):
    f()
    return np.median(np.array([f() for _ in range(reps)]), axis=0)


print(f"{name}: m {m} n {n} nz {Ax.size}; arguments on the device; medians of 3 after one warm-up", flush=True)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                                            # noqa: E731
dAx, dw = dev(Ax), dev(rng.uniform(0.5, 2.0, m))
for damped in (False, True):
    for k in (1, 32):
        dB, dXbar = dev(rng.standard_normal((k, m))), dev(rng.standard_normal((k, n)))                       # (column-major m x k, n x k)
        dX = torch.zeros((k, n), dtype=torch.float64, device="cuda")
        gA, gB = torch.zeros(Ax.size, dtype=torch.float64, device="cuda"), torch.zeros((k, m), dtype=torch.float64, device="cuda")
        gw, gD = torch.zeros(m, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
        cls = pkg.DampedLeastSquares if damped else pkg.LeastSquares
        L = cls(m, n, Ap, Ai, Ax, nrhs=k, ordering=3, Quser=Q)
        if damped:
            solve = lambda: L.solve_dev(dB.data_ptr(), dX.data_ptr(), ax_ptr=dAx.data_ptr(), w_ptr=dw.data_ptr(), lam=1.0)   # noqa: E731
            adj = lambda refine, entries: L.adjoint_dev(                                                     # noqa: E731
                dX.data_ptr(), dXbar.data_ptr(), w_ptr=dw.data_ptr(), axbar_ptr=gA.data_ptr() if entries else None, bbar_ptr=gB.data_ptr(),
                wbar_ptr=gw.data_ptr(), dbar_ptr=gD.data_ptr() if entries else None, refine=refine)
        else:
            solve = lambda: L.solve_dev(dB.data_ptr(), dX.data_ptr(), ax_ptr=dAx.data_ptr(), resid=False)   # noqa: E731
            adj = lambda refine, entries: L.adjoint_dev(dX.data_ptr(), dXbar.data_ptr(), axbar_ptr=gA.data_ptr() if entries else None,   # noqa: E731
                                                        bbar_ptr=gB.data_ptr(), refine=refine)

        def one_solve():
            ms, _ = wall(solve)
            i = L.info
            return ms, i["ms_factorize"], i["ms_solve"]

        s = median(one_solve)
        kind = "damped lambda 1" if damped else "plain"
        print(f"{kind} nrhs {k}: solve wall {s[0]:.2f} ms, factorization {s[1]:.2f} ms, back substitution {s[2]:.2f} ms (device); "
              f"rank {int(L.info['rank'])}/{n}", flush=True)
        for refine in (0, 1):
            def one_adjoint(entries=True):
                ms, info = wall(lambda: adj(refine, entries))
                return ms, info["ms"], info["ms_passes"], info["normal_resid"]

            a = median(one_adjoint)
            b = median(lambda: one_adjoint(False))
            print(f"{kind} nrhs {k} refine {refine}: adjoint wall {a[0]:.2f} ms, device {a[1]:.2f} ms, of it the two triangular passes "
                  f"{a[2]:.2f} ms ({100 * a[2] / a[1]:.0f}%) and k_lsa_entries with its staging {a[1] - b[1]:.2f} ms; normal residual {a[3]:.1e}; "
                  f"adjoint / solve {a[0] / s[0]:.2f} (wall)", flush=True)
        assert L.info["analyses"] == 1 and L.info["plans"] == 1
        print(f"{kind} nrhs {k}: device bytes of the object {L.info['device_bytes'] / 1e9:.3f} GB", flush=True)
        L.close()
