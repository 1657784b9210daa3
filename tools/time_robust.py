"""Robust least squares on one fixture, plain object and damped object (lambda = 1e-2), 10 % of b replaced by gross outliers, Huber
with the MAD scale:
  reweighting  device ms of one reweighting (robust_weights_dev with everything resident), split by events into the residual (with
               |w0 o r|), the selection and the weights, next to the device ms of the solve it belongs to (factorization + back
               substitution of the object's info)
  loop         wall ms of solve_robust_dev (w, r, a, x never leave the device) next to the same loop written in Python with
               robust_weights() and solve(): w goes through the host every iteration, and on the plain object so do the weighted values
Both loops run the same number of solves (a fixed max_iter, rtol = 0) from the same start.  One call of each kind warms up first.
usage: python tools/time_robust.py [fixture] [solves]"""
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
SOLVES = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LAM = 1e-2
g = load_golden(name)
S = Symbolic(g)
Ap, Ai, Ax = g["in_Ap"].astype(np.int64), g["in_Ai"].astype(np.int64), g["in_Ax"].astype(np.float64)
m, n = S.m, S.n
Q = S.Qfill if S.Qfill is not None else np.arange(n)
rng = np.random.default_rng(1)
cols = np.repeat(np.arange(n), np.diff(Ap))
xt = rng.standard_normal(n)
b = np.zeros(m)
np.add.at(b, Ai, Ax * xt[cols])
b += 1e-3 * rng.standard_normal(m)
bad = rng.choice(m, m // 10, replace=False)
b[bad] = 100.0 * rng.choice([-1.0, 1.0], bad.size)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def python_loop(L, damped):
    """the driver's loop with w through the host (rtol = 0: SOLVES solves)"""
    w = np.ones(m)
    x = None
    for it in range(SOLVES):
        if it > 0:
            w = L.robust_weights(b, x, loss="huber")[1]
        x = L.solve(b, w=w, lam=LAM)[0] if damped else L.solve(w * b, Ax=w[Ai] * Ax)[0]
    return x


print(f"{name}: m {m} n {n} nz {Ax.size}, Huber, MAD scale, {bad.size} rows of b replaced by +-100, {SOLVES} solves per loop", flush=True)
db = torch.from_numpy(b).cuda()
dx, dw, dr = (torch.zeros(k, dtype=torch.float64, device="cuda") for k in (n, m, m))
for damped in (False, True):
    cls = pkg.DampedLeastSquares if damped else pkg.LeastSquares
    extra = dict(lam=LAM) if damped else {}
    label = "damped (lambda 1e-2)" if damped else "plain"
    L = cls(m, n, Ap, Ai, Ax, nrhs=1, ordering=3, Quser=Q)
    loop = lambda: L.solve_robust_dev(db.data_ptr(), dx.data_ptr(), w_ptr=dw.data_ptr(), loss="huber", max_iter=SOLVES, rtol=0.0, **extra)  # noqa: E731
    info = loop()
    x_dev = dx.cpu().numpy().copy()
    # one reweighting from the loop's x, everything resident
    rows = []
    for _ in range(7):
        L.robust_weights_dev(db.data_ptr(), dx.data_ptr(), r_ptr=dr.data_ptr(), w_ptr=dw.data_ptr(), loss="huber")
        t = L.robust_times()
        rows.append((t["residual"], t["selection"], t["weights"], t["total"]))
    r = np.median(np.array(rows), axis=0)
    i = L.info
    print(f"{label}: one reweighting {r[3]:.3f} ms on the device = residual {r[0]:.3f} + selection {r[1]:.3f} + weights {r[2]:.3f}; the solve it "
          f"belongs to: factorization {i['ms_factorize']:.2f} ms + back substitution {i['ms_solve']:.2f} ms; the feature holds "
          f"{info['robust_bytes'] / 1e6:.2f} MB of {i['device_bytes'] / 1e9:.3f} GB", flush=True)
    t_dev = np.median([wall(loop)[0] for _ in range(3)])
    info = loop()
    python_loop(L, damped)
    t_py = np.median([wall(lambda: python_loop(L, damped))[0] for _ in range(3)])
    x_py = python_loop(L, damped)
    print(f"{label}: solve_robust {t_dev:.1f} ms wall for {info['solves']} solves ({info['ms_reweight']:.3f} ms of it the reweightings on the "
          f"device); the Python loop with w through the host {t_py:.1f} ms; ratio {t_py / t_dev:.3f}; same bits: "
          f"{bool(np.array_equal(x_py, x_dev))}; sigma {info['sigma']:.4g}, |x - x_true|_inf {np.abs(x_dev - xt).max():.3g}", flush=True)
    assert L.info["analyses"] == 1 and L.info["plans"] == 1
    L.close()
