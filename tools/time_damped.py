"""Damped, weighted least squares min |W (A x - b)|^2 + lambda |x|^2 for eight lambda = 1e-4 .. 1e3 on one fixture, one right-hand
side, three ways:
  damped      ONE DampedLeastSquares, solve_dev per lambda with A's values, w, b and x resident on the device: wall ms of the call,
              device ms of building the values (damped_info: builder kernels + the tolerance's norm, events), of the factorization
              and of the back substitution.  The wall time holds the one host wait of the default tolerance.
  plain       LeastSquares.solve_dev on the same matrix (no damping, no weights, values on the device): what the n extra rows and
              the builder cost.  (Its copy back of the values for the default tolerance is part of its wall time.)
  new object  the only route without the damped mode: [W A; D] and [W b; 0] built on the host and a NEW LeastSquares on them per
              lambda -- host build, create (analysis, plan), solve (upload, factorization, back substitution), wall ms each.  It
              gets the same column order GIVEN, so that all three routes factorize in one order; what COLAMD on the explicit matrix
              costs a caller who has no order at hand is one more line (default ordering, lambda = 1).
Every object is created with the default tolerance (tol = -2), the path that computes the largest column norm at every solve: on
the device for the damped object, on the host (after a copy back of the device values) for the plain one.
One call of each kind warms up first (the first factorization sets the pattern and sizes the arenas).
usage: python tools/time_damped.py [fixture]"""
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
tol = -2.0
Ap, Ai, Ax = g["in_Ap"].astype(np.int64), g["in_Ai"].astype(np.int64), g["in_Ax"].astype(np.float64)
m, n = S.m, S.n
Q = S.Qfill if S.Qfill is not None else np.arange(n)
LAMBDAS = [10.0 ** e for e in range(-4, 4)]
rng = np.random.default_rng(1)
b = rng.standard_normal(m)
w = rng.uniform(0.5, 2.0, m)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def explicit(lam):
    """[W A; sqrt(lam) I] and [W b; 0] on the host, in the damped object's layout"""
    cols = np.repeat(np.arange(n), np.diff(Ap))
    Cp = Ap + np.arange(n + 1)
    Ci, Cx = np.zeros(Ax.size + n, np.int64), np.zeros(Ax.size + n)
    pos = np.arange(Ax.size) + cols
    Ci[pos], Cx[pos] = Ai, w[Ai] * Ax
    Ci[Ap[1:] + np.arange(n)], Cx[Ap[1:] + np.arange(n)] = m + np.arange(n), np.sqrt(lam)
    return Cp, Ci, Cx, np.concatenate([w * b, np.zeros(n)])


dAx, dw, db = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (Ax, w, b))
dx = torch.zeros(n, dtype=torch.float64, device="cuda")
print(f"{name}: m {m} n {n} nz {Ax.size}, one right-hand side, default tolerance (tol = {tol})", flush=True)

# ---- plain ----
P = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=1, ordering=3, Quser=Q, tol=tol)
P.solve_dev(db.data_ptr(), dx.data_ptr(), ax_ptr=dAx.data_ptr())
rows = []
for _ in range(5):
    ms, _ = wall(lambda: P.solve_dev(db.data_ptr(), dx.data_ptr(), ax_ptr=dAx.data_ptr()))
    i = P.info
    rows.append((ms, i["ms_factorize"], i["ms_solve"]))
r = np.median(np.array(rows), axis=0)
print(f"plain LeastSquares.solve_dev: wall {r[0]:.2f} ms, factorization {r[1]:.2f} ms, back substitution {r[2]:.2f} ms (device), "
      f"device {P.info['device_bytes'] / 1e9:.3f} GB, nf {int(P.info['nf'])}, flops {P.info['flops']:.4g}, tol used {P.info['tol']:.6e}", flush=True)
P.close()

# ---- damped ----
t0 = time.perf_counter()
D = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=1, ordering=3, Quser=Q, tol=tol)
create_ms = (time.perf_counter() - t0) * 1e3
solve = lambda lam: D.solve_dev(db.data_ptr(), dx.data_ptr(), ax_ptr=dAx.data_ptr(), w_ptr=dw.data_ptr(), lam=lam)     # noqa: E731
solve(1.0)
print(f"damped: create {create_ms:.1f} ms once; device {D.info['device_bytes'] / 1e9:.3f} GB ({D.damped_info['damped_bytes'] / 1e6:.2f} MB "
      f"of it the damped mode's own), nf {int(D.info['nf'])}", flush=True)
damped = {}
for lam in LAMBDAS:
    rows = []
    for _ in range(3):
        ms, resid = wall(lambda: solve(lam))
        i = D.info
        rows.append((ms, D.damped_info["ms_build"], i["ms_factorize"], i["ms_solve"]))
    r = np.median(np.array(rows), axis=0)
    damped[lam] = r[0]
    print(f"damped lambda {lam:.0e}: wall {r[0]:.2f} ms, build {r[1]:.3f} ms, factorization {r[2]:.2f} ms, back substitution {r[3]:.2f} ms "
          f"(device); rank {int(i['rank'])}/{n} retries {int(i['retries'])} flops {i['flops']:.4g} tol used {i['tol']:.6e} resid {resid[0]:.6e}", flush=True)
assert D.info["analyses"] == 1 and D.info["plans"] == 1
D.close()

# ---- a new object per lambda ----
Cp, Ci, Cx, be = explicit(1.0)
given = dict(ordering=3, Quser=Q)
F = pkg.LeastSquares(m + n, n, Cp, Ci, Cx, nrhs=1, tol=tol, **given)
F.solve(be)
F.close()
slower = []
for lam in LAMBDAS:
    t_build, (Cp, Ci, Cx, be) = wall(lambda: explicit(lam))
    t_create, F = wall(lambda: pkg.LeastSquares(m + n, n, Cp, Ci, Cx, nrhs=1, tol=tol, **given))
    t_solve, (x, resid) = wall(lambda: F.solve(be))
    i = F.info
    F.close()
    total = t_build + t_create + t_solve
    if damped[lam] > total:
        slower.append(lam)
    print(f"new object lambda {lam:.0e}: wall {total:.1f} ms = host build {t_build:.1f} + create {t_create:.1f} + solve {t_solve:.1f} "
          f"(factorization {i['ms_factorize']:.2f} ms on the device, flops {i['flops']:.4g}); damped / new object {damped[lam] / total:.3f}; resid {resid[0]:.6e}",
          flush=True)
print("damped slower than a new object at lambda: " + (", ".join(f"{v:.0e}" for v in slower) if slower else "none"), flush=True)
Cp, Ci, Cx, be = explicit(1.0)
t_create, F = wall(lambda: pkg.LeastSquares(m + n, n, Cp, Ci, Cx, nrhs=1, tol=tol))
t_solve, _ = wall(lambda: F.solve(be))
i = F.info
F.close()
print(f"new object, default ordering (COLAMD of the explicit matrix), lambda 1e+00: create {t_create:.1f} ms + solve {t_solve:.1f} ms "
      f"(factorization {i['ms_factorize']:.2f} ms on the device, flops {i['flops']:.4g}, nf {int(i['nf'])})", flush=True)
