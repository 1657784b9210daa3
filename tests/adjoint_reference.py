"""The yardstick of the adjoint of the least-squares solve (stmmqr_ls_adjoint): a dense numpy adjoint, restricted to a given live set.

With C = [W A; D] (plain: C = A), Bt = [W B; 0], x the solution and xbar its cotangent:
    z = (C_live' C_live)^-1 xbar_live (zero on dead columns), by R^-1 R^-T of a dense QR of C(:, live) plus one refinement step,
    rt = Bt - C x, ut = C z, G = rt z' - ut x' (the gradient with respect to every entry of C, dense),
    Axbar[p] = w_i G[i, j], Bbar = w o ut[:m], wbar_i = 2 sum_k rt[i,k] ut[i,k] / w_i (0 where w_i = 0), Dbar_j = G[m + j, j],
    dbar_j = sqrt(lam) Dbar_j, lambdabar = -sum_j s_j^2 sum_k x[j,k] z[j,k].
tests/test_adjoint_cpu.py validates it against central differences of numpy.linalg.lstsq and against torch autograd of the dense
normal equations; tests/test_gpu_adjoint.py holds the device against it.

The bars (bars()): delta = solve_tol(kappa, floor=0) is the relative error the project allows a solution through factors of
condition kappa = cond_2(C(:, live)); the device's z carries it, x is the same array on both sides.  Propagated, 2-norms:
    g       delta sum_k (|rt_k| |z_k| + |ut_k| |x_k| + |C|_2 |x_k| |z_k|)          (the issue's bar; Axbar: times |w_i|, Dbar as it is)
    Bbar    delta |w_i| |C|_2 |z_k|                                                  (ut_k = C z_k)
    wbar    (2 / |w_i|) delta sum_k |rt_k| (|ut_k| + |C|_2 |z_k|)
    dbar    sqrt(lam) times the bar of g;    lambdabar    delta sum_j s_j^2 sum_k |x_k| |z_k|  (at most max s^2 times that)
"""
import numpy as np
import scipy.sparse as sp

from stmmqr_testlib import solve_tol


def columns_of(n, Ap):
    return np.repeat(np.arange(n), np.diff(np.asarray(Ap, np.int64)))


def dense_c(m, n, Ap, Ai, Ax, w=None, D=None):
    """the dense C: A (w, D None), or [W A; D]"""
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n)).toarray()
    if w is not None:
        A = np.asarray(w)[:, None] * A
    return A if D is None else np.vstack([A, np.diag(D)])


def dense_bt(B, w, n, damped):
    B = np.asarray(B, float).reshape(B.shape[0], -1)
    top = B if w is None else np.asarray(w)[:, None] * B
    return np.vstack([top, np.zeros((n, B.shape[1]))]) if damped else top


def basic_solution(C, Bt, live):
    """argmin |C(:, live) y - Bt|, zero on the dead columns"""
    X = np.zeros((C.shape[1], Bt.shape[1]))
    if len(live):
        X[live] = np.linalg.lstsq(C[:, live], Bt, rcond=None)[0]
    return X


def normal_solve(C, V, live, refine=1):
    """(C_live' C_live)^-1 V_live, zero on dead columns: R^-1 R^-T of a dense QR and `refine` refinement steps"""
    Z = np.zeros_like(V, dtype=float)
    if not len(live):
        return Z
    Cl = C[:, live]
    R = np.linalg.qr(Cl, mode="r")
    rr = lambda v: np.linalg.solve(R, np.linalg.solve(R.T, v))                                               # noqa: E731
    zl = rr(V[live])
    for _ in range(refine):
        zl = zl + rr(V[live] - Cl.T @ (Cl @ zl))
    Z[live] = zl
    return Z


def adjoint(m, n, Ap, Ai, Ax, B, X, Xbar, live=None, w=None, d=None, lam=None, refine=1):
    """every gradient of the formulas above as a dict; damped when lam is not None (D = sqrt(lam) * d, d None = all 1).  X, Xbar
    n x nrhs; live: the live columns (None: all)."""
    damped = lam is not None
    live = np.arange(n) if live is None else np.asarray(live, np.int64)
    X = np.asarray(X, float).reshape(n, -1)
    Xbar = np.asarray(Xbar, float).reshape(n, -1)
    s = None if not damped else (np.ones(n) if d is None else np.asarray(d, float))
    D = None if not damped else np.sqrt(lam) * s
    C = dense_c(m, n, Ap, Ai, Ax, w, D)
    Bt = dense_bt(B, w, n, damped)
    Z = normal_solve(C, Xbar, live, refine)
    rt, ut = Bt - C @ X, C @ Z
    G = rt @ Z.T - ut @ X.T
    cols = columns_of(n, Ap)
    wv = np.ones(m) if w is None else np.asarray(w, float)
    out = {"C": C, "Bt": Bt, "Z": Z, "rt": rt, "ut": ut, "G": G, "live": live,
           "Axbar": wv[Ai] * G[Ai, cols], "Bbar": wv[:, None] * ut[:m]}
    if damped:
        rtu = np.sum(rt[:m] * ut[:m], axis=1)
        out["wbar"] = np.where(wv == 0, 0.0, 2.0 * rtu / np.where(wv == 0, 1.0, wv))
        out["Dbar"] = G[m + np.arange(n), np.arange(n)]
        out["dbar"] = np.sqrt(lam) * out["Dbar"]
        out["lambdabar"] = float(-np.sum(s ** 2 * np.sum(X * Z, axis=1)))
        out["s"] = s
    return out


def bars(ref, X, m, w=None, lam=None):
    """the allowed |error| per quantity (module docstring) and kappa; scalars, or arrays over the rows where w enters"""
    C, Z, rt, ut, live = ref["C"], ref["Z"], ref["rt"], ref["ut"], ref["live"]
    X = np.asarray(X, float).reshape(C.shape[1], -1)
    kappa = float(np.linalg.cond(C[:, live])) if len(live) else 1.0
    delta = solve_tol(kappa, floor=0)
    nc = float(np.linalg.norm(C, 2))
    nx, nz = np.linalg.norm(X, axis=0), np.linalg.norm(Z, axis=0)
    nrt, nut = np.linalg.norm(rt, axis=0), np.linalg.norm(ut, axis=0)
    g = delta * float(np.sum(nrt * nz + nut * nx + nc * nx * nz))
    wv = np.ones(m) if w is None else np.abs(np.asarray(w, float))
    out = {"kappa": kappa, "delta": delta, "g": g, "Axbar_rows": g * wv, "Bbar": delta * nc * wv[:, None] * nz[None, :]}
    if lam is not None:
        out["wbar"] = 2.0 * delta * float(np.sum(nrt * (nut + nc * nz))) / np.where(wv == 0, 1.0, wv)
        out["Dbar"] = g
        out["dbar"] = np.sqrt(lam) * g
        out["lambdabar"] = delta * float(np.max(ref["s"] ** 2)) * float(np.sum(nx * nz))
    return out


def loss_by_lstsq(m, n, Ap, Ai, Ax, B, Xbar, w=None, d=None, lam=None):
    """L = <Xbar, x> with x = numpy.linalg.lstsq of the dense problem: what central differences are taken of"""
    damped = lam is not None
    D = None if not damped else np.sqrt(lam) * (np.ones(n) if d is None else np.asarray(d, float))
    C = dense_c(m, n, Ap, Ai, Ax, w, D)
    X = np.linalg.lstsq(C, dense_bt(B, w, n, damped), rcond=None)[0]
    return float(np.sum(np.asarray(Xbar, float).reshape(n, -1) * X))
