"""Cases of the resident-operation pin (tests/test_gpu_resident_pin.py, tests/golden/make_resident_pin.py): every operation on the
factors resident in HBM, on plans that take each path of the host layer (dead columns and Qfill, the split Q-apply / back substitution
/ R' pass with and without the grouped T4, recycled slabs with the per-level and the whole-tree scratch, R-only plans, a plan of
[A B], the plan of a transpose), with 1 and 33 right-hand sides (STMMQR_RHS_BATCH defaults to 32: a full batch and a ragged one).

run_case(pkg, name) -> {key: array}: per output one SHA-256 digest per column (after + 0.0: the sign of a zero is not pinned) and,
so that a failure shows how far off it is, the first HEAD entries of column 0 as numbers (of the one-vector call; column 0 of the
batch of 33 is the same right-hand side); the scalars (rank, the condest's out[0..7], the seminormal solve's info);
plan.device_bytes() after the factorization and after all operations.  pack / unpack: a case's entries as four arrays of the pin
file (an .npz entry costs more than a digest, and the file has to stay small)."""
import hashlib
import importlib
import os

import numpy as np
import scipy.sparse as sp

from stmmqr_testlib import Symbolic, load_golden, scalar

I64 = np.int64
HEAD = 128                     # entries of column 0 kept as numbers (the whole column where it is no longer)
NRHS = (1, 33)
SPLIT = {"STMMQR_QBIG_MIN": "1", "STMMQR_RTBIG_MIN": "1"}

# name -> (kind, fixture, environment while the plan is made and used, keepH)
CASES = {
    "rankdef_default": ("plan", "syn_rankdef_grid", {}, 1),
    "rankdef_split_t4": ("plan", "syn_rankdef_grid", SPLIT, 1),
    "rankdef_split_per_panel": ("plan", "syn_rankdef_grid", {**SPLIT, "STMMQR_QT4": "0"}, 1),
    "dwt992_recycle_level_scratch": ("plan", "dwt_992", {"STMMQR_RECYCLE": "2", "STMMQR_RESIDENT_CACHE": "0"}, 1),
    "dwt992_recycle_tree_scratch": ("plan", "dwt_992", {"STMMQR_RECYCLE": "2", "STMMQR_RESIDENT_CACHE": "1"}, 1),
    "dwt992_r_only": ("plan", "dwt_992", {}, 0),
    "grid2d_least_squares": ("ls", "syn_grid2d", {}, 0),
    "grid2d_transpose_minnorm": ("transpose", "syn_grid2d", {}, 1),
}


def digests(Y):
    """(ncol, 32) uint8: SHA-256 of every column of Y (a vector is one column)"""
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y.reshape(Y.shape[0], -1, order="F") if Y.ndim else Y.reshape(1, 1)
    return np.array([np.frombuffer(hashlib.sha256((np.ascontiguousarray(Y[:, j]) + 0.0).tobytes()).digest(), np.uint8)
                     for j in range(Y.shape[1])]).reshape(Y.shape[1], 32)


def keep(out, key, Y, numbers=True):
    Y = np.asarray(Y, dtype=np.float64)
    out[key + "/sha"] = digests(Y)
    if numbers:
        out[key + "/col0"] = (Y.reshape(Y.shape[0], -1, order="F")[:HEAD, 0] if Y.ndim else Y.reshape(1)) + 0.0


def pack(name, out):
    """the entries of one case as four arrays: the keys, their sizes, the digests (uint8) and everything else (float64) end to end"""
    keys = sorted(out)
    flat = [np.asarray(out[k]).ravel() for k in keys]
    u1 = [a for a in flat if a.dtype == np.uint8]
    f8 = [a.astype(np.float64) for a in flat if a.dtype != np.uint8]
    return {f"{name}/keys": np.array(keys), f"{name}/sizes": np.array([a.size for a in flat], I64),
            f"{name}/u1": np.concatenate(u1) if u1 else np.zeros(0, np.uint8), f"{name}/f8": np.concatenate(f8) if f8 else np.zeros(0)}


def unpack(z, name):
    """{key: flat array} of one case of the pin file"""
    out, at = {}, {"u1": 0, "f8": 0}
    for k, n in zip(z[f"{name}/keys"], z[f"{name}/sizes"]):
        kind = "u1" if str(k).endswith("/sha") else "f8"
        out[str(k)] = z[f"{name}/{kind}"][at[kind]:at[kind] + int(n)]
        at[kind] += int(n)
    return out


def rhs(rows, k, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((rows, k)))


def condest(pkg, out, key, call, ncol):
    """call(out8, v) of a condest entry point with host arrays: all eight doubles of `out` and the vector"""
    capi = importlib.import_module(pkg.__name__ + ".capi")
    res, v = np.zeros(8), np.zeros(max(ncol, 1))
    rc = call(capi.lib, res.ctypes.data, v.ctypes.data)
    if rc != 0:
        raise pkg.StmmqrError(f"condest failed ({rc}): {pkg.last_error()}")
    out[key + "/out"] = res
    keep(out, key + "/v", v[:ncol])


def plan_operations(pkg, plan, out, m, n, keep_h, with_a):
    """every operation the plan allows, 1 and 33 right-hand sides"""
    for k in NRHS:
        Bm, Bn, t, one = rhs(m, k, 100 + k), rhs(n, k, 200 + k), f"k{k}", k == 1
        if keep_h:
            for method in (0, 1):
                keep(out, f"qmult{method}/{t}", plan.qmult(method, Bm), one)
            for method in (2, 3):
                keep(out, f"qmult{method}/{t}", plan.qmult(method, np.asfortranarray(Bm.T)).T, one)
            keep(out, f"solve/{t}", plan.solve(Bm), one)
            for perm in (False, True):
                keep(out, f"solve_minnorm{int(perm)}/{t}", plan.solve_minnorm(Bn, permuted=perm), one)
        for system in (0, 1):
            keep(out, f"rsolve{system}/{t}", plan.rsolve(system, Bm), one)
        for system in (2, 3):
            keep(out, f"rsolve{system}/{t}", plan.rsolve(system, Bn), one)
        for trans in (0, 1):
            for perm in (False, True):
                keep(out, f"rmult{trans}{int(perm)}/{t}", plan.rmult(Bm if trans else Bn, trans=trans, permuted=perm), one)
        if with_a:
            for trans in (0, 1):
                keep(out, f"spmv{trans}/{t}", plan.spmv(Bm if trans else Bn, trans=trans), one)
            for refine in (0, 1):
                X, info = plan.solve_seminormal(Bm, refine=refine)
                keep(out, f"seminormal{refine}/{t}", X, one)
                out[f"seminormal{refine}/{t}/info"] = np.float64(info)
    for kind in (1, 2):
        condest(pkg, out, f"condest{kind}", lambda lib, o, v: lib.stmmqr_plan_condest(plan._h, n, kind, 0, o, v, 0), n)
    keep(out, "covariance_diag", plan.covariance_diag())
    lev, var = plan.leverage(with_var=True)
    keep(out, "leverage/lev", lev)
    keep(out, "leverage/var", var)
    d = np.arange(n, dtype=I64)
    keep(out, "covariance_entries/diag", plan.covariance_entries(d, d))


def in_pattern_pairs(sym, ncol, per_front=3):
    """the first off-diagonal pairs of every front inside the pattern of the selected inverse, in the caller's column order: a pivot column of a
    front and a later column of that front's list (Super, Rp, Rj of the symbolic analysis; Qfill maps R's order to the caller's)"""
    Super, Rp, Rj = (np.asarray(sym[k], I64) for k in ("Super", "Rp", "Rj"))
    q = sym.get("Qfill")
    q = np.arange(ncol, dtype=I64) if q is None or np.size(q) == 0 else np.asarray(q, I64)
    I, J = [], []
    for f in range(int(sym["nf"])):
        cols = Rj[Rp[f]:Rp[f + 1]]
        k1 = int(Super[f])
        for k2 in cols[1:1 + per_front]:
            if k1 < ncol and k2 < ncol:
                I.append(int(q[k1])); J.append(int(q[int(k2)]))
    return np.array(I, I64), np.array(J, I64)


def run_plan_case(pkg, fixture, keep_h, out):
    g = load_golden(fixture)
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": keep_h}
    plan = pkg.HipQR(sym)
    try:
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        out["device_bytes/factorized"] = np.float64(plan.device_bytes())
        out["rank"] = np.int64(plan.result_sizes()[1])
        plan_operations(pkg, plan, out, S.m, S.n, keep_h, True)
        I, J = in_pattern_pairs(sym, S.n)
        keep(out, "covariance_entries/pairs", plan.covariance_entries(np.concatenate([I, J]), np.concatenate([J, I])))
        out["device_bytes/after"] = np.float64(plan.device_bytes())
    finally:
        plan.close()


def run_ls_case(pkg, fixture, out):
    g = load_golden(fixture)
    m, n = int(scalar(g, "in_m")), int(scalar(g, "in_n"))
    L = pkg.LeastSquares(m, n, g["in_Ap"], g["in_Ai"], g["in_Ax"], nrhs=3, tol=float(scalar(g, "in_tol")))
    try:
        X, resid = L.solve(rhs(m, 3, 303))
        keep(out, "solve/X", X)
        keep(out, "solve/resid", resid)
        out["rank"] = np.int64(L.info["rank"])
        out["device_bytes/factorized"] = np.float64(L.plan().device_bytes())
        keep(out, "variances", L.variances())
        keep(out, "leverages", L.leverages())
        sym = L.symbolic()
        I, J = in_pattern_pairs(sym, n)
        d = np.arange(n, dtype=I64)
        keep(out, "covariance", L.covariance(np.concatenate([d, I, J]), np.concatenate([d, J, I])))
        for kind in (1, 2):
            condest(pkg, out, f"condest{kind}", lambda lib, o, v: lib.stmmqr_ls_condest(L._h, kind, 0, o, v, 0), n)
        Xc, rc = L.plan().solve_carried(3)
        keep(out, "solve_carried/X", Xc)
        keep(out, "solve_carried/resid", rc)
        out["device_bytes/after"] = np.float64(L.plan().device_bytes())
    finally:
        L.close()


def run_transpose_case(pkg, fixture, out):
    g = load_golden(fixture)
    m, n = int(scalar(g, "in_m")), int(scalar(g, "in_n"))
    A = sp.csc_matrix((g["in_Ax"], g["in_Ai"], g["in_Ap"]), shape=(m, n)).T.tocsc()
    A.sort_indices()
    Ap, Ai, Ax = A.indptr.astype(I64), A.indices.astype(I64), A.data.astype(np.float64)
    sym = pkg.analyze(n, m, Ap, Ai)
    plan = pkg.HipQR(sym)
    try:
        plan.factorize(Ax, float(scalar(g, "in_tol")), m, Ap, Ai)
        out["device_bytes/factorized"] = np.float64(plan.device_bytes())
        out["rank"] = np.int64(plan.result_sizes()[1])
        for k in NRHS:
            for perm in (False, True):
                keep(out, f"solve_minnorm{int(perm)}/k{k}", plan.solve_minnorm(rhs(m, k, 400 + k), permuted=perm), k == 1)
        out["device_bytes/after"] = np.float64(plan.device_bytes())
    finally:
        plan.close()


def run_case(pkg, name):
    kind, fixture, env, keep_h = CASES[name]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    out = {}
    try:
        if kind == "plan":
            run_plan_case(pkg, fixture, keep_h, out)
        elif kind == "ls":
            run_ls_case(pkg, fixture, out)
        else:
            run_transpose_case(pkg, fixture, out)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return {k: np.asarray(v) for k, v in out.items()}
