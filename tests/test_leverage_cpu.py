"""Leverages from the blocks of the selected inverse, host half (no GPU): the pair sums of tests/leverage_reference.py on the CPU
oracle's factorizations -- every pair of every row is found in the block of the front of its earlier column -- against the row sums of
Q1^2 of a dense QR of the live columns, the ncol cut on [A B], and the refusal of a null plan / object by the four entry points
through the C ABI.  This pins the lookups that csrc/stmmqr_leverage.hip restates on the device."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

from leverage_reference import dense_leverages, leverages
from selinv_reference import to_caller_order
from stmmqr_testlib import Symbolic, load_golden, scalar, solve_tol

PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
NAMES = ["syn_chain", "syn_star", "syn_grid2d", "syn_grid3d", "syn_rand60x40", "syn_wide5x8", "syn_dupcol", "syn_emptycol",
         "syn_rankdef_grid", "dwt_992"]                      # (= tests/test_selinv_cpu.py::NAMES)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def live_columns(S, N, n):
    """live mask of the first n columns, the caller's column order"""
    q = np.asarray(S.Qfill[:n]) if S.Qfill is not None else np.arange(n)
    live = np.zeros(n, bool)
    live[q[np.asarray(N.Rdead[:n]) == 0]] = True
    return live


def judge(h, A, live, label):
    """the three checks of a set of leverages against the dense reference; bound: 3 solve_tol(cond(A_live)), absolute"""
    m = A.shape[0]
    rank = int(live.sum())
    ref = dense_leverages(A, live)
    kappa = float(np.linalg.cond(A[:, live])) if rank else 1.0
    bound = 3 * solve_tol(kappa)
    diff = float(np.max(np.abs(np.asarray(h, float) - ref), initial=0.0))
    total = float(np.sum(h))
    print(f"\n[leverage cpu] {label}: rank {rank}/{live.size} cond {kappa:.2e} max |h - rowsums(Q1^2)| {diff:.2e} |sum h - rank| "
          f"{abs(total - rank):.2e} (bound {bound:.2e})")
    assert diff <= bound
    assert abs(total - rank) <= m * bound
    assert np.all(h >= -bound) and np.all(h <= 1 + bound)


@pytest.mark.parametrize("name", NAMES)
def test_pair_sums_match_the_dense_projector(oracle, name):
    g = load_golden(name)
    S = Symbolic(g)
    m, n = int(S.m), int(S.n)
    Ap, Ai, Ax = g["in_Ap"], g["in_Ai"], g["in_Ax"]
    N = oracle.factorize(S, Ap, Ai, Ax, scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    h, Z = leverages(S, N, m, Ap, Ai, Ax)                    # (asserts that every pair of every row is found)
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n)).toarray()
    judge(h, A, live_columns(S, N, n), name)
    # the diagonal entries are the variances
    for k in range(0, n, max(1, n // 7)):
        assert Z.entry(k, k) == Z.var[k]
    for f in range(int(S.nf)):
        p1, fn = int(S.Rp[f]), int(S.Rp[f + 1] - S.Rp[f])
        assert np.all(np.diff(S.Rj[p1:p1 + fn]) > 0), "Rj is not ascending inside a front"


@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_rankdef_grid", "syn_grid2d"])
@pytest.mark.parametrize("nrhs", [1, 3])
def test_ncol_cut_on_the_augmented_factorization(pkg, oracle, name, nrhs):
    """[A B] factorized with ntol = n: cut at ncol = n, the leverages are those of A alone"""
    g = load_golden(name)
    m, n = int(scalar(g, "in_m")), int(scalar(g, "in_n"))
    Ap, Ai, Ax, tol = g["in_Ap"], g["in_Ai"], g["in_Ax"], float(scalar(g, "in_tol"))
    L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs, tol=tol, symbolic_only=True)
    try:
        sym = L.symbolic()
    finally:
        L.close()
    S = Symbolic({"sym_" + k: (v if isinstance(v, np.ndarray) else np.array([v])) for k, v in sym.items()})
    B = np.asfortranarray(np.random.default_rng(5).standard_normal((m, nrhs)))
    Bp = np.concatenate([Ap, Ap[-1] + m * np.arange(1, nrhs + 1)]).astype(np.int64)
    Bi = np.concatenate([Ai, np.tile(np.arange(m, dtype=np.int64), nrhs)])
    Bx = np.concatenate([Ax, B.reshape(-1, order="F")])
    N = oracle.factorize(S, Bp, Bi, Bx, tol, n)
    h, Z = leverages(S, N, m, Bp, Bi, Bx, ncol=n)
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n)).toarray()
    live = live_columns(S, N, n)
    judge(h, A, live, f"{name} nrhs {nrhs}")
    assert not np.any(np.asarray(to_caller_order(S, Z.var), float)[~live])


def test_null_plan_and_null_object_are_refused(pkg):
    lib = pkg.lib
    buf, idx = np.zeros(4), np.zeros(4, np.int64)
    calls = [
        (lib.stmmqr_plan_leverage, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int], (None, 4, buf.ctypes.data, None, 0)),
        (lib.stmmqr_plan_covariance_entries, [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
         (None, 4, 4, idx.ctypes.data, idx.ctypes.data, buf.ctypes.data, 0)),
        (lib.stmmqr_ls_leverage, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int], (None, buf.ctypes.data, None, 0)),
        (lib.stmmqr_ls_covariance_entries, [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
         (None, 4, idx.ctypes.data, idx.ctypes.data, buf.ctypes.data, 0)),
    ]
    for fn, argtypes, args in calls:
        fn.argtypes = argtypes
        assert fn(*args) == -4                               # STMMQR_ERR_INVALID
        assert lib.stmmqr_last_error().decode() != ""
    assert not buf.any()
