"""Selected inversion of R'R, host half (no GPU): the front-wise recurrence of tests/selinv_reference.py -- position tables, dead
columns, the child -> parent gather, the ncol cut -- on the CPU oracle's factorizations, against sum(|R^-T e_j|^2) from
resident_reference.Factors (an independent path over the whole R), and the refusal of a null plan through the C ABI.  This pins
the maps that csrc/stmmqr_selinv.hip restates on the device."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

from resident_reference import LD, Factors
from selinv_reference import SparseR, selinv_diag, to_caller_order
from stmmqr_testlib import Symbolic, cond_probe, load_golden, scalar, solve_tol

PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
NAMES = ["syn_chain", "syn_star", "syn_grid2d", "syn_grid3d", "syn_rand60x40", "syn_wide5x8", "syn_dupcol", "syn_emptycol",
         "syn_rankdef_grid", "dwt_992"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def rt_reference(Fa):
    """(var in R's column order, live mask): |R^-T e_j|^2 over the live columns, from the whole R at once"""
    Z = Fa.rtsolve(np.eye(Fa.n))
    var = (Z ** 2).sum(axis=0)
    live = np.zeros(Fa.n, bool)
    live[Fa.pivot_col] = True
    return var, live


@pytest.mark.parametrize("name", NAMES)
def test_recurrence_matches_rtsolve(oracle, name):
    g = load_golden(name)
    S = Symbolic(g)
    N = oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    Fa = Factors(S, N)
    ref, live = rt_reference(Fa)
    var = selinv_diag(S, N)
    assert np.array_equal(live, np.asarray(N.Rdead[:S.n]) == 0)
    assert not np.any(var[~live]), "dead columns must be exactly 0"
    kappa = cond_probe(oracle, S, N)
    ratio = float(np.max(np.abs(var[live] - ref[live]) / ref[live], initial=0.0))
    print(f"\n[selinv cpu] {name}: nf {S.nf} rank {Fa.rank}/{S.n} cond_probe {kappa:.2e} max rel diff {ratio:.2e} "
          f"(allowed {3 * solve_tol(kappa):.2e})")
    assert np.all(var[live] > 0)
    assert ratio <= 3 * solve_tol(kappa)


@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_rankdef_grid", "syn_grid2d"])
@pytest.mark.parametrize("nrhs", [1, 3])
def test_ncol_cut_on_the_augmented_factorization(pkg, oracle, name, nrhs):
    """[A B] factorized with ntol = n: the recurrence cut at ncol = n gives diag((A_live' A_live)^-1) of A alone"""
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
    var = np.asarray(to_caller_order(S, selinv_diag(S, N, ncol=n)), float)
    q = np.asarray(S.Qfill[:n])
    live = np.zeros(n, bool)
    live[q[np.asarray(N.Rdead[:n]) == 0]] = True
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n)).toarray()[:, live]
    ref = np.diag(np.linalg.inv(np.asarray(A.T @ A, LD).astype(float)))
    kappa = float(np.linalg.cond(A))
    assert not np.any(var[~live])
    ratio = float(np.max(np.abs(var[live] - ref) / ref))
    print(f"\n[selinv cpu] {name} nrhs {nrhs}: rank {int(live.sum())}/{n} cond {kappa:.2e} max rel diff {ratio:.2e}")
    assert ratio <= 3 * solve_tol(kappa * kappa)            # (the reference inverts A'A in fp64: cond^2)


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "syn_dupcol", "dwt_992"])
def test_sparse_rt_solve_is_the_dense_one(oracle, name):
    """SparseR (the reference of the large fixtures in tests/test_gpu_selinv.py) does Factors.rtsolve's arithmetic: the same bits"""
    g = load_golden(name)
    S = Symbolic(g)
    N = oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    Fa, Sr = Factors(S, N), SparseR(S, N)
    assert Sr.rank == Fa.rank and Sr.pivot_col == list(Fa.pivot_col)
    B = np.random.default_rng(1).standard_normal((S.n, 3))
    assert np.array_equal(Fa.rtsolve(B)[:Fa.rank], Sr.rtsolve(B))


def test_null_plan_is_refused(pkg):
    fn = pkg.lib.stmmqr_plan_covariance_diag
    fn.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_int]
    var = np.zeros(4)
    assert fn(None, 4, var.ctypes.data, 0) == -4            # STMMQR_ERR_INVALID
    assert pkg.lib.stmmqr_last_error().decode() != ""
    fl = pkg.lib.stmmqr_ls_covariance_diag
    fl.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    assert fl(None, var.ctypes.data, 0) == -4
