"""stmmqr_plan_h_sparse, the part that needs no GPU: the symbol is declared, exported and bound, an object that holds the host half only
refuses with the library's message, and the numpy walker the GPU tests measure against (tests/hsparse_reference.py) gives, on the
reference's own factorization, the Hp / Hi / Hx / HTau that this library's qr_rcount and qr_rconvert make of the same object, bit for
bit (the route of tests/test_export.py, whose own yardstick is the reference's output).  (The feature adds no function to the pure
csrc/stmmqr_restables.{h,cpp} -- the counts, offsets and positions are computed by the kernels --, so there is no stand-alone sanitizer
program for it.)"""
import ctypes as C
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

from hsparse_reference import walk_h
from stmmqr_testlib import Symbolic, load_golden
from test_export import dp, ip, reference_objects
from test_refactor_cpu import full_matrix

ROOT = Path(__file__).resolve().parent.parent
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
I64 = np.int64
# the fixtures of tests/test_gpu_hsparse.py that store the reference's whole packed stack (the five larger ones keep a sketch of it)
FULL_STACK = ["syn_dense6x4", "syn_wide5x8", "syn_emptycol", "syn_dupcol", "syn_chain", "syn_star", "syn_rand60x40", "syn_grid2d",
              "syn_rankdef_grid"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def test_declared_exported_and_bound(pkg):
    header = (ROOT / "include" / "stmmqr_hip.h").read_text()
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))      # (comments out, one blank between words)
    assert ("int stmmqr_plan_h_sparse(stmmqr_plan *plan, stm_long *Hp, stm_long *Hi, double *Hx, double *HTau, stm_long *HPinv, "
            "stm_long colcap, stm_long cap, stm_long *info , int on_device);") in plain
    lib = pkg.capi.lib
    assert hasattr(lib, "stmmqr_plan_h_sparse")
    assert len(lib.stmmqr_plan_h_sparse.argtypes) == 10
    assert callable(pkg.capi.HipQR.h_sparse) and callable(pkg.capi.SparseQR.h_sparse)
    assert not hasattr(pkg.capi.LeastSquares, "h_sparse")                    # (it stores no Q)
    info = np.full(4, -7, I64)
    assert lib.stmmqr_plan_h_sparse(None, None, None, None, None, None, 0, 0, ip(info), 0) == -4
    assert np.all(info == -7)


def test_host_only_object_refuses(pkg):
    m, n, Ap, Ai, Ax = full_matrix("syn_star")
    Q = pkg.SparseQR.lq(m, n, Ap, Ai, Ax, device=-2)
    try:
        with pytest.raises(pkg.StmmqrError, match="no factorization held by the plan") as e:
            Q.h_sparse()
        assert e.value.code == -4
    finally:
        Q.close()
    Q = pkg.SparseQR(m, n, Ap, Ai, Ax, symbolic_only=True)
    try:
        with pytest.raises(pkg.StmmqrError, match="no factorization held by the plan") as e:
            Q.h_sparse()
        assert e.value.code == -4
        with pytest.raises(pkg.StmmqrError, match="no factorization held by the plan"):
            Q.h_sparse(device=True)                                          # (refused before torch is looked for)
    finally:
        Q.close()


@pytest.mark.parametrize("name", FULL_STACK)
def test_walker_equals_rcount_rconvert(pkg, name):
    g = load_golden(name)
    assert "num_Stack" in g and len(g["num_Stack"]) >= int(np.sum(g["num_rh_size"]))
    K = reference_objects(pkg, g)
    S, N = K["S"], K["N"]
    lib = pkg.lib
    lib.qr_rcount.restype = None
    lib.qr_rconvert.restype = None
    H2p = np.zeros(S.rjsize + 2, I64)
    nh = C.c_long(0)
    lib.qr_rcount(C.byref(S), C.byref(N), C.c_long(0), C.c_long(S.m), C.c_long(S.n), 0, None, None, ip(H2p), C.byref(nh))
    hnz = int(H2p[nh.value])
    Hi, Hx, Ht = np.zeros(max(hnz, 1), I64), np.zeros(max(hnz, 1)), np.zeros(max(nh.value, 1))
    lib.qr_rconvert(C.byref(S), C.byref(N), C.c_long(0), C.c_long(S.m), C.c_long(S.n), 0, None, None, None, None, None, None, ip(H2p), ip(Hi),
                    dp(Hx), dp(Ht))
    W = walk_h(Symbolic(g), g["num_Stack"], g["num_Rblock_off"], g["num_HStair"], g["num_HTau"], g["num_Hii"], g["num_Hm"])
    assert W["nh"] == nh.value
    assert np.array_equal(W["Hp"], H2p[:nh.value + 1])
    assert np.array_equal(W["Hi"], Hi[:hnz])
    assert np.array_equal(W["Hx"].view(I64), Hx[:hnz].view(I64)) and np.array_equal(W["HTau"].view(I64), Ht[:nh.value].view(I64))
    assert W["visited"] - W["zeros"] == hnz
