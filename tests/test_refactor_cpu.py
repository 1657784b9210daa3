"""SparseQR.refactorize, the part that needs no GPU: the value maps the host half records while it splits A into R1 and Y
(stmmqr_sparseqr_refactor_maps) -- where every entry of Y and of R1 and the pivot of every live singleton row sits in the caller's
storage.  The device side of a refactorization gathers new values through exactly these tables, so what is asserted here is what
tests/test_gpu_refactor.py relies on.  Also the stand-alone program tests/refactor_selftest.cpp under AddressSanitizer + UBSan (the
recipe of tests/test_nullspace_cpu.py: g++, no preload of any kind), which checks the same identities in C++, through a
transposition as stmmqr_sparselq hands it over, and the object's release hook."""
import importlib
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from stmmqr_testlib import load_golden

ROOT = Path(__file__).resolve().parent.parent
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
CSRC = ROOT / PKG / "csrc"
SOURCES = ["stmmqr_mmio.cpp", "stmmqr_symbolic.cpp", "stmmqr_colamd.cpp", "stmmqr_sparseqr.cpp"]
MAPS = ["syn_wide5x8", "syn_star", "syn_emptycol", "bcsstk14", "lns_3937", "ex18"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def full_matrix(name):
    """(m, n, Ap, Ai, Ax) of the caller's full matrix of a fixture"""
    g = load_golden(name)
    return int(g["A_m"][0]), int(g["A_n"][0]), g["A_p"], g["A_i"], g["A_x"]


def new_values(Ax, zero=None, Ap=None):
    """Ax2 = Ax (1 + 0.25 cos(0.7 p + 0.3)); zero = a column: Ax3, that column of Ax2 set to zero"""
    p = np.arange(Ax.size, dtype=np.float64)
    out = Ax * (1.0 + 0.25 * np.cos(0.7 * p + 0.3))
    if zero is not None:
        out[Ap[zero]:Ap[zero + 1]] = 0.0
    return out


@pytest.mark.parametrize("name", MAPS)
def test_maps(pkg, name):
    m, n, Ap, Ai, Ax = full_matrix(name)
    Q = pkg.SparseQR(m, n, Ap, Ai, Ax, symbolic_only=True, relax=pkg.relax_for_qr(n, int(Ap[-1])))
    try:
        info, M, Y = Q.info, Q.refactor_maps(), Q.Y()
        n1rows, n1cols = int(info["n1rows"]), int(info["n1cols"])
        assert n1cols > 0 and Y is not None
        nz = int(Ap[-1])
        assert M["counts"].tolist() == [nz, int(Y[0][-1]), nz - int(Y[0][-1]), n1rows]
        assert np.array_equal(Y[2], Ax[M["ysrc"]])
        assert np.array_equal(np.sort(np.concatenate([M["ysrc"], M["r1src"]])), np.arange(nz))
        assert M["pivsrc"].size == n1rows and np.all(np.abs(Ax[M["pivsrc"]]) > Q.tol)
        # a pivot is an entry of R1, in a singleton column: one of the first n1cols columns of the order
        cols = np.repeat(np.arange(n), np.diff(Ap))
        assert np.isin(M["pivsrc"], M["r1src"]).all() and np.isin(cols[M["pivsrc"]], Q.Q1fill[:n1cols]).all()
    finally:
        Q.close()


def test_no_maps_without_singletons(pkg):
    m, n, Ap, Ai, Ax = full_matrix("syn_grid3d")
    Q = pkg.SparseQR(m, n, Ap, Ai, Ax, symbolic_only=True)
    try:
        M = Q.refactor_maps()
        assert int(Q.info["n1cols"]) == 0
        assert M["ysrc"] is None and M["r1src"] is None and M["pivsrc"] is None
        assert M["counts"].tolist() == [int(Ap[-1]), int(Ap[-1]), 0, 0]
    finally:
        Q.close()


def transposed(m, n, Ap, Ai, Ax):
    """(A' in compressed columns, tsrc): tsrc[q] = the storage position in A of entry q of A' -- by numpy alone"""
    cols = np.repeat(np.arange(n), np.diff(Ap))
    tsrc = np.lexsort((cols, Ai))                                  # by row of A, then by column: the columns of A' one after the other
    Tp = np.concatenate([[0], np.cumsum(np.bincount(Ai, minlength=m))]).astype(np.int64)
    return (Tp, np.ascontiguousarray(cols[tsrc], np.int64), np.ascontiguousarray(Ax[tsrc])), tsrc


@pytest.mark.parametrize("name,flip", [("syn_rand60x40", False), ("syn_rand60x40", True), ("syn_wide5x8", False)])
def test_lq_maps_are_composed_with_the_transposition(pkg, name, flip):
    """An LQ object takes values in A's own order: its maps are those of the object of A' read through the transposition, which is
    made here with numpy.  syn_rand60x40 (60 x 40; A' has singletons), its transpose (40 x 60; A' has none: ysrc IS the transposition)
    and syn_wide5x8.  The LQ objects are made through the host half alone (device -2)."""
    m, n, Ap, Ai, Ax = full_matrix(name)
    if flip:
        (Ap, Ai, Ax), _ = transposed(m, n, Ap, Ai, Ax)
        m, n = n, m
    (Tp, Ti, Tx), tsrc = transposed(m, n, Ap, Ai, Ax)
    nz = int(Ap[-1])
    Q = pkg.SparseQR.lq(m, n, Ap, Ai, Ax, device=-2)
    T = pkg.SparseQR(n, m, Tp, Ti, Tx, symbolic_only=True)
    try:
        M, MT = Q.refactor_maps(), T.refactor_maps()
        assert M["counts"].tolist() == MT["counts"].tolist() and Q.info["n1cols"] == T.info["n1cols"]
        if int(T.info["n1cols"]) == 0:
            assert flip == (name == "syn_rand60x40")
            assert np.array_equal(M["ysrc"], tsrc) and M["r1src"] is None and M["pivsrc"] is None
            assert np.array_equal(Tx, Ax[M["ysrc"]])
        else:
            for k in ("ysrc", "r1src", "pivsrc"):
                assert np.array_equal(M[k], tsrc[MT[k]]), k
            assert np.array_equal(Q.Y()[2], Ax[M["ysrc"]])
            assert np.array_equal(np.sort(np.concatenate([M["ysrc"], M["r1src"]])), np.arange(nz))
            assert np.all(np.abs(Ax[M["pivsrc"]]) > Q.tol)
        with pytest.raises(pkg.StmmqrError, match="host half"):
            Q.numeric()
    finally:
        Q.close()
        T.close()


@pytest.mark.parametrize("name,col", [("syn_wide5x8", None), ("syn_star", None), ("syn_emptycol", None), ("syn_rankdef_grid", None),
                                      ("syn_rand60x40", None), ("syn_grid3d", None), ("bcsstk14", None), ("lns_3937", None), ("ex18", None),
                                      ("syn_grid3d", 5), ("syn_rand60x40", 7), ("bcsstk14", 900)])
def test_new_values_keep_the_structure(pkg, name, col):
    """the precondition of tests/test_gpu_refactor.py: Ax2 (and Ax3 with the named column zeroed) gives the singletons and the column
    order Ax gives, so that a refactorized object can be compared with a fresh one bit for bit"""
    m, n, Ap, Ai, Ax = full_matrix(name)
    rx = pkg.relax_for_qr(n, int(Ap[-1]))
    a = pkg.SparseQR(m, n, Ap, Ai, Ax, symbolic_only=True, relax=rx)
    b = pkg.SparseQR(m, n, Ap, Ai, new_values(Ax, col, Ap), symbolic_only=True, relax=rx)
    try:
        ia, ib = a.info, b.info
        assert (ia["n1rows"], ia["n1cols"]) == (ib["n1rows"], ib["n1cols"]) and np.array_equal(a.Q1fill, b.Q1fill)
    finally:
        a.close()
        b.close()


def _write_mtx(path, m, n, Ap, Ai, Ax):
    cols = np.repeat(np.arange(n), np.diff(Ap))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (m, n, len(Ax)))
        np.savetxt(f, np.c_[Ai + 1, cols + 1, Ax], fmt="%d %d %.17g")


def test_maps_and_release_hook_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "refactor_selftest"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", str(exe)] + [str(CSRC / s) for s in SOURCES] + [str(ROOT / "tests" / "refactor_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    files = []
    for name in MAPS + ["syn_grid3d", "syn_rand60x40"]:
        _write_mtx(tmp_path / f"{name}.mtx", *full_matrix(name))
        files.append(str(tmp_path / f"{name}.mtx"))
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=600,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"})
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "ok (0 failures)"
