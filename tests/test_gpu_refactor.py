"""SparseQR.refactorize (stmmqr_sparseqr_refactorize) on the GPU: a factorized object that is given new values of the same pattern
must be, bit for bit, the object a fresh SparseQR makes of those values -- tolerance, Y, every Q and R operation, the exported R
and H -- whether the values come as a host array or a device pointer, with and without H, through a rank change and back, and
for SparseQR.lq objects (values in A's own order).  Values whose singleton structure does not hold are refused with
STMMQR_ERR_STALE and leave the object as it was.  "Equal" is equality of bits (bits(), as tests/test_gpu_carried.py compares).

The values (test_refactor_cpu.new_values): Ax2 = Ax (1 + 0.25 cos(0.7 p + 0.3)) over the storage positions p; Ax3 = Ax2 with one
named column set to zero.  That they keep the singletons and the column order of Ax is asserted (tests/test_refactor_cpu.py checks
it without a GPU; here the fresh object's n1rows / n1cols / Q1fill are compared with the refactorized one's).

Not tested here: the "no valid factorization" state after a factorization that fails once the values were accepted -- it cannot be
reached on a GPU without provoking a failure."""
import importlib

import numpy as np
import pytest

from test_gpu_sparseqr import entry
from test_refactor_cpu import full_matrix, new_values, transposed

pytestmark = pytest.mark.gpu
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
ERR_INVALID, ERR_STALE = -4, -7
FIXTURES = ["syn_wide5x8", "syn_star", "syn_emptycol", "syn_rankdef_grid", "syn_rand60x40", "syn_grid3d", "bcsstk14", "lns_3937", "ex18"]
NRHS = 2


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    assert p.device_count() >= 1
    return p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def make(pkg, mat, Ax=None, **kw):
    m, n, Ap, Ai, Ax0 = mat
    return pkg.SparseQR(m, n, Ap, Ai, Ax0 if Ax is None else Ax, relax=pkg.relax_for_qr(n, int(Ap[-1])), **kw)


def operands(m, n):
    X = np.asfortranarray(np.stack([entry(np.arange(m), j) for j in range(NRHS)], axis=1))
    Bm = np.asfortranarray(np.stack([entry(np.arange(m) + 5, j + 2) for j in range(NRHS)], axis=1))
    Bn = np.asfortranarray(np.stack([entry(np.arange(n) + 5, j + 2) for j in range(NRHS)], axis=1))
    return X, Bm, Bn


def snapshot(Q, keep_h=True, full=True):
    """everything an object answers, as a dict of arrays.  full=False: the structure, the tolerance and the solves only."""
    info = Q.info
    out = {"structure": np.array([info["rank"], info["n1rows"], info["n1cols"]]), "Q1fill": Q.Q1fill.astype(np.float64),
           "tol": np.array([Q.tol])}
    X, Bm, Bn = operands(Q.m, Q.n)
    for s in range(4):
        out[f"solve{s}"] = Q.solve(s, Bm if s <= 1 else Bn)
    if not full:
        return out
    Y = Q.Y()
    if Y is not None:
        out["Yp"], out["Yi"], out["Yx"] = Y[0].astype(np.float64), Y[1].astype(np.float64), Y[2]
    if keep_h:
        for k in range(4):
            out[f"qmult{k}"] = Q.qmult(k, X if k <= 1 else np.asfortranarray(X.T))
    for k, v in Q.export_r(with_h=keep_h).items():
        out["export_" + k] = np.asarray(v, np.float64)
    return out


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k} differs"


_fresh = {}


def fresh(pkg, name, which, col=None, keep_h=True, full=True):
    """the snapshot of a new object on Ax (which 1), Ax2 (2) or Ax3 (3, column col zeroed): made once per module"""
    key = (name, which, col, keep_h, full)
    if key not in _fresh:
        mat = full_matrix(name)
        Ax = mat[4] if which == 1 else new_values(mat[4], col if which == 3 else None, mat[2])
        Q = make(pkg, mat, Ax, keep_h=keep_h)
        try:
            _fresh[key] = snapshot(Q, keep_h, full)
        finally:
            Q.close()
    return _fresh[key]


def plan_bytes(pkg, Q):
    lib = pkg.capi.lib
    return float(lib.stmmqr_plan_device_bytes(lib.stmmqr_sparseqr_plan(Q._h)))


@pytest.mark.parametrize("name", FIXTURES)
def test_equal_to_a_fresh_object_and_round_trip(pkg, name):
    """cases 1 and 2: host array, device pointer, then the first values again"""
    import torch
    mat = full_matrix(name)
    Ax2 = new_values(mat[4])
    Q = make(pkg, mat)
    try:
        first = snapshot(Q)
        assert_same(first, fresh(pkg, name, 1), "as first made")
        Q.refactorize(Ax2)
        ri = Q.refactor_info
        assert np.array_equal(bits(np.array([ri[0]])), bits(fresh(pkg, name, 2)["tol"]))
        assert ri[4] == 1 and ri[5] == 0 and ri[6] == 2 and ri["rebuilt"] == 0
        assert_same(snapshot(Q), fresh(pkg, name, 2), "refactorize(Ax2)")
        bytes1 = plan_bytes(pkg, Q)
        # the same values as a device pointer, over the first values again (so that the call has work to undo)
        Q.refactorize(mat[4])
        d = torch.from_numpy(np.ascontiguousarray(Ax2)).cuda()
        torch.cuda.synchronize()
        Q.refactorize(dev_ptr=d.data_ptr())
        assert_same(snapshot(Q), fresh(pkg, name, 2), "refactorize(device pointer)")
        with pytest.raises(pkg.StmmqrError, match="host"):
            Q.solve_seminormal(np.ones(Q.m))
        # round trip
        Q.refactorize(mat[4])
        assert_same(snapshot(Q), first, "round trip")
        ri = Q.refactor_info
        assert ri[4] == 4 and ri[6] == 2 and ri[5] == 0
        assert plan_bytes(pkg, Q) == bytes1
        assert int(Q.info["retries"]) == 0
        if Q.m >= Q.n and int(Q.info["rank"]) == Q.n:
            x, _ = Q.solve_seminormal(np.ones(Q.m))                 # (host values again: works)
            assert np.isfinite(x).all()
    finally:
        Q.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_without_h(pkg, name):
    """keep_h=False objects take new values as well: the solves"""
    mat = full_matrix(name)
    Q = make(pkg, mat, keep_h=False)
    try:
        Q.refactorize(new_values(mat[4]))
        assert_same(snapshot(Q, keep_h=False, full=False), fresh(pkg, name, 2, keep_h=False, full=False), "refactorize(Ax2), R only")
        assert Q.refactor_info[6] == 2
    finally:
        Q.close()


@pytest.mark.parametrize("name,col", [("syn_grid3d", 5), ("syn_rand60x40", 7)])
def test_full_rank_to_rank_deficient_and_back(pkg, name, col):
    mat = full_matrix(name)
    Q = make(pkg, mat)
    try:
        rank0 = int(Q.info["rank"])
        assert rank0 == mat[1]
        Q.refactorize(new_values(mat[4], col, mat[2]))
        assert int(Q.info["rank"]) == rank0 - 1
        assert_same(snapshot(Q), fresh(pkg, name, 3, col), "refactorize(Ax3)")
        Q.refactorize(new_values(mat[4]))
        assert int(Q.info["rank"]) == rank0
        assert_same(snapshot(Q), fresh(pkg, name, 2), "refactorize(Ax2) after Ax3")
    finally:
        Q.close()


@pytest.mark.parametrize("name", ["syn_star", "bcsstk14"])
def test_stale(pkg, name):
    mat = full_matrix(name)
    m, n, Ap, Ai, Ax = mat
    lib = pkg.capi.lib
    Q = make(pkg, mat)
    try:
        M = Q.refactor_maps()
        n1rows = int(M["counts"][3])
        assert n1rows >= 1
        bad = new_values(Ax)
        p = int(M["pivsrc"][n1rows - 1])                            # the pivot of the last live singleton
        bad[p] = 0.0
        col = int(np.searchsorted(Ap, p, side="right") - 1)
        before = snapshot(Q)
        rc = lib.stmmqr_sparseqr_refactorize(Q._h, bad.ctypes.data, 0)
        assert rc == ERR_STALE
        msg = pkg.capi.last_error()
        assert f"column {col} of A" in msg and f"live row {n1rows - 1})" in msg, msg
        assert_same(snapshot(Q), before, "after STMMQR_ERR_STALE")
        ri = Q.refactor_info
        assert ri[5] == 1 and ri[4] == 0
        with pytest.raises(pkg.StmmqrError) as ei:
            Q.refactorize(bad)
        assert ei.value.code == ERR_STALE and Q.refactor_info[5] == 2
        # rebuild=True: a new native object with the same arguments, swapped in
        F = make(pkg, mat, bad)
        try:
            want = snapshot(F, full=False)
        finally:
            F.close()
        Q.refactorize(bad, rebuild=True)
        assert Q.refactor_info["rebuilt"] == 1
        assert_same(snapshot(Q, full=False), want, "rebuild=True")
        with pytest.raises(pkg.StmmqrError, match="rebuild"):
            Q.refactorize(dev_ptr=1, rebuild=True)
    finally:
        Q.close()
    # no tolerance (tol = -1): |a| > -1 always holds, as in a fresh object: the same values are not stale
    Q = make(pkg, mat, tol=-1.0)
    F = make(pkg, mat, bad, tol=-1.0)
    try:
        assert (Q.info["n1rows"], Q.info["n1cols"]) == (F.info["n1rows"], F.info["n1cols"]) and np.array_equal(Q.Q1fill, F.Q1fill)
        Q.refactorize(bad)
        assert Q.refactor_info[5] == 0 and Q.tol == -1.0
        got, want = snapshot(Q, full=False), snapshot(F, full=False)
        # (a zero pivot on R1's diagonal: both objects divide by it in the same place)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), k
    finally:
        Q.close()
        F.close()


def lq_cases():
    m, n, Ap, Ai, Ax = full_matrix("syn_wide5x8")
    yield "syn_wide5x8", (m, n, Ap, Ai, Ax)
    m, n, Ap, Ai, Ax = full_matrix("syn_rand60x40")
    (Tp, Ti, Tx), _ = transposed(m, n, Ap, Ai, Ax)
    yield "syn_rand60x40 transposed", (n, m, Tp, Ti, Tx)


@pytest.mark.parametrize("which", [0, 1])
def test_lq(pkg, which):
    import scipy.sparse as sp
    name, (m, n, Ap, Ai, Ax) = list(lq_cases())[which]
    Ax2 = new_values(Ax)
    rx = pkg.relax_for_qr(m, int(Ap[-1]))
    Q = pkg.SparseQR.lq(m, n, Ap, Ai, Ax, relax=rx)
    F = pkg.SparseQR.lq(m, n, Ap, Ai, Ax2, relax=rx)
    try:
        assert (Q.info["n1rows"], Q.info["n1cols"]) == (F.info["n1rows"], F.info["n1cols"]) and np.array_equal(Q.Q1fill, F.Q1fill)
        Q.refactorize(Ax2)
        assert np.array_equal(bits(np.array([Q.tol])), bits(np.array([F.tol]))) and Q.info["rank"] == F.info["rank"]
        A2 = sp.csc_matrix((Ax2, Ai, Ap), shape=(m, n))
        b = A2 @ entry(np.arange(n), 1)                            # in the range of A2
        x, xf = Q.min2norm(b), F.min2norm(b)
        assert np.array_equal(bits(x), bits(xf)), name
        assert np.linalg.norm(A2 @ x[:, 0] - b) <= 1e-12 * np.linalg.norm(b)
        assert Q.refactor_info[6] == 2
    finally:
        Q.close()
        F.close()


def test_refusals(pkg):
    lib = pkg.capi.lib
    mat = full_matrix("syn_star")
    m, n, Ap, Ai, Ax = mat
    Ax2 = new_values(Ax)
    S = make(pkg, mat, symbolic_only=True)
    try:
        assert lib.stmmqr_sparseqr_refactorize(S._h, Ax2.ctypes.data, 0) == ERR_INVALID and "numeric" in pkg.capi.last_error()
    finally:
        S.close()
    assert lib.stmmqr_sparseqr_refactorize(None, Ax2.ctypes.data, 0) == ERR_INVALID and "null object" in pkg.capi.last_error()
    tol = 1e-9
    Q = make(pkg, mat, tol=tol)
    F = make(pkg, mat, Ax2, tol=tol)
    try:
        before = snapshot(Q, full=False)
        assert lib.stmmqr_sparseqr_refactorize(Q._h, None, 0) == ERR_INVALID and "null values" in pkg.capi.last_error()
        assert lib.stmmqr_sparseqr_refactorize(Q._h, None, 1) == ERR_INVALID
        assert_same(snapshot(Q, full=False), before, "after a refusal")
        # an explicit tolerance stays whatever the values are
        Q.refactorize(Ax2)
        assert Q.tol == tol and Q.refactor_info[0] == tol
        assert_same(snapshot(Q), snapshot(F), "explicit tolerance")
    finally:
        Q.close()
        F.close()
