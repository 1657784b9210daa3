"""Products with R and R' on the resident factors (stmmqr_plan_rmult; kernels: csrc/stmmqr_rmult.hip).

Yardstick: Factors.R of tests/resident_reference.py -- the whole rank x n factor, dead pivot columns included, rebuilt in long double
from the plan's own downloaded factors.  Tolerance, componentwise and from the dot-product bound, which holds for any order of
summation:  |got - ref|_i <= (k + 2) eps (|R| |x|)_i,  k = the longest sum: maxfn for R x (a row of R lies in one front), the rank
for R' y (a column of R has at most one entry per row).

The kernels' slab and chunk constants (csrc/stmmqr_device.h, read from there and pinned here): a workgroup of R x owns
STM_RM_ROWS = 256 rows and stages STM_RM_XC = 256 entries of x per pass; a workgroup of R' y owns STM_RM_COLS = 64 columns.  DENSE
holds single fronts with each of these dimensions at the constant + 1 and with ragged tails."""
import importlib
import os
import re
from pathlib import Path

import numpy as np
import pytest

from minnorm_reference import SMALL, qfill_of
from resident_reference import LD, Factors, make_front, stair_csc, symbolic_of
from stmmqr_testlib import EPS, Symbolic, load_golden, numeric_from_gpu, scalar

pytestmark = pytest.mark.gpu
BATCHES = (1, 2, 3, 5)
NAMES = SMALL + ["bcsstk14", "lns_3937"]
ROOT = Path(__file__).resolve().parent.parent
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
RM_ROWS, RM_XC, RM_COLS = 256, 256, 64


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    assert p.device_count() >= 1
    return p


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module(PKG + ".capi")


@pytest.fixture
def env():
    saved = {}

    def put(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = str(v)
    yield put
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def test_constants_are_the_kernels():
    text = (ROOT / PKG / "csrc" / "stmmqr_device.h").read_text()
    got = {k: int(v) for k, v in re.findall(r"#define STM_RM_(ROWS|XC|COLS) (\d+)", text)}
    assert got == {"ROWS": RM_ROWS, "XC": RM_XC, "COLS": RM_COLS}


def golden_plan(pkg, name, keep_h=True):
    g = load_golden(name)
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}
    plan = pkg.HipQR(sym)
    plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    return g, S, plan


def inputs(m, n, seed=23):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((n, max(BATCHES)))), np.asfortranarray(rng.standard_normal((m, max(BATCHES))))


def batched(call, B, what):
    """column j of every batch size carries the bits of its one-vector call -> the columns of the one-vector calls"""
    one = np.stack([np.asarray(call(B[:, j].copy())).ravel() for j in range(B.shape[1])], axis=1)
    for k in BATCHES[1:]:
        Y = call(B[:, :k].copy())
        for j in range(k):
            assert np.array_equal(Y[:, j], one[:, j]), f"{what}: column {j} of a batch of {k} differs from the one-vector call"
    return one


def on_device(pkg, capi, plan, X, trans, permuted, yrows):
    """the same call with device pointers and padded leading dimensions"""
    xr, k = X.shape
    ldx, ldy = xr + 3, yrows + 5
    Xd = np.full((ldx, k), np.nan, order="F")
    Xd[:xr] = X
    Yd = np.full((ldy, k), -3.0, order="F")
    dx, dy = pkg.device_alloc(Xd.nbytes), pkg.device_alloc(Yd.nbytes)
    try:
        pkg.device_copy(dx, Xd.ctypes.data, Xd.nbytes)
        pkg.device_copy(dy, Yd.ctypes.data, Yd.nbytes)
        assert capi.lib.stmmqr_plan_rmult(plan._h, trans, dx, ldx, dy, ldy, k, int(permuted), 1) == 0
        pkg.device_copy(Yd.ctypes.data, dy, Yd.nbytes)
    finally:
        pkg.device_free(dx); pkg.device_free(dy)
    assert np.all(Yd[yrows:] == -3.0)
    return Yd[:yrows]


def excess(got, ref, bound):
    """largest |got - ref| in units of the componentwise bound (<= 1 passes); a zero bound wants an exact zero"""
    d = np.abs(np.asarray(got, LD) - ref)
    if np.any(d[bound == 0] != 0):
        return float("inf")
    return float((d[bound > 0] / bound[bound > 0]).max(initial=0))


def check_products(pkg, capi, plan, Fa, q, maxfn, label, plan0=None):
    """both trans and both permuted of one factorization against Fa.R; -> (X, Y = rmult(0, X)) of the unpermuted call"""
    m, n, rank = Fa.m, Fa.n, Fa.rank
    X, Yin = inputs(m, n)
    R, aR = Fa.R, np.abs(Fa.R)
    out = None
    for permuted in (False, True):
        # ---- R x ----
        Y = batched(lambda v: plan.rmult(v, 0, permuted), X, f"{label} rmult(0, permuted={permuted})")
        Xr = np.asarray(X if permuted else X[q], LD)
        ref, bound = R @ Xr, (maxfn + 2) * EPS * (aR @ np.abs(Xr))
        e0 = excess(Y[:rank], ref, bound)
        assert np.all(Y[rank:] == 0.0), "rows beyond the rank are not zero"
        assert np.array_equal(on_device(pkg, capi, plan, X, 0, permuted, m), Y)
        # ---- R' y ----
        Z = batched(lambda v: plan.rmult(v, 1, permuted), Yin, f"{label} rmult(1, permuted={permuted})")
        Yr = np.asarray(Yin[:rank], LD)
        zref, zbound = R.T @ Yr, (rank + 2) * EPS * (aR.T @ np.abs(Yr))
        Zr = Z if permuted else Z[q]                                         # Z[Qfill[k]] = z[k]
        e1 = excess(Zr, zref, zbound)
        Y2 = Yin.copy()
        Y2[rank:] += 10.0                                                    # rows beyond the rank are ignored
        assert np.array_equal(plan.rmult(Y2, 1, permuted), Z)
        assert np.array_equal(on_device(pkg, capi, plan, Yin, 1, permuted, n), Z)
        print(f"\n[rmult] {label} permuted={permuted}: R x {e0:.3f}, R'y {e1:.3f} of the componentwise bound (k = {maxfn} / {rank})")
        assert e0 <= 1.0 and e1 <= 1.0
        if plan0 is not None:                                                # the plan without H: the same bits
            assert np.array_equal(plan0.rmult(X, 0, permuted), Y)
            assert np.array_equal(plan0.rmult(Yin, 1, permuted), Z)
        if not permuted:
            out = (X, Y)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_products_on_fixtures(pkg, capi, name):
    g, S, plan = golden_plan(pkg, name)
    _, _, plan0 = golden_plan(pkg, name, keep_h=False)
    try:
        Fa = Factors(S, numeric_from_gpu(S, plan.download()))
        X, Y = check_products(pkg, capi, plan, Fa, qfill_of(S), int(S.maxfn), name, plan0)
        if Fa.rank == S.n:                                                   # no dead column: A x = Q (R (E'x)), the README's parity bound
            AX = plan.spmv(X)
            d = np.linalg.norm(plan.qmult(1, Y) - AX, axis=0)
            lim = 1e-13 * np.linalg.norm(g["in_Ax"]) * np.linalg.norm(X, axis=0)
            print(f"  |Q R E'x - A x| / (1e-13 |A|_F |x|) = {float((d / lim).max()):.3f}")
            assert np.all(d <= lim)
    finally:
        plan.close(); plan0.close()


def test_levels_rebuilt_per_pass(pkg, capi, env):
    """recycled slabs with a scratch of one tree level: every pass puts each level back into front form before it reads it"""
    env(STMMQR_RECYCLE=2, STMMQR_RESIDENT_CACHE=0)
    g, S, plan = golden_plan(pkg, "dwt_992")
    try:
        Fa = Factors(S, numeric_from_gpu(S, plan.download()))
        check_products(pkg, capi, plan, Fa, qfill_of(S), int(S.maxfn), "dwt_992 recycled, level scratch")
    finally:
        plan.close()


# ---- single dense fronts, sized by the kernels' constants ----
def dupcol_front():
    F, St = make_front(60, 40)
    F[:, 7] = F[:, 3]
    F[:, 20] = 2.0 * F[:, 11]
    F[:, 21] = F[:, 0] - F[:, 1]
    return F, St, 37


DENSE = {
    "70x33 full": lambda: (*make_front(70, 33), 33),
    "300x257 ramp": lambda: (*make_front(300, 257, "ramp"), 257),           # RM_ROWS + 1 rows of R, RM_XC + 1 and 4 RM_COLS + 1 columns
    "40x300 rows run out": lambda: (*make_front(40, 300), 40),               # 40 rows of R over RM_XC + 44 columns
    "80x65 full": lambda: (*make_front(80, 65), 65),                         # RM_COLS + 1 columns
    "600x523 full": lambda: (*make_front(600, 523), 523),                    # 2 RM_ROWS + 11 rows, 2 RM_XC + 11 and 8 RM_COLS + 11 columns
    "60x40 duplicated columns": dupcol_front,                                # three dead pivots keep the rows above them
}


@pytest.mark.parametrize("shape", list(DENSE))
def test_dense_fronts(pkg, capi, shape):
    F, St, rank = DENSE[shape]()
    m, n = F.shape
    Ap, Ai, Ax = stair_csc(F, St)
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    assert sym["nf"] == 1
    plans = []
    try:
        for keep_h in (1, 0):
            p = pkg.HipQR({**sym, "keepH": keep_h})
            plans.append(p)
            assert p.factorize(Ax, 1e-10, n, Ap, Ai)["retries"] == 0
        S = symbolic_of(sym)
        G = plans[0].download()
        assert G.rank == rank
        Fa = Factors(S, numeric_from_gpu(S, G))
        assert (Fa.rank < n) == (shape.startswith("60x40") or shape.startswith("40x300"))
        check_products(pkg, capi, plans[0], Fa, np.arange(n), int(sym["maxfn"]), shape, plans[1])
    finally:
        for p in plans:
            p.close()


def test_refusals(pkg, capi):
    lib = capi.lib
    g = load_golden("syn_grid2d")
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    fresh = pkg.HipQR(sym)
    try:
        with pytest.raises(pkg.StmmqrError) as e:
            fresh.rmult(np.ones(S.n))
        assert e.value.code == -4 and "no factorization" in str(e.value)
        fresh.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        y0 = fresh.rsolve(0, np.ones(S.m))
        x = np.ones((S.n, 2), order="F")
        Y = np.full((S.m, 2), 7.0, order="F")
        call = lambda trans, ldx, ldy, nrhs: lib.stmmqr_plan_rmult(fresh._h, trans, x.ctypes.data, ldx, Y.ctypes.data, ldy, nrhs, 0, 0)
        assert call(0, S.n - 1, S.m, 1) == -4 and "leading dimension" in capi.last_error()
        assert call(0, S.n, S.m - 1, 1) == -4 and "leading dimension" in capi.last_error()
        assert call(2, S.n, S.m, 1) == -4 and "rmult" in capi.last_error()
        assert call(0, S.n, S.m, -1) == -4
        assert lib.stmmqr_plan_rmult(fresh._h, 0, None, S.n, Y.ctypes.data, S.m, 1, 0, 0) == -4
        assert lib.stmmqr_plan_rmult(fresh._h, 0, x.ctypes.data, S.n, None, S.m, 1, 0, 0) == -4
        assert lib.stmmqr_plan_rmult(None, 0, x.ctypes.data, S.n, Y.ctypes.data, S.m, 1, 0, 0) == -4
        assert call(0, S.n, S.m, 0) == 0
        assert np.all(Y == 7.0)                                              # nrhs = 0 writes nothing, and no refusal wrote anything
        assert np.array_equal(fresh.rsolve(0, np.ones(S.m)), y0)             # the plan stays usable
        assert call(0, S.n, S.m, 2) == 0
        assert np.array_equal(Y[:, 0], fresh.rmult(np.ones(S.n)))
    finally:
        fresh.close()


def test_new_buffers_are_outside_device_bytes(pkg):
    """What this pins: stmmqr_plan_device_bytes reports the same figure after the first transposed product (which makes the
    pass vectors and the index of the transposed product) as before it, and the plan's other operations give the same bits
    afterwards.  That those buffers are made at the first call and not before is the host code's `ensure_rtmult`; no test
    observes device memory directly."""
    g, S, plan = golden_plan(pkg, "syn_grid3d")
    try:
        y = plan.rsolve(0, np.ones(S.m))
        before = plan.device_bytes()
        plan.rmult(np.ones(S.n), 0)
        plan.rmult(np.ones(S.m), 1)
        assert plan.device_bytes() == before
        assert np.array_equal(plan.rsolve(0, np.ones(S.m)), y)
    finally:
        plan.close()
