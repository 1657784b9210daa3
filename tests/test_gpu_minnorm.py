"""The minimum-norm solve on the resident factors, x = Q (R' \\ (E'b)) (stmmqr_plan_solve_minnorm, stmmqr_sparseqr_min2norm), and
the R' pass underneath it that splits a front's columns over workgroups (k_rtbig_init / k_rtbig_step) where k_rtsolve cannot hold the
front in LDS -- or everywhere, with STMMQR_RTBIG_MIN=1.

References: tests/minnorm_reference.py (long double from the downloaded factors; validated against np.linalg.lstsq in
tests/test_minnorm_cpu.py).  Tolerances: solve_tol(cond_probe) for solutions, as the R' tests of tests/test_gpu_qsolve.py and
tests/test_gpu_resident_shapes.py; 1e-12 for what only Q was applied to; 1e-10 for the driver's residual expression."""
import importlib
import os
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import resident_reference as rr
from minnorm_reference import SMALL, minnorm_from_factors, qfill_of
from resident_reference import Factors, make_front, rel, stair_csc, symbolic_of
from stmmqr_testlib import Symbolic, cond_probe, load_golden, numeric_from_gpu, scalar, solve_tol

pytestmark = pytest.mark.gpu
BATCHES = (1, 2, 3, 5)
SPLIT_NAMES = SMALL + ["lns_3937", "bcsstk14"]
REFUSAL = "too wide for the one-workgroup R' solve"
MM = Path(__file__).resolve().parent / "golden" / "mm"


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


@pytest.fixture
def env():
    """set environment knobs for the plans created inside a test, restored afterwards"""
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


def golden_plan(pkg, name, keep_h=True):
    g = load_golden(name)
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}
    plan = pkg.HipQR(sym)
    plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    return g, S, plan


def rhs(n, seed=11):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, max(BATCHES))))


_REF = {}


def reference(oracle, name, S, plan):
    """(Factors, cond_probe, B, long-double solution) of a fixture, from the factors of the first plan that asks (every plan of a
    fixture holds a factorization of the same matrix); computed once per fixture and shared"""
    if name not in _REF:
        N = numeric_from_gpu(S, plan.download())
        Fa = Factors(S, N)
        B = rhs(S.n)
        _REF[name] = (Fa, cond_probe(oracle, S, N), B, minnorm_from_factors(Fa, B, qfill_of(S)))
    return _REF[name]


def batched(call, B, what):
    """call on every batch size; column j carries the bits of its one-vector call.  -> the columns of the one-vector calls"""
    one = np.stack([np.asarray(call(B[:, j].copy())).ravel() for j in range(B.shape[1])], axis=1)
    for k in BATCHES[1:]:
        Y = call(B[:, :k].copy())
        for j in range(k):
            assert np.array_equal(Y[:, j], one[:, j]), f"{what}: column {j} of a batch of {k} differs from the one-vector call"
    return one


# ---- 1. default knobs: the same kernels as the composition, without the host round trip ----
@pytest.mark.parametrize("name", SMALL)
def test_default_knobs_equal_the_composed_calls_bit_for_bit(pkg, oracle, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        Fa, kappa, B, Xref = reference(oracle, name, S, plan)
        X = batched(plan.solve_minnorm, B, "solve_minnorm")
        Xp = batched(lambda v: plan.solve_minnorm(v, permuted=True), B, "solve_minnorm permuted")
        assert np.array_equal(X, plan.qmult(1, plan.rsolve(3, B)))
        assert np.array_equal(Xp, plan.qmult(1, plan.rsolve(2, B)))
    finally:
        plan.close()
    d = rel(X, Xref)
    print(f"\n[minnorm] {name}: default knobs vs long double {d:.2e} (allowed {solve_tol(kappa):.1e})")
    assert d <= solve_tol(kappa)
    assert rel(Xp, minnorm_from_factors(Fa, B, None)) <= solve_tol(kappa)


# ---- 2. every front through the split kernels ----
def check_split(pkg, oracle, name, label):
    g, S, plan = golden_plan(pkg, name)
    try:
        Fa, kappa, B, Xref = reference(oracle, name, S, plan)
        X = batched(plan.solve_minnorm, B, label)
        Xp = plan.solve_minnorm(B, permuted=True)
        QtX = plan.qmult(0, X)
        q = qfill_of(S)
        dead = q[np.setdiff1d(np.arange(S.n), Fa.pivot_col)]
        if dead.size:                                                        # the equations of the dead columns are ignored
            B2 = B.copy()
            B2[dead] += 10.0
            assert np.array_equal(plan.solve_minnorm(B2), X)
        y = plan.rsolve(0, QtX[:, 0].copy())                                 # (the plan serves the other operations as before)
        assert np.all(np.isfinite(y))
    finally:
        plan.close()
    allowed = solve_tol(kappa)
    d, dp = rel(X, Xref), rel(Xp, minnorm_from_factors(Fa, B, None))
    tail = float(np.linalg.norm(QtX[Fa.rank:]) / max(np.linalg.norm(X), 1e-300))
    print(f"\n[minnorm] {label}: vs long double {d:.2e} / permuted {dp:.2e} (allowed {allowed:.1e}); |Q'x beyond the rank| / |x| {tail:.2e}")
    assert d <= allowed and dp <= allowed
    assert tail <= 1e-12                                                     # rows of the intermediate beyond the rank contribute nothing
    return S, X, kappa


@pytest.mark.parametrize("name", SPLIT_NAMES)
def test_every_front_split(pkg, oracle, env, name):
    _, _, p0 = golden_plan(pkg, name)                                        # default knobs first: one workgroup per front
    try:
        X0 = p0.solve_minnorm(rhs(p0.sym["n"]))
    finally:
        p0.close()
    env(STMMQR_RTBIG_MIN=1)
    S, X, kappa = check_split(pkg, oracle, name, f"{name} all split")
    d = rel(X, X0)
    print(f"  split vs one-workgroup kernels {d:.2e}")
    assert d <= solve_tol(kappa)
    assert S.nf > 0


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "dwt_992"])
def test_every_front_split_with_levels_rebuilt_per_pass(pkg, oracle, env, name):
    env(STMMQR_RTBIG_MIN=1, STMMQR_RECYCLE=2, STMMQR_RESIDENT_CACHE=0)
    check_split(pkg, oracle, name, f"{name} all split, recycled, level scratch")


# ---- 3. split and one-workgroup fronts feeding each other ----
def test_mixed_levels(pkg, oracle, env):
    g = load_golden("dwt_992")
    S = Symbolic(g)
    size = (np.asarray(S.Fm[:S.nf]) * np.diff(np.asarray(S.Rp[:S.nf + 1]))).astype(np.int64)
    par = np.asarray(S.Parent[:S.nf])
    kids = np.flatnonzero((par >= 0) & (par < S.nf))
    chosen = None
    for t in np.unique(size):                                               # the planner's rule: split when Fm * fn >= threshold
        big = size >= t
        up = np.any(big[kids] & ~big[par[kids]])                            # a split child under a one-workgroup parent
        down = np.any(~big[kids] & big[par[kids]])                          # ... and the reverse
        if up and down:
            chosen = int(t)
            break
    assert chosen is not None, "no threshold gives both kinds of parent-child pair"
    env(STMMQR_RTBIG_MIN=chosen)
    nbig = int((size >= chosen).sum())
    assert 0 < nbig < S.nf
    check_split(pkg, oracle, "dwt_992", f"dwt_992 mixed ({nbig} of {S.nf} fronts split, threshold {chosen})")


# ---- 4., 5. dense one-front plans beyond the LDS limit, default knobs ----
def dense_plan(pkg, m, n):
    F, St = make_front(m, n)
    Ap, Ai, Ax = stair_csc(F, St)
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    assert sym["nf"] == 1
    np.testing.assert_array_equal(sym["PLinv"], np.arange(m))
    assert not rr.rt_fits(int(sym["Fm"][0]), int(sym["Rp"][1] - sym["Rp"][0]))
    plan = pkg.HipQR(sym)
    stats = plan.factorize(Ax, 1e-10, n, Ap, Ai)
    assert stats["retries"] == 0
    return F, sym, plan


def refused_then_solved(pkg, plan, B, batches):
    """on a fresh plan, before anything else has run: system 3 is refused as pinned; the minimum-norm solve is not"""
    with pytest.raises(pkg.StmmqrError) as e:
        plan.rsolve(3, B[:, 0].copy())
    assert e.value.code == -3 and REFUSAL in str(e.value)
    one = np.stack([plan.solve_minnorm(B[:, j].copy()) for j in range(B.shape[1])], axis=1)
    for k in batches:
        if k > 1:
            assert np.array_equal(plan.solve_minnorm(B[:, :k].copy()), one[:, :k])
    return one


@pytest.mark.parametrize("shape", [(48, 10921), (512, 10600)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_wide_fronts_beyond_the_lds_limit(pkg, oracle, shape):
    m, n = shape
    F, sym, plan = dense_plan(pkg, m, n)
    try:
        B = rhs(n, seed=m + n)
        X = refused_then_solved(pkg, plan, B, (1, 5))
        G = plan.download()
    finally:
        plan.close()
    S = symbolic_of(sym)
    N = numeric_from_gpu(S, G)
    Fa = Factors(S, N)
    assert Fa.rank == G.rank == m
    kappa = cond_probe(oracle, S, N)
    d = rel(X, minnorm_from_factors(Fa, B, None))
    live = Fa.pivot_col
    res = float(max(np.linalg.norm(F[:, live].T @ X[:, j] - B[live, j]) / (np.linalg.norm(F[:, live]) * np.linalg.norm(X[:, j]) + np.linalg.norm(B[live, j]))
                    for j in range(X.shape[1])))
    print(f"\n[minnorm] dense {m}x{n}: vs long double {d:.2e} (allowed {solve_tol(kappa):.1e}), residual {res:.2e}")
    assert d <= solve_tol(kappa)
    assert res <= 1e-10


def test_wide_triangle_of_205_blocks(pkg):
    """One dense front with 6552 live pivot columns: 20 * 6552 + 48 > 131072 bytes, 205 blocks of 32.  The issue's shape is
    6600 x 6552; the float64 reference QR of that takes more than a few seconds on 16 CPUs, so this is the smallest m >= n, the
    square 6552 x 6552.  The reference is x = Q (R' \\ b) with the float64 Q, R of LAPACK's Householder QR (Q applied as its
    reflectors rather than formed: the same Q at half the cost).  The tolerance is solve_tol of a LOWER estimate of cond(R) from
    three probes each way (an SVD of R would take longer than everything else here): never wider than solve_tol(cond(R))."""
    n = m = 6552
    assert (n + 31) // 32 == 205 and 20 * n + 48 > 131072
    F, sym, plan = dense_plan(pkg, m, n)
    try:
        B = rhs(n, seed=3)[:, :2]
        with pytest.raises(pkg.StmmqrError) as e:
            plan.rsolve(3, B[:, 0].copy())
        assert e.value.code == -3 and REFUSAL in str(e.value)
        X = plan.solve_minnorm(B)
        assert np.array_equal(plan.solve_minnorm(B[:, 1].copy()), X[:, 1])
        rank = plan.download().rank
    finally:
        plan.close()
    assert rank == n
    (qr, tau), R = sla.qr(F, mode="raw")
    Y = sla.solve_triangular(R, B, trans="T")
    ref, _, info = sla.lapack.dormqr("L", "N", qr, tau, np.asfortranarray(Y), max(1, 64 * m))
    assert info == 0
    rng = np.random.default_rng(1)
    Z = rng.standard_normal((n, 3))
    up = np.linalg.norm(R @ Z, axis=0) / np.linalg.norm(Z, axis=0)
    dn = np.linalg.norm(sla.solve_triangular(R, Z), axis=0) / np.linalg.norm(Z, axis=0)
    kappa = float(up.max() * dn.max())
    d = rel(X, ref)
    res = float(max(np.linalg.norm(F.T @ X[:, j] - B[:, j]) / (np.linalg.norm(F) * np.linalg.norm(X[:, j]) + np.linalg.norm(B[:, j])) for j in range(2)))
    print(f"\n[minnorm] dense {m}x{n}: vs float64 QR {d:.2e} (cond(R) >= {kappa:.2e}, allowed {solve_tol(kappa):.1e}), residual {res:.2e}")
    assert d <= solve_tol(kappa)
    assert res <= 1e-10


# ---- 6. the flagship structure ----
def test_c5mini_standin(pkg):
    g, S, plan = golden_plan(pkg, "c5mini_standin")
    try:
        b = rhs(S.n, seed=6)[:, 0].copy()
        with pytest.raises(pkg.StmmqrError) as e:
            plan.rsolve(3, b)
        assert e.value.code == -3 and REFUSAL in str(e.value)
        x = plan.solve_minnorm(b)
        rank = plan.download().rank
    finally:
        plan.close()
    assert S.m == S.n == rank                                               # square and full rank: the solution is unique
    assert np.all(np.isfinite(x))
    M = sp.csc_matrix((g["in_Ax"], g["in_Ai"], g["in_Ap"]), shape=(S.m, S.n))
    res = float(np.linalg.norm(M.T @ x - b) / (np.linalg.norm(g["in_Ax"]) * np.linalg.norm(x) + np.linalg.norm(b)))
    print(f"\n[minnorm] c5mini_standin: residual of M'x = b {res:.2e}")
    assert res <= 1e-10


# ---- 7. the object: the QR object of A' gives the minimum-norm solution of A x = b ----
def transposed(name):
    g = load_golden(name)
    m, n = int(scalar(g, "in_m")), int(scalar(g, "in_n"))
    A = sp.csc_matrix((g["in_Ax"], g["in_Ai"], g["in_Ap"]), shape=(m, n)).T.tocsc()
    A.sort_indices()
    return A


@pytest.mark.parametrize("name", ["syn_wide5x8", "syn_rand60x40", "rect_wide_skew_banner.mtx"])
def test_object_min2norm(pkg, name):
    """A x = b must be solvable for a minimum-norm solution to exist: b = A x0 (a wide A of full row rank takes any b, the 8 x 5
    transpose of syn_wide5x8 does not)"""
    if name.endswith(".mtx"):
        m, n, Ap, Ai, Ax = pkg.read_matrix_market(MM / name)
        A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n))
    else:
        A = transposed(name)
    m, n = A.shape
    Ad = A.toarray()
    B = np.asfortranarray(Ad @ np.random.default_rng(m + n).standard_normal((n, 3)))
    q = pkg.SparseQR.lq(m, n, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64))
    try:
        info = q.info
        X = q.min2norm(B)
        comp = q.qmult(1, q.solve(3, B))
        x1 = q.min2norm(B[:, 1].copy())
    finally:
        q.close()
    sing = name.endswith(".mtx")
    assert (info["n1cols"] > 0) == sing
    ref = np.linalg.lstsq(Ad, B, rcond=None)[0]
    sv = np.linalg.svd(Ad, compute_uv=False)
    kappa = float(sv[0] / sv[sv > sv[0] * max(m, n) * np.finfo(float).eps].min())
    d = rel(X, ref)
    print(f"\n[minnorm] lq({name}) {m}x{n}: n1cols {int(info['n1cols'])}, min2norm vs lstsq {d:.2e} (cond {kappa:.1e})")
    assert X.shape == (n, 3)
    assert d <= solve_tol(kappa)
    assert np.array_equal(x1.ravel(), X[:, 1])
    if sing:
        assert rel(X, comp) <= solve_tol(kappa)
    else:
        assert np.array_equal(X, comp)


# ---- 8. refusals: the plan stays usable ----
def test_refusals(pkg):
    capi = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd.capi")
    lib = capi.lib
    g, S, p0 = golden_plan(pkg, "syn_grid2d", keep_h=False)
    try:
        with pytest.raises(pkg.StmmqrError, match="keepH") as e:
            p0.solve_minnorm(np.ones(S.n))
        assert e.value.code == -4
        assert np.all(np.isfinite(p0.rsolve(0, np.ones(S.m))))
    finally:
        p0.close()
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    fresh = pkg.HipQR(sym)                                                   # nothing factorized
    try:
        with pytest.raises(pkg.StmmqrError) as e:
            fresh.solve_minnorm(np.ones(S.n))
        assert e.value.code == -4 and "no factorization" in str(e.value)
        fresh.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        y0 = fresh.rsolve(0, np.ones(S.m))
        b = np.ones((S.n, 2), order="F")
        X = np.full((S.m, 2), 7.0, order="F")
        call = lambda ldb, ldx, nrhs: lib.stmmqr_plan_solve_minnorm(fresh._h, b.ctypes.data, ldb, X.ctypes.data, ldx, nrhs, 0, 0)
        assert call(S.n - 1, S.m, 1) == -4 and "leading dimension" in capi.last_error()
        assert call(S.n, S.m - 1, 1) == -4 and "leading dimension" in capi.last_error()
        assert lib.stmmqr_plan_solve_minnorm(fresh._h, None, S.n, X.ctypes.data, S.m, 1, 0, 0) == -4
        assert lib.stmmqr_plan_solve_minnorm(None, b.ctypes.data, S.n, X.ctypes.data, S.m, 1, 0, 0) == -4
        assert call(S.n, S.m, 0) == 0
        assert np.all(X == 7.0)                                              # nrhs = 0 writes nothing (and the refusals wrote nothing)
        assert np.array_equal(fresh.rsolve(0, np.ones(S.m)), y0)             # the plan stays usable
        assert call(S.n, S.m, 2) == 0
        assert np.array_equal(X[:, 0], fresh.solve_minnorm(np.ones(S.n)))
    finally:
        fresh.close()


def test_device_pointers_and_leading_dimensions(pkg):
    """on_device: B and X are device arrays with ldb > n and ldx > m; the bits of the host call, and the padding rows untouched"""
    lib = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd.capi").lib
    g, S, plan = golden_plan(pkg, "syn_rankdef_grid")
    m, n, k = S.m, S.n, 3
    ldb, ldx = n + 3, m + 5
    try:
        B = rhs(n)[:, :k]
        want = plan.solve_minnorm(B)
        Bd = np.full((ldb, k), np.nan, order="F")
        Bd[:n] = B
        Xd = np.full((ldx, k), -3.0, order="F")
        db, dx = pkg.device_alloc(Bd.nbytes), pkg.device_alloc(Xd.nbytes)
        try:
            pkg.device_copy(db, Bd.ctypes.data, Bd.nbytes)
            pkg.device_copy(dx, Xd.ctypes.data, Xd.nbytes)
            assert lib.stmmqr_plan_solve_minnorm(plan._h, db, ldb, dx, ldx, k, 0, 1) == 0
            pkg.device_copy(Xd.ctypes.data, dx, Xd.nbytes)
        finally:
            pkg.device_free(db); pkg.device_free(dx)
    finally:
        plan.close()
    assert np.array_equal(Xd[:m], want)
    assert np.all(Xd[m:] == -3.0)
