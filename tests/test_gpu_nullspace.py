"""The null-space basis of R and the minimum-norm projector on the resident factors (stmmqr_plan_nullspace, _project_minnorm,
_solve_lsminnorm, stmmqr_ls_nullspace, _project_minnorm).

Yardstick: tests/nullspace_reference.py on the plan's own downloaded factors (Factors): N_ref by back substitution and the projection
x - N y by a Householder least-squares solve of N y = x, both in long double (validated without a GPU in tests/test_nullspace_cpu.py).
Bounds (EPS = 2^-52, r live and d dead columns):
* |R N(:, k)|_2 in long double <= 4 x the larger of what the float64 emulation of the same two steps (the column of R, one
  solve_triangular) leaves on that column and (r + 2) EPS |R_live|_F |N(:, k)|_2; |A_in E N(:, k)|_2 <= tol + that;
* |N - N_ref| <= solve_tol(cond2(R_live)) |N_ref(:, k)| per column;
* the projector: info[3] >= 1 - (d + 2) EPS, |N_ref' x_out| <= 8 (d + 2) EPS |N_ref|_F |x_in|, |x_out| <= |x_in| (1 + 8 (d + 2) EPS),
  |R E'(x_out - x_in)| <= the R N bound times |z|_1, |x_out - yardstick| <= solve_tol(cond2(R_live) max(1, |W_ref|_2)) |x_in|.
cond2 of a triangle beyond 2000 rows (ex18, reorientation_8) is the power iteration's lower bound: a tighter tolerance, never a wider
one.  On lns_3937 (d = 2086, r = 1822) the long double references would take ten seconds and more: the per-column checks of R N run
on 48 evenly spaced columns, and N_ref / the yardstick come from the float64 route of tests/nullspace_reference.py, whose error
eps cond2(R_live) lies far inside the tolerances made of cond2(R_live).  |N_ref' x_out| is not made of it and is long double on every
fixture: one forward substitution with R11' per vector (nullspace_reference.nref_t_apply), never N_ref itself.
Single dense fronts with exact duplicate columns sit on the panel edges (d = 1, 31, 32, 33, 64) and, with STMMQR_NULL_SLAB=64, on the
slab edges (ncol = 63, 65, 127, 129, 191)."""
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

import nullspace_reference as nr
from minnorm_reference import dense_of, qfill_of
from resident_reference import LD, Factors, make_front, stair_csc, symbolic_of
from stmmqr_testlib import EPS, Symbolic, load_golden, numeric_from_gpu, scalar, solve_tol

pytestmark = pytest.mark.gpu
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
DEFICIENT = ["syn_dupcol", "syn_rankdef_grid", "syn_wide5x8", "ex18", "reorientation_8", "dwt_992", "lns_3937"]
EXACT = ["syn_dupcol", "syn_rankdef_grid", "syn_wide5x8", "dwt_992"]
FULL_RANK = ["syn_chain", "bcsstk14"]
# (m, n, d) of the single fronts: the panel edges of the Cholesky factorization, ncol one below / above a multiple of the 64-row slab
FRONTS = [(70, 63, 1), (72, 65, 31), (130, 127, 32), (135, 129, 33), (200, 191, 64)]


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


def sym_of(S, keep_h=True):
    return {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}


def golden_plan(pkg, name, keep_h=True, scale=1.0):
    g = load_golden(name)
    S = Symbolic(g)
    plan = pkg.HipQR(sym_of(S, keep_h))
    plan.factorize(g["in_Ax"] * scale, scalar(g, "in_tol") * abs(scale), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
    return g, S, plan


def dup_front(m, n, d):
    """a dense m x n front whose d columns `dup` are exact copies of the nearest earlier column that is none"""
    F, St = make_front(m, n)
    rng = np.random.default_rng(7 * n + d)
    dup = np.sort(rng.choice(np.arange(1, n), size=d, replace=False))
    isdup = np.zeros(n, bool)
    isdup[dup] = True
    for j in dup:
        src = j - 1
        while isdup[src]:
            src -= 1
        F[:, j] = F[:, src]
    return F, St, dup


def front_plan(pkg, m, n, d):
    F, St, dup = dup_front(m, n, d)
    Ap, Ai, Ax = stair_csc(F, St)
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    plan = pkg.HipQR(sym)
    plan.factorize(Ax, 1e-10, n, Ap, Ai)
    return symbolic_of(sym), plan, sp.csc_matrix(F), dup


class Ref:
    """everything the checks of one factorization share, computed once"""

    def __init__(self, S, plan, A, tol):
        Nn = numeric_from_gpu(S, plan.download())
        self.Fa = Fa = Factors(S, Nn)
        self.n, self.A, self.tol, self.q = Fa.n, A, float(tol), qfill_of(S)
        self.rdead = np.asarray(Nn.Rdead[:Fa.n]) != 0
        self.R11, self.R12, self.pc, self.jd = nr.blocks(Fa)
        self.r, self.d = self.pc.size, self.jd.size
        self.heavy = nr.is_heavy(self.r, self.d, self.n)
        self.Nref = nr.nullspace_ref(Fa)
        self.nfro = float(np.sqrt((np.asarray(self.Nref, float) ** 2).sum()))
        self.condR = nr.cond2(self.R11)
        self.normW = nr.norm2(self.Nref[self.pc])
        self.cols = np.arange(self.d) if not self.heavy else np.unique(np.linspace(0, self.d - 1, 48).astype(int))
        self._bound = None

    def rn_bound(self, N):
        """(bound, emulation's residual) on the columns self.cols for the device's N (R's column order)"""
        if self._bound is None:
            self._bound = nr.rn_bound(self.R11, self.R12[:, self.cols], np.asarray(nr.colnorm(N[:, self.cols]), float))
        return self._bound


_REF = {}


def reference(key, S, plan, A, tol):
    if key not in _REF:
        _REF[key] = Ref(S, plan, A, tol)
    return _REF[key]


def golden_reference(name, g, S, plan):
    A = sp.csc_matrix((g["in_Ax"], g["in_Ai"], g["in_Ap"]), shape=(S.m, S.n))
    return reference(name, S, plan, A, scalar(g, "in_tol"))


def check_basis(plan, ref, label):
    n, d, pc, jd, q = ref.n, ref.d, ref.pc, ref.jd, ref.q
    N1 = plan.nullspace(permuted=True)
    N0 = plan.nullspace()
    assert N1.shape == (n, d) == N0.shape and d == int(ref.rdead.sum()) and np.array_equal(jd, np.flatnonzero(ref.rdead))
    assert np.array_equal(N1[jd], np.eye(d))                                  # exactly the identity on the dead columns
    assert np.array_equal(N0[q], N1)                                          # N0[Qfill[k]] = N1[k], bit for bit
    cols = ref.cols
    bound, emu = ref.rn_bound(N1)
    res = np.asarray(nr.rn_residual(ref.R11, ref.R12[:, cols], N1[pc][:, cols]), float)
    ratio = float(np.max(res / bound))
    AN = np.linalg.norm(np.asarray(ref.A @ N0[:, cols]), axis=0)
    aratio = float(np.max(AN / (ref.tol + bound)))
    dn = np.asarray(nr.colnorm(np.asarray(N1, LD) - ref.Nref), float) / np.asarray(nr.colnorm(ref.Nref), float)
    allowed = solve_tol(ref.condR)
    print(f"\n[nullspace] {label}: n {n}, d {d}, cond2(R_live) {ref.condR:.2e}, |W|_2 {ref.normW:.2e}; |R N(:,k)| / bound {ratio:.2e} "
          f"(largest |R N(:,k)| {res.max():.2e}, emulation {emu.max():.2e}); |A E N(:,k)| / (tol + bound) {aratio:.2e} (largest {AN.max():.2e}, tol {ref.tol:.2e}); "
          f"|N - N_ref| / |N_ref| {dn.max():.2e} (allowed {allowed:.1e})")
    assert ratio <= 1.0
    assert aratio <= 1.0
    assert dn.max() <= allowed
    return N0, N1


def check_projector(plan, ref, X, label, again=True, orth_to_ref=True):
    """X in the caller's column order (n x k); orth_to_ref False: the check against N_ref is left to the test that holds it alone"""
    d, pc, jd, q = ref.d, ref.pc, ref.jd, ref.q
    X = np.asarray(X, float).reshape(ref.n, -1)
    Y, info = plan.project_minnorm(X, with_info=True)
    xin, xout = np.asarray(X[q], LD), np.asarray(Y[q], LD)                     # R's column order
    nin, nout = np.asarray(nr.colnorm(xin), float), np.asarray(nr.colnorm(xout), float)
    orth_allowed = 8 * (d + 2) * EPS * ref.nfro * nin
    orth = np.asarray(nr.colnorm(nr.nref_t_apply(ref.R11, ref.R12, pc, jd, xout)), float)
    z = xin[jd] - xout[jd]                                                    # x_out = x_in - N z, N the identity on jd
    D = xout - xin
    rres = np.asarray(nr.colnorm(ref.R11 @ D[pc] + ref.R12 @ D[jd]), float)
    N1 = plan.nullspace(permuted=True)
    bound, _ = ref.rn_bound(N1)
    rallowed = float(bound.max()) * np.asarray(np.abs(z).sum(axis=0), float)
    want = nr.project_ref(ref.Nref, xin)
    err = np.asarray(nr.colnorm(xout - want), float)
    allowed = solve_tol(ref.condR * max(1.0, ref.normW)) * nin
    print(f"\n[projector] {label}: d {info['d']}, min diag L - 1 = {info['min_diag_L'] - 1.0:.2e}, device's |N'x| / (|N| |x|) {info['orth']:.2e}; "
          f"|N_ref'x_out| / allowed {float(np.max(orth / orth_allowed)):.3e} (= {float(np.max(orth / (ref.nfro * nin))):.2e} of |N| |x|); "
          f"|x_out| / |x_in| {float(np.max(nout / nin)):.4f}; |R E'(x_out - x_in)| / allowed {float(np.max(rres / np.maximum(rallowed, 1e-300))):.2e}; "
          f"|x_out - yardstick| / |x_in| {float(np.max(err / nin)):.2e} (allowed {allowed[0] / nin[0]:.1e})")
    assert info["d"] == d
    assert info["min_diag_L"] >= 1.0 - (d + 2) * EPS
    assert abs(info["norm_N"] - ref.nfro) <= solve_tol(ref.condR) * ref.nfro
    assert np.all(nout <= nin * (1 + 8 * (d + 2) * EPS))
    assert np.all(rres <= rallowed)
    assert np.all(err <= allowed)
    if orth_to_ref:
        assert np.all(orth <= orth_allowed)
    if again:
        Y2 = plan.project_minnorm(Y)
        change = np.linalg.norm(Y2 - Y, axis=0)
        print(f"  projected again: change / allowed {float(np.max(change / orth_allowed)):.3e}")
        assert np.all(change <= orth_allowed)
    return Y, info


def rhs_for(ref, plan, m, k=2, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ref.n, k)), plan.solve(rng.standard_normal((m, k)))


@pytest.mark.parametrize("name", DEFICIENT)
def test_basis_on_fixtures(pkg, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        check_basis(plan, golden_reference(name, g, S, plan), name)
    finally:
        plan.close()


@pytest.mark.parametrize("name", DEFICIENT)
def test_projector_on_fixtures(pkg, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        ref = golden_reference(name, g, S, plan)
        Xr, Xb = rhs_for(ref, plan, S.m)
        check_projector(plan, ref, Xr, name + " random", orth_to_ref=False)
        check_projector(plan, ref, Xb, name + " basic solution", orth_to_ref=False)
    finally:
        plan.close()


@pytest.mark.parametrize("name", DEFICIENT)
def test_projection_is_orthogonal_to_the_reference_basis(pkg, name):
    """|N_ref' x_out| <= 8 (d + 2) EPS |N_ref|_F |x_in|, held against the REFERENCE basis: x_out is orthogonal to the device's own N, so
    this measures (N_ref - N)' x_out, the forward error of W = R11^-1 R12.  Without the refinement step of the build (a residual whose
    row sums are carried in two doubles) lns_3937, cond2(R11) = 8.3e12, missed it by 16 to 95 times; with it, 2.2e-6 of the bound."""
    g, S, plan = golden_plan(pkg, name)
    try:
        ref = golden_reference(name, g, S, plan)
        worst = []
        for label, X in zip(("random", "basic solution"), rhs_for(ref, plan, S.m)):
            Y = plan.project_minnorm(X)
            nin = np.linalg.norm(X, axis=0)
            orth = np.asarray(nr.colnorm(nr.nref_t_apply(ref.R11, ref.R12, ref.pc, ref.jd, Y[ref.q])), float)
            allowed = 8 * (ref.d + 2) * EPS * ref.nfro * nin
            print(f"\n[projector] {name} {label}: |N_ref'x_out| / allowed {float(np.max(orth / allowed)):.3e} (= {float(np.max(orth / (ref.nfro * nin))):.2e} of |N| |x|)")
            worst.append(float(np.max(orth / allowed)))
        assert max(worst) <= 1.0
    finally:
        plan.close()


@pytest.mark.parametrize("name", DEFICIENT)
def test_a_null_vector_projects_to_nothing(pkg, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        ref = golden_reference(name, g, S, plan)
        N0 = plan.nullspace()
        k = sorted({0, ref.d // 2, ref.d - 1})
        Y = plan.project_minnorm(N0[:, k])
        got = np.linalg.norm(Y, axis=0)
        allowed = 8 * (ref.d + 2) * EPS * ref.nfro * np.linalg.norm(N0[:, k], axis=0)
        print(f"\n[projector] {name}: |P N(:,k)| / allowed {float(np.max(got / allowed)):.3e}")
        assert np.all(got <= allowed)
    finally:
        plan.close()


@pytest.mark.parametrize("m,n,d", FRONTS)
def test_single_fronts_on_the_panel_and_slab_edges(pkg, env, m, n, d):
    env(STMMQR_NULL_SLAB=64)
    S, plan, A, dup = front_plan(pkg, m, n, d)
    try:
        ref = reference(("front", m, n, d), S, plan, A, 1e-10)
        assert np.array_equal(ref.jd, dup)
        check_basis(plan, ref, f"front {m}x{n} d {d}")
        Xr, Xb = rhs_for(ref, plan, m)
        check_projector(plan, ref, Xr, f"front {m}x{n} d {d} random")
        Y, _ = check_projector(plan, ref, Xb, f"front {m}x{n} d {d} basic solution")
    finally:
        plan.close()
    # another slab height: other partial sums, the same projection to rounding
    env(STMMQR_NULL_SLAB=2048)
    S, plan, A, dup = front_plan(pkg, m, n, d)
    try:
        Y2 = plan.project_minnorm(Xb)
        assert np.all(np.linalg.norm(Y2 - Y, axis=0) <= solve_tol(ref.condR * max(1.0, ref.normW)) * np.linalg.norm(Xb, axis=0))
    finally:
        plan.close()


@pytest.mark.parametrize("name", EXACT)
def test_whole_path_against_lstsq(pkg, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        A = dense_of(S.m, S.n, g["in_Ap"], g["in_Ai"], g["in_Ax"])
        s = np.linalg.svd(A, compute_uv=False)
        cond = float(s[0] / s[s > 1e-10 * s[0]][-1])
        for k in (1, 3):
            B = np.random.default_rng(20 + k).standard_normal((S.m, k))
            X, info = plan.solve_lsminnorm(B if k > 1 else B[:, 0], with_info=True)
            assert X.shape == ((S.n,) if k == 1 else (S.n, k))
            want = np.linalg.lstsq(A, B, rcond=1e-10)[0]
            err = float(np.max(np.linalg.norm(X.reshape(S.n, -1) - want, axis=0) / np.linalg.norm(want, axis=0)))
            print(f"\n[lsminnorm] {name}, {k} right-hand sides: |x - lstsq| / |lstsq| {err:.2e} (allowed {solve_tol(cond):.1e}), d {info['d']}")
            assert err <= solve_tol(cond)
            assert info["d"] == S.n - int((s > 1e-10 * s[0]).sum())
    finally:
        plan.close()


def test_same_bits(pkg, capi):
    """dwt_992: d = 496 crosses the batch edge of the build of N fifteen times, 33 vectors cross that of the projection once"""
    g, S, plan = golden_plan(pkg, "dwt_992")
    _, _, plan0 = golden_plan(pkg, "dwt_992", keep_h=False)
    n = S.n
    try:
        X = np.random.default_rng(3).standard_normal((n, 33))
        Y, info = plan.project_minnorm(X, with_info=True)
        assert info["built"]
        for j in (0, 7, 31, 32):
            assert np.array_equal(plan.project_minnorm(X[:, j]), Y[:, j])     # column j of a batch = the one-vector call
        Y2, info2 = plan.project_minnorm(X, with_info=True)
        assert np.array_equal(Y2, Y) and not info2["built"]                   # two calls; the second one found N and L
        assert info2["orth"] == info["orth"] and info2["min_diag_L"] == info["min_diag_L"]
        N = plan.nullspace()
        assert np.array_equal(plan.nullspace(), N)
        # plans with and without H
        Y0, info0 = plan0.project_minnorm(X, with_info=True)
        assert info0["built"] and np.array_equal(Y0, Y) and np.array_equal(plan0.nullspace(), N)
        # host and device output
        d = N.shape[1]
        dX, dN = pkg.device_alloc(8 * n * 33), pkg.device_alloc(8 * n * d)
        try:
            Xf = np.asfortranarray(X)
            pkg.device_copy(dX, Xf.ctypes.data, 8 * n * 33)
            info3 = np.zeros(8)
            assert capi.lib.stmmqr_plan_project_minnorm(plan._h, n, dX, n, 33, 0, 1, info3.ctypes.data_as(capi.c_double_p)) == 0
            Yd = np.zeros((n, 33), order="F")
            pkg.device_copy(Yd.ctypes.data, dX, 8 * n * 33)
            nd = capi.C.c_long(0)
            assert capi.lib.stmmqr_plan_nullspace(plan._h, n, capi.C.byref(nd), dN, n, 0, 1) == 0 and nd.value == d
            Nd = np.zeros((n, d), order="F")
            pkg.device_copy(Nd.ctypes.data, dN, 8 * n * d)
        finally:
            pkg.device_free(dX); pkg.device_free(dN)
        assert np.array_equal(Yd, Y) and np.array_equal(Nd, N) and info3[1] == info["orth"]
        # a new factorization with other values: built again, other results
        plan.factorize(g["in_Ax"] * 1.5, scalar(g, "in_tol") * 1.5, int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        Y4, info4 = plan.project_minnorm(X, with_info=True)
        assert info4["built"] and not np.array_equal(Y4, Y)
        assert np.all(np.linalg.norm(Y4 - Y, axis=0) <= 1e-9 * np.linalg.norm(X, axis=0))   # (A scaled: the same null space)
    finally:
        plan.close(); plan0.close()


def test_least_squares_object(pkg):
    """ncol < n: the plan of a LeastSquares object holds [A B]; its null space is that of A"""
    g = load_golden("syn_dupcol")
    m, n = int(scalar(g, "in_m")), int(scalar(g, "in_n"))
    A = dense_of(m, n, g["in_Ap"], g["in_Ai"], g["in_Ax"])
    ls = pkg.LeastSquares(m, n, g["in_Ap"], g["in_Ai"], g["in_Ax"], nrhs=2)
    try:
        with pytest.raises(pkg.StmmqrError, match="no solve yet"):
            ls.nullspace()
        with pytest.raises(pkg.StmmqrError, match="no solve yet"):
            ls.project_minnorm(np.ones(n))
        B = np.random.default_rng(8).standard_normal((m, 2))
        X, resid = ls.solve(B)
        N = ls.nullspace()
        s = np.linalg.svd(A, compute_uv=False)
        rank = int((s > 1e-10 * s[0]).sum())
        assert N.shape == (n, n - rank) and n - rank == 2
        assert np.all(np.linalg.norm(A @ N, axis=0) <= 1e-10)
        Xm, info = ls.project_minnorm(X, with_info=True)
        want = np.linalg.lstsq(A, B, rcond=1e-10)[0]
        err = float(np.max(np.linalg.norm(Xm - want, axis=0) / np.linalg.norm(want, axis=0)))
        print(f"\n[ls] syn_dupcol: |x - lstsq| / |lstsq| {err:.2e}, |x_min| / |x_basic| {np.linalg.norm(Xm) / np.linalg.norm(X):.3f}")
        assert err <= solve_tol(float(s[0] / s[rank - 1])) and info["d"] == 2
        assert np.allclose(np.linalg.norm(B - A @ Xm, axis=0), resid, rtol=1e-10, atol=1e-12)      # the residuals do not change
        X2, resid2 = ls.solve(B)
        assert np.array_equal(resid2, resid) and np.array_equal(X2, X)
        pab = ls.plan()
        assert np.array_equal(pab.nullspace(ncol=n), N)
        with pytest.raises(pkg.StmmqrError, match="carried solve"):
            pab.nullspace(ncol=n - 1)                                         # a view that ends elsewhere: ntol = n
    finally:
        ls.close()


@pytest.mark.parametrize("name", FULL_RANK)
def test_full_rank_is_a_no_op(pkg, capi, name):
    g, S, plan = golden_plan(pkg, name)
    try:
        plan.solve(np.ones(S.m))
        before = plan.device_bytes()
        X = np.random.default_rng(1).standard_normal((S.n, 3))
        Y, info = plan.project_minnorm(X, with_info=True)
        assert np.array_equal(Y, X) and info["d"] == 0 and not info["built"]
        assert plan.nullspace().shape == (S.n, 0)
        nd = capi.C.c_long(5)
        assert capi.lib.stmmqr_plan_nullspace(plan._h, S.n, capi.C.byref(nd), None, S.n, 0, 0) == 0 and nd.value == 0
        B = np.random.default_rng(2).standard_normal(S.m)
        assert np.array_equal(plan.solve_lsminnorm(B), plan.solve(B))
        assert plan.device_bytes() == before
    finally:
        plan.close()


def test_memory_is_counted_and_released(pkg):
    g, S, plan = golden_plan(pkg, "dwt_992")
    try:
        plan.solve(np.ones(S.m))
        before = plan.device_bytes()
        N = plan.nullspace()
        n, d = N.shape
        held = plan.device_bytes()
        assert held - before >= 8 * (n * d + d * d)
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        assert plan.device_bytes() == before
        assert np.array_equal(plan.nullspace(), N) and plan.device_bytes() == held
    finally:
        plan.close()


# ---- refusals: STMMQR_ERR_INVALID (-4) with a message that says why; the plan still solves afterwards ----
@pytest.fixture
def dupcol(pkg):
    g, S, plan = golden_plan(pkg, "syn_dupcol")
    b = np.arange(1.0, S.m + 1)
    x0 = plan.solve(b)
    yield g, S, plan
    assert np.array_equal(plan.solve(b), x0)
    assert plan.nullspace().shape == (S.n, 2)
    plan.close()


def test_refuses_null_plan_and_nothing_factorized(pkg, capi, dupcol):
    g, S, plan = dupcol
    lib, nd, X = capi.lib, capi.C.c_long(0), np.ones(S.n)
    assert lib.stmmqr_plan_nullspace(None, S.n, capi.C.byref(nd), None, S.n, 0, 0) == -4 and "no factorization" in capi.last_error()
    assert lib.stmmqr_plan_project_minnorm(None, S.n, X.ctypes.data, S.n, 1, 0, 0, None) == -4 and "no factorization" in capi.last_error()
    assert lib.stmmqr_plan_solve_lsminnorm(None, X.ctypes.data, S.m, X.ctypes.data, S.n, 1, 0, None) == -4
    fresh = pkg.HipQR(sym_of(S))
    try:
        for call in (fresh.nullspace, lambda: fresh.project_minnorm(X), lambda: fresh.solve_lsminnorm(np.ones(S.m))):
            with pytest.raises(pkg.StmmqrError, match="no factorization") as e:
                call()
            assert e.value.code == -4
    finally:
        fresh.close()


def test_refuses_bad_pointers_and_leading_dimensions(capi, dupcol):
    g, S, plan = dupcol
    lib, nd = capi.lib, capi.C.c_long(7)
    X, N = np.full((S.n, 2), 3.0, order="F"), np.full((S.n, 2), 3.0, order="F")
    B = np.ones((S.m, 2), order="F")
    assert lib.stmmqr_plan_nullspace(plan._h, S.n, None, N.ctypes.data, S.n, 0, 0) == -4 and "ndead" in capi.last_error()
    assert lib.stmmqr_plan_nullspace(plan._h, S.n, capi.C.byref(nd), N.ctypes.data, S.n - 1, 0, 0) == -4 and "leading dimension" in capi.last_error()
    assert lib.stmmqr_plan_project_minnorm(plan._h, S.n, None, S.n, 2, 0, 0, None) == -4 and "X is NULL" in capi.last_error()
    assert lib.stmmqr_plan_project_minnorm(plan._h, S.n, X.ctypes.data, S.n, -1, 0, 0, None) == -4 and "nrhs" in capi.last_error()
    assert lib.stmmqr_plan_project_minnorm(plan._h, S.n, X.ctypes.data, S.n - 1, 2, 0, 0, None) == -4 and "leading dimension" in capi.last_error()
    assert lib.stmmqr_plan_solve_lsminnorm(plan._h, None, S.m, X.ctypes.data, S.n, 2, 0, None) == -4 and "bad solve arguments" in capi.last_error()
    assert lib.stmmqr_plan_solve_lsminnorm(plan._h, B.ctypes.data, S.m - 1, X.ctypes.data, S.n, 2, 0, None) == -4
    assert lib.stmmqr_plan_solve_lsminnorm(plan._h, B.ctypes.data, S.m, X.ctypes.data, S.n - 1, 2, 0, None) == -4
    assert nd.value == 7 and np.all(X == 3.0) and np.all(N == 3.0)           # no refusal wrote anything
    assert lib.stmmqr_plan_project_minnorm(plan._h, S.n, X.ctypes.data, S.n, 0, 0, 0, None) == 0 and np.all(X == 3.0)   # nrhs = 0


def test_refuses_ncol_out_of_range_and_a_view_that_is_none(capi, dupcol):
    g, S, plan = dupcol
    lib, nd, X = capi.lib, capi.C.c_long(0), np.ones(S.n)
    for ncol in (-1, S.n + 1):
        assert lib.stmmqr_plan_nullspace(plan._h, ncol, capi.C.byref(nd), None, S.n + 1, 0, 0) == -4 and "ncol" in capi.last_error()
        assert lib.stmmqr_plan_project_minnorm(plan._h, ncol, X.ctypes.data, S.n + 1, 1, 0, 0, None) == -4 and "ncol" in capi.last_error()
    assert lib.stmmqr_plan_nullspace(plan._h, S.n - 1, capi.C.byref(nd), None, S.n, 0, 0) == -4 and "carried solve" in capi.last_error()
    assert lib.stmmqr_plan_project_minnorm(plan._h, S.n - 1, X.ctypes.data, S.n, 1, 0, 0, None) == -4 and "carried solve" in capi.last_error()


def test_refuses_a_plan_without_h_for_the_whole_path(pkg):
    g, S, plan = golden_plan(pkg, "syn_dupcol", keep_h=False)
    try:
        with pytest.raises(pkg.StmmqrError, match="keepH") as e:
            plan.solve_lsminnorm(np.ones(S.m))
        assert e.value.code == -4
        assert plan.nullspace().shape == (S.n, 2)                             # the other two read R only
        assert plan.project_minnorm(np.ones(S.n)).shape == (S.n,)
    finally:
        plan.close()


def test_refuses_a_plan_that_does_not_hold_the_whole_tree(pkg):
    g = load_golden("syn_rankdef_grid")
    S = Symbolic(g)
    parent = np.full(S.nf, -1)
    for f in range(S.nf):
        for c in range(int(S.Childp[f]), int(S.Childp[f + 1])):
            parent[int(S.Child[c])] = f
    group = np.zeros(S.nf, np.int32)
    f = int(parent[0])
    while f >= 0:
        group[f] = 1
        f = int(parent[f])
    assert group.any() and not group.all()
    plan = pkg.HipQR(sym_of(S))
    try:
        plan.set_groups(group)
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])
        for call in (plan.nullspace, lambda: plan.project_minnorm(np.ones(S.n)), lambda: plan.solve_lsminnorm(np.ones(S.m))):
            with pytest.raises(pkg.StmmqrError, match="whole tree") as e:
                call()
            assert e.value.code == -4
        assert plan.result_sizes()[1] == S.n - 3                              # the plan stays usable
    finally:
        plan.close()
