"""Damped, weighted least squares on the GPU: DampedLeastSquares (stmmqr_ls_create_damped / stmmqr_ls_solve_damped) against the plain
LeastSquares of the explicit matrix [W A; D | W B; 0] (bit for bit: the same analysis, the same values, the same tolerance), against
numpy.linalg.lstsq of the dense augmented matrix (the yardstick tests/test_damped_cpu.py validates without a GPU), against the plain
object of A at lambda = 0, and against itself (no state between solves, device pointers, refusals)."""
import importlib

import numpy as np
import pytest

from leverage_reference import allowed, dense_leverages
from stmmqr_testlib import EPS, cond_probe, numeric_from_gpu, solve_tol
from test_carried_cpu import symbolic_of
from test_damped_cpu import (RANKDEF, REAL, SMALL, argument_refusals, damping_cases, dense_of, explicit, explicit_rhs, matrix_of, scales,
                             weights)

pytestmark = pytest.mark.gpu

FULL = [nm for nm in SMALL + REAL if nm not in RANKDEF]


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def rhs(m, k, seed=31):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((m, k)))


def column_norms(n, Ap, Ai, Ax, w):
    v = Ax if w is None else w[Ai] * Ax
    return np.array([np.linalg.norm(v[Ap[j]:Ap[j + 1]]) for j in range(n)])


def clamps(cn):
    """scale_min / scale_max between the quartiles of the non-zero column norms: both clamps act wherever the norms differ"""
    nz = np.sort(cn[cn > 0])
    return float(nz[len(nz) // 4]) * 1.0000001, float(nz[(3 * len(nz)) // 4]) * 0.9999999


# ---- 1: the plain object of the explicit matrix, bit for bit ----
@pytest.mark.parametrize("tol", [-2.0, 1e-9])
@pytest.mark.parametrize("name", SMALL + REAL)
def test_bits_of_the_plain_object_of_the_explicit_matrix(pkg, name, tol):
    """X, resid and info["tol"] of a damped solve have the bits of LeastSquares on [W A; D] with B' = [W B; 0], ordering 3 with the
    damped object's Qfill[:n] and the same tol argument: w given and None, d given, scale 0 and 1; tol = -2 is the device's rule
    (k_rf_colnorm on the built values) against the host's.  The two Qfill are asserted equal first; with a GIVEN order the plain
    object takes the permutation as it is (no singleton search), so no fixture here makes it reorder -- the empty column of
    syn_emptycol, a singleton of the explicit matrix, included -- and none needs the weaker comparison.
    (On the code before the damped mode there is no DampedLeastSquares: this test cannot pass there.)"""
    m, n, Ap, Ai, Ax = matrix_of(name)
    k = 2
    B = rhs(m, k)
    w, s = weights(m), scales(n)
    smin, smax = clamps(column_norms(n, Ap, Ai, Ax, w))
    cases = [("w, scale 0", dict(w=w, lam=1e-2)), ("d", dict(d=s, lam=0.3)), ("w, d", dict(w=w, d=s, lam=2.0)),
             ("w, scale 1", dict(w=w, lam=1e-3, scale=1, scale_min=smin, scale_max=smax)), ("scale 1", dict(lam=10.0, scale=1))]
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k, tol=tol)
    P = None
    try:
        Q = L.symbolic()["Qfill"]
        for label, kw in cases:
            X, resid, dnorm, D = L.solve(B, **kw)
            if "d" in kw:
                assert np.array_equal(bits(D), bits(np.sqrt(kw["lam"]) * s)), "D_jj = sqrt(lambda) * d_j, one product"
            elif not kw.get("scale"):
                assert np.array_equal(bits(D), bits(np.full(n, np.sqrt(kw["lam"]))))
            Cp, Ci, Cx = explicit(m, n, Ap, Ai, Ax, kw.get("w"), D)
            Be = explicit_rhs(B, kw.get("w"), n)
            if P is None:
                P = pkg.LeastSquares(m + n, n, Cp, Ci, Cx, nrhs=k, ordering=3, Quser=Q[:n], tol=tol)
                assert np.array_equal(P.symbolic()["Qfill"], Q)
            Xp, rp = P.solve(Be, Ax=Cx)
            ti, tp = L.info["tol"], P.info["tol"]
            print(f"[damped bits] {name} tol {tol} {label}: tol used {ti:.17g} rank {int(L.info['rank'])}/{n} resid {resid}")
            assert bits(np.array([ti]))[0] == bits(np.array([tp]))[0]
            assert int(L.info["rank"]) == int(P.info["rank"])
            assert np.array_equal(bits(X), bits(Xp)) and np.array_equal(bits(resid), bits(rp))
        assert L.info["analyses"] == 1 and L.info["plans"] == 1 and L.info["retries"] == 0
    finally:
        L.close()
        if P is not None:
            P.close()


# ---- 2: the dense solution ----
@pytest.mark.parametrize("name", SMALL)
def test_against_the_dense_solution(pkg, name):
    """numpy.linalg.lstsq of the dense [W A; D] and [W B; 0]: |x - x_ref| <= solve_tol(cond_2) |x_ref| (the bar of the CPU file), rank
    n since every D_jj is above the tolerance, and x_j == 0.0 exactly for the empty column of syn_emptycol"""
    m, n, Ap, Ai, Ax = matrix_of(name)
    k = 3
    B = rhs(m, k)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    try:
        for (label, w, D), kw in zip(damping_cases(m, n), (dict(lam=1e-2), dict(d=scales(n), lam=0.3))):
            X, resid, dnorm, Dg = L.solve(B, w=w, **kw)
            info = L.info
            assert np.array_equal(bits(Dg), bits(D))
            Cd = dense_of(m + n, n, *explicit(m, n, Ap, Ai, Ax, w, D))
            Be = explicit_rhs(B, w, n)
            Xr = np.linalg.lstsq(Cd, Be, rcond=None)[0]
            kappa = float(np.linalg.cond(Cd))
            dx = np.linalg.norm(X - Xr, axis=0) / np.maximum(np.linalg.norm(Xr, axis=0), 1e-300)
            print(f"[damped dense] {name} {label}: cond {kappa:.2e} |x - lstsq| / |lstsq| {dx.max():.2e} (allowed {solve_tol(kappa):.1e}) "
                  f"rank {int(info['rank'])}/{n} tol {info['tol']:.2e}")
            assert D.min() > info["tol"] and int(info["rank"]) == n and info["retries"] == 0
            assert np.all(dx <= solve_tol(kappa))
            for j in np.flatnonzero(np.diff(Ap) == 0):
                assert np.all(X[j, :] == 0.0)
        if name == "syn_emptycol":
            assert np.any(np.diff(Ap) == 0)
    finally:
        L.close()


# ---- 3: lambda = 0, no weights: the plain object of A ----
@pytest.mark.parametrize("name", SMALL + REAL)
def test_lambda_zero_is_the_plain_problem(pkg, oracle, name):
    """D = 0 and W = I: the problem of the plain object, on another tree (n more rows), so no bits.  Full rank: X within
    solve_tol(cond_probe) of the plain object's, cond_probe of a plan of A alone in the same column order.  Rank-deficient: the same
    rank and the same residual norms to that bar (times |b_j|)."""
    m, n, Ap, Ai, Ax = matrix_of(name)
    k = 2
    B = rhs(m, k)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    P = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    try:
        X, resid, dnorm, D = L.solve(B)
        Xp, rp = P.solve(B)
        rank, rankp, tol = int(L.info["rank"]), int(P.info["rank"]), P.info["tol"]
        q = P.symbolic()["Qfill"][:n]
    finally:
        L.close(); P.close()
    assert np.all(D == 0.0) and np.all(dnorm == 0.0)
    sym = {kk: v for kk, v in pkg.analyze(m, n, Ap, Ai, Qfill=q).items() if kk != "info"}
    plan = pkg.HipQR({**sym, "keepH": 1})
    try:
        plan.factorize(Ax, tol, n, Ap, Ai)
        S = symbolic_of(sym)
        kappa = cond_probe(oracle, S, numeric_from_gpu(S, plan.download()))
    finally:
        plan.close()
    bar = solve_tol(kappa)
    dr = np.abs(resid - rp) / np.linalg.norm(B, axis=0)
    print(f"[damped lambda 0] {name}: rank {rank} (plain {rankp}) of {n}, cond_probe {kappa:.2e}, resid diff / |b| {dr.max():.2e} (allowed {bar:.1e})")
    assert rank == rankp
    assert np.all(dr <= bar)
    if name in FULL:
        assert rank == n
        dx = np.linalg.norm(X - Xp, axis=0) / np.maximum(np.linalg.norm(Xp, axis=0), 1e-300)
        print(f"  |x - x_plain| / |x_plain| {dx.max():.2e}")
        assert np.all(dx <= bar)
    else:
        assert rank < n


# ---- 4: resid, dnorm, D_out ----
@pytest.mark.parametrize("name", SMALL)
def test_resid_dnorm_and_marquardt_scales(pkg, name):
    """resid[j] against sqrt(|W (b - A x)|^2 + |D x|^2) recomputed in float64 from the returned X, to solve_tol(kappa) |W b_j| (and
    the squares to the same number, as the issue words it); dnorm against |D x_j| to (n + 4) eps relative: a product and a sum of n
    squares, a root; the Marquardt D against sqrt(lambda) clip(|W A(:,j)|) to (k + 4) eps relative, k the longest column.
    syn_emptycol: the zero column gets scale_min, and both clamps act (asserted on the reference's side)."""
    import scipy.sparse as sp
    m, n, Ap, Ai, Ax = matrix_of(name)
    k = 2
    B = rhs(m, k)
    w = weights(m)
    cn = column_norms(n, Ap, Ai, Ax, w)
    smin, smax = clamps(cn)
    lam = 0.04
    if name in ("syn_emptycol", "syn_rand60x40"):
        assert np.any((cn > 0) & (cn < smin)) and np.any(cn > smax) and np.any((cn >= smin) & (cn <= smax))
    if name == "syn_emptycol":
        assert np.any(cn == 0.0)
    want = np.sqrt(lam) * np.where(cn == 0.0, smin, np.clip(cn, smin, smax))
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    try:
        X, resid, dnorm, D = L.solve(B, w=w, lam=lam, scale=1, scale_min=smin, scale_max=smax)
        assert int(L.info["rank"]) == n
    finally:
        L.close()
    longest = int(np.diff(Ap).max())
    dd = np.abs(D - want) / want
    print(f"[damped scales] {name}: max |D - want| / want {dd.max():.2e} (allowed {(longest + 4) * EPS:.2e}); clamped below "
          f"{int(((cn > 0) & (cn < smin)).sum())} above {int((cn > smax).sum())} zero {int((cn == 0).sum())}")
    assert np.all(dd <= (longest + 4) * EPS)
    assert np.all(D[cn == 0.0] == np.sqrt(lam) * smin)
    A = sp.csc_matrix((Ax, Ai, Ap), shape=(m, n))
    kappa = float(np.linalg.cond(dense_of(m + n, n, *explicit(m, n, Ap, Ai, Ax, w, D))))
    for j in range(k):
        dx = np.linalg.norm(D * X[:, j])
        true2 = float(np.sum((w * (B[:, j] - A @ X[:, j])) ** 2) + dx ** 2)
        wb = np.linalg.norm(w * B[:, j])
        print(f"  rhs {j}: resid {resid[j]:.16e} recomputed {np.sqrt(true2):.16e} dnorm {dnorm[j]:.16e} |D x| {dx:.16e}")
        assert abs(resid[j] - np.sqrt(true2)) <= solve_tol(kappa) * wb
        assert abs(resid[j] ** 2 - true2) <= solve_tol(kappa) * wb
        assert abs(dnorm[j] - dx) <= (n + 4) * EPS * dx
        assert resid[j] <= wb * (1 + solve_tol(kappa))                    # x = 0 costs |W b|: the minimum is not above it


# ---- 5: no state between solves ----
@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_emptycol", "syn_star", "bcsstk14"])
def test_no_state_between_solves(pkg, name):
    """one object, four solves whose inputs differ in every way that could leave something behind -- weights then none, another
    lambda, new values then those of create --, each bit-equal to a fresh object's single solve with those inputs"""
    m, n, Ap, Ai, Ax = matrix_of(name)
    k = 2
    rng = np.random.default_rng(41)
    B = rhs(m, k)
    w1, w2 = weights(m, 42), weights(m, 43)
    Ax2 = Ax * (1.0 + 1e-3 * rng.standard_normal(Ax.size))
    steps = [dict(w=w1, lam=1e-2), dict(lam=5.0), dict(Ax=Ax2, w=w2, lam=1e-2), dict(lam=0.0)]
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    try:
        got = [L.solve(B, **kw) for kw in steps]
        info = L.info
    finally:
        L.close()
    assert info["analyses"] == 1 and info["plans"] == 1 and info["solves"] == 4 and info["retries"] == 0
    for i, kw in enumerate(steps):
        kw = dict(kw)
        F = pkg.DampedLeastSquares(m, n, Ap, Ai, kw.pop("Ax", Ax), nrhs=k)
        try:
            ref = F.solve(B, **kw)
        finally:
            F.close()
        for a, b, what in zip(got[i], ref, ("X", "resid", "dnorm", "D")):
            assert np.array_equal(bits(a), bits(b)), f"solve {i + 1}: {what} is not a fresh object's"


# ---- 6: device pointers ----
@pytest.mark.parametrize("nrhs", [1, 33])
@pytest.mark.parametrize("name", ["syn_rand60x40", "bcsstk14"])
def test_device_pointers(pkg, name, nrhs):
    """solve_dev with every array on the device gives the bits of solve(); 33 right-hand sides cross one STMMQR_RHS_BATCH of 32 in the
    carried back substitution"""
    import torch
    m, n, Ap, Ai, Ax = matrix_of(name)
    B = rhs(m, nrhs)
    w, s = weights(m), scales(n)
    Ax2 = Ax * (1.0 + 1e-3 * np.random.default_rng(44).standard_normal(Ax.size))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                                       # noqa: E731
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=nrhs)
    try:
        for kw in (dict(w=w, d=s, lam=0.5, Ax=Ax2), dict(w=w, lam=1e-2, scale=1), dict(lam=1e-2)):
            X, resid, dnorm, D = L.solve(B, **kw)
            dB = dev(B.T)
            dX = torch.zeros((nrhs, n), dtype=torch.float64, device="cuda")
            dr, dn = torch.zeros(nrhs, dtype=torch.float64, device="cuda"), torch.zeros(nrhs, dtype=torch.float64, device="cuda")
            dD = torch.zeros(n, dtype=torch.float64, device="cuda")
            keep = {kk: dev(kw[kk]) for kk in ("w", "d", "Ax") if kk in kw}
            ptr = lambda kk: keep[kk].data_ptr() if kk in keep else None                                   # noqa: E731
            torch.cuda.synchronize()
            r = L.solve_dev(dB.data_ptr(), dX.data_ptr(), ax_ptr=ptr("Ax"), w_ptr=ptr("w"), d_ptr=ptr("d"), lam=kw["lam"],
                            scale=kw.get("scale", 0), resid_ptr=dr.data_ptr(), dnorm_ptr=dn.data_ptr(), D_ptr=dD.data_ptr())
            torch.cuda.synchronize()
            Xd = np.asfortranarray(dX.cpu().numpy().T)
            assert np.array_equal(bits(Xd), bits(X.reshape(n, nrhs)))
            assert np.array_equal(bits(r), bits(resid)) and np.array_equal(bits(dr.cpu().numpy()), bits(resid))
            assert np.array_equal(bits(dn.cpu().numpy()), bits(dnorm)) and np.array_equal(bits(dD.cpu().numpy()), bits(D))
        assert L.info["analyses"] == 1 and L.info["plans"] == 1 and L.info["solves"] == 6
    finally:
        L.close()


# ---- 7: diagnostics ----
@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_wide5x8"])
def test_diagnostics_of_a_damped_fit(pkg, name):
    """variances() against the diagonal of the dense inv(A'W^2 A + D^2), the bar of tests/test_gpu_selinv.py (its judge); leverages()
    (m + n values) against the dense hat diagonal of [W A; D], the bar of tests/test_gpu_leverage.py (leverage_reference.allowed, its
    worst); the first m sum to the trace of the ridge hat matrix, all of them to n.  kappa: cond_2 of the dense [W A; D].
    condest(), both kinds, two-sided as tests/test_gpu_condest.py holds every estimate (its check_estimate, as its test of the carried
    view uses it): against R11 read from the damped object's own downloaded factors -- the 1-norm exact to (r + 2) eps, the 2-norm and
    both inverse estimates equal to the yardstick's own Hager / power run on R11 to solve_tol with the same round count, never above
    the exact norms, and |R11 E'v| inv_norm = 1 for the returned vector.  R11 is then tied to the dense matrix: its exact conditions are
    those of R of the dense [W A; D](:, Qfill) to solve_tol, so the estimate is a lower bound of the dense condition, within the factor
    the yardstick's run on that condition gives."""
    from types import SimpleNamespace
    import condest_reference as cr
    from test_gpu_condest import check_estimate
    from test_gpu_leverage import dense_variances, worst
    from test_gpu_selinv import judge
    m, n, Ap, Ai, Ax = matrix_of(name)
    w = weights(m)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=1)
    try:
        with pytest.raises(pkg.StmmqrError) as e:                            # before any solve
            L.leverages()
        assert e.value.code == -4
        x, resid, dnorm, D = L.solve(rhs(m, 1)[:, 0], w=w, lam=0.25)
        assert int(L.info["rank"]) == n
        var, lev = L.variances(), L.leverages()
        lev2, var2 = L.diagnostics()
        c1, c2 = L.condest(1, with_vector=True), L.condest(2, with_vector=True)
        Sab, Nab = symbolic_of(L.symbolic()), L.plan().download()
        cv = L.covariance(np.array([0, n - 1]), np.array([0, n - 1]))
        N0 = L.nullspace()
        q = L.symbolic()["Qfill"][:n]
        R = L.r_sparse()
    finally:
        L.close()
    assert lev.shape == (m + n,) and var.shape == (n,)
    assert np.array_equal(bits(lev), bits(lev2)) and np.array_equal(bits(var), bits(var2))
    assert np.array_equal(bits(cv), bits(var[[0, n - 1]]))
    assert N0.shape == (n, 0) and len(R["ptr"]) == n + 1
    Cd = dense_of(m + n, n, *explicit(m, n, Ap, Ai, Ax, w, D))
    kappa = float(np.linalg.cond(Cd))
    live = np.ones(n, bool)
    judge(var, dense_variances(Cd, live), live, kappa, f"damped {name}")
    ref = dense_leverages(Cd, live)
    al = allowed(ref, np.abs(Cd).sum(axis=1), float(np.max(dense_variances(Cd, live))), kappa)
    r = worst(lev, ref, al)
    edf, trace = float(lev[:m].sum()), float(ref[:m].sum())
    print(f"[damped diagnostics] {name}: cond {kappa:.2e} max |h - ref| / allowed {r:.2e}; effective dof {edf:.12f} (dense {trace:.12f}) "
          f"sum {float(lev.sum()):.12f} of {n}; condest 1-norm {c1['cond']:.3e} 2-norm {c2['cond']:.3e}")
    assert r <= 1
    assert abs(edf - trace) <= float(al[:m].sum()) and abs(float(lev.sum()) - n) <= float(al.sum())
    assert edf < n                                                           # the D rows carry the rest
    R11, cols = cr.rlive_from_r_only(Sab, Nab, ncol=n)
    assert R11.shape == (n, n) and np.array_equal(cols, np.arange(n))
    T11 = np.asarray(R11, float)
    ex = cr.exact(T11)
    view = SimpleNamespace(rank=n, n=n, Rlive=R11, pivot_col=cols)
    check_estimate(c1, 1, view, ex, q, f"damped {name}", True, cr.hager(T11))
    check_estimate(c2, 2, view, ex, q, f"damped {name}", True, cr.power2(T11, 8))
    k1 = float(np.linalg.cond(np.linalg.qr(Cd[:, q], mode="r"), 1))          # (the 1-norm condition belongs to R of this column order)
    print(f"  exact conditions of R11 {ex['cond1']:.6e} / {ex['cond2']:.6e}, of the dense matrix {k1:.6e} / {kappa:.6e}; estimate / dense "
          f"{c1['cond'] / k1:.3f} / {c2['cond'] / kappa:.3f}")
    assert abs(ex["cond2"] - kappa) <= solve_tol(kappa) * kappa and abs(ex["cond1"] - k1) <= solve_tol(k1) * k1
    assert c2["cond"] <= kappa * (1.0 + 4 * (n + 2) * EPS) * (1.0 + 2 * solve_tol(kappa))
    assert c1["cond"] <= k1 * (1.0 + (n + 2) * EPS) * (1.0 + 2 * solve_tol(k1))


# ---- 8: refusals on a live object ----
def test_refusals_leave_the_object_usable(pkg):
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    k = 2
    B = rhs(m, k)
    w = weights(m)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    P = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    try:
        first = L.solve(B, w=w, lam=1e-2)
        Xp0, rp0 = P.solve(B)

        def after():
            again = L.solve(B, w=w, lam=1e-2)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again))
            Xp, rp = P.solve(B)
            assert np.array_equal(bits(Xp), bits(Xp0)) and np.array_equal(bits(rp), bits(rp0))

        assert len(argument_refusals(pkg, L, P, m, n, k, after=after)) == 16
        for bad in (np.ones(m + 1), np.ones(m - 1)):
            with pytest.raises(pkg.StmmqrError):
                L.solve(B, w=bad, lam=1.0)
            after()
        assert L.info["solves"] == 1 + 16 + 2 and L.info["retries"] == 0 and L.info["analyses"] == 1 and L.info["plans"] == 1
        di = L.damped_info
        assert di["ms_build"] > 0 and di["damped_bytes"] >= 8 * (Ax.size + n) + 4 * (Ax.size + n + 1)
    finally:
        L.close(); P.close()
