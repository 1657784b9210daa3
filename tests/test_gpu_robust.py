"""Robust least squares on the GPU (stmmqr_ls_solve_robust, stmmqr_ls_robust_weights, stmmqr_median_abs) against the numpy
yardstick of tests/robust_reference.py, which tests/test_robust_cpu.py validates without a GPU: the selection bit for bit, the
unweighted residual to its derived bound, the stages on the device's own data, the driver as the loop of its parts (bit for bit), the
fits, the refusals.  None of the entry points exists before this feature: every test here fails there."""
import importlib

import numpy as np
import pytest

import robust_reference as rr
from leverage_reference import allowed, dense_leverages
from stmmqr_testlib import EPS, solve_tol
from test_damped_cpu import dense_of, explicit, matrix_of
from test_robust_cpu import (DRIVER_CASES, FIT_CASES, FIT_RTOL, FIXTURES, LAM, driver_problem, driver_rule, estimating_residual,
                             fit_runs, prior_weights, robust_refusals, sparse_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def dzeros(k):
    import torch
    return torch.zeros(max(k, 1), dtype=torch.float64, device="cuda")


def sync():
    import torch
    torch.cuda.synchronize()


# ---- 1: the selection ----
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 4097, 100003]


def value_set(kind, n, rng):
    """(v, mask or None) of a selection case"""
    if kind == "normal":
        return rng.standard_normal(n), None
    if kind == "all equal":
        return np.full(n, -3.25), None
    if kind == "two values":
        return rng.choice([1.5, -2.5], n), None
    if kind == "mostly zeros":
        v = rng.standard_normal(n)
        v[rng.random(n) < 0.6] = 0.0
        v[: (n + 2) // 2] = 0.0
        return rng.permutation(v), None
    if kind == "denormal to 1e300":
        v = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-310, 300, n)
        v[0] = 1e-310
        v[-1] = -1e300
        return rng.permutation(v), None
    if kind == "signed zeros":
        return rng.choice([0.0, -0.0], n), None
    v = rng.standard_normal(n)
    mask = rng.uniform(0.5, 2.0, n) * rng.choice([1.0, -1.0], n)
    if kind == "mask":
        mask[rng.random(n) < 0.4] = 0.0
        mask[rng.integers(n)] = -0.0
    else:
        keep = rng.choice(n, min(n, {"mask, one left": 1, "mask, two left": 2, "mask, none left": 0}[kind]), replace=False)
        m2 = np.zeros(n)
        m2[keep] = mask[keep]
        mask = m2
    return v, mask


@pytest.mark.parametrize("kind", ["normal", "all equal", "two values", "mostly zeros", "denormal to 1e300", "signed zeros", "mask",
                                  "mask, one left", "mask, two left", "mask, none left"])
def test_selection_has_the_bits_of_numpy_partition(pkg, kind):
    """lo, hi, the median and the count of median_abs against numpy.partition on abs(mask * v) over the unmasked entries, for every
    length that crosses a wave, a workgroup, the grid's stride; host arrays, device pointers and a second call give the same bits"""
    rng = np.random.default_rng(17)
    for n in LENGTHS:
        v, mask = value_set(kind, n, rng)
        med, lo, hi, c = rr.median_abs(v, mask)
        got = pkg.median_abs(v, mask)
        again = pkg.median_abs(v, mask)
        dv, dm, dout = dev(v), None if mask is None else dev(mask), dzeros(4)
        sync()
        pkg.median_abs_dev(dv.data_ptr(), n, dout.data_ptr(), None if dm is None else dm.data_ptr())
        sync()
        out = dout.cpu().numpy()
        want = np.array([med, lo, hi, float(c)])
        have = np.array([got["median"], got["lo"], got["hi"], float(got["count"])])
        assert np.array_equal(bits(have), bits(want)), f"{kind} n = {n}: {have} against {want}"
        assert np.array_equal(bits(out), bits(want)), f"{kind} n = {n}, device pointers: {out} against {want}"
        assert again == got
        if c == 0:
            assert np.all(have == 0.0)


# ---- 2: the residual ----
def residual_bound(m, n, Ap, Ai, Ax, x, b):
    """(b - A x in longdouble, the bound per row): a row of nnz_i entries is nnz_i products and nnz_i additions in one accumulator and
    one subtraction from b_i -- at most (nnz_i + 2) roundings, each at most eps of a partial result bounded by |A_i,:| |x| + |b_i|"""
    cols = np.repeat(np.arange(n), np.diff(Ap))
    ref = np.asarray(b, np.longdouble).copy()
    np.subtract.at(ref, Ai, np.asarray(Ax, np.longdouble) * np.asarray(x, np.longdouble)[cols])
    mag = np.abs(np.asarray(b, float))
    np.add.at(mag, Ai, np.abs(Ax) * np.abs(x)[cols])
    nnz = np.bincount(Ai, minlength=m)
    return ref, (nnz + 2) * EPS * mag


@pytest.mark.parametrize("name", FIXTURES)
def test_residual_is_the_unweighted_one(pkg, name):
    """r_out against b - A x in numpy.longdouble for a random x: on a damped object AFTER a solve that gave a tenth of the rows weight 0
    (their residuals are those of A, not of W A), on a plain object after a weighted robust solve (its values on the device are
    weighted ones then), and with a device Ax that differs from the values of create"""
    m, n, Ap, Ai, Ax = matrix_of(name)
    rng = np.random.default_rng(23)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    w = prior_weights(m)
    Ax2 = Ax * rng.uniform(0.5, 2.0, Ax.size)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax)
    P = pkg.LeastSquares(m, n, Ap, Ai, Ax)
    try:
        L.solve(b, w=w, lam=LAM)
        P.solve_robust(b, loss="tukey", w0=w, max_iter=2)
        for obj, label in ((L, "damped"), (P, "plain")):
            ref, bound = residual_bound(m, n, Ap, Ai, Ax, x, b)
            r, wr, stat = obj.robust_weights(b, x, w0=w)
            err = np.abs(r.astype(np.longdouble) - ref).astype(float)
            print(f"[robust resid] {name} {label}: max |r - ref| / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
                  f"rows of weight 0: {int(np.sum(w == 0))}")
            assert np.all(err <= bound)
            assert np.all(r[w == 0] != 0.0), "a row of weight 0 keeps its residual"
            # a device Ax that is not the one of create, everything by device pointers
            ref2, bound2 = residual_bound(m, n, Ap, Ai, Ax2, x, b)
            db, dx, dax, dr, dw = dev(b), dev(x), dev(Ax2), dzeros(m), dzeros(m)
            sync()
            obj.robust_weights_dev(db.data_ptr(), dx.data_ptr(), r_ptr=dr.data_ptr(), w_ptr=dw.data_ptr(), ax_ptr=dax.data_ptr())
            sync()
            r2 = dr.cpu().numpy()[:m]
            assert np.all(np.abs(r2.astype(np.longdouble) - ref2).astype(float) <= bound2)
            r3 = obj.robust_weights(b, x, Ax=Ax2)[0]                                               # ... and as a host array
            assert np.array_equal(bits(r3), bits(r2))
            assert np.array_equal(bits(obj.robust_weights(b, x)[0]), bits(r)), "Ax = None: the values of create again"
    finally:
        L.close(); P.close()


# ---- 3: the stages on the device's own data ----
@pytest.mark.parametrize("loss", rr.LOSSES)
@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_star", "epb1"])
def test_stages_on_the_device_s_own_residual(pkg, name, loss):
    """With r_out downloaded: sigma has the bits of mad_factor * the numpy median of abs(w0 * r), floored; every w is within 4 eps |w0|
    of w0 f(a / sigma); the sum of rho is within 1e-13 of the yardstick's (summed in longdouble); the two counts are exact up to the
    rows whose u lies within 4 eps of cc, of which there are at most two"""
    m, n, Ap, Ai, Ax = matrix_of(name)
    rng = np.random.default_rng(29)
    x = rng.standard_normal(n)
    b = rr.outlier_problem(sparse_of(name), 31)[0]
    w0 = prior_weights(m)
    cc = rr.L1_CC if loss == "l1" else rr.cc_of(loss)
    P = pkg.LeastSquares(m, n, Ap, Ai, Ax)
    try:
        for prior, kw in ((w0, dict()), (None, dict(mad_factor=2.0, sigma_min=1e3)), (w0, dict(sigma=0.75))):
            r, w, stat = P.robust_weights(b, x, loss=loss, cc=cc if loss == "l1" else None, w0=prior, **kw)
            w0v = np.ones(m) if prior is None else prior
            a = np.abs(w0v * r)
            sigma = rr.scale_of(a, prior, kw.get("sigma", 0.0), kw.get("mad_factor", rr.MAD), kw.get("sigma_min", 0.0))
            assert bits([stat["sigma"]])[0] == bits([sigma])[0], f"sigma {stat['sigma']!r} against {sigma!r}"
            if "sigma" not in kw:
                med, lo, hi, c = rr.median_abs(r, prior)
                assert (stat["lo"], stat["hi"], int(stat["count"])) == (lo, hi, c)
            wy, sy = rr.weights_from(r, loss, cc, prior, **kw)
            near = int(np.sum(np.abs(sy["u"] - cc) <= 4 * EPS * cc))
            dw = np.abs(w - wy)
            print(f"[robust stages] {name} {loss} {kw}: sigma {sigma:.6g} max |w - yardstick| / (eps |w0|) "
                  f"{np.max(dw / np.maximum(EPS * np.abs(w0v), 1e-300)):.2f} loss {stat['loss']:.17g} (yardstick {sy['loss']:.17g}) "
                  f"rejected {int(stat['rejected'])} unit {int(stat['unit'])} rows within 4 eps of cc {near}")
            assert np.all(dw <= 4 * EPS * np.abs(w0v))
            assert abs(stat["loss"] - sy["loss"]) <= 1e-13 * abs(sy["loss"])
            assert near <= 2
            assert abs(int(stat["rejected"]) - sy["rejected"]) <= near and abs(int(stat["unit"]) - sy["unit"]) <= near
            assert stat["flags"] == 0.0
    finally:
        P.close()


def test_exact_fit_and_planted_outlier(pkg):
    """syn_star with integer values and an integer x: b = A x holds exactly, so r = 0, the median is 0, sigma = 0 after its floor of 0:
    w has the bits of w0, the flag is set, the loss is 0 -- for every loss, no division by zero formed.  Then one entry of b moved by 1e6
    under Tukey: that row's multiplier is exactly 0.0 and it is the one row counted as rejected."""
    m, n, Ap, Ai, Ax = matrix_of("syn_star")
    rng = np.random.default_rng(37)
    Axi = np.round(4 * Ax) + np.where(np.round(4 * Ax) == 0, 1.0, 0.0)
    x = rng.integers(-5, 6, n).astype(float)
    b = np.zeros(m)
    np.add.at(b, Ai, Axi * x[np.repeat(np.arange(n), np.diff(Ap))])
    w0 = prior_weights(m)
    for cls in (pkg.LeastSquares, pkg.DampedLeastSquares):
        L = cls(m, n, Ap, Ai, Axi)
        try:
            for loss in rr.LOSSES:
                r, w, stat = L.robust_weights(b, x, loss=loss, cc=rr.L1_CC if loss == "l1" else None, w0=w0)
                assert np.all(r == 0.0) and stat["sigma"] == 0.0 and stat["flags"] == 1.0 and stat["loss"] == 0.0
                assert np.array_equal(bits(w), bits(w0)) and stat["rejected"] == 0.0
            k = int(np.flatnonzero(w0 != 0)[3])
            b2 = b.copy()
            b2[k] += 1e6
            r, w, stat = L.robust_weights(b2, x, loss="tukey", w0=w0, sigma=1.0)
            assert w[k] == 0.0 and not np.signbit(w[k]) and stat["rejected"] == 1.0
            assert np.array_equal(bits(np.delete(w, k)), bits(np.delete(w0, k)))
        finally:
            L.close()


# ---- 4: the driver is the loop of its parts ----
def python_loop(L, damped, Ai, Ax, b, rule):
    """the loop of stmmqr_ls_solve_robust written with robust_weights and the object's own solve, w going through the host"""
    rule = dict(rule)
    w0, x0, max_iter, rtol = rule.pop("w0", None), rule.pop("x0", None), rule.pop("max_iter"), rule.pop("rtol")
    sigma_iters = rule.pop("sigma_iters", -1)
    m = b.size
    w = np.ones(m) if w0 is None else w0.copy()
    x, nrew, sig, hist = None, 0, 0.0, []

    def reweigh(xc):
        nonlocal nrew, sig
        frozen = sig if (sigma_iters >= 0 and nrew >= max(sigma_iters, 1)) else 0.0
        r, wn, stat = L.robust_weights(b, xc, w0=w0, sigma=frozen, **rule)
        nrew, sig = nrew + 1, stat["sigma"]
        return wn

    if x0 is not None:
        x = x0.copy()
        w = reweigh(x)
    converged = False
    for it in range(max_iter):
        if it > 0:
            w = reweigh(x)
        xn = L.solve(b, w=w, lam=LAM)[0] if damped else L.solve(w * b, Ax=w[Ai] * Ax)[0]
        if x is not None:
            converged = bool(np.max(np.abs(xn - x), initial=0.0) <= rtol * np.max(np.abs(xn), initial=0.0))
        x = xn
        hist.append(sig)
        if converged:
            break
    return x, w, np.array(hist), len(hist), converged


@pytest.mark.parametrize("name,damped", sorted({(c[0], c[1]) for c in DRIVER_CASES}))
def test_driver_is_the_loop_of_its_parts(pkg, name, damped):
    """solve_robust against the Python loop of robust_weights and solve(w=...) (damped) or solve(w * b, Ax = w[Ai] * Ax) (plain): X, w,
    sigma per solve, the number of solves and the converged flag agree bit for bit; so do device pointers; nothing is analysed or
    planned again; and the plain object afterwards solves with Ax = None to the bits of a new plain object"""
    m, n, Ap, Ai, Ax = matrix_of(name)
    b = driver_problem(name)[1]
    cls = pkg.DampedLeastSquares if damped else pkg.LeastSquares
    extra = dict(lam=LAM) if damped else {}
    L, Lp = cls(m, n, Ap, Ai, Ax), cls(m, n, Ap, Ai, Ax)
    try:
        for lab in [c[2] for c in DRIVER_CASES if c[:2] == (name, damped)]:
            rule = driver_rule(lab, m, n)
            X, w, info = L.solve_robust(b, **rule, **extra)
            Xp, wp, sp_, solves, conv = python_loop(Lp, damped, Ai, Ax, b, rule)
            print(f"[robust driver] {name} {'damped' if damped else 'plain'} {lab}: {info['solves']} solves (loop {solves}) converged "
                  f"{info['converged']} sigma {info['sigma']:.6g} rejected {int(info['rejected'])} reweighting ms {info['ms_reweight']:.3f}")
            assert (info["solves"], info["converged"]) == (solves, conv)
            assert np.array_equal(bits(X), bits(Xp)) and np.array_equal(bits(w), bits(wp))
            assert np.array_equal(bits(info["hist"][:, 0]), bits(sp_))
            # device pointers
            db, dX, dw, dres = dev(b), dzeros(n), dzeros(m), dzeros(1)
            dw0 = dev(rule["w0"]) if "w0" in rule else None
            dx0 = dev(rule["x0"]) if "x0" in rule else None
            kw = {k: v for k, v in rule.items() if k not in ("w0", "x0")}
            sync()
            di = L.solve_robust_dev(db.data_ptr(), dX.data_ptr(), w_ptr=dw.data_ptr(), resid_ptr=dres.data_ptr(),
                                    w0_ptr=None if dw0 is None else dw0.data_ptr(), x0_ptr=None if dx0 is None else dx0.data_ptr(), **kw, **extra)
            sync()
            assert np.array_equal(bits(dX.cpu().numpy()[:n]), bits(X)) and np.array_equal(bits(dw.cpu().numpy()[:m]), bits(w))
            assert np.array_equal(bits(di["hist"]), bits(info["hist"])) and di["solves"] == info["solves"]
            assert bits(dres.cpu().numpy()[:1])[0] == bits([info["resid"]])[0]
        assert L.info["analyses"] == 1 and L.info["plans"] == 1
        assert info["robust_bytes"] >= 4 * (m + 1 + 2 * int(Ap[-1])) and L.info["device_bytes"] > info["robust_bytes"]
        if not damped:
            fresh = pkg.LeastSquares(m, n, Ap, Ai, Ax)
            try:
                Xa, ra = L.solve(b)
                Xf, rf = fresh.solve(b)
            finally:
                fresh.close()
            assert np.array_equal(bits(Xa), bits(Xf)) and np.array_equal(bits(ra), bits(rf)), "Ax = None uploads the values of create again"
    finally:
        L.close(); Lp.close()


# ---- 5: it fits ----
@pytest.mark.parametrize("case", FIT_CASES, ids=lambda c: f"{c[0]}-{'damped' if c[1] else 'plain'}")
def test_it_fits(pkg, case):
    """b = A x_true + 1e-3 noise, 15 % of the rows replaced by +-100 (tests/test_robust_cpu.py: the cases, and why epb1 is fitted with
    the damping and a small max_iter).  Huber with a fixed scale and rtol = 1e-12: |A'(psi(u) sign r) - D^2 x / sigma|_inf of the
    device's result is at most ten times what the yardstick's own result leaves at the same rtol and max_iter, plus
    solve_tol(kappa) * sum_i |A_ij| |psi_i| (the rule of DESIGN 6q for a quantity that two correct solves give differently); kappa is
    cond_2 of the dense [W A; D] with the final multipliers, for epb1 its upper bound sqrt(|W A|_1 |W A|_inf + lambda) / sqrt(lambda).
    |x - x_true| of the Huber and Tukey fits is below the L2 fit's.  Tukey on a plain object: the loss does not increase once the scale
    is frozen (with damping the loop lowers sum rho + |D x|^2 / (2 sigma^2), so sum rho alone is not held to that).  On the damped
    object leverages() and variances() agree with the dense [W A; D] built from w_out within leverage_reference.allowed (epb1: on a
    sample of rows and columns through a sparse factorization of the normal equations, with 1 / lambda bounding the variances).
    Measured: see DESIGN 6r."""
    name, damped, seed, sigma, max_iter = case
    m, n, Ap, Ai, Ax = matrix_of(name)
    A, b, xt, D, l2, hub, tuk = fit_runs(*case)
    cls = pkg.DampedLeastSquares if damped else pkg.LeastSquares
    extra = dict(lam=LAM) if damped else {}
    L = cls(m, n, Ap, Ai, Ax)
    try:
        X2 = L.solve_robust(b, loss="l2", max_iter=1, **extra)[0]
        Xt, wt, it = L.solve_robust(b, loss="tukey", sigma_iters=2, max_iter=max_iter, rtol=FIT_RTOL, **extra)
        Xh, wh, ih = L.solve_robust(b, loss="huber", sigma=sigma, max_iter=max_iter, rtol=FIT_RTOL, **extra)
        lev, var = (L.leverages(), L.variances()) if damped else (None, None)
    finally:
        L.close()
    g, scale = estimating_residual(A, b, Xh, sigma, D)
    gy, _ = estimating_residual(A, b, hub[0], sigma, D)
    if name == "epb1":
        WA = abs(A.multiply(wh[:, None]).tocsc())
        kappa = float(np.sqrt(WA.sum(axis=0).max() * WA.sum(axis=1).max() + LAM) / np.sqrt(LAM))
    else:
        C = wh[:, None] * A
        kappa = float(np.linalg.cond(np.vstack([C, np.diag(D)]) if damped else C))
    bar = 10 * np.abs(gy).max() + solve_tol(kappa) * scale
    e2, eh, et = (float(np.abs(x - xt).max()) for x in (X2, Xh, Xt))
    print(f"[robust fit] {name} {'damped' if damped else 'plain'}: Huber {ih['solves']} solves (yardstick {hub[2]['solves']}) converged "
          f"{ih['converged']}; |estimating equation|_inf device {np.abs(g).max():.3e} yardstick {np.abs(gy).max():.3e} "
          f"worst entry / bar {np.max(np.abs(g) / bar):.3e} kappa {kappa:.3g}; |x - x_true|_inf L2 {e2:.4g} Huber {eh:.4g} Tukey {et:.4g} "
          f"({it['solves']} solves, {int(it['rejected'])} rows rejected)")
    assert np.all(np.abs(g) <= bar)
    assert eh < e2 and et < e2
    if not damped:
        h = it["hist"][:, 1]
        assert np.all(np.diff(h[2:]) <= 1e-12 * h[2:-1])
    if damped and name != "epb1":
        Cd = dense_of(m + n, n, *explicit(m, n, Ap, Ai, Ax, wh, D))
        live = np.ones(n, bool)
        vref = np.diag(np.linalg.inv(Cd.T @ Cd))
        kd = float(np.linalg.cond(Cd))
        ref = dense_leverages(Cd, live)
        al = allowed(ref, np.abs(Cd).sum(axis=1), float(vref.max()), kd)
        assert np.all(np.abs(lev - ref) <= al)
        assert np.all(np.abs(var - vref) <= allowed(vref, np.ones(n), float(vref.max()), kd))
    elif damped:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        WAs = A.multiply(wh[:, None]).tocsc()
        lu = spla.splu((WAs.T @ WAs + LAM * sp.identity(n)).tocsc())
        rng = np.random.default_rng(41)
        rows, cols = rng.choice(m, 40, replace=False), rng.choice(n, 40, replace=False)
        rowsT = WAs.tocsr()[rows].toarray().T
        ref = np.einsum("ij,ij->j", rowsT, lu.solve(rowsT))
        E = np.zeros((n, cols.size))
        E[cols, np.arange(cols.size)] = 1.0
        vref = lu.solve(E)[cols, np.arange(cols.size)]
        al = allowed(ref, np.abs(rowsT).sum(axis=0), 1.0 / LAM, kappa)
        assert np.all(np.abs(lev[rows] - ref) <= al)
        assert np.all(np.abs(var[cols] - vref) <= allowed(vref, np.ones(cols.size), 1.0 / LAM, kappa))


# ---- 6: the refusals ----
def test_refusals_leave_the_objects_usable(pkg):
    """every refusal (tests/test_robust_cpu.py lists them) on live objects, each followed by a successful call on the same object"""
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    b = driver_problem("syn_rand60x40")[1]
    P, L = pkg.LeastSquares(m, n, Ap, Ai, Ax), pkg.DampedLeastSquares(m, n, Ap, Ai, Ax)
    P2 = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=2)
    try:
        ref = [P.solve_robust(b, max_iter=3)[0], L.solve_robust(b, max_iter=3, lam=LAM)[0], P2.solve(np.stack([b, b], axis=1))[0]]

        def after():
            got = [P.solve_robust(b, max_iter=3)[0], L.solve_robust(b, max_iter=3, lam=LAM)[0], P2.solve(np.stack([b, b], axis=1))[0]]
            assert all(np.array_equal(bits(g), bits(r)) for g, r in zip(got, ref))

        assert len(robust_refusals(pkg, P, L, P2, m, n, after)) == 28
    finally:
        P.close(); L.close(); P2.close()
