"""Robust least squares (stmmqr_ls_solve_robust, stmmqr_ls_robust_weights, stmmqr_median_abs), host half (no GPU): the numpy yardstick
of tests/robust_reference.py -- psi = rho' by central differences, the median against numpy.median, the Huber fixed point against its
estimating equation --, the cases tests/test_gpu_robust.py runs (the yardstick converges on each within the max_iter that test
passes), and the C-ABI refusals, every one of which is decided before the device is looked at."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

import robust_reference as rr
from stmmqr_testlib import EPS
from test_damped_cpu import matrix_of

PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
FIXTURES = ["syn_rand60x40", "syn_star", "syn_grid3d", "syn_emptycol", "syn_dupcol", "epb1"]
LAM = 1e-2                                  # the damping of every damped case


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def sparse_of(name):
    m, n, Ap, Ai, Ax = matrix_of(name)
    return sp.csc_matrix((Ax, Ai, Ap), shape=(m, n))


def prior_weights(m, seed=5):
    """inverse standard deviations in [0.5, 2], a tenth of the rows switched off"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, m)
    w[rng.choice(m, max(1, m // 10), replace=False)] = 0.0
    return w


# ---- the cases of the driver test (tests/test_gpu_robust.py, 4): 10 % of b replaced, the scale floored at ten times the noise (the
# small fixtures leave few degrees of freedom: without a floor the MAD of an almost interpolating fit collapses), rtol 1e-6 ----
DRIVER_SEED, DRIVER_SHARE, DRIVER_SIGMA_MIN, DRIVER_RTOL, DRIVER_MAX_ITER = 3, 0.1, 1e-2, 1e-6, 100
ALL5 = ["huber mad", "tukey frozen", "l1", "x0", "w0 zeros"]
DRIVER_CASES = ([("syn_grid3d", damped, lab) for damped in (False, True) for lab in ALL5] +
                [(nm, False, lab) for nm in ("syn_star", "syn_emptycol", "syn_rand60x40") for lab in ALL5] +
                [("syn_emptycol", True, lab) for lab in ("huber mad", "tukey frozen", "x0", "w0 zeros")] +
                [("syn_dupcol", False, lab) for lab in ("huber mad", "tukey frozen", "x0", "w0 zeros")])


def driver_rule(label, m, n):
    """the keyword arguments of solve_robust (and of the yardstick's irls) for a case label"""
    kw = {"huber mad": dict(loss="huber"), "tukey frozen": dict(loss="tukey", sigma_iters=2), "l1": dict(loss="l1", cc=rr.L1_CC),
          "x0": dict(loss="huber", x0=np.zeros(n)), "w0 zeros": dict(loss="cauchy", w0=prior_weights(m))}[label]
    return dict(kw, sigma_min=DRIVER_SIGMA_MIN, rtol=DRIVER_RTOL, max_iter=DRIVER_MAX_ITER)


def driver_problem(name):
    A = sparse_of(name)
    return A, rr.outlier_problem(A.toarray(), DRIVER_SEED, share=DRIVER_SHARE)[0]


# ---- the cases of the fit test (5): b = A x_true + 1e-3 noise, 15 % of the rows replaced by +-100.  (name, damped, seed, the fixed
# scale of the Huber fit, max_iter).  epb1 is square: on a plain object every fit with positive weights interpolates b, so it is
# fitted with the damping; its max_iter is what keeps the test at seconds, and both sides stop there. ----
FIT_CASES = [("syn_rand60x40", False, 1, 0.1, 250), ("syn_rand60x40", True, 2, 0.01, 400), ("epb1", True, 1, 0.1, 6)]
FIT_RTOL = 1e-12


def fit_problem(name, seed):
    A = sparse_of(name)
    b, xt, bad = rr.outlier_problem(A if name == "epb1" else A.toarray(), seed)
    return A, b, xt, bad


def fit_runs(name, damped, seed, sigma, max_iter):
    """the yardstick's L2, Huber (fixed scale) and Tukey (scale frozen after two estimates) fits of a case"""
    A, b, xt, bad = fit_problem(name, seed)
    Ad = A if name == "epb1" else A.toarray()
    D = np.full(A.shape[1], np.sqrt(LAM)) if damped else None
    l2 = rr.irls(Ad, b, "l2", max_iter=1, D=D)
    hub = rr.irls(Ad, b, "huber", sigma=sigma, max_iter=max_iter, rtol=FIT_RTOL, D=D)
    tuk = rr.irls(Ad, b, "tukey", sigma_iters=2, max_iter=max_iter, rtol=FIT_RTOL, D=D)
    return Ad, b, xt, D, l2, hub, tuk


def estimating_residual(A, b, x, sigma, D=None, w0=None):
    """A'(w0 o psi(u) o sign r) - D^2 x / sigma for the Huber loss: zero at the minimiser of sum rho(u) + |D x|^2 / (2 sigma^2);
    also sum_i |A_ij| |psi_i|, what rounding in the product is measured against"""
    g, p = rr.estimating_equation(A, b, x, "huber", rr.DEFAULT_CC["huber"], sigma, w0)
    if D is not None:
        g = g - (D * D) * x / sigma
    return g, abs(A).T @ np.abs(p)


@pytest.mark.parametrize("loss", rr.LOSSES)
def test_psi_is_the_derivative_of_rho(loss):
    """u f(u)^2 against the central difference of rho with h = 1e-6: the truncation h^2 |rho'''| / 6 and the rounding eps rho / h are
    both below 1e-8 (1 + rho) on the grid, which avoids nothing -- every rho here is continuously differentiable at cc"""
    cc = rr.L1_CC if loss == "l1" else rr.cc_of(loss)
    u = np.concatenate([np.linspace(0.01, 3 * cc, 400), [cc, 0.5 * cc, 2 * cc]])
    h = 1e-6
    d = (rr.f_rho(loss, cc, u + h)[1] - rr.f_rho(loss, cc, u - h)[1]) / (2 * h)
    err = np.abs(d - rr.psi(loss, cc, u))
    # at u = cc the second derivative jumps (Huber, Tukey, L1): the central difference is then first order, h |jump| / 4
    slack = np.where(np.abs(u - cc) <= h, h * max(1.0, 1.0 / cc), 0.0)
    print(f"[robust cpu] {loss}: max |central difference - psi| {err.max():.2e}")
    assert np.all(err <= 1e-8 * (1 + rr.f_rho(loss, cc, u)[1]) + slack)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 1001])
def test_median_of_the_yardstick(n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n)
    med, lo, hi, c = rr.median_abs(v)
    assert c == n and lo <= hi and med == float(np.median(np.abs(v)))
    mask = rng.uniform(0.5, 2.0, n) * (rng.random(n) < 0.6)
    med, lo, hi, c = rr.median_abs(v, mask)
    assert c == int(np.count_nonzero(mask))
    if c:
        assert med == float(np.median(np.abs(mask * v)[mask != 0]))
    else:
        assert (med, lo, hi) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("case", FIT_CASES[:2], ids=lambda c: f"{c[0]}-{'damped' if c[1] else 'plain'}")
def test_huber_fixed_point_satisfies_its_estimating_equation(case):
    """With the scale fixed the loop stops at a step <= rtol max |x|.  One more step from x would be (A'W^2 A + D^2)^-1 sigma g(x), so
    |g|_inf <= |A'W^2 A + D^2|_inf |next step|_inf / sigma, and the next step is no longer than the last one of a contracting loop:
    the bar is that with the last step's bound rtol max |x| (twice it, for the rounding of the solves)."""
    name, damped, seed, sigma, max_iter = case
    A, b, xt, D, l2, (x, w, info), tuk = fit_runs(*case)
    assert info["converged"], f"{info['solves']} solves"
    g, scale = estimating_residual(A, b, x, sigma, D)
    N = (w[:, None] * A).T @ (w[:, None] * A) + (0 if D is None else np.diag(D * D))
    bar = 2 * np.abs(N).sum(axis=1).max() * FIT_RTOL * np.abs(x).max() / sigma
    print(f"[robust cpu] {name} {'damped' if damped else 'plain'}: {info['solves']} solves, |estimating equation|_inf {np.abs(g).max():.2e} "
          f"(bar {bar:.2e})")
    assert np.abs(g).max() <= bar


@pytest.mark.parametrize("case", FIT_CASES, ids=lambda c: f"{c[0]}-{'damped' if c[1] else 'plain'}")
def test_fit_cases_of_the_gpu_test(case):
    """the robust fits beat the L2 fit on the data the GPU test uses, and the yardstick converges within its max_iter (epb1: both sides
    stop at max_iter, see FIT_CASES)"""
    name, damped, seed, sigma, max_iter = case
    A, b, xt, D, l2, hub, tuk = fit_runs(*case)
    e2, eh, et = (np.abs(f[0] - xt).max() for f in (l2, hub, tuk))
    print(f"[robust cpu] {name}: |x - x_true|_inf L2 {e2:.3g} Huber {eh:.3g} ({hub[2]['solves']} solves) Tukey {et:.3g} ({tuk[2]['solves']})")
    assert eh < e2 and et < e2
    if name != "epb1":
        assert hub[2]["converged"] and tuk[2]["converged"]
    if not damped:                                          # (with damping the loop lowers sum rho + |D x|^2 / (2 sigma^2), not sum rho)
        h = tuk[2]["hist"][:, 1]
        assert np.all(np.diff(h[2:]) <= 1e-12 * h[2:-1])


@pytest.mark.parametrize("name,damped", sorted({(c[0], c[1]) for c in DRIVER_CASES}))
def test_driver_cases_converge_in_the_yardstick(name, damped):
    A, b = driver_problem(name)
    m, n = A.shape
    D = np.full(n, np.sqrt(LAM)) if damped else None
    for lab in [c[2] for c in DRIVER_CASES if c[:2] == (name, damped)]:
        x, w, info = rr.irls(A.toarray(), b, D=D, **driver_rule(lab, m, n))
        print(f"[robust cpu] {name} {'damped' if damped else 'plain'} {lab}: {info['solves']} solves, sigma {info['sigma']:.3g}")
        assert info["converged"], lab


# ---- the refusals ----
def raw_robust(pkg, handle, rb, dmp, m, n, B=True, X=True, max_iter=5, rtol=1e-8, weights_only=False):
    """the two entry points with host arrays and the structs given as they are (None: a NULL pointer)"""
    capi = importlib.import_module(PKG + ".capi")
    b, x, w, r = np.zeros(max(m, 1)), np.zeros(max(n, 1)), np.full(max(m, 1), 7.0), np.full(max(m, 1), 7.0)
    stat = np.full(8, 7.0)
    rbp = None if rb is None else C.byref(rb)
    if weights_only:
        rc = pkg.lib.stmmqr_ls_robust_weights(handle, None, 0, rbp, b.ctypes.data if B else None, x.ctypes.data if X else None, r.ctypes.data,
                                              w.ctypes.data, 0, stat.ctypes.data_as(capi.c_double_p))
    else:
        rc = pkg.lib.stmmqr_ls_solve_robust(handle, None, 0, rbp, None if dmp is None else C.byref(dmp), b.ctypes.data if B else None, None,
                                            max_iter, rtol, -1, x.ctypes.data if X else None, w.ctypes.data, None, 0, None,
                                            stat.ctypes.data_as(capi.c_double_p))
    assert np.all(w == 7.0) and np.all(stat == 7.0) or rc == 0, "a refusal writes nothing"
    capi._check(rc, "robust")


def robust_refusals(pkg, P, L, P2, m, n, after=lambda: None):
    """every refusal of stmmqr_ls_solve_robust and stmmqr_ls_robust_weights that the header lists, but the host half (shared with the GPU
    test, where the objects are live and after() makes a successful call): P a plain object, L a damped one, P2 one created with
    nrhs = 2.  Each raises with the code -4 and names its cause."""
    capi = importlib.import_module(PKG + ".capi")
    rule = lambda **kw: capi.LsRobust(kw.get("loss", 1), kw.get("cc", 0.0), kw.get("sigma", 0.0), kw.get("mad", 0.0), kw.get("smin", 0.0), None)  # noqa: E731
    damp = lambda w=None, lam=LAM: capi.LsDamping(w, None, lam, 0, 1e-6, 1e32, None, None)                 # noqa: E731
    seen = []

    def refused(word, handle, rb, dmp=None, both=True, **kw):
        for weights_only in ((False, True) if both else (False,)):
            with pytest.raises(pkg.StmmqrError) as e:
                raw_robust(pkg, handle, rb, dmp, m, n, weights_only=weights_only, **kw)
            assert e.value.code == -4 and word in str(e.value), str(e.value)
        seen.append(word)
        after()

    refused("null object", None, rule())
    refused("nrhs = 2", P2._h, rule())
    refused("null rule", P._h, None)
    for loss in (-1, 5, 99):
        refused("loss must be 0 .. 4", P._h, rule(loss=loss))
    for cc in (0.0, -1.0):
        refused("cc > 0 required", P._h, rule(loss=4, cc=cc))
    for kw in (dict(sigma=np.nan), dict(sigma=np.inf), dict(smin=np.nan), dict(smin=np.inf), dict(cc=np.inf), dict(cc=np.nan), dict(mad=np.nan),
               dict(mad=-np.inf)):
        refused("must be finite", P._h, rule(**kw))
    refused("sigma is negative", P._h, rule(sigma=-1.0))
    refused("sigma_min is negative", L._h, rule(smin=-1e-300), damp())
    for it in (0, -3):
        refused("max_iter", P._h, rule(), both=False, max_iter=it)
    for rtol in (-1e-300, np.nan):
        refused("rtol", P._h, rule(), both=False, rtol=rtol)
    refused("given on a plain object", P._h, rule(), damp(), both=False)
    refused("needs its damping", L._h, rule(), None, both=False)
    keep = np.ones(max(m, 1))
    refused("dmp->w must be NULL", L._h, rule(), damp(w=keep.ctypes.data), both=False)
    refused("lambda", L._h, rule(), damp(lam=-1.0), both=False)
    refused("B or X is NULL", P._h, rule(), B=False)
    refused("B or X is NULL", L._h, rule(), damp(), X=False)
    return seen


def test_refusals_on_the_host_half(pkg):
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    P = pkg.LeastSquares(m, n, Ap, Ai, Ax, symbolic_only=True)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, symbolic_only=True)
    P2 = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=2, symbolic_only=True)
    try:
        assert len(robust_refusals(pkg, P, L, P2, m, n)) == 28
        # good arguments: the host half alone does not fit, and says so
        for call in (lambda: P.solve_robust(np.zeros(m)), lambda: L.solve_robust(np.zeros(m), lam=LAM),
                     lambda: P.robust_weights(np.zeros(m), np.zeros(n)), lambda: L.robust_weights(np.zeros(m), np.zeros(n))):
            with pytest.raises(pkg.StmmqrError) as e:
                call()
            assert e.value.code == -4 and "host half" in str(e.value)
        with pytest.raises(pkg.StmmqrError) as e:
            P.solve_robust(np.zeros(m), loss="biweight")
        assert "unknown loss" in str(e.value)
        assert P.info["solves"] == 0 and L.info["solves"] == 0
    finally:
        P.close(); L.close(); P2.close()


def test_capi_imports_without_torch():
    """the binding names nothing of torch at import (its HIP runtime is found by path, torch is not imported)"""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    code = (f"import sys, importlib; sys.path.insert(0, {str(root)!r}); m = importlib.import_module({PKG + '.capi'!r}); "
            "assert 'torch' not in sys.modules; assert m.LsRobust and m.median_abs and m.LeastSquares.solve_robust")
    subprocess.run([sys.executable, "-c", code], check=True)
