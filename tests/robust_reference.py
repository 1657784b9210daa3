"""The numpy yardstick of the robust fits (stmmqr_ls_solve_robust): the five pairs f / rho written with the operations of
include/stmmqr_hip.h in their order (divisions and square roots are correctly rounded on both sides, so f has the device's bits where
no fused multiply-add is formed), the median as the two middle order statistics, one reweighting, and the IRLS loop on dense lstsq
with the driver's stop rule.  tests/test_robust_cpu.py validates it without a GPU; tests/test_gpu_robust.py holds the device to it."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LOSSES = ["l2", "huber", "cauchy", "tukey", "l1"]
DEFAULT_CC = {"l2": 1.0, "huber": 1.345, "cauchy": 2.3849, "tukey": 4.6851}
MAD = 1.4826
L1_CC = 0.05                       # the smoothing the tests give the L1 loss (it has no default)


def cc_of(loss, cc=None):
    return float(cc) if cc is not None and cc > 0 else DEFAULT_CC[loss]


def f_rho(loss, cc, u):
    """(f(u), rho(u)) for an array u >= 0: the row multiplier sqrt(psi(u) / u) and the objective"""
    u = np.asarray(u, np.float64)
    t = u / cc
    t2 = t * t
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == "l2":
            return np.ones_like(u), (u * u) / 2.0
        if loss == "huber":
            return np.where(u <= cc, 1.0, np.sqrt(cc / u)), np.where(u <= cc, (u * u) / 2.0, cc * (u - cc / 2.0))
        if loss == "cauchy":
            return 1.0 / np.sqrt(1.0 + t2), ((cc * cc) / 2.0) * np.log1p(t2)
        if loss == "tukey":
            g = 1.0 - t2
            return np.where(u < cc, g, 0.0), np.where(u < cc, ((cc * cc) / 6.0) * (1.0 - (g * g) * g), (cc * cc) / 6.0)
        if loss == "l1":
            return 1.0 / np.sqrt(np.maximum(u, cc)), np.where(u >= cc, u, (u * u) / (2.0 * cc) + cc / 2.0)
    raise ValueError(loss)


def psi(loss, cc, u):
    """rho' = u f^2"""
    f = f_rho(loss, cc, u)[0]
    return u * f * f


def median_parts(a):
    """(0.5 * (lo + hi), lo, hi, count) of a 1-d array, lo = a_(floor((c - 1) / 2)), hi = a_(floor(c / 2)); zeros for no entry"""
    a = np.asarray(a, np.float64).reshape(-1)
    c = a.size
    if c == 0:
        return 0.0, 0.0, 0.0, 0
    k0, k1 = (c - 1) // 2, c // 2
    p = np.partition(a, (k0, k1))
    lo, hi = float(p[k0]), float(p[k1])
    return 0.5 * (lo + hi), lo, hi, c


def median_abs(v, mask=None):
    v = np.asarray(v, np.float64).reshape(-1)
    if mask is None:
        return median_parts(np.abs(v))
    mask = np.asarray(mask, np.float64).reshape(-1)
    return median_parts(np.abs(mask * v)[mask != 0])


def scale_of(a, w0, sigma=0.0, mad_factor=MAD, sigma_min=0.0):
    """the scale of a reweighting from a = |w0 o r|: the given one, or mad_factor * median over w0 != 0; floored"""
    if sigma > 0:
        return max(float(sigma), float(sigma_min))
    med = median_parts(a if w0 is None else a[np.asarray(w0) != 0])[0]
    return max(mad_factor * med, float(sigma_min))


def weights_from(r, loss, cc, w0=None, sigma=0.0, mad_factor=MAD, sigma_min=0.0):
    """one reweighting from the unweighted residual r -> (w, stat) with stat = sigma, loss, rejected, unit, flag, and u"""
    r = np.asarray(r, np.float64)
    w0v = np.ones_like(r) if w0 is None else np.asarray(w0, np.float64)
    a = np.abs(w0v * r)
    s = scale_of(a, w0, sigma, mad_factor, sigma_min)
    if s == 0.0:
        return w0v.copy(), dict(sigma=0.0, loss=0.0, rejected=0, unit=r.size, flag=1, u=np.zeros_like(r))
    u = a / s
    f, rho = f_rho(loss, cc, u)
    w = w0v * f
    return w, dict(sigma=s, loss=float(np.sum(rho.astype(np.longdouble))), rejected=int(np.sum((w == 0) & (w0v != 0))),
                   unit=int(np.sum(f == 1.0)), flag=0, u=u)


def weighted_solve(A, w, b, D=None):
    """argmin |W (A x - b)|^2 + |D x|^2 and the residual norm of the stacked problem: dense lstsq of [W A; D]; a scipy sparse A (full
    column rank of [W A; D] assumed) goes through the sparse LU of the normal equations"""
    n = A.shape[1]
    if sp.issparse(A):
        WA = sp.diags(w) @ A
        N = WA.T @ WA
        if D is not None:
            N = N + sp.diags(np.asarray(D) ** 2)
        x = spla.spsolve(N.tocsc(), WA.T @ (w * b))
        res = np.sqrt(np.sum((WA @ x - w * b) ** 2) + (0.0 if D is None else np.sum((D * x) ** 2)))
        return x, float(res)
    C, rhs = w[:, None] * np.asarray(A, np.float64), w * b
    if D is not None:
        C, rhs = np.vstack([C, np.diag(D)]), np.concatenate([rhs, np.zeros(n)])
    x = np.linalg.lstsq(C, rhs, rcond=None)[0]
    return x, float(np.linalg.norm(C @ x - rhs))


def irls(A, b, loss, cc=None, sigma=0.0, w0=None, x0=None, max_iter=50, rtol=1e-8, sigma_iters=-1, D=None, mad_factor=MAD, sigma_min=0.0):
    """the driver's loop on weighted_solve -> (x, w, info): x0 None = the first solve uses w0 alone; a reweighting from the last
    x before every further solve; stop after the first solve with max |x - xprev| <= rtol max |x|; the scale estimated in the first
    max(sigma_iters, 1) reweightings (sigma_iters < 0: always) unless given."""
    m, n = A.shape
    cc = cc_of(loss, cc)
    w = np.ones(m) if w0 is None else np.asarray(w0, np.float64).copy()
    x, nrew, stat = None, 0, dict(sigma=0.0, loss=0.0, rejected=0)
    hist = []

    def reweigh(xc):
        nonlocal nrew, stat
        s = sigma
        if s == 0 and sigma_iters >= 0 and nrew >= max(sigma_iters, 1):
            s = stat["sigma"]
        wn, stat = weights_from(b - A @ xc, loss, cc, w0, s, mad_factor, sigma_min)
        nrew += 1
        return wn

    if x0 is not None:
        x = np.asarray(x0, np.float64).copy()
        w = reweigh(x)
    converged = False
    for it in range(max_iter):
        if it > 0:
            w = reweigh(x)
        xn, res = weighted_solve(A, w, b, D)
        step = np.inf if x is None else float(np.max(np.abs(xn - x), initial=0.0))
        converged = x is not None and step <= rtol * float(np.max(np.abs(xn), initial=0.0))
        x = xn
        hist.append((stat["sigma"], stat["loss"], step, res))
        if converged:
            break
    return x, w, dict(solves=len(hist), converged=converged, sigma=stat["sigma"], loss=stat["loss"], rejected=stat["rejected"],
                      hist=np.array(hist))


def estimating_equation(A, b, x, loss, cc, sigma, w0=None):
    """A'(w0 o psi(u) o sign(r)) at x with the scale fixed: zero at the minimiser of sum rho(|w0 r| / sigma)"""
    r = b - A @ x
    w0v = np.ones_like(r) if w0 is None else np.asarray(w0, np.float64)
    u = np.abs(w0v * r) / sigma
    p = w0v * psi(loss, cc, u) * np.sign(r)
    return A.T @ p, p


def outlier_problem(A, seed, share=0.15, noise=1e-3, gross=100.0):
    """b = A x_true + noise, a share of the rows replaced by +-gross -> (b, x_true, the rows replaced)"""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    xt = rng.standard_normal(n)
    b = A @ xt + noise * rng.standard_normal(m)
    bad = rng.choice(m, max(1, int(round(share * m))), replace=False)
    b[bad] = gross * rng.choice([-1.0, 1.0], bad.size)
    return b, xt, np.sort(bad)
