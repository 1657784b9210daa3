"""The adjoint of the least-squares solve, without a GPU: the dense numpy yardstick of tests/adjoint_reference.py against central
differences of numpy.linalg.lstsq and against torch autograd of the dense normal equations; the refusals of stmmqr_ls_adjoint that
need no device; and that capi still imports without torch."""
import importlib
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import adjoint_reference as ar
from stmmqr_testlib import EPS
from test_damped_cpu import matrix_of, scales, weights

PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
FIXTURES = ["syn_rand60x40", "syn_star"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module(PKG)


def case_of(name, damped, nrhs=2):
    """the problem, the damping of the issue (w from weights() with one entry 0, d = scales(), lam = 0.3) and a cotangent"""
    m, n, Ap, Ai, Ax = matrix_of(name)
    rng = np.random.default_rng(41)
    B, Xbar = rng.standard_normal((m, nrhs)), rng.standard_normal((n, nrhs))
    kw = {}
    if damped:
        w = weights(m)
        w[m // 3] = 0.0
        kw = dict(w=w, d=scales(n), lam=0.3)
    return m, n, Ap, Ai, Ax, B, Xbar, kw


@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_yardstick_against_central_differences(name, damped):
    """<gradient, direction> against (L(theta + h dir) - L(theta - h dir)) / 2h of L = <Xbar, lstsq(theta)>, h = 1e-6, for random
    directions over each of Ax, B, w, d, lam alone and over all together.  Central differences at h = 1e-6 carry a truncation error
    of h^2 and a rounding error of eps / h = 2e-10, both relative to the size of L's derivatives: the bar is 1e-7 of
    |gradient| |direction| (the issue measured 2e-9)."""
    m, n, Ap, Ai, Ax, B, Xbar, kw = case_of(name, damped)
    C = ar.dense_c(m, n, Ap, Ai, Ax, kw.get("w"), None if not damped else np.sqrt(kw["lam"]) * kw["d"])
    assert np.linalg.matrix_rank(C) == n
    X = ar.basic_solution(C, ar.dense_bt(B, kw.get("w"), n, damped), np.arange(n))
    ref = ar.adjoint(m, n, Ap, Ai, Ax, B, X, Xbar, **kw)
    if damped:
        assert ref["wbar"][m // 3] == 0.0
    theta = {"Ax": Ax, "B": B}
    grad = {"Ax": ref["Axbar"], "B": ref["Bbar"]}
    if damped:
        theta.update(w=kw["w"], d=kw["d"], lam=np.array(kw["lam"]))
        grad.update(w=ref["wbar"], d=ref["dbar"], lam=np.array(ref["lambdabar"]))
    rng = np.random.default_rng(43)
    h = 1e-6

    def loss(t):
        extra = {k: (float(t[k]) if k == "lam" else t[k]) for k in ("w", "d", "lam") if k in t}
        return ar.loss_by_lstsq(m, n, Ap, Ai, t["Ax"], t["B"], Xbar, **extra)

    worst = 0.0
    for which in list(theta) + ["all"]:
        keys = list(theta) if which == "all" else [which]
        dirs = {k: rng.standard_normal(np.shape(theta[k])) for k in keys}
        plus = {k: theta[k] + h * dirs[k] if k in dirs else theta[k] for k in theta}
        minus = {k: theta[k] - h * dirs[k] if k in dirs else theta[k] for k in theta}
        fd = (loss(plus) - loss(minus)) / (2 * h)
        an = sum(float(np.sum(grad[k] * dirs[k])) for k in keys)
        scale = np.sqrt(sum(float(np.sum(grad[k] ** 2)) for k in keys)) * np.sqrt(sum(float(np.sum(dirs[k] ** 2)) for k in keys))
        worst = max(worst, abs(fd - an) / scale)
        print(f"[adjoint cpu] {name} damped {damped} d/d{which}: fd {fd:.12e} adjoint {an:.12e} rel {abs(fd - an) / scale:.2e}")
        assert abs(fd - an) <= 1e-7 * scale
    print(f"[adjoint cpu] {name} damped {damped}: worst disagreement with central differences {worst:.2e}")


@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_yardstick_against_torch_autograd_of_the_normal_equations(name, damped):
    """x = (C'C)^-1 C'Bt written in torch (float64, CPU) from leaf tensors Ax, B, w, d, lam, backward of <Xbar, x>: every gradient
    entry.  The normal equations lose kappa^2 eps of their solution and autograd differentiates the same expression, so the bar per
    quantity is 100 kappa^2 eps times its largest entry (kappa <= 121 here: 3e-10)."""
    torch = pytest.importorskip("torch")
    m, n, Ap, Ai, Ax, B, Xbar, kw = case_of(name, damped)
    cols = ar.columns_of(n, Ap)
    t = lambda v: torch.tensor(np.asarray(v, float), dtype=torch.float64, requires_grad=True)               # noqa: E731
    tAx, tB = t(Ax), t(B)
    leaves = {"Axbar": tAx, "Bbar": tB}
    A = torch.zeros((m, n), dtype=torch.float64).index_put((torch.tensor(Ai), torch.tensor(cols)), tAx)
    if damped:
        tw, td, tl = t(kw["w"]), t(kw["d"]), t(kw["lam"])
        leaves.update(wbar=tw, dbar=td, lambdabar=tl)
        Cm = torch.cat([tw[:, None] * A, torch.diag(torch.sqrt(tl) * td)])
        Bt = torch.cat([tw[:, None] * tB, torch.zeros((n, B.shape[1]), dtype=torch.float64)])
    else:
        Cm, Bt = A, tB
    Xt = torch.linalg.solve(Cm.T @ Cm, Cm.T @ Bt)
    (Xt * torch.tensor(Xbar)).sum().backward()
    X = Xt.detach().numpy()
    ref = ar.adjoint(m, n, Ap, Ai, Ax, B, X, Xbar, **kw)
    kappa = float(np.linalg.cond(ref["C"]))
    bar = 100 * kappa ** 2 * EPS
    for key, leaf in leaves.items():
        got, want = leaf.grad.numpy(), np.asarray(ref[key])
        err = float(np.max(np.abs(got - want))) / max(float(np.max(np.abs(want))), 1e-300)
        print(f"[adjoint cpu] {name} damped {damped} {key}: kappa {kappa:.3g} max |autograd - yardstick| / max |yardstick| {err:.2e} "
              f"(allowed {bar:.1e})")
        assert err <= bar


def test_adjoint_refusals_on_the_host_half(pkg):
    """an object that holds the host half only refuses the adjoint, naming the cause; a null object likewise"""
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    X = np.zeros((n, 2))
    for cls in (pkg.LeastSquares, pkg.DampedLeastSquares):
        L = cls(m, n, Ap, Ai, Ax, nrhs=2, symbolic_only=True)
        try:
            with pytest.raises(pkg.StmmqrError) as e:
                L.adjoint(X, X)
            assert e.value.code == -4 and "host half" in str(e.value)
            with pytest.raises(pkg.StmmqrError) as e:
                L.adjoint_dev(0, 0)
            assert e.value.code == -4 and "host half" in str(e.value)
            with pytest.raises(pkg.StmmqrError) as e:
                L.adjoint_z()
            assert e.value.code == -4
            with pytest.raises(pkg.StmmqrError):
                L.adjoint(np.zeros((n, 3)), np.zeros((n, 3)))                       # (the Python layer: the wrong number of columns)
            assert L.info["solves"] == 0 and L.info["analyses"] == 1 and L.info["plans"] == 0
        finally:
            L.close()
    info = np.zeros(8)
    rc = pkg.lib.stmmqr_ls_adjoint(None, X.ctypes.data, n, X.ctypes.data, n, None, 1, None, None, m, None, None, 0,
                                   info.ctypes.data_as(importlib.import_module(PKG + ".capi").c_double_p))
    assert rc == -4 and "null object" in pkg.lib.stmmqr_last_error().decode()


def test_capi_imports_without_torch():
    """a fresh interpreter imports the package and capi, and torch is not among its modules: autograd.py is imported on request"""
    root = Path(__file__).resolve().parent.parent
    code = (f"import sys, importlib; sys.path.insert(0, {str(root)!r}); p = importlib.import_module({PKG!r}); "
            f"importlib.import_module({PKG!r} + '.capi'); assert hasattr(p, 'LeastSquares'); "
            "assert 'torch' not in sys.modules, 'capi pulled torch in'; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
