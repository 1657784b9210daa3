"""The adjoint of the least-squares solve on the GPU (stmmqr_ls_adjoint, LeastSquares.adjoint / DampedLeastSquares.adjoint, autograd.lstsq)
against the dense numpy yardstick of tests/adjoint_reference.py on the live set the device reports, with the bars that module
derives from solve_tol; exact zeros, the dead set, bits, the torch layer, refusals, and one real-size check against central differences.
(On the code before the adjoint neither the symbol nor the methods exist: no test here can pass there.)

Measured on the MI355X, the largest error / bar of each group of cases (the table of DESIGN.md 6q): plain small fixtures 4.4e-3
(syn_grid3d), damped small fixtures 4.6e-3 (syn_grid3d), bcsstk14 damped lam 1e-2 8.5e-8 (kappa 6.2e6, kappa^2 eps 8.6e-3), the dead
sets 1.2e-3 (syn_rankdef_grid)."""
import importlib

import numpy as np
import pytest

import adjoint_reference as ar
from stmmqr_testlib import EPS
from test_damped_cpu import SMALL, matrix_of, scales, weights

pytestmark = pytest.mark.gpu

PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
NRHS = [1, 2, 33]                                           # 33: past a batch edge (STMMQR_RHS_BATCH = 32)
DAMPINGS = {"w lam 1e-2": lambda m, n: dict(w=weights(m), lam=1e-2), "d lam 0.3": lambda m, n: dict(d=scales(n), lam=0.3)}


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    assert p.device_count() >= 1
    return p


@pytest.fixture(scope="module")
def ag():
    return importlib.import_module(PKG + ".autograd")


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def data(m, n, k, seed=51):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((m, k))), np.asfortranarray(rng.standard_normal((n, k)))


def live_columns(L, n):
    """the live columns of A, in A's numbering, from Rdead of the object's plan"""
    N = L.plan().download()
    q = L.symbolic()["Qfill"][:n]
    return np.sort(q[np.flatnonzero(np.asarray(N.Rdead[:n]) == 0)])


def solve_and_adjoint(L, B, Xbar, kw, refine=1):
    """-> X, {Axbar, Bbar, wbar, Dbar, info}"""
    if kw:
        X = L.solve(B, **kw)[0]
        a, b, wb, Db, info = L.adjoint(X, Xbar, w=kw.get("w"), refine=refine)
        return X, dict(Axbar=a, Bbar=b, wbar=wb, Dbar=Db, info=info)
    X = L.solve(B)[0]
    a, b, info = L.adjoint(X, Xbar, refine=refine)
    return X, dict(Axbar=a, Bbar=b, info=info)


def worst_ratio(got, ref, bar, m, keys):
    """the largest |error| / bar over the named quantities, and which"""
    worst, at = 0.0, ""
    for key in keys:
        allowed = {"Axbar": None, "Bbar": bar["Bbar"]}.get(key, bar.get(key))
        err = np.abs(np.asarray(got[key], float).reshape(np.shape(ref[key])) - ref[key])
        if key == "Axbar":
            allowed = bar["Axbar_rows"][got["rows"]]
        ratio = float(np.max(err / np.maximum(allowed, 1e-300))) if err.size else 0.0
        print(f"    {key}: max |error| {float(np.max(err)) if err.size else 0.0:.2e} max |value| "
              f"{float(np.max(np.abs(ref[key]))) if err.size else 0.0:.2e} error / bar {ratio:.2e}")
        if ratio > worst:
            worst, at = ratio, key
    return worst, at


def check_case(pkg, ag, torch, name, kind, nrhs):
    m, n, Ap, Ai, Ax = matrix_of(name)
    kw = DAMPINGS[kind](m, n) if kind != "plain" else {}
    B, Xbar = data(m, n, nrhs)
    cls = pkg.DampedLeastSquares if kw else pkg.LeastSquares
    L = cls(m, n, Ap, Ai, Ax, nrhs=nrhs)
    try:
        X, got = solve_and_adjoint(L, B, Xbar, kw)
        live = live_columns(L, n)
        assert got["info"]["live"] == live.size
        ref = ar.adjoint(m, n, Ap, Ai, Ax, B, X, Xbar, live=live, **kw)
        bar = ar.bars(ref, X, m, w=kw.get("w"), lam=kw.get("lam"))
        k2e = bar["kappa"] ** 2 * EPS
        print(f"[adjoint] {name} {kind} nrhs {nrhs}: live {live.size}/{n} kappa {bar['kappa']:.3g} kappa^2 eps {k2e:.1e} bar of g {bar['g']:.1e} "
              f"max |g| {np.max(np.abs(ref['G'])):.1e} normal resid {got['info']['normal_resid']:.1e}")
        assert k2e <= 1e-2, "refinement earns its u kappa only below that"
        got["rows"] = np.asarray(Ai)
        keys = ["Axbar", "Bbar"] + (["wbar", "Dbar"] if kw else [])
        if kw:
            # dbar and lambdabar from the Python layer (CPU tensors: the host entry points)
            t = lambda v, g=True: torch.tensor(np.asarray(v, float), dtype=torch.float64, requires_grad=g)   # noqa: E731
            tAx, tB, td, tl = t(Ax), t(B), t(kw["d"] if "d" in kw else np.ones(n)), t(kw["lam"])
            tw = t(kw["w"]) if "w" in kw else None
            Xt = ag.lstsq(L, tAx, tB, w=tw, d=td, lam=tl)
            assert np.array_equal(bits(Xt.detach().numpy()), bits(X))
            (Xt * torch.tensor(Xbar)).sum().backward()
            got["dbar"], got["lambdabar"] = td.grad.numpy(), float(tl.grad)
            assert np.array_equal(bits(tAx.grad.numpy()), bits(got["Axbar"])) and np.array_equal(bits(tB.grad.numpy()), bits(got["Bbar"]))
            keys += ["dbar", "lambdabar"]
        worst, at = worst_ratio(got, ref, bar, m, keys)
        print(f"[adjoint] {name} {kind} nrhs {nrhs}: largest error / bar {worst:.2e} ({at})")
        assert worst <= 1.0
        return worst
    finally:
        L.close()


# ---- 1: against the yardstick on the live set the device reports ----
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_star", "syn_grid3d"])
def test_plain_against_the_yardstick(pkg, ag, torch, name, nrhs):
    check_case(pkg, ag, torch, name, "plain", nrhs)


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("kind", list(DAMPINGS))
@pytest.mark.parametrize("name", SMALL)
def test_damped_against_the_yardstick(pkg, ag, torch, name, kind, nrhs):
    check_case(pkg, ag, torch, name, kind, nrhs)


@pytest.mark.parametrize("nrhs", NRHS)
def test_bcsstk14_damped_against_the_yardstick(pkg, ag, torch, nrhs):
    """kappa = 6.2e6, kappa^2 eps = 8.6e-3 at lam = 1e-2 (the condition of every case, asserted in check_case)"""
    check_case(pkg, ag, torch, "bcsstk14", "w lam 1e-2", nrhs)


# ---- 2: exact zeros and structure ----
def test_empty_column_and_zero_damping(pkg):
    """syn_emptycol: the plain object has no entry in the empty column and handles it in the bisection; the damped object at lam = 0
    has D = 0, the column is dead, Dbar is 0.0 everywhere and every output is finite"""
    m, n, Ap, Ai, Ax = matrix_of("syn_emptycol")
    empty = np.flatnonzero(np.diff(Ap) == 0)
    assert empty.size >= 1
    B, Xbar = data(m, n, 2)
    P = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=2)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=2)
    try:
        X, got = solve_and_adjoint(P, B, Xbar, {})
        live = live_columns(P, n)
        assert not np.isin(empty, live).any() and np.all(X[empty] == 0.0)
        ref = ar.adjoint(m, n, Ap, Ai, Ax, B, X, Xbar, live=live)
        bar = ar.bars(ref, X, m)
        assert np.all(np.abs(got["Axbar"] - ref["Axbar"]) <= bar["g"]) and np.all(np.isfinite(got["Bbar"]))
        assert np.all(P.adjoint_z()[empty] == 0.0)
        X, got = solve_and_adjoint(L, B, Xbar, dict(w=weights(m), lam=0.0))
        assert np.all(got["Dbar"] == 0.0) and np.all(X[empty] == 0.0) and np.all(L.adjoint_z()[empty] == 0.0)
        for key in ("Axbar", "Bbar", "wbar"):
            assert np.all(np.isfinite(got[key]))
    finally:
        P.close(); L.close()


def test_zero_weight_and_lambda_zero_through_autograd(pkg, ag, torch):
    """wbar_i == 0.0 where w_i == 0; at lam = 0 dbar == 0 and lambdabar is finite and equals the yardstick's"""
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    B, Xbar = data(m, n, 2)
    w = weights(m)
    w[[3, m - 1]] = 0.0
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=2)
    try:
        X, got = solve_and_adjoint(L, B, Xbar, dict(w=w, lam=0.5))
        has_entries = np.bincount(Ai, minlength=m) > 0
        assert np.all(got["wbar"][[3, m - 1]] == 0.0) and np.all(got["wbar"][has_entries & (w != 0)] != 0.0)
        t = lambda v: torch.tensor(np.asarray(v, float), dtype=torch.float64, requires_grad=True)           # noqa: E731
        tAx, tB, tw, td, tl = t(Ax), t(B), t(w), t(scales(n)), t(0.0)
        Xt = ag.lstsq(L, tAx, tB, w=tw, d=td, lam=tl)
        (Xt * torch.tensor(Xbar)).sum().backward()
        ref = ar.adjoint(m, n, Ap, Ai, Ax, B, Xt.detach().numpy(), Xbar, w=w, d=scales(n), lam=0.0)
        bar = ar.bars(ref, Xt.detach().numpy(), m, w=w, lam=0.0)
        assert np.all(td.grad.numpy() == 0.0) and np.isfinite(float(tl.grad))
        print(f"[adjoint] lambdabar at lam = 0: {float(tl.grad):.12e} yardstick {ref['lambdabar']:.12e} bar {bar['lambdabar']:.1e}")
        assert abs(float(tl.grad) - ref["lambdabar"]) <= bar["lambdabar"] and ref["lambdabar"] != 0.0
    finally:
        L.close()


def test_null_outputs_are_not_written(pkg, torch):
    """device pointers: one buffer of a guard pattern holds the outputs side by side; with an output NULL its neighbours' and its own
    place keep the pattern, and what is asked for has the bits of the call that asks for everything"""
    m, n, Ap, Ai, Ax = matrix_of("syn_grid3d")
    k, anz = 2, int(Ap[-1])
    B, Xbar = data(m, n, k)
    w = weights(m)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    try:
        X = L.solve(B, w=w, lam=1e-2)[0]
        dev = torch.device("cuda", 0)
        up = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a).T), dtype=torch.float64, device=dev)   # noqa: E731
        tX, tXb, tw = up(X), up(Xbar), up(w)
        sizes = dict(ax=anz, bb=m * k, wb=m, db=n)
        off, at = {}, 8
        for key, sz in sizes.items():
            off[key] = at
            at += sz + 8
        guard = -1.2345678e300

        def run(asked):
            buf = torch.full((at,), guard, dtype=torch.float64, device=dev)
            ptr = {key: (buf.data_ptr() + 8 * off[key] if key in asked else None) for key in sizes}
            torch.cuda.synchronize()
            L.adjoint_dev(tX.data_ptr(), tXb.data_ptr(), w_ptr=tw.data_ptr(), axbar_ptr=ptr["ax"], bbar_ptr=ptr["bb"], wbar_ptr=ptr["wb"],
                          dbar_ptr=ptr["db"])
            return buf.cpu().numpy()

        full = run(set(sizes))
        pattern = bits(np.array([guard]))[0]
        written = np.zeros(at, bool)
        for key, sz in sizes.items():
            written[off[key]:off[key] + sz] = True
        assert np.all(bits(full)[~written] == pattern) and not np.any(bits(full)[written] == pattern)
        for asked in ({"ax"}, {"bb"}, {"wb"}, {"db"}, {"ax", "db"}, set()):
            part = run(asked)
            mask = np.zeros(at, bool)
            for key in asked:
                mask[off[key]:off[key] + sizes[key]] = True
            assert np.all(bits(part)[~mask] == pattern), f"asked for {sorted(asked)}: something else was written"
            assert np.array_equal(bits(part)[mask], bits(full)[mask])
    finally:
        L.close()


def test_refine_zero_against_refine_one(pkg):
    m, n, Ap, Ai, Ax = matrix_of("syn_grid3d")
    B, Xbar = data(m, n, 2)
    for kw in ({}, dict(w=weights(m), lam=1e-2)):
        L = (pkg.DampedLeastSquares if kw else pkg.LeastSquares)(m, n, Ap, Ai, Ax, nrhs=2)
        try:
            X, g1 = solve_and_adjoint(L, B, Xbar, kw, refine=1)
            _, g0 = solve_and_adjoint(L, B, Xbar, kw, refine=0)
            ref = ar.adjoint(m, n, Ap, Ai, Ax, B, X, Xbar, live=live_columns(L, n), **kw)
            bar = ar.bars(ref, X, m, w=kw.get("w"), lam=kw.get("lam"))
            assert g0["info"]["refine_steps"] == 0 and g1["info"]["refine_steps"] == 1
            print(f"[adjoint] refine 0 -> 1 normal residual {g0['info']['normal_resid']:.2e} -> {g1['info']['normal_resid']:.2e}")
            assert g1["info"]["normal_resid"] <= g0["info"]["normal_resid"]
            assert np.all(np.abs(g0["Axbar"] - g1["Axbar"]) <= bar["Axbar_rows"][Ai])
            assert np.all(np.abs(g0["Bbar"] - g1["Bbar"]) <= bar["Bbar"])
        finally:
            L.close()


# ---- 3: the dead set ----
@pytest.mark.parametrize("name", ["syn_dupcol", "syn_rankdef_grid"])
def test_dead_columns(pkg, name):
    m, n, Ap, Ai, Ax = matrix_of(name)
    B, Xbar = data(m, n, 2)
    L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=2)
    try:
        X, got = solve_and_adjoint(L, B, Xbar, {})
        live = live_columns(L, n)
        assert int(L.info["rank"]) == live.size < n
        ref = ar.adjoint(m, n, Ap, Ai, Ax, B, X, Xbar, live=live)
        bar = ar.bars(ref, X, m)
        dead_entry = ~np.isin(ar.columns_of(n, Ap), live)
        assert dead_entry.any() and np.all(got["Axbar"][dead_entry] == 0.0)
        ratio = max(np.max(np.abs(got["Axbar"] - ref["Axbar"])) / bar["g"], np.max(np.abs(got["Bbar"] - ref["Bbar"]) / bar["Bbar"]))
        print(f"[adjoint] {name}: rank {live.size}/{n} kappa of the live columns {bar['kappa']:.3g} largest error / bar {ratio:.2e}")
        assert bar["kappa"] ** 2 * EPS <= 1e-2 and ratio <= 1.0
    finally:
        L.close()


# ---- 4: bits ----
@pytest.mark.parametrize("name", ["syn_grid3d", "epb1"])
def test_bits(pkg, torch, name):
    """host arrays and device pointers, two calls, a column of a 33-column call against the same column carried alone (Bbar; Axbar
    sums over the right-hand sides, so it is compared where there is one)"""
    m, n, Ap, Ai, Ax = matrix_of(name)
    anz = int(Ap[-1])
    k = 33
    B, Xbar = data(m, n, k)
    w = weights(m)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a).reshape(np.shape(a)[0], -1).T), dtype=torch.float64, device=dev)   # noqa: E731
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    L1 = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=1)
    try:
        kw = dict(w=w, lam=1e-2)
        X, got = solve_and_adjoint(L, B, Xbar, kw)
        _, again = solve_and_adjoint(L, B, Xbar, kw)
        for key in ("Axbar", "Bbar", "wbar", "Dbar"):
            assert np.array_equal(bits(got[key]), bits(again[key])), key
        tX, tXb, tw = up(X), up(Xbar), up(w)
        out = {key: torch.zeros(sz, dtype=torch.float64, device=dev) for key, sz in dict(ax=anz, bb=m * k, wb=m, db=n).items()}
        torch.cuda.synchronize()
        L.adjoint_dev(tX.data_ptr(), tXb.data_ptr(), w_ptr=tw.data_ptr(), axbar_ptr=out["ax"].data_ptr(), bbar_ptr=out["bb"].data_ptr(),
                      wbar_ptr=out["wb"].data_ptr(), dbar_ptr=out["db"].data_ptr())
        assert np.array_equal(bits(out["ax"].cpu().numpy()), bits(got["Axbar"]))
        assert np.array_equal(bits(out["bb"].cpu().numpy().reshape(k, m).T), bits(got["Bbar"]))
        assert np.array_equal(bits(out["wb"].cpu().numpy()), bits(got["wbar"])) and np.array_equal(bits(out["db"].cpu().numpy()), bits(got["Dbar"]))
        # a column that sits in the batch of 32 against the same column carried alone (column 32 is the whole second batch: the
        # passes run with one vector), on the SAME factors.  (A separate nrhs = 1 object is no yardstick for bits: it factorizes
        # another matrix, [A b], and its R11 differs from this one's in the last bits -- measured, 1 to 2 units.)
        for col in (0, 31):
            Xb2 = Xbar.copy()
            Xb2[:, [col, 32]] = Xbar[:, [32, col]]
            _, b2, _, _, _ = L.adjoint(X, Xb2, w=w)
            assert np.array_equal(bits(b2[:, 32]), bits(got["Bbar"][:, col])), f"column {col} of Bbar, alone in a batch"
            assert np.array_equal(bits(b2[:, col]), bits(got["Bbar"][:, 32]))
        # nrhs = 1: the layouts of k_lsa_entries coincide (no staging); two calls, host arrays and device pointers
        X1 = L1.solve(B[:, 5], **kw)[0]
        a1, b1, wb1, D1, _ = L1.adjoint(X1, Xbar[:, 5], w=w)
        a1b, b1b, *_ = L1.adjoint(X1, Xbar[:, 5], w=w)
        assert np.array_equal(bits(a1), bits(a1b)) and np.array_equal(bits(b1), bits(b1b))
        o1 = torch.zeros(anz, dtype=torch.float64, device=dev)
        tX1, tXb1 = up(X1), up(Xbar[:, 5])
        torch.cuda.synchronize()
        L1.adjoint_dev(tX1.data_ptr(), tXb1.data_ptr(), w_ptr=tw.data_ptr(), axbar_ptr=o1.data_ptr())
        assert np.array_equal(bits(o1.cpu().numpy()), bits(a1))
    finally:
        L.close(); L1.close()


# ---- 5: the torch layer ----
def torch_inputs(torch, name, damped, nrhs, dev):
    m, n, Ap, Ai, Ax = matrix_of(name)
    B, _ = data(m, n, nrhs)
    t = lambda v: torch.tensor(np.asarray(v, float), dtype=torch.float64, device=dev, requires_grad=True)   # noqa: E731
    ins = [t(Ax), t(B[:, 0] if nrhs == 1 else B)]
    if damped:
        ins += [t(weights(m)), t(scales(n)), t(0.3)]
    return (m, n, Ap, Ai, Ax), ins


@pytest.mark.parametrize("where", ["cpu", "cuda"])
@pytest.mark.parametrize("nrhs", [1, 2])
@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("name", ["syn_rand60x40", "syn_star"])
def test_gradcheck(pkg, ag, torch, name, damped, nrhs, where):
    mat, ins = torch_inputs(torch, name, damped, nrhs, torch.device(where))
    L = (pkg.DampedLeastSquares if damped else pkg.LeastSquares)(*mat, nrhs=nrhs)
    try:
        f = (lambda Ax, B, w, d, lam: ag.lstsq(L, Ax, B, w=w, d=d, lam=lam)) if damped else (lambda Ax, B: ag.lstsq(L, Ax, B))
        assert torch.autograd.gradcheck(f, ins)
        assert L.info["analyses"] == 1 and L.info["plans"] == 1
    finally:
        L.close()


@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_autograd_has_the_bits_of_adjoint_and_survives_stale_factors(pkg, ag, torch, where):
    """the gradients are adjoint()'s; two forwards through one object and then backward of the first: one repeated solve, and the
    gradients of a fresh object; only what requires a gradient gets one"""
    mat, ins = torch_inputs(torch, "syn_rand60x40", True, 2, torch.device(where))
    m, n, Ap, Ai, Ax = mat
    _, Xbar = data(m, n, 2)
    tXbar = torch.tensor(Xbar, dtype=torch.float64, device=ins[0].device)
    L, F = pkg.DampedLeastSquares(*mat, nrhs=2), pkg.DampedLeastSquares(*mat, nrhs=2)
    try:
        tAx, tB, tw, td, tl = ins
        X1 = ag.lstsq(L, tAx, tB, w=tw, d=td, lam=tl)
        X2 = ag.lstsq(L, tAx * 1.5, tB, w=tw, d=td, lam=tl)                      # another solve: the factors on the device are X2's
        (X1 * tXbar).sum().backward()
        assert L.resolves == 1
        first = [t.grad.detach().cpu().numpy().copy() for t in ins]
        for t in ins:
            t.grad = None
        (ag.lstsq(F, tAx, tB, w=tw, d=td, lam=tl) * tXbar).sum().backward()
        assert F.resolves == 0
        for a, t in zip(first, ins):
            assert np.array_equal(bits(a), bits(t.grad.detach().cpu().numpy()))
        Xn = X1.detach().cpu().numpy()
        a, b, wb, Db, _ = F.adjoint(Xn, Xbar, w=tw.detach().cpu().numpy())
        assert np.array_equal(bits(a), bits(first[0])) and np.array_equal(bits(b), bits(first[1])) and np.array_equal(bits(wb), bits(first[2]))
        assert np.array_equal(bits(np.sqrt(0.3) * Db), bits(first[3]))
        assert X2.shape == X1.shape
        # gradients only where they are required
        for t in ins:
            t.grad = None
        Xp = ag.lstsq(F, tAx.detach(), tB, w=tw.detach(), d=td.detach(), lam=0.3)
        (Xp * tXbar).sum().backward()
        assert tB.grad is not None and tAx.grad is None and tw.grad is None and td.grad is None
        assert np.array_equal(bits(tB.grad.detach().cpu().numpy()), bits(first[1]))
        with pytest.raises(pkg.StmmqrError, match="scale"):
            ag.lstsq(F, tAx, tB, w=tw, lam=0.3, scale=1)
    finally:
        L.close(); F.close()


# ---- 6: refusals on a live object ----
def test_refusals_on_a_live_object(pkg):
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    k = 2
    B, Xbar = data(m, n, k)
    w = weights(m)
    capi = importlib.import_module(PKG + ".capi")
    P, L = pkg.LeastSquares(m, n, Ap, Ai, Ax, nrhs=k), pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=k)
    try:
        for obj in (P, L):
            with pytest.raises(pkg.StmmqrError, match="no solve yet"):
                obj.adjoint(np.zeros((n, k)), Xbar)
        XP, wantP = solve_and_adjoint(P, B, Xbar, {})
        XL, wantL = solve_and_adjoint(L, B, Xbar, dict(w=w, lam=1e-2))
        guard = np.full(max(int(Ap[-1]), m * k), 7.0)

        def raw(obj, X=XL, ldx=n, Xb=Xbar, ldxb=n, wv=None, refine=1, ax=guard, bb=None, ldbb=m, wb=None, db=None):
            p = lambda a: None if a is None else a.ctypes.data                                              # noqa: E731
            return pkg.lib.stmmqr_ls_adjoint(obj._h, p(X), ldx, p(Xb), ldxb, p(wv), refine, p(ax), p(bb), ldbb, p(wb), p(db), 0, None)

        seen = 0

        def refused(call, word):
            nonlocal seen
            assert call() == -4 and word in pkg.lib.stmmqr_last_error().decode(), pkg.lib.stmmqr_last_error().decode()
            assert np.all(guard == 7.0), "a refusal writes nothing"
            seen += 1
            X, got = solve_and_adjoint(P, B, Xbar, {})
            assert np.array_equal(bits(got["Axbar"]), bits(wantP["Axbar"]))
            X, got = solve_and_adjoint(L, B, Xbar, dict(w=w, lam=1e-2))
            assert np.array_equal(bits(got["Axbar"]), bits(wantL["Axbar"])) and np.array_equal(bits(got["Dbar"]), bits(wantL["Dbar"]))

        small = np.zeros(m)
        refused(lambda: raw(L, X=None), "NULL")
        refused(lambda: raw(L, Xb=None), "NULL")
        refused(lambda: raw(L, ldx=n - 1), "leading dimension")
        refused(lambda: raw(L, ldxb=n - 1), "leading dimension")
        refused(lambda: raw(L, bb=guard, ldbb=m - 1), "ldbb")
        refused(lambda: raw(L, refine=-1), "refine")
        refused(lambda: raw(P, X=XP, wv=w), "plain object")
        refused(lambda: raw(P, X=XP, wb=small), "plain object")
        refused(lambda: raw(P, X=XP, db=small), "plain object")
        assert seen == 9
        for obj in (P, L):
            assert obj.info["analyses"] == 1 and obj.info["plans"] == 1
        assert isinstance(capi._adjoint_info(np.zeros(8)), dict)
    finally:
        P.close(); L.close()


# ---- 7: one real-size consistency check ----
def test_epb1_directional_derivative(pkg):
    """epb1 damped, lam = 1e-2: <gradient, direction> for a random direction over (Ax, B, w, d, lam) against central differences of
    <Xbar, x> (two more solves) at the relative step h = 1e-6.  The tolerance is not fixed in advance: the numpy yardstick runs the
    same check on syn_rand60x40 at the same step against numpy.linalg.lstsq, and the device is allowed ten times the yardstick's own
    disagreement with its finite differences (which, not the adjoint, set the floor).
    Measured on the MI355X: device 1.4e-14, yardstick 3.7e-12 (both relative to |gradient| |direction|)."""
    h = 1e-6

    def disagreement(m, n, Ax, B, w, d, lam, Xbar, solve, gradients, seed=61):
        rng = np.random.default_rng(seed)
        theta = dict(Ax=Ax, B=B, w=w, d=d, lam=np.array(lam))
        dirs = {key: rng.standard_normal(np.shape(v)) * np.abs(v).max() for key, v in theta.items()}
        grad = gradients(theta)
        loss = lambda t: float(np.sum(Xbar * solve(t)))                                                     # noqa: E731
        fd = (loss({key: theta[key] + h * dirs[key] for key in theta}) - loss({key: theta[key] - h * dirs[key] for key in theta})) / (2 * h)
        an = sum(float(np.sum(grad[key] * dirs[key])) for key in theta)
        scale = np.sqrt(sum(float(np.sum(grad[key] ** 2)) for key in theta)) * np.sqrt(sum(float(np.sum(dirs[key] ** 2)) for key in theta))
        return abs(fd - an) / scale, fd, an

    # the yardstick against numpy.linalg.lstsq
    m, n, Ap, Ai, Ax = matrix_of("syn_rand60x40")
    B, Xbar = data(m, n, 1)

    def np_solve(t):
        C = ar.dense_c(m, n, Ap, Ai, t["Ax"], t["w"], np.sqrt(float(t["lam"])) * t["d"])
        return np.linalg.lstsq(C, ar.dense_bt(t["B"], t["w"], n, True), rcond=None)[0]

    def np_grad(t):
        r = ar.adjoint(m, n, Ap, Ai, t["Ax"], t["B"], np_solve(t), Xbar, w=t["w"], d=t["d"], lam=float(t["lam"]))
        return dict(Ax=r["Axbar"], B=r["Bbar"], w=r["wbar"], d=r["dbar"], lam=np.array(r["lambdabar"]))

    floor, fd0, an0 = disagreement(m, n, Ax, B, weights(m), scales(n), 1e-2, Xbar, np_solve, np_grad)
    # the device on epb1
    m, n, Ap, Ai, Ax = matrix_of("epb1")
    B, Xbar = data(m, n, 1)
    L = pkg.DampedLeastSquares(m, n, Ap, Ai, Ax, nrhs=1)
    try:
        dev_solve = lambda t: L.solve(t["B"], Ax=t["Ax"], w=t["w"], d=t["d"], lam=float(t["lam"]))[0].reshape(n, 1)   # noqa: E731

        def dev_grad(t):
            X = dev_solve(t)
            a, b, wb, Db, _ = L.adjoint(X, Xbar, w=t["w"])
            Z = L.adjoint_z()
            lam = float(t["lam"])
            return dict(Ax=a, B=b, w=wb, d=np.sqrt(lam) * Db, lam=np.array(-np.sum(t["d"] ** 2 * np.sum(X * Z, axis=1))))

        got, fd, an = disagreement(m, n, Ax, B, weights(m), scales(n), 1e-2, Xbar, dev_solve, dev_grad)
        print(f"[adjoint] directional derivative: yardstick on syn_rand60x40 fd {fd0:.10e} adjoint {an0:.10e} disagreement {floor:.2e}; "
              f"device on epb1 fd {fd:.10e} adjoint {an:.10e} disagreement {got:.2e} (allowed {10 * floor:.2e})")
        assert got <= 10 * floor
    finally:
        L.close()
