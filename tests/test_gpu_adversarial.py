"""Rank decisions next to the tolerance and the refresh of the Gram-based panel, on the dense fronts of
tests/adversarial_fronts.py (columns whose pivot is tol * 8 or tol / 8, at the edges of the 32-column panels and the
8-column sub-panels, one whole sub-panel dead, a dead last pivot, tiny columns at or beyond ntol).

The decision |beta| <= tol is coded once per panel path (dev_panel / dev_subpanel_reg, dev_tall_group, dev_wave_panel,
k_front_wg, k_panel_ca); every path must decide each column as the long-double column loop does (the decisions are at
least 3.8x away from tol there, tests/test_adversarial_cpu.py), and its factors must reproduce the front to 1e-13 -- the
parity bound of the project (README, compare_numeric(backward_tol=1e-13)).  F and Tau are not compared entry by entry:
cond(R) is about 1e9 on these fronts, the fp64 column loop itself is 2e-8 away from long double on R's diagonal; only the
backward quantities are determined.

Part A: the qr_front seam, path by path.  Part B: the same fronts as one-front plans (k_panel_pc, k_panel_ca_pc, passenger
and rider updates, pair / quad sweeps)."""
import importlib

import numpy as np
import pytest

from adversarial_fronts import TOL, backward_metrics, crafted_columns, make_adversarial, ref_front
from stmmqr_testlib import I64, Symbolic, aqr_probe_error, numeric_from_gpu

pytestmark = pytest.mark.gpu
KINDS = ("full", "ramp", "steps")


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


# ---------------------------------------------------------------------------------------------------------------------
# Part A: the qr_front seam
# ---------------------------------------------------------------------------------------------------------------------
WG = dict(big_front_cols=128)                                                # k_front_wg
LDS = dict(big_front_cols=8, tall_min_rows=1 << 30, panel_algo=1)            # one workgroup, panel image in LDS
PIPE = dict(big_front_cols=8, tall_min_rows=0, panel_algo=1)                 # wave panel (short) / column pipeline (tall)
GRAM = dict(big_front_cols=8, panel_algo=2)                                  # k_panel_ca, every panel
AUTO = dict(big_front_cols=8, panel_algo=0)                                  # Gram panel by the default rule


def _cases():
    out = []

    def add(path, opts, dbg, ms, kinds=KINDS, piv=(96, 96)):
        for m in ms:
            for kind in kinds:
                out.append(pytest.param(opts, dbg, m, kind, piv[0], piv[1], id=f"{path}-{m}-{kind}-npiv{piv[0]}-ntol{piv[1]}"))

    add("wg", WG, None, (186, 700))
    add("lds", LDS, None, (186, 1300))
    add("wave", PIPE, None, (186,))
    add("pipe-short", PIPE, 16384, (186,))
    add("pipe", PIPE, None, (1300, 2600, 4500))              # 8-, 4- and 2-column groups
    add("pipe", PIPE, None, (8300,), ("full", "ramp"))       # above 8192 rows: one workgroup
    add("gram", GRAM, None, (186, 1300, 2600))               # one slab and several
    for late in (0, 2):                                      # the slab workgroup that starts late owns the chain
        add(f"gram-late{late}", GRAM, 2048 + (late << 20), (1300,))
    add("gram-auto", AUTO, None, (4500,))
    for path, opts in (("lds", LDS), ("pipe", PIPE), ("gram", GRAM)):
        add(path, opts, None, (1300,), ("full",), (96, 90))  # column 95 is tiny, but at ntol or beyond: it stays live
        add(path, opts, None, (1300,), ("full",), (64, 64))  # columns 64, 70, 95 are not pivotal: they stay live
    return out


@pytest.mark.parametrize("opts,dbg,m,kind,npiv,ntol", _cases())
def test_qr_front_adversarial(pkg, oracle, monkeypatch, opts, dbg, m, kind, npiv, ntol):
    n = 96
    F0, St0, _ = make_adversarial(m, n, kind)
    rank, St, Rdead, _ = ref_front(F0, St0, npiv, TOL, ntol)
    Fg, Sg = F0.copy(order="F"), St0.copy()
    base = pkg.get_options()
    pkg.set_options(**opts)
    if dbg is not None:
        monkeypatch.setenv("STMMQR_DBG", str(dbg))
    try:
        rg, Tg, Dg, flg = pkg.qr_front(m, n, npiv, TOL, ntol, Fg, Sg)
    finally:
        if dbg is not None:
            monkeypatch.delenv("STMMQR_DBG")
        pkg.set_options(**{k: base[k] for k in opts})
    Fo, So = F0.copy(order="F"), St0.copy()
    _, _, _, flo = oracle.front(Fo, So, npiv, TOL, ntol)
    assert np.all(np.isfinite(Fg)) and np.all(np.isfinite(Tg))
    wrong = np.flatnonzero(np.asarray(Dg) != Rdead).tolist()
    assert not wrong, f"dead/live decision differs from long double at columns {wrong}"
    assert rg == rank
    np.testing.assert_array_equal(Sg, St)
    assert flg == flo
    e_live, e_dead, orth = backward_metrics(F0, Fg, Sg, Tg, Dg, npiv)
    print(f"\n{m}x{n} {kind} npiv={npiv} ntol={ntol} {opts} dbg={dbg}: e_live {e_live:.2e} orth {orth:.2e} e_dead {e_dead:.2e}")
    assert e_live <= 1e-13
    assert orth <= 1e-13
    assert e_dead <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# Part B: one-front plans
# ---------------------------------------------------------------------------------------------------------------------
N_PLAN = 160
PLAN_CONFIGS = [("default", {}, None), ("gram", dict(panel_algo=2), None),
                ("lookahead0", dict(lookahead=0), None), ("lookahead1", dict(lookahead=1), None), ("lookahead2", dict(lookahead=2), None),
                ("pair", dict(pair_update=1), "1"), ("quad", dict(pair_update=4), "1")]


def _dense_csc(F):
    m, n = F.shape
    Ap = np.arange(0, m * n + 1, m, dtype=I64)
    Ai = np.tile(np.arange(m, dtype=I64), n)
    return Ap, Ai, np.ascontiguousarray(F.T).ravel()


def _testlib_symbolic(sym):
    return Symbolic({"sym_" + k: (v if isinstance(v, np.ndarray) else np.array([v])) for k, v in sym.items() if k != "info"})


@pytest.mark.parametrize("m", [700, 2600, 4500])
def test_one_front_plan_adversarial(pkg, oracle, monkeypatch, m):
    """At n = 160 (five panels) the quad sweep of the `quad` configuration has no column (ncbp = 0 after panel 3) and the pair
    sweep has two column blocks once: the sweeps themselves are covered by tests/test_gpu_sweeps.py."""
    n = N_PLAN
    F0, St0, crafted = make_adversarial(m, n, "full")
    rank, _, Rdead, _ = ref_front(F0, St0, n, TOL, n)
    assert rank == n - 15
    Ap, Ai, Ax = _dense_csc(F0)
    sym = pkg.analyze(m, n, Ap, Ai, Qfill=None)
    assert sym["nf"] == 1                       # a dense pattern is one front holding every row and column
    np.testing.assert_array_equal(sym["PLinv"], np.arange(m))
    S = _testlib_symbolic(sym)
    rng = np.random.default_rng(m)
    X = np.asfortranarray(rng.standard_normal((m, 3)))
    base = pkg.get_options()
    results = {}
    for name, opts, pair_min in PLAN_CONFIGS:
        pkg.set_options(**opts)
        if pair_min is not None:
            monkeypatch.setenv("STMMQR_PAIR_MIN", pair_min)
        plan = None
        try:
            plan = pkg.HipQR(sym)
            stats = plan.factorize(Ax, TOL, n, Ap, Ai)
            N = plan.download()
            QtX = plan.qmult(0, X)
            if name == "default":
                # other values through the same plan, then these again: nothing of a factorization with dead columns is left behind
                G0, _, _ = make_adversarial(m, n, "full", craft=False)
                stats_g = plan.factorize(_dense_csc(G0)[2], TOL, n, Ap, Ai)
                Ng = plan.download()
                stats_2 = plan.factorize(Ax, TOL, n, Ap, Ai)
                N2 = plan.download()
        finally:
            if plan is not None:
                plan.close()
            if pair_min is not None:
                monkeypatch.delenv("STMMQR_PAIR_MIN")
            pkg.set_options(**{k: base[k] for k in opts})
        assert stats["retries"] == 0, name
        wrong = np.flatnonzero(N.Rdead[:n] != Rdead).tolist()
        assert not wrong, f"{name}: dead/live decision differs from long double at columns {wrong}"
        assert N.rank == rank, name
        assert np.all(np.isfinite(N.Stack[:N.rh_total])) and np.all(np.isfinite(N.HTau)), name
        err = aqr_probe_error(oracle, S, numeric_from_gpu(S, N), Ap, Ai, Ax, live_only=True)
        qn = np.abs(np.linalg.norm(QtX, axis=0) / np.linalg.norm(X, axis=0) - 1).max()
        print(f"\n{m}x{n} plan {name}: probe error {err:.2e}  | ||Q'x|| / ||x|| - 1 | {qn:.2e}")
        assert err <= 1e-13, name
        assert qn <= 1e-12, name
        results[name] = N
        if name == "default":
            assert stats_g["retries"] == 0 and stats_2["retries"] == 0
            assert Ng.rank == n and not Ng.Rdead[:n].any()
            assert N2.rank == N.rank and N2.rh_total == N.rh_total
            for k in ("Rdead", "HStair", "HTau"):
                np.testing.assert_array_equal(getattr(N2, k), getattr(N, k), err_msg=k)
            np.testing.assert_array_equal(N2.Stack[:N2.rh_total], N.Stack[:N.rh_total])
    first = results["default"]
    for name, N in results.items():
        assert N.rank == first.rank, name
        np.testing.assert_array_equal(N.Rdead, first.Rdead, err_msg=name)
    assert sorted(np.flatnonzero(first.Rdead[:n]).tolist()) == [k for k, (d, _) in crafted.items() if d < TOL]
