"""The pair and quad sweeps of the trailing update (csrc/stmmqr_sweep.hip: k_upd_w2 / y2 / c2, k_upd_wq / yq / cq) on dense and
staircase fronts chosen for the edges of their indexing and masks -- tests/sweep_cases.py has the inputs and the shape arithmetic,
tests/test_sweep_cases_cpu.py proves what the list covers (slabs per workgroup 1 / 2 / 4 / 8 and both sides of every threshold inside
one front, one slab group without a ticket, a partial last group, a last slab of one row, one and many column blocks, last blocks of
1 / 31 / 32 columns, fronts that end 0 .. 3 panels into a sweep, rows that run out in every panel of a sweep, panels of one sweep
with different rows, dead reflectors and whole dead panels, two fronts in one launch).

Every case is a one-front plan (one case: two fronts, diag(A, B)) from pkg.analyze, factorized with STMMQR_PAIR_MIN = 1 under
options.pair_update = 1 (sweeps of two panels) and 4 (of four).  Per sweep form:

  that the sweep ran: the factorization runs with STMMQR_DBG = 65536, under which the host prints one line per front of every sweep
      launch with the front's own column blocks; the (front, panel, ncbp) with ncbp > 0 must be those sweep_cases.launches derives
      from the shapes -- never none, except the quad on fronts of five panels (sweep_cases.NO_QUAD_COLUMNS: the pair's cases);
  the CPU oracle (as tests/test_gpu_block0.py): rank, HStair, Rdead, rh_total and the flop count exact; HTau and Stack[:rh_total]
      within 1e-11 of their 2-norms;
  per column of every front, so that one wrong tile cannot hide in a whole-factor norm: the relative 2-norm distance of the column
      (R above the diagonal, the reflector below) from the oracle's, gate 1e-11 -- unless the fp64 oracle itself is further than
      1e-12 from the long-double column loop (sweep_cases.ld_front) on some column of that input: then ten times that distance
      (the square-ish fronts and those with fewer rows than columns; fronts of up to 600 rows, measured in the test itself on the CPU);
  in long double from the returned factors, fronts of up to 600 rows: adversarial_fronts.backward_metrics on the front unpacked from
      its R+H block -- e_live <= 1e-13, orth <= 1e-13, e_dead <= tol (the gates of tests/test_gpu_adversarial.py; without a
      tolerance the only `dead` columns are those behind the last row, whose columns of A = QR are held to e_live's accuracy:
      e_dead <= 1e-13 ||F||_F); taller fronts and the two-front case: aqr_probe_error(live_only) <= 1e-13 and
      | ||Q'x|| / ||x|| - 1 | <= 1e-12;
  stats: no retry, no reschedule.

And between the forms (test_other_forms_and_same_bits): pair_update = 0 gives the same integers and factors within the same gates
of each sweep result (the rounding differs: DESIGN.md 7); lookahead = 0 and 2 give the same bits (sweep steps stay on one stream);
STMMQR_TUNE = 1 (one slab per workgroup, full slot stride) gives the same bits where every sweep of the case has one slab per
workgroup anyway.  Where a workgroup takes 2, 4 or 8 slabs the code does NOT promise the bits of the one-slab form: a grouped
workgroup carries ONE accumulator chain through all its slabs, the one-slab form starts every slab at zero and adds the partial sums
afterwards -- there the gates are asserted instead."""
import importlib

import numpy as np
import pytest

import sweep_cases as sc
from adversarial_fronts import backward_metrics
from stmmqr_testlib import aqr_probe_error, numeric_from_gpu

pytestmark = pytest.mark.gpu
SMALL = 600                    # fronts of up to this many rows: long double on the whole front
_REF, _RUN = {}, {}            # per case: the inputs and the oracle's factors, once; per (case, sweep): the factorization under test


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
    assert p.device_count() >= 1
    return p


def reference(pkg, oracle, case):
    """inputs, symbolic phase, the oracle's factors in front form and the per-column gate of a case: computed once, shared, read-only"""
    if case.name in _REF:
        return _REF[case.name]
    R = type("Ref", (), {})()
    R.fronts = [sc.make_front(fr) for fr in case.fronts]
    R.sym, R.S, R.Ap, R.Ai, R.Ax = sc.analyzed(pkg, R.fronts)
    R.n = int(R.sym["n"])
    R.No = oracle.factorize(R.S, R.Ap, R.Ai, R.Ax, case.tol, R.n)
    R.No.rh_total = int(R.No.c.rh_total)
    R.dense = R.No.dense = [sc.unpack_front(R.No, R.S, f)[0] for f in range(len(case.fronts))]
    R.small = len(case.fronts) == 1 and sc.front_rows(case.fronts[0]) <= SMALL
    R.gate, R.d_oracle = 1e-11, None
    if R.small:
        fm = sc.front_rows(case.fronts[0])
        A, St, Rdead = sc.ld_front(R.fronts[0][0][:fm], np.minimum(R.fronts[0][1], fm), case.tol)
        assert np.array_equal(St, R.No.HStair[:R.n]) and np.array_equal(Rdead, R.No.Rdead[:R.n])
        R.d_oracle = float(sc.column_distances(R.dense[0], A).max())
        if R.d_oracle > 1e-12:
            R.gate = 10 * R.d_oracle
    rng = np.random.default_rng(len(case.name))
    R.X = np.asfortranarray(rng.standard_normal((int(R.sym["m"]), 3)))
    for a in R.dense + [R.X]:
        a.setflags(write=False)
    _REF[case.name] = R
    return R


def same_integers(A, B):
    assert (A.rank, A.rh_total) == (B.rank, B.rh_total)
    for k in ("HStair", "Rdead", "Rblock_off"):
        assert np.array_equal(getattr(A, k), getattr(B, k)), k


def same_bits(A, B):
    same_integers(A, B)
    assert np.array_equal(A.HTau, B.HTau)
    assert np.array_equal(A.Stack[:A.rh_total], B.Stack[:B.rh_total])


def within_gates(A, B, S, nfronts, gate, label):
    """A against B: the norm-wise gate of the project on HTau and the packed factors, and `gate` per column of every front"""
    rj = int(S.rjsize)
    dT, dF = np.linalg.norm(A.HTau[:rj] - B.HTau[:rj]), np.linalg.norm(A.Stack[:A.rh_total] - B.Stack[:B.rh_total])
    nT, nF = max(np.linalg.norm(B.HTau[:rj]), 1), np.linalg.norm(B.Stack[:B.rh_total])
    worst = 0.0
    for f in range(nfronts):
        d = sc.column_distances(sc.unpack_front(A, S, f)[0], B.dense[f] if hasattr(B, "dense") else sc.unpack_front(B, S, f)[0])
        k = int(np.argmax(d))
        print(f"    {label} front {f}: worst column {k} at {d[k]:.3e} (gate {gate:.1e})")
        worst = max(worst, float(d[k]))
        assert d[k] <= gate, (label, f, k, d[k])
    print(f"    {label}: |dTau| {dT / nT:.3e}  |dF| {dF / nF:.3e}  worst column {worst:.3e}")
    assert dT <= 1e-11 * nT and dF <= 1e-11 * nF, label
    return worst


def run(pkg, monkeypatch, R, case, env=None, **options):
    monkeypatch.setenv("STMMQR_PAIR_MIN", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        return sc.factorize(pkg, R.sym, R.Ap, R.Ai, R.Ax, case.tol, R.n, **options)
    finally:
        monkeypatch.delenv("STMMQR_PAIR_MIN")
        for k in env or {}:
            monkeypatch.delenv(k)


def sweep_result(pkg, oracle, monkeypatch, capfd, case, w):
    """the factorization under pair_update = 1 (w = 2) / 4 (w = 4), its sweep launches counted; once per (case, w)"""
    if (case.name, w) in _RUN:
        return _RUN[case.name, w]
    R = reference(pkg, oracle, case)
    capfd.readouterr()
    st, N, QtX = run(pkg, monkeypatch, R, case, env={"STMMQR_DBG": str(sc.SWEEP_LINES)}, X=R.X, pair_update=1 if w == 2 else 4)
    ran, forms = sc.reported_launches(capfd.readouterr().err)
    want = sorted(sc.case_launches(case, w))
    print(f"\n{case.name}, sweeps of {w}: {len(ran)} launches with columns reported, {len(want)} expected: {want}")
    assert ran == want and forms <= {w}
    assert bool(want) != (w == 4 and case.name in sc.NO_QUAD_COLUMNS)
    _RUN[case.name, w] = (st, N, QtX)
    return st, N, QtX


@pytest.mark.parametrize("w", [2, 4])
@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_sweep_against_oracle_and_long_double(pkg, oracle, monkeypatch, capfd, name, w):
    case = sc.BY_NAME[name]
    R = reference(pkg, oracle, case)
    st, N, QtX = sweep_result(pkg, oracle, monkeypatch, capfd, case, w)
    S, No, n = R.S, R.No, R.n
    assert st["retries"] == 0 and st["reschedules"] == 0
    # ---- the CPU oracle ----
    assert N.rank == No.c.rank == sum(sc.expected_rank(fr) for fr in case.fronts) and N.rh_total == No.c.rh_total
    np.testing.assert_array_equal(N.HStair[:S.rjsize], No.HStair[:S.rjsize])
    np.testing.assert_array_equal(N.Rdead[:n], No.Rdead[:n])
    assert st["flops"] == No.c.flopcount
    assert np.all(np.isfinite(N.Stack[:N.rh_total])) and np.all(np.isfinite(N.HTau))
    if R.d_oracle is not None:
        print(f"    oracle against long double, worst column: {R.d_oracle:.3e}")
    within_gates(N, No, S, len(case.fronts), R.gate, f"pair_update={1 if w == 2 else 4} against the oracle")
    # ---- long double from the returned factors ----
    if R.small:
        fm = sc.front_rows(case.fronts[0])
        F0 = R.fronts[0][0][:fm]
        Fout, St, Tau = sc.unpack_front(N, S, 0)
        e_live, e_dead, orth = backward_metrics(F0, Fout, St, Tau, N.Rdead[:n], n)
        print(f"    e_live {e_live:.2e}  e_dead {e_dead:.2e}  orth {orth:.2e}")
        assert e_live <= 1e-13 and orth <= 1e-13
        assert e_dead <= (case.tol if case.tol > 0 else 1e-13 * np.linalg.norm(F0))
    else:
        err = aqr_probe_error(oracle, S, numeric_from_gpu(S, N), R.Ap, R.Ai, R.Ax, live_only=True)
        qn = np.abs(np.linalg.norm(QtX, axis=0) / np.linalg.norm(R.X, axis=0) - 1).max()
        print(f"    probe error {err:.2e}  | ||Q'x|| / ||x|| - 1 | {qn:.2e}")
        assert err <= 1e-13 and qn <= 1e-12


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_other_forms_and_same_bits(pkg, oracle, monkeypatch, capfd, name):
    case = sc.BY_NAME[name]
    R = reference(pkg, oracle, case)
    st0, N0, _ = run(pkg, monkeypatch, R, case, pair_update=0)
    assert st0["retries"] == 0 and st0["reschedules"] == 0
    for w in (2, 4):
        pu = 1 if w == 2 else 4
        st, N, _ = sweep_result(pkg, oracle, monkeypatch, capfd, case, w)
        # ---- panel by panel: the same integers, the same gates ----
        same_integers(N0, N)
        assert st0["flops"] == st["flops"]
        within_gates(N0, N, R.S, len(case.fronts), R.gate, f"pair_update=0 against {pu}")
        # ---- lookahead 0 against 2: the same bits ----
        stl, Nl, _ = run(pkg, monkeypatch, R, case, pair_update=pu, lookahead=0)
        assert stl["retries"] == 0 and stl["reschedules"] == 0
        same_bits(Nl, N)
        # ---- one slab per workgroup against the default rule ----
        stt, Nt, _ = run(pkg, monkeypatch, R, case, env={"STMMQR_TUNE": "1"}, pair_update=pu)
        assert stt["retries"] == 0 and stt["reschedules"] == 0
        grouped = any(s.spw > 1 for fr in case.fronts for s in sc.front_sweeps(fr, w) if s.work)
        if grouped:
            same_integers(Nt, N)
            within_gates(Nt, N, R.S, len(case.fronts), R.gate, f"pair_update={pu}, one slab per workgroup against grouped slabs")
        else:
            same_bits(Nt, N)
