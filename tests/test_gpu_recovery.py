"""Recovery paths of the cut schedule and the phased interface, alone and combined: a front that outlives its cut schedule
(STMMQR_ERR_RESCHEDULE, stats.reschedules), a bounded panel wait that runs out (stats.retries; STMMQR_DBG bit 12 simulates it,
no fault), an R+H arena that overflows, a captured hipGraph replayed while its key matches -- and the plan that is used again
after each of them.  Every result is checked as the neighbouring tests check theirs: integers bit-identical, the factors against
the CPU oracle (ftol 1e-10) or bit-identical to a healthy plan that runs the same kernels, exact retry / reschedule counts."""
import importlib

import numpy as np
import pytest

from parity import compare_integers, compare_numeric
from stmmqr_testlib import Symbolic, load_golden, numeric_from_gpu, scalar

pytestmark = pytest.mark.gpu
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
INTS = ("Hm", "Hr", "HStair", "HPinv", "Rdead", "Rblock_off", "Hii")

# Fronts that outlive their cut schedule in a whole-tree plan (big_front_cols 64 and 16 alike), counted once on an MI355X with
# STMMQR_DBG_EARLY=1 (one "[early]" line per front at the failing finish).  The count is deterministic: it depends only on the
# plan-time estimate fm_est and on integer ranks that are bit-exact against the reference.  The full-rank fixtures have none, and
# so do syn_rankdef_grid and cvxqp3: their dead columns never push a front past its schedule.
OUTLIVING = {"lns_3937": 55, "bayer10": 19}
LAST_OUTLIVING = {"lns_3937": 219, "bayer10": 2086}       # the highest-numbered such front (Post order: its ancestors come after it)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    assert p.device_count() >= 1, "no GPU visible"
    assert "gfx950" in p.device_name(0)
    return p


def sym_dict(S):
    return {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}


def setup(name):
    g = load_golden(name)
    S = Symbolic(g)
    return g, S, sym_dict(S), scalar(g, "in_tol"), int(scalar(g, "in_ntol"))


def same_bits(X, A):
    assert (X.rank, X.rh_total) == (A.rank, A.rh_total)
    for k in INTS + ("HTau",):
        assert np.array_equal(getattr(X, k), getattr(A, k)), k
    assert np.array_equal(X.Stack[:X.rh_total], A.Stack[:A.rh_total], equal_nan=True)


def against_golden_and_oracle(oracle, S, G, g, name):
    compare_integers(S, numeric_from_gpu(S, G), g)
    No = oracle.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    compare_numeric(oracle, S, G, No, g, ftol=1e-10, name=name)


@pytest.mark.parametrize("name", ["lns_3937", "bayer10", "syn_rankdef_grid", "epb1"])
def test_outliving_fronts_are_pinned(pkg, monkeypatch, capfd, name):
    """the fronts that outlive the cut schedule, counted by the library itself (STMMQR_DBG_EARLY), and the one reschedule they cost"""
    g, S, sym, tol, ntol = setup(name)
    monkeypatch.setenv("STMMQR_DBG_EARLY", "1")
    plan = pkg.HipQR(sym)
    try:
        capfd.readouterr()
        st = plan.factorize(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
        err = capfd.readouterr().err
    finally:
        plan.close()
    fronts = [int(l.split()[2]) for l in err.splitlines() if l.startswith("[early] front ")]
    assert len(fronts) == OUTLIVING.get(name, 0)
    assert max(fronts, default=-1) == LAST_OUTLIVING.get(name, -1)
    assert st["reschedules"] == (1 if name in OUTLIVING else 0) and st["retries"] == 0
    assert st["flops"] == scalar(g, "flopcount")


@pytest.mark.parametrize("name", ["epb1", "grid20_standin"])
def test_panel_wait_timeout_keeps_the_cut_schedule(pkg, oracle, monkeypatch, name):
    """A wait that ran out leaves its front unfinished, which also looks like a front that outlived its schedule.  It must be
    reported as what it is: one serial retry on the SAME (cut) schedule, no reschedule -- and the plan keeps the cut schedule."""
    g, S, sym, tol, ntol = setup(name)
    pkg.set_options(tall_min_rows=0, big_front_cols=16)
    try:
        fresh = pkg.HipQR(sym)
        st_f = fresh.factorize(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
        H = fresh.download()
        fresh.close()
        plan = pkg.HipQR(sym)
        try:
            monkeypatch.setenv("STMMQR_DBG", "4096")
            st1 = plan.factorize(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
            monkeypatch.delenv("STMMQR_DBG")
            G = plan.download()
            st2 = plan.factorize(g["in_Ax"], tol, ntol)
            G2 = plan.download()
        finally:
            monkeypatch.delenv("STMMQR_DBG", raising=False)
            plan.close()
    finally:
        pkg.set_options(tall_min_rows=0, big_front_cols=64)
    assert st_f["retries"] == 0 and st_f["reschedules"] == 0
    assert st1["retries"] == 1 and st1["reschedules"] == 0
    assert st1["flops"] == st2["flops"] == scalar(g, "flopcount")
    against_golden_and_oracle(oracle, S, G, g, name)
    assert st2["retries"] == 0 and st2["reschedules"] == 0
    assert st2["nsteps"] == st_f["nsteps"]                      # the cut schedule survived the retry
    same_bits(G2, H)


def _two_phases(sym, last):
    """group 1: the strict ancestors of front `last`; group 0: everything else (every child runs no later than its parent)"""
    from stmmqr_testlib import I64
    nf = int(sym["nf"])
    parent = np.full(nf, -1, I64)
    Child, Childp = sym["Child"], sym["Childp"]
    for f in range(nf):
        for q in range(int(Childp[f]), int(Childp[f + 1])):
            parent[int(Child[q])] = f
    group = np.zeros(nf, np.int32)
    f = int(parent[last])
    while f >= 0:
        group[f] = 1
        f = int(parent[f])
    return group


@pytest.mark.parametrize("name", ["lns_3937"])
def test_schedule_failure_survives_a_later_group_retry(pkg, oracle, monkeypatch, name):
    """One phased plan on the cut schedule, two groups: group 0 holds the fronts that outlive their schedule, group 1 (their
    ancestors) has pipelined panels whose wait runs out (STMMQR_DBG bit 12, read per group).  The group retry of group 1 must not
    erase group 0's verdict: finish says STMMQR_ERR_RESCHEDULE.  The next begin of the same plan takes the full schedule by itself
    (no set_early_end call) and gives the bits of a healthy full-schedule plan of the same grouping."""
    g, S, sym, tol, ntol = setup(name)
    group = _two_phases(sym, LAST_OUTLIVING[name])
    assert group.sum() >= 1
    pkg.set_options(tall_min_rows=0, big_front_cols=16)
    try:
        healthy = pkg.HipQR(sym)
        healthy.set_groups(group)
        healthy.set_early_end(0)
        healthy.begin(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
        healthy.run_group(0)
        healthy.run_group(1)
        st_h = healthy.finish()
        H = healthy.download()
        healthy.close()
        plan = pkg.HipQR(sym)
        try:
            plan.set_groups(group)
            plan.set_early_end(1)
            plan.begin(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
            plan.run_group(0)
            monkeypatch.setenv("STMMQR_DBG", "4096")
            plan.run_group(1)
            monkeypatch.delenv("STMMQR_DBG")
            with pytest.raises(pkg.StmmqrError) as ei:
                plan.finish()
            assert ei.value.code == pkg.capi.ERR_RESCHEDULE
            plan.begin(g["in_Ax"], tol, ntol)
            plan.run_group(0)
            plan.run_group(1)
            st = plan.finish()
            G = plan.download()
            plan.begin(g["in_Ax"], tol, ntol)
            plan.run_group(0)
            plan.run_group(1)
            st3 = plan.finish()
        finally:
            monkeypatch.delenv("STMMQR_DBG", raising=False)
            plan.close()
    finally:
        pkg.set_options(tall_min_rows=0, big_front_cols=64)
    assert st_h["retries"] == 0 and st["retries"] == 0 and st3["retries"] == 0
    assert st3["reschedules"] == 0
    assert st["flops"] == st_h["flops"] == scalar(g, "flopcount")
    same_bits(G, H)
    against_golden_and_oracle(oracle, S, G, g, name)


@pytest.mark.parametrize("native", [False, True])
@pytest.mark.parametrize("name,nranks", [("lns_3937", 2), ("bayer10", 2)])
def test_reschedule_with_shared_fronts_rebegins_as_documented(pkg, name, nranks, native):
    """Sharded plans with shared fronts (spread_partition, span > 1) on the cut schedule, rank-deficient input: a rank's finish says
    STMMQR_ERR_RESCHEDULE, the ranks agree, and -- as include/stmmqr_hip.h documents -- the plan that failed simply begins again
    (it has switched to the full schedule by itself and must still know its shared fronts); only the others are told by
    set_early_end(0).  native=False, the Python phase loop: every cross-rank wait is a queue get with a time limit; native=True:
    the whole factorization as one native call per rank (stmmqr_factorize_phases, its own shared-front loop)."""
    import queue
    import threading
    import torch  # noqa: F401  (LocalComm's tensors)
    from test_gpu_sharded import LocalComm, _thread_transport
    sh = importlib.import_module(PKG + ".sharded")
    g, S, sym, tol, ntol = setup(name)
    pkg.set_options(pair_update=0, big_front_cols=16)
    try:
        ref = pkg.qr_factorize(sym, g["in_Ap"], g["in_Ai"], g["in_Ax"], tol, ntol)
        owner, phase, span = sh.spread_partition(sym, nranks, min_step_flops=0, min_share=0.01, min_cols=32, min_panels_per_rank=1)
        assert int((span > 1).sum()) >= 1
        queues = {(a, b): queue.Queue() for a in range(nranks) for b in range(nranks)}
        boxes = {(a, b): queue.Queue() for a in range(nranks) for b in range(nranks)}
        out, errs = [None] * nranks, []

        def work(r):
            try:
                comm = LocalComm(r, nranks, queues, None)
                if native:
                    comm.native = _thread_transport(pkg, r, nranks, boxes)
                plan = pkg.HipQR(sym)
                sp = sh.ShardPlan(plan, sym, owner, phase, comm, span)
                assert sp.early and len(sp.shared) >= 1
                bad = 0
                try:
                    st = sh._factorize_sharded_once(plan, sp, g["in_Ax"], tol, ntol, comm, g["in_Ap"], g["in_Ai"], None)
                except pkg.StmmqrError as e:
                    if e.code != pkg.capi.ERR_RESCHEDULE:
                        raise
                    bad = 1
                agreed = sh._any_rank(comm, bad)
                if agreed:
                    if not bad:
                        plan.set_early_end(0)
                    st = sh._factorize_sharded_once(plan, sp, g["in_Ax"], tol, ntol, comm, None, None, None)
                out[r] = (st, sh.shard_of(plan.download(), sym, sp.mine, plan, sp, r), bad, agreed)
                plan.close()
            except BaseException as e:       # noqa: BLE001 (reported by the main thread)
                errs.append((r, e))

        th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
        for t in th:
            t.start()
        for t in th:
            t.join(600)
        assert not errs, errs
        assert all(o is not None for o in out)
    finally:
        pkg.set_options(pair_update=4, big_front_cols=64)
    assert all(o[3] == 1 for o in out)                          # the fixture does reschedule ...
    assert sum(o[2] for o in out) >= 1                          # ... because some rank's front outlived the cut schedule
    assert sum(o[0]["retries"] for o in out) == 0
    G = sh.merge_shards(sym, [o[1] for o in out], ntol)
    assert sum(o[0]["flops"] for o in out) == ref.stats["flops"]
    assert (G.rank, G.rank1, G.maxfrank, G.maxfm, G.rh_total) == (ref.rank, ref.rank1, ref.maxfrank, ref.maxfm, ref.rh_total)
    for k in INTS + ("HTau",):
        np.testing.assert_array_equal(getattr(G, k), getattr(ref, k), err_msg=k)
    np.testing.assert_array_equal(G.Stack[:G.rh_total], ref.Stack[:ref.rh_total])


@pytest.mark.parametrize("name", ["lns_3937", "bayer10"])
def test_reschedule_on_a_recycling_plan_is_not_an_arena_overflow(pkg, oracle, monkeypatch, name):
    """Slab recycling (STMMQR_RECYCLE=2) with a front that outlives the cut schedule: the unfinished fronts pack what they hold,
    which the recycled arena need not fit.  The verdict is the schedule's (one reschedule, no retry), the arena is not grown for
    it, and the next factorization of the plan still recycles with the arena of a fresh plan."""
    g, S, sym, tol, ntol = setup(name)
    monkeypatch.setenv("STMMQR_RECYCLE", "2")
    fresh = pkg.HipQR(sym)
    st_f = fresh.factorize(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
    H = fresh.download()
    st_f2 = fresh.factorize(g["in_Ax"], tol, ntol)            # (a download allocates buffers of its own: compare like with like)
    fresh.close()
    plan = pkg.HipQR(sym)
    try:
        st1 = plan.factorize(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
        G = plan.download()
        st2 = plan.factorize(g["in_Ax"], tol, ntol)
        G2 = plan.download()
    finally:
        plan.close()
    assert st_f["retries"] == 0 and st_f["reschedules"] == 1
    assert st1["retries"] == 0 and st1["reschedules"] == 1
    assert st2["retries"] == 0 and st2["reschedules"] == 0
    assert st1["device_bytes"] == st_f["device_bytes"] and st2["device_bytes"] == st_f2["device_bytes"]
    assert st1["flops"] == st2["flops"] == scalar(g, "flopcount")
    same_bits(G, H)
    same_bits(G2, H)
    against_golden_and_oracle(oracle, S, G, g, name)


KNOBS = [("STMMQR_PASSENGERS", "0"), ("STMMQR_CA_RIDERS", "0"), ("STMMQR_PASS_MAXWG", "1"), ("STMMQR_PASS_TILES", "0")]


@pytest.mark.parametrize("name", ["grid20_standin", "epb1"])
def test_graph_key_follows_the_capture_time_knobs(pkg, monkeypatch, name):
    """options.use_graph: the captured schedule is replayed while its key matches.  The passenger knobs of the environment decide
    what run_schedule launches at capture time, so a plan factorized again under another value must capture again: the same
    launch count as a fresh plan under that value, and (these knobs only move launches) the same bits."""
    g, S, sym, tol, ntol = setup(name)
    pkg.set_options(use_graph=1)
    try:
        plan = pkg.HipQR(sym)
        try:
            st0 = plan.factorize(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
            A = plan.download()
            moved = 0
            for k, v in KNOBS:
                monkeypatch.setenv(k, v)
                st = plan.factorize(g["in_Ax"], tol, ntol)
                X = plan.download()
                other = pkg.HipQR(sym)
                st_f = other.factorize(g["in_Ax"], tol, ntol, g["in_Ap"], g["in_Ai"])
                other.close()
                monkeypatch.delenv(k)
                assert st["nlaunch"] == st_f["nlaunch"], k
                assert st["retries"] == st_f["retries"] == 0
                moved += st_f["nlaunch"] != st0["nlaunch"]
                same_bits(X, A)
            st9 = plan.factorize(g["in_Ax"], tol, ntol)           # ... and back to the defaults
            assert st9["nlaunch"] == st0["nlaunch"]
        finally:
            plan.close()
    finally:
        pkg.set_options(use_graph=0)
    assert moved >= 1                                            # (some knob does change what is launched here)
