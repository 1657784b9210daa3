"""The windowed download of the packed factors of a plan that recycles its slabs (stmmqr_plan_download: k_rh_window with H,
k_r_window without, two bounce buffers in flight) at window edges the tests choose.

STMMQR_DOWNLOAD_WIN shrinks the window (256 MB by default: one window for every small fixture), STMMQR_KEEP_FRONTS forces which
fronts keep their slab and are packed on the fly, HipQR.front_kept tells which did.  tests/pack_window_cases.py models the layout,
classifies every window edge by what it cuts and aims windows at the exact positions (tests/test_pack_window_cases_cpu.py checks
that model against the reference's own factors and shows that the windows used here reach every class of edge).

Yardstick in every test: a plan of the same symbolic input and keepH under STMMQR_RECYCLE=0 -- the arena laid out in Post order by
k_rh_copy / k_r_copy and downloaded by ONE hipMemcpy, no code shared with the window kernels.  Everything here moves data: equal
means equal in every bit.  The stack buffer of every download is filled with a NaN of a payload no factor has and carries 64 guard
doubles: a hole in the windows and a write beyond rh_total both show."""
import contextlib
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from pack_window_cases import CLASSES, classify_edges, packed_layout, window_list
from stmmqr_testlib import Symbolic, load_golden, scalar
from test_pack_window_cases_cpu import GPU_FIXTURES, UNREACHABLE

pytestmark = pytest.mark.gpu
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"
I64, U64 = np.int64, np.uint64
SENTINEL = U64(0x7FF8DEADBEEF0BAD)        # a quiet NaN with a payload of its own
GUARD = 64
KNOBS = ("STMMQR_RECYCLE", "STMMQR_KEEP_FRONTS", "STMMQR_DOWNLOAD_WIN", "STMMQR_RESIDENT_CACHE", "STMMQR_PLAN_CACHE")
# edges by class met by test_windows_equal_one_copy: [keepH][kept | staged][class]
TALLY = {kh: {who: {c: 0 for c in CLASSES} for who in ("kept", "staged")} for kh in (1, 0)}


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module(PKG)
    assert p.device_count() >= 1
    return p


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module(PKG + ".capi")


@contextlib.contextmanager
def knobs(**kw):
    """the environment knobs of this module set to kw and nothing else, restored afterwards"""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in kw.items():
            assert k in KNOBS
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture
def env():
    """a test starts with none of the module's knobs set; env(NAME=value, ...) sets some for the rest of the test; all restored"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}

    def put(**kw):
        for k, v in kw.items():
            assert k in KNOBS
            os.environ[k] = str(v)
    yield put
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def new_plan(pkg, g, keep_h):
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1 if keep_h else 0}
    plan = pkg.HipQR(sym)
    try:
        plan.fstats = factorize(plan, g)
    except Exception:
        plan.close()
        raise
    return S, plan


def factorize(plan, g):
    return plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")), g["in_Ap"], g["in_Ai"])


def raw_download(capi, plan):
    """stmmqr_plan_download itself into a sentinel-filled stack of rh_total + GUARD doubles -> dict of everything it returns"""
    total = plan.result_sizes()[0]
    s = plan.sym
    out = {"Stack": np.full(total + GUARD, SENTINEL, U64).view(np.float64), "Rblock_off": np.zeros(max(s["nf"], 1), I64),
           "Rdead": np.zeros(max(s["n"], 1), np.int8), "HStair": np.zeros(max(s["rjsize"], 1), I64), "HTau": np.zeros(max(s["rjsize"], 1)),
           "Hii": np.zeros(max(s["hisize"], 1), I64), "HPinv": np.zeros(max(s["m"], 1), I64), "Hm": np.zeros(max(s["nf"], 1), I64),
           "Hr": np.zeros(max(s["nf"], 1), I64), "scalars": np.zeros(4, I64)}
    ip = lambda a: a.ctypes.data_as(capi.c_long_p)
    dp = lambda a: a.ctypes.data_as(capi.c_double_p)
    rc = capi.lib.stmmqr_plan_download(plan._h, dp(out["Stack"]), ip(out["Rblock_off"]), C.cast(out["Rdead"].ctypes.data, C.c_char_p),
                                       ip(out["HStair"]), dp(out["HTau"]), ip(out["Hii"]), ip(out["HPinv"]), ip(out["Hm"]), ip(out["Hr"]),
                                       ip(out["scalars"]), None)
    assert rc == 0, capi.last_error()
    out["rh_total"] = total
    return out


def assert_download_is(got, ref, what):
    """a raw download against the yardstick's: no sentinel left, the guard untouched, every array bit for bit"""
    total = ref["rh_total"]
    assert got["rh_total"] == total, what
    bits, want = got["Stack"].view(U64), ref["Stack"].view(U64)
    holes = np.flatnonzero(bits[:total] == SENTINEL)
    assert holes.size == 0, f"{what}: {holes.size} positions never written, the first at {holes[:8]}"
    assert np.all(bits[total:] == SENTINEL), f"{what}: written beyond rh_total at {total + np.flatnonzero(bits[total:] != SENTINEL)[:8]}"
    bad = np.flatnonzero(bits[:total] != want[:total])
    assert bad.size == 0, f"{what}: {bad.size} doubles of the stack differ, the first at {bad[:8]} of {total}"
    for k in ("Rblock_off", "HStair", "Rdead", "Hm", "Hr", "Hii", "HPinv", "scalars"):
        assert np.array_equal(got[k], ref[k]), f"{what}: {k}"
    assert np.array_equal(got["HTau"].view(U64), ref["HTau"].view(U64)), f"{what}: HTau"


_yard = {}


def yardstick(pkg, capi, name, keep_h):
    """the STMMQR_RECYCLE=0 plan of a fixture: its raw download and (with H) Q'b, Q b and the solve of a fixed b -- made once, left
    unchanged"""
    key = (name, bool(keep_h))
    if key not in _yard:
        g = load_golden(name)
        with knobs(STMMQR_RECYCLE="0"):
            S, plan = new_plan(pkg, g, keep_h)
            try:
                assert plan.front_kept(0) == -1, "the yardstick plan recycles its slabs"
                assert plan.fstats["retries"] == 0
                ref = raw_download(capi, plan)
                assert np.all(ref["Stack"].view(U64)[ref["rh_total"]:] == SENTINEL)
                assert not np.any(ref["Stack"].view(U64)[:ref["rh_total"]] == SENTINEL)
                if keep_h:
                    b = rhs(S)
                    ref["qtb"], ref["qb"] = plan.qmult(0, b), plan.qmult(1, b)
                    ref["x"] = plan.solve(b) if int(ref["scalars"][0]) == S.n else None
            finally:
                plan.close()
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _yard[key] = (g, S, ref)
    return _yard[key]


def rhs(S):
    return np.cos(np.arange(S.m) * 0.37)


def kept_fronts(plan, nf):
    flags = [plan.front_kept(f) for f in range(nf)]
    assert all(v in (0, 1) for v in flags), "the plan does not recycle its slabs"
    return [f for f, v in enumerate(flags) if v]


# ---- a: every window of the list against the one copy ----
@pytest.mark.parametrize("keep", [0, 1, 3])
@pytest.mark.parametrize("keep_h", [1, 0])
@pytest.mark.parametrize("name", GPU_FIXTURES)
def test_windows_equal_one_copy(pkg, capi, env, name, keep_h, keep):
    g, S, ref = yardstick(pkg, capi, name, keep_h)
    env(STMMQR_RECYCLE="2", STMMQR_KEEP_FRONTS=keep)
    _, plan = new_plan(pkg, g, keep_h)
    try:
        assert plan.fstats["retries"] == 0
        kept = kept_fronts(plan, S.nf)
        assert len(kept) == min(keep, S.nf)
        first = raw_download(capi, plan)                       # (the default window: one launch)
        assert_download_is(first, ref, f"{name} keepH={keep_h} keep={keep} default window")
        L = packed_layout(S, first["HStair"], first["Hm"], keep_h)
        assert L["rh_total"] == ref["rh_total"] and np.array_equal(L["block_off"][:S.nf], first["Rblock_off"][:S.nf])
        for f in range(S.nf):                                  # the model and the device agree on every column offset
            assert np.array_equal(plan.front_rhoff(f, L["fronts"][f]["fn"]), L["fronts"][f]["off"]), (name, f)
        windows = window_list(L, kept)
        per_dl = [max(1, -(-L["rh_total"] // w)) for w in windows]
        print(f"[download windows] {name} keepH={keep_h} keep={keep}: rh_total {L['rh_total']}, kept {kept}, {len(windows)} downloads of "
              f"{per_dl} windows")
        assert windows and max(per_dl) <= 4096
        for w in windows:
            env(STMMQR_DOWNLOAD_WIN=w)
            assert_download_is(raw_download(capi, plan), ref, f"{name} keepH={keep_h} keep={keep} kept={kept} window={w}")
            for who, d in classify_edges(L, kept, w).items():
                for c, v in d.items():
                    TALLY[keep_h][who][c] += v
    finally:
        plan.close()


# ---- c: the knob is what sizes the bounce buffer ----
def test_the_knob_is_in_force(pkg, capi, env):
    g, S, ref = yardstick(pkg, capi, "dwt_992", 1)
    total = ref["rh_total"]
    env(STMMQR_RECYCLE="2")
    _, plan = new_plan(pkg, g, 1)
    try:
        assert plan.front_kept(0) in (0, 1)
        held = plan.device_bytes()
        env(STMMQR_DOWNLOAD_WIN=257)
        assert_download_is(raw_download(capi, plan), ref, "window 257")
        assert plan.device_bytes() - held == 2 * min(257, total) * 8           # two windows in flight, counted as d_bounce
        held = plan.device_bytes()
        env(STMMQR_DOWNLOAD_WIN=61)
        assert_download_is(raw_download(capi, plan), ref, "window 61")
        assert plan.device_bytes() == held                                     # (the buffer is not shrunk)
        env(STMMQR_DOWNLOAD_WIN=total)
        assert_download_is(raw_download(capi, plan), ref, "window rh_total")
        assert plan.device_bytes() - held == 2 * (total - 257) * 8
    finally:
        plan.close()


# ---- d: more than one workgroup per front ----
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("keep_h", [1, 0])
def test_more_than_one_workgroup_per_front(pkg, capi, env, keep_h, keep):
    """reorientation_8 (one front of 3045 columns; 7.5 M doubles of factors with H, 4.6 M without): windows of 131072 and 262144
    doubles give 2 and 4 workgroups per front in the copy of a staged block and in the column loop of a kept front"""
    g, S, ref = yardstick(pkg, capi, "reorientation_8", keep_h)
    assert ref["rh_total"] >= 3 * 131072
    env(STMMQR_RECYCLE="2", STMMQR_KEEP_FRONTS=keep)
    _, plan = new_plan(pkg, g, keep_h)
    try:
        assert plan.fstats["retries"] == 0 and len(kept_fronts(plan, S.nf)) == keep
        for w in (131072, 262144):
            env(STMMQR_DOWNLOAD_WIN=w)
            assert_download_is(raw_download(capi, plan), ref, f"reorientation_8 keepH={keep_h} keep={keep} window={w}")
    finally:
        plan.close()


# ---- e: a second factorization of the plan, another window ----
def test_second_factorization_and_other_window(pkg, capi, env):
    g, S, ref = yardstick(pkg, capi, "lns_3937", 1)
    env(STMMQR_RECYCLE="2")
    _, plan = new_plan(pkg, g, 1)
    try:
        env(STMMQR_DOWNLOAD_WIN=257)
        assert_download_is(raw_download(capi, plan), ref, "first factorization, window 257")
        assert factorize(plan, g)["retries"] == 0
        env(STMMQR_DOWNLOAD_WIN=4099)
        assert_download_is(raw_download(capi, plan), ref, "second factorization, window 4099")
    finally:
        plan.close()


# ---- f: those who get their factors through the download ----
def seam_arrays(pkg, g, S):
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    args = (g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    N = pkg.qr_factorize(sym, *args)
    out = {k: getattr(N, k) for k in ("Rblock_off", "Rdead", "HStair", "HTau", "Hii", "HPinv", "Hm", "Hr")}
    out["Stack"] = N.Stack[:N.rh_total]
    out["scalars"] = np.array([N.rank, N.rank1, N.maxfrank, N.maxfm], I64)
    pkg.plan_cache_clear()
    M = pkg.qr_factorize_seam(sym, *args)                      # the exported qr_factorize with the reference's structs
    try:
        drop_in = M.arrays()
        # (the seam's Hii is allocated, not cleared: a front's fm row ids are what qr_hpinv wrote, the rest of its slot is not data)
        drop_in["Hii"] = np.concatenate([drop_in["Hii"][S.Hip[f]:S.Hip[f] + drop_in["Hm"][f]] for f in range(S.nf)])
        drop_in["scalars"] = np.array([M.rank, M.rank1, M.maxfrank, M.maxfm], I64)
    finally:
        M.close()
        pkg.plan_cache_clear()
    return out, drop_in


def assert_same_arrays(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x.view(U64) if x.dtype == np.float64 else x, y.view(U64) if y.dtype == np.float64 else y), (what, k)


@pytest.mark.parametrize("name", ["syn_rankdef_grid", "dwt_992"])
def test_consumers_of_the_download(pkg, name):
    g = load_golden(name)
    S = Symbolic(g)
    with knobs(STMMQR_RECYCLE="0"):
        ref = seam_arrays(pkg, g, S)
    with knobs(STMMQR_RECYCLE="2", STMMQR_KEEP_FRONTS="1", STMMQR_DOWNLOAD_WIN="257"):
        got = seam_arrays(pkg, g, S)
    assert ref[0]["Stack"].size > 257
    assert_same_arrays(got[0], ref[0], f"{name}: qr_factorize")
    assert_same_arrays(got[1], ref[1], f"{name}: the drop-in qr_factorize")
    if name != "dwt_992":
        return
    m, n = int(g["A_m"][0]), int(g["A_n"][0])
    exports = []
    for kw in (dict(), dict(STMMQR_RECYCLE="2", STMMQR_KEEP_FRONTS="1", STMMQR_DOWNLOAD_WIN="257")):
        with knobs(**kw):
            Q = pkg.SparseQR(m, n, g["A_p"], g["A_i"], g["A_x"], relax=pkg.relax_for_qr(n, int(g["A_p"][-1])))
            try:
                exports.append(Q.export_r())
            finally:
                Q.close()
    assert exports[0]["Rp"][-1] > 257
    assert_same_arrays({k: v for k, v in exports[1].items() if isinstance(v, np.ndarray)},
                       {k: v for k, v in exports[0].items() if isinstance(v, np.ndarray)}, "dwt_992: SparseQR.export_r")


# ---- g: the resident-factor operations on a forced kept set ----
@pytest.mark.parametrize("cache", ["0", "1"])
@pytest.mark.parametrize("keep", [0, 1, 3])
@pytest.mark.parametrize("name", ["syn_rankdef_grid", "dwt_992"])
def test_resident_operations_with_forced_kept_fronts(pkg, capi, env, name, keep, cache):
    g, S, ref = yardstick(pkg, capi, name, 1)
    env(STMMQR_RECYCLE="2", STMMQR_KEEP_FRONTS=keep, STMMQR_RESIDENT_CACHE=cache)
    _, plan = new_plan(pkg, g, 1)
    try:
        assert len(kept_fronts(plan, S.nf)) == min(keep, S.nf)
        b = rhs(S)
        for _ in range(2):                                     # (the second round reads the cached front forms, or rebuilds them)
            assert np.array_equal(plan.qmult(0, b).view(U64), ref["qtb"].view(U64))
            assert np.array_equal(plan.qmult(1, b).view(U64), ref["qb"].view(U64))
        if ref["x"] is not None:
            assert np.array_equal(plan.solve(b).view(U64), ref["x"].view(U64))
        assert_download_is(raw_download(capi, plan), ref, f"{name} keep={keep} cache={cache}: download after the operations")
    finally:
        plan.close()


# ---- b: every class of edge was met (keep this test LAST: it reads what test_windows_equal_one_copy counted) ----
def test_every_edge_class_was_hit():
    assert any(v for kh in TALLY.values() for who in kh.values() for v in who.values()), \
        "test_windows_equal_one_copy has not run in this session: run the whole module"
    missing = []
    for kh in (1, 0):
        for who in ("kept", "staged"):
            for c in CLASSES:
                if c in "CD" and not kh:
                    continue
                print(f"[edge classes] keepH={kh} {who} {c}: {TALLY[kh][who][c]}")
                # (excused only where tests/test_pack_window_cases_cpu.py records the class as unreachable on EVERY fixture)
                excused = all(c in UNREACHABLE.get((name, bool(kh), who), "") for name in GPU_FIXTURES)
                if TALLY[kh][who][c] == 0 and not excused:
                    missing.append(f"keepH={kh} {who} fronts: class {c}")
    assert not missing, "no window edge of: " + "; ".join(missing)
