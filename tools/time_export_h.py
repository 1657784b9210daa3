"""H, HTau and HPinv out of the resident factors, the host export next to the device one:
  (a) stmmqr_plan_export_r with H minus the same call without H, on the same plan: what H adds to one download of the packed stack
      and qr_rcount + qr_rconvert on one host thread (the host yardstick; both calls download the whole R+H stack)
  (b) stmmqr_plan_h_sparse, host arrays   counted, scanned and compacted on the device; hnz entries, nh columns and m rows cross the bus
  (c) stmmqr_plan_h_sparse, device arrays the count call and the fill call (which counts again) separately, nothing crosses the bus
  (d) (b) and (c) on a plan made with STMMQR_RECYCLE=2 STMMQR_RESIDENT_CACHE=0: the scratch holds one tree level, so the count walk and
      the fill walk each put every level back into front form
A warm plan; every call is complete on return (the plan's stream is synchronised) and is timed by the host wall clock: 1 call to warm
up, then calls until 0.3 s and at least 3 of them have passed -- median (min) in ms.  For (c) also bytes / time: the rows of the front
columns below the diagonals read once per walk (8 B per entry visited; a fill call walks twice) plus 16 B per entry written -- counted
from info (info[2], info[1]), not measured.
usage: python tools/time_export_h.py [--with-c5] [fixture ...]"""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stmmqr_testlib import Symbolic, load_golden, scalar  # noqa: E402

pkg = importlib.import_module("stm-multifrontal-qr-factorization-empowered-by-gcn_amd")
capi = pkg.capi
lib = capi.lib
I64 = np.int64


def timed(f, warm=1, least=3, window=0.3):
    for _ in range(warm):
        f()
    t = []
    t_end = time.perf_counter() + window
    while len(t) < least or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t))


def symbolic_struct(sym):
    """the qr_symbolic stmmqr_plan_export_r reads, from the fixture's arrays (kept alive in the returned dict)"""
    keep, S = {}, capi.QrSymbolicC()
    for k in ("m", "n", "anz", "nf", "maxfn", "rjsize", "do_rank_detection", "maxstack", "hisize", "keepH", "ntasks", "ns"):
        setattr(S, k, int(sym.get(k, 1 if k in ("keepH", "ntasks", "ns") else 0) or 0))
    for k in ("Sp", "Sj", "Qfill", "PLinv", "Sleft", "Parent", "Child", "Childp", "Super", "Rp", "Rj", "Post", "Hip", "Fm", "Cm"):
        a = sym.get(k)
        if a is not None and len(a):
            keep[k] = np.ascontiguousarray(a, I64)
            setattr(S, k, keep[k].ctypes.data_as(capi.c_long_p))
    return S, keep


def host_export(plan, S, m, with_h):
    Rp, Ri, Rx = capi.c_long_p(), capi.c_long_p(), capi.c_double_p()
    Hp, Hi, Hx, Ht, nh = capi.c_long_p(), capi.c_long_p(), capi.c_double_p(), capi.c_double_p(), C.c_long(0)
    h = (C.byref(nh), C.byref(Hp), C.byref(Hi), C.byref(Hx), C.byref(Ht)) if with_h else (None,) * 5
    rc = lib.stmmqr_plan_export_r(plan._h, C.byref(S), m, C.byref(Rp), C.byref(Ri), C.byref(Rx), *h)
    assert rc == 0, capi.last_error()
    for p in (Rp, Ri, Rx) + ((Hp, Hi, Hx, Ht) if with_h else ()):
        lib.stmmqr_free(C.cast(p, C.c_void_p))


def make_plan(g, S):
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}, "keepH": 1}
    plan = pkg.HipQR(sym)
    plan.set_pattern(g["in_Ap"], g["in_Ai"])
    for _ in range(2):
        plan.factorize(g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    return sym, plan


def count_info(plan):
    info = np.zeros(4, I64)
    assert lib.stmmqr_plan_h_sparse(plan._h, None, None, None, None, None, 0, 0, info.ctypes.data_as(capi.c_long_p), 0) == 0, capi.last_error()
    return info


def device_calls(plan, m, nh, hnz):
    """-> (count call, fill call, release) on device arrays"""
    info = np.zeros(4, I64)
    ip = info.ctypes.data_as(capi.c_long_p)
    dev = [pkg.device_alloc(8 * (nh + 1)), pkg.device_alloc(8 * max(hnz, 1)), pkg.device_alloc(8 * max(hnz, 1)), pkg.device_alloc(8 * max(nh, 1)),
           pkg.device_alloc(8 * max(m, 1))]

    def count():
        assert lib.stmmqr_plan_h_sparse(plan._h, None, None, None, None, dev[4], 0, 0, ip, 1) == 0, capi.last_error()

    def fill():
        assert lib.stmmqr_plan_h_sparse(plan._h, dev[0], dev[1], dev[2], dev[3], dev[4], nh, hnz, ip, 1) == 0, capi.last_error()

    def release():
        for d in dev:
            pkg.device_free(d)
    return count, fill, release


def host_call(plan, m, nh, hnz):
    Hp, Hi, Hx = np.zeros(nh + 1, I64), np.zeros(max(hnz, 1), I64), np.zeros(max(hnz, 1))
    HTau, HPinv, info = np.zeros(max(nh, 1)), np.zeros(max(m, 1), I64), np.zeros(4, I64)

    def run():
        assert lib.stmmqr_plan_h_sparse(plan._h, Hp.ctypes.data, Hi.ctypes.data, Hx.ctypes.data, HTau.ctypes.data, HPinv.ctypes.data, nh, hnz,
                                        info.ctypes.data_as(capi.c_long_p), 0) == 0, capi.last_error()
    return run


fmt = lambda mm: f"{mm[0]:.3f} ({mm[1]:.3f})"
args = [a for a in sys.argv[1:] if not a.startswith("--")]
names = args or (["bcsstk14", "reorientation_8", "xenon1_colamd_standin"] + (["c5_standin"] if "--with-c5" in sys.argv else []))
for name in names:
    g = load_golden(name)
    S = Symbolic(g)
    m, n = S.m, S.n
    for layout in ({}, {"STMMQR_RECYCLE": "2", "STMMQR_RESIDENT_CACHE": "0"}):
        os.environ.update(layout)
        sym, plan = make_plan(g, S)
        info = count_info(plan)
        nh, hnz, visited = int(info[0]), int(info[1]), int(info[2])
        tag = "cache=0" if layout else "default"
        out = [f"{name} [{tag}] m {m} n {n} nf {S.nf} nh {nh} hnz {hnz} visited {visited}"]
        if not layout and name != "c5_standin":                             # (no host arrays of that size)
            Sc, keep = symbolic_struct(sym)
            th, tr = timed(lambda: host_export(plan, Sc, m, True)), timed(lambda: host_export(plan, Sc, m, False))
            out.append(f"(a) export_r with H {fmt(th)} ms, without {fmt(tr)} ms: H adds {th[0] - tr[0]:.3f} ms")
        if name != "c5_standin":
            out.append(f"(b) h_sparse host {fmt(timed(host_call(plan, m, nh, hnz)))} ms")
        count, fill, release = device_calls(plan, m, nh, hnz)
        tc, tf = timed(count), timed(fill)
        release()
        gbs = lambda byts, ms: byts / (ms * 1e-3) / 1e9
        out.append(f"(c) device count {fmt(tc)} ms = {gbs(8 * visited, tc[0]):.1f} GB/s, fill {fmt(tf)} ms = "
                   f"{gbs(16 * visited + 16 * hnz, tf[0]):.1f} GB/s")
        plan.close()
        for k in layout:
            os.environ.pop(k, None)
        print(" | ".join(out), flush=True)
