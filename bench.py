#!/usr/bin/env python3
"""bench.py -- numerical-factorization GFLOP/s of the MI355X path (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload NAME] [--dump-outputs DIR] [--full [--no-cpu]]

A "step" is one numeric factorization (qr_factorize interval = the reference's "Factorize time",
STMMQR/src/qr/SparseQR.c:346-355) of one matrix whose symbolic analysis is a committed fixture and whose values
are already resident in HBM when the timed region starts; the factors stay in HBM (the D2H of the packed R+H is
reported separately in DESIGN.md, never in `value`).  Flops are the reference's own count
(SparseQR_factorize.c:1571), verified equal to the reference's on the same matrix.

N > 1: `--gpus N` starts N ranks itself (one process per GPU, torch.distributed, backend nccl = RCCL) unless a launcher
already did; default mode "sharded": ONE matrix, subtrees on the ranks, contribution blocks up a tree of joins with
point-to-point messages, value = the matrix's flops / max-over-ranks time (strong scaling; the flop share of the
critical path is printed).  `--mode replicas`: every rank its own matrix (weak scaling).

Prints ONE JSON line on rank 0: `metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` (wall time of one timed
step) and the workload's `config`.  A plain run does only that: set-up, W warm-up steps, K timed steps, the line.

--dump-outputs DIR: after the timed steps, the factors the last step left in HBM (what a caller of the timed path downloads)
are written as DIR/<name>.npy, float64, at most 64 MB in all (fixed stratified samples of larger arrays; see dump_outputs).

--full: everything else the benchmark measures, after the timed steps and outside `value`: the detail pass and the `roofline`
object, Q'b and the least-squares solve on the resident factors (`f1_resident_factors`), the drop-in seam and the own symbolic
phase, the large-front block of the default N = 1 workload, and the `cpu_baseline` object (the compiled reference, or the CPU
restatement where it is not built; `--no-cpu` leaves it out).
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
PKG = "stm-multifrontal-qr-factorization-empowered-by-gcn_amd"

PEAK_FP64_MFMA_TFLOPS = 78.6      # MI355X dense fp64 matrix peak (= fp64 vector peak on gfx950)
PEAK_HBM_GBS = 8000.0             # MI355X_MICROARCH.md: 8.0 TB/s spec (6.3 TB/s measured copy)


ORDERING_NAMES = {5: "AMD", 2: "COLAMD", 7: "default (COLAMD: qrtest without an ordering argument)", 11: "METIS", 6: "NESDIS"}
FETCH_CORRECTION = 1.0 / 0.545    # gfx950 FETCH_SIZE under-reports streaming reads by one half (MI355X_MICROARCH.md, HBM);
                                  # calibrated on this code's own 8-byte-per-lane streams: k_rh_copy / k_cpack read exactly
                                  # what they write, rocprofv3 reports FETCH = 0.54-0.55 x WRITE (profiles/r01_i_pmc_summary.txt)


def host_cores():
    """cores this process may really use: the affinity mask, cut by the cgroup CPU quota when there is one"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            t = open(path).read().split()
            if path.endswith("cpu.max"):
                if t[0] != "max":
                    n = min(n, max(1, int(int(t[0]) / int(t[1]))))
            else:
                q = int(t[0]); per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
        except Exception:
            pass
    return n


def host_shape():
    """(sockets, NUMA nodes, CPUs) as the reference's get_plat.sh reads them from lscpu (STMMQR/get_plat.sh:3-5): what its TPSM pool is
    compiled for (include/tpsm/Numainfo.h).  None when lscpu does not say."""
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=20).stdout
        v = {}
        for line in out.splitlines():
            if line.startswith("Socket(s):"):
                v["s"] = int(line.split()[1])
            elif line.startswith("NUMA node(s):"):
                v["n"] = int(line.split()[2])
            elif line.startswith("CPU(s):"):
                v["c"] = int(line.split()[1])
        return (v["s"], v["n"], v["c"])
    except Exception:
        return None


def _refdump_run(refdump, mtx, ordering, reps, threads, timeout, grain=1, pool=None):
    """one refdump process: `reps` SparseQR runs of the compiled reference, best qr_factorize time.
    grain = 1: serial qr_kernel(0) with `threads` MKL threads (the reference's BLAS-internal threading, STMMQR/README.md:94).
    grain > 1: the reference's own tree parallelism -- TPSM pool of `pool` threads, SPQR_grain = grain
    (SparseQR_multithreads.c:86-115), MKL sequential inside the tasks.  Returns a dict, or {"error": ...}."""
    mkl = threads if grain <= 1 else 1
    env = dict(os.environ, MKL_NUM_THREADS=str(mkl), OMP_NUM_THREADS=str(mkl),
               MKL_THREADING_LAYER="SEQUENTIAL" if mkl == 1 else "GNU", MKL_DYNAMIC="FALSE")
    if pool:
        env["REFDUMP_POOL"] = str(pool)
    what = f"{threads} core(s), {reps} run(s)" + (f", TPSM pool {pool}, SPQR_grain {grain}" if grain > 1 else "")
    print(f"[bench] cpu baseline: reference on {what} ...", file=sys.stderr, flush=True)
    try:
        pr = subprocess.run([str(refdump), str(mtx), ordering, str(grain), "d", "-", str(reps)], capture_output=True, text=True, env=env,
                            timeout=timeout)
    except subprocess.TimeoutExpired:
        print(f"[bench] cpu baseline: the leg on {what} exceeded {timeout:.0f} s and was dropped", file=sys.stderr, flush=True)
        return {"error": f"no result within {timeout:.0f} s (killed)"}
    res = {}
    for line in pr.stdout.splitlines():
        if line.startswith("REF factorize seconds"):
            res["seconds"] = float(line.split(":")[1].split()[0])
        elif line.startswith("nf ="):
            res["flops"] = float(line.split("flops =")[1].split()[0])
        elif line.startswith("REF qmult(QTX) seconds"):
            t = line.replace(":", " ").split()
            res["qmult_qtx_seconds"] = float(t[3]); res["solve_seconds"] = float(t[6])
    if "seconds" in res and "flops" in res:
        return res
    tail = (pr.stderr.strip().splitlines() or pr.stdout.strip().splitlines() or [""])
    return {"error": f"exit code {pr.returncode}: " + " | ".join(tail[:4])[:300]}


def _write_mtx(path, m, n, Ap, Ai, Ax):
    cols = np.repeat(np.arange(n), np.diff(Ap))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (m, n, len(Ax)))
        np.savetxt(f, np.c_[Ai + 1, cols + 1, Ax], fmt="%d %d %.17g")


def cpu_baseline(name, g, budget_s=30.0, mtx_path=None, flops=None):
    """The REAL reference (oracle/_ref/refdump, built by oracle/Makefile) timed on this host, three legs:
      1. 1 core (SPQR_grain = 1, MKL sequential: STMMQR/README.md:71-72),
      2. all cores through MKL threads (SPQR_grain = 1, MKL_NUM_THREADS = nproc),
      3. all cores through the reference's own TPSM tree parallelism (pool of 4 x nproc threads, SPQR_grain = 2 x nproc), under a
         time limit because the pool can deadlock; a leg that fails is reported with its error, never dropped
         silently.
    Repetitions are sized from THIS host's first run of each leg, not from the fixture: a leg whose first run took < 20 s is
    run twice more (best of 3), a longer one stands as best of 1.  `value` is the fastest leg.
    Falls back to the CPU restatement (kind "port") when the reference build is not present."""
    refdump = ROOT / "oracle" / "_ref" / "refdump"
    ref_s = float(g["fac_seconds"][0]) if "fac_seconds" in g else 0.0     # seconds in the build container: guard for the huge ones only
    nproc = host_cores()
    if ref_s > 150.0:
        # one run of the reference is minutes to most of an hour (c5mid / c5 stand-ins): not repeated inside a bench run;
        # the figure is the compiled reference's own time when the golden fixture was made (tests/golden/make_golden.py)
        fl = float(g["flopcount"][0])
        return {"value": fl / ref_s * 1e-9, "unit": "GFLOP/s", "cores": 1, "kind": "reference", "seconds": ref_s,
                "sample": f"{name}: NOT re-run here -- qr_factorize of the compiled reference took {ref_s:.0f} s on one core of "
                          f"the build container when the golden fixture was generated (fac_seconds of the fixture)"}
    if refdump.exists():
        try:
            with tempfile.TemporaryDirectory() as td:
                if mtx_path is not None:
                    mtx = Path(mtx_path)
                else:
                    mtx = Path(td) / "a.mtx"
                    if "A_p" in g:
                        _write_mtx(mtx, int(g["A_m"][0]), int(g["A_n"][0]), g["A_p"], g["A_i"], g["A_x"])
                    else:
                        _write_mtx(mtx, int(g["in_m"][0]), int(g["in_n"][0]), g["in_Ap"], g["in_Ai"], g["in_Ax"])
                ordering = str(int(g["ordering"][0])) if "ordering" in g else "-1"
                omap = {"5": "0", "2": "1", "11": "2", "6": "3"}      # QR_ORDERING_* -> refdump selector
                osel = omap.get(ordering, "-1")
                fl_known = float(flops if flops is not None else g["flopcount"][0])
                legs = []
                plan = [dict(threads=1, grain=1, pool=None, mode="serial qr_kernel, MKL sequential")]
                if nproc > 1:
                    plan.append(dict(threads=nproc, grain=1, pool=None, mode="serial qr_kernel, MKL threads = nproc"))
                    plan.append(dict(threads=nproc, grain=2 * nproc, pool=4 * nproc,
                                     mode="TPSM tree parallelism: pool 4 x nproc, SPQR_grain 2 x nproc, MKL sequential"))
                for leg in plan:
                    tpsm = leg["grain"] > 1
                    # (the pool deadlocks when more tasks wait than it has threads, SURVEY.md 3.3: a TPSM leg that needs more than six times
                    #  the serial leg's time on this host is not going to be the fastest leg -- it is cut there, not after five minutes)
                    t_serial = min([l["seconds"] for l in legs if "seconds" in l], default=max(ref_s, 1.0))
                    first_to = min(300.0, max(30.0, 6.0 * t_serial)) if tpsm else max(120.0, 12 * max(ref_s, 1.0))
                    rec = {"cores": leg["threads"], "mode": leg["mode"]}
                    exe = refdump
                    if tpsm:
                        # The pool is configured at compile time for ONE host shape (Numainfo.h); oracle/Makefile builds it for the shapes
                        # in TPSM_VARIANTS.  A pool built for another shape dies in TPSM_init (round 4: signal 11), so it is not started.
                        shape = host_shape()
                        exe = refdump.parent / ("refdump_tpsm_%d_%d_%d" % shape) if shape else None
                        if exe is None or not exe.exists():
                            have = sorted(q.name.replace("refdump_tpsm_", "") for q in refdump.parent.glob("refdump_tpsm_*"))
                            rec["skipped"] = (f"no TPSM build for this host shape (sockets_nodes_cpus = {shape}); built: {have} "
                                              f"(oracle/Makefile, TPSM_VARIANTS)")
                            legs.append(rec)
                            continue
                        # (the pool size must be a multiple of the NUMA nodes and at most the CPUs: tpsm_main.c:389-393, tpsm_main.h:35)
                        pool = min(max(4 * nproc, shape[1]), shape[2])
                        leg = dict(leg, pool=pool - pool % shape[1])
                        rec["mode"] = (f"TPSM tree parallelism ({exe.name}): pool {leg['pool']}, SPQR_grain {leg['grain']}, MKL sequential")
                    r = _refdump_run(exe, mtx, osel, 1, leg["threads"], first_to, leg["grain"], leg["pool"])
                    if "error" in r:
                        rec["error"] = r["error"]
                        legs.append(rec)
                        continue
                    best, reps = r, 1
                    if r["seconds"] < 20.0:
                        r2 = _refdump_run(exe, mtx, osel, 2, leg["threads"], max(120.0, 8 * r["seconds"] + 60.0), leg["grain"], leg["pool"])
                        if "error" not in r2:
                            reps = 3
                            if r2["seconds"] < best["seconds"]:
                                best = r2
                    fl = best["flops"] if best["flops"] > 0 else fl_known    # (the reference counts flops in serial mode only)
                    rec.update({"value": fl / best["seconds"] * 1e-9, "unit": "GFLOP/s", "seconds": best["seconds"], "best_of": reps,
                                "flops": fl,
                                **({k: best[k] for k in ("qmult_qtx_seconds", "solve_seconds") if k in best})})
                    legs.append(rec)
                good = [l for l in legs if "value" in l]
                if good:
                    best = max(good, key=lambda l: l["value"])
                    return {"value": best["value"], "unit": "GFLOP/s", "cores": best["cores"], "kind": "reference",
                            "sample": f"{name}: qr_factorize of the compiled reference on this host ({nproc} cores); "
                                      f"legs: " + "; ".join(
                                          (f"{l['cores']} core(s) [{l['mode']}] {l['seconds'] * 1e3:.1f} ms best of {l['best_of']}" if "value" in l
                                           else f"{l['cores']} core(s) [{l['mode']}] SKIPPED: {l['skipped']}" if "skipped" in l
                                           else f"{l['cores']} core(s) [{l['mode']}] FAILED: {l['error']}") for l in legs),
                            "seconds": best["seconds"], "legs": legs, "host_cores": nproc}
        except Exception as e:  # fall through to the port
            print(f"[bench] reference baseline failed: {e}", file=sys.stderr)
    from stmmqr_testlib import Oracle, Symbolic, scalar
    orc = Oracle()
    S = Symbolic(g)
    t0 = time.perf_counter()
    N = orc.factorize(S, g["in_Ap"], g["in_Ai"], g["in_Ax"], scalar(g, "in_tol"), int(scalar(g, "in_ntol")))
    sec = time.perf_counter() - t0
    return {"value": N.c.flopcount / sec * 1e-9, "unit": "GFLOP/s", "cores": 1, "kind": "port",
            "sample": f"{name}: one run of oracle/stmmqr_oracle.c (scalar C restatement), {sec * 1e3:.1f} ms",
            "seconds": sec}


# ---------------------------------------------------------------------------------------------------------------
# kernel micro-benchmarks of SURVEY.md 8(d): synthetic single fronts through the qr_front seam, one synthetic
# assembly through the qr_assemble seam; device time = HIP events around the seam's kernels (stmmqr_last_seam_ms)
# ---------------------------------------------------------------------------------------------------------------
MICRO_FRONTS = [(64, 96, 32), (266, 422, 124), (380, 380, 380), (2048, 3072, 1024), (8192, 12288, 4096)]


def micro_front_input(idx, fm, fn, dense=False):
    """entries N(0,1), seed 1234 + idx, staircase Stair[k] = min(fm, (k+1) fm / fn + 8), zeros below it (SURVEY.md 8d:
    with fm < fn the diagonal overtakes this staircase after a few dozen columns, so these fronts are almost triangular
    and measure per-panel latency); dense = True: Stair[k] = fm, the full Householder QR of the same entries"""
    rng = np.random.default_rng(1234 + idx)
    F = np.asfortranarray(rng.standard_normal((fm, fn)))
    if dense:
        return F, np.full(fn, fm, np.int64)
    stair = np.minimum(fm, (np.arange(fn, dtype=np.int64) + 1) * fm // fn + 8).astype(np.int64)
    for k in range(fn):
        F[stair[k]:, k] = 0.0
    return F, stair


def micro_assembly_input(seed=99, P=8, FN=6144, FP=1024, CN=3000, NS=96):
    """Parent front with FN columns (FP pivotal), NS rows of S and two children with cm = cn = CN whose columns map to
    random monotone subsets of the parent's columns (SURVEY.md 8d names the parent 4096 x 6144; with two children of
    3000 rows each the parent has NS + 2 CN rows, so fm = 6096 here)."""
    rng = np.random.default_rng(seed)
    n = 2 * P + FN
    Super = np.array([0, P, 2 * P, 2 * P + FP], np.int64)
    Rp = np.array([0, P + CN, 2 * (P + CN), 2 * (P + CN) + FN], np.int64)
    Rj = np.zeros(Rp[-1], np.int64)
    for c in range(2):
        Rj[Rp[c]:Rp[c] + P] = np.arange(c * P, (c + 1) * P)
        Rj[Rp[c] + P:Rp[c + 1]] = 2 * P + np.sort(rng.choice(FN, CN, replace=False))
    Rj[Rp[2]:] = 2 * P + np.arange(FN)
    Fmap = np.zeros(n, np.int64)
    Fmap[2 * P:] = np.arange(FN)
    left = 2 * P + (np.arange(NS) * FP) // NS                      # leftmost column of S row r (a parent pivot)
    Sp, Sj = [0], []
    for r in range(NS):
        rest = 2 * P + np.sort(rng.choice(np.arange(left[r] - 2 * P + 1, FN), 7, replace=False))
        Sj.extend([left[r]] + list(rest))
        Sp.append(len(Sj))
    Sp, Sj = np.array(Sp, np.int64), np.array(Sj, np.int64)
    Sx = rng.standard_normal(len(Sj))
    Sleft = np.searchsorted(left, np.arange(n + 2), side="left").astype(np.int64)
    Child, Childp = np.array([0, 1], np.int64), np.array([0, 0, 0, 2], np.int64)
    Cm, Hr, Hip = np.array([CN, CN, 0], np.int64), np.zeros(3, np.int64), np.array([0, CN, 2 * CN], np.int64)
    fm = NS + 2 * CN
    Hii = np.zeros(2 * CN + fm, np.int64)
    Hii[:2 * CN] = 1000 + np.arange(2 * CN)
    csize = CN * (CN + 1) // 2
    Cb = {0: rng.standard_normal(csize), 1: rng.standard_normal(csize)}
    nbytes = 8 * (fm * FN + 2 * csize + len(Sj)) + 4 * (len(Sj) + 2 * (CN + CN))
    return dict(f=2, fm=fm, Super=Super, Rp=Rp, Rj=Rj, Sp=Sp, Sj=Sj, Sleft=Sleft, Child=Child, Childp=Childp, Sx=Sx,
                Fmap=Fmap, Cm=Cm, Cblocks=Cb, Hr=Hr, Stair=np.zeros(FN, np.int64), Hii=Hii, Hip=Hip), nbytes, (fm, FN)


def run_micro(pkg, args):
    fronts = []
    orc = None
    if args.full and not args.no_cpu:
        from stmmqr_testlib import Oracle                # CPU baseline leg only
        orc = Oracle()
    for idx, (fm, fn, fp, dense) in enumerate([(a, b, c, d) for d in (False, True) for (a, b, c) in MICRO_FRONTS]):
        idx %= len(MICRO_FRONTS)
        F0, st0 = micro_front_input(idx, fm, fn, dense)
        best, flops, rank = None, 0.0, 0
        for _ in range(max(1, args.warmup) + max(1, min(args.steps, 3))):
            F, st = F0.copy(order="F"), st0.copy()
            rank, _, _, flops = pkg.qr_front(fm, fn, fp, -1.0, fp, F, st)
            ms = pkg.last_seam_ms()
            best = ms if best is None else min(best, ms)
        row = {"fm": fm, "fn": fn, "fp": fp, "staircase": "dense" if dense else "survey", "rank": rank, "flops": flops,
               "device_ms": best,
               "gflops": flops / best * 1e-6, "frac_fp64_peak": flops / best * 1e-9 / PEAK_FP64_MFMA_TFLOPS}
        if orc is not None and flops <= 5e9:                 # (bounded CPU sample: the scalar port does ~1 GFLOP/s)
            F, st = F0.copy(order="F"), st0.copy()
            t0 = time.perf_counter()
            r2, _, _, fl2 = orc.front(F, st, fp, -1.0, fp)
            sec = time.perf_counter() - t0
            row["cpu_port_ms"] = sec * 1e3
            row["cpu_port_gflops"] = fl2 / sec * 1e-9
            row["rank_matches_cpu"] = bool(r2 == rank and fl2 == flops)
        fronts.append(row)
        del F0
    a, nbytes, shape = micro_assembly_input()
    best = None
    for _ in range(3):
        a["Stair"][:] = 0
        F, _ = pkg.qr_assemble(**a)
        ms = pkg.last_seam_ms()
        best = ms if best is None else min(best, ms)
    total_in = a["Sx"].sum() + a["Cblocks"][0].sum() + a["Cblocks"][1].sum()
    asm = {"parent": f"{shape[0]}x{shape[1]}, 2 children cm=cn=3000, 96 S rows", "algorithmic_bytes": nbytes,
           "device_ms": best, "GBps": nbytes / best * 1e-6, "frac_hbm": nbytes / best * 1e-6 / PEAK_HBM_GBS,
           "entries_conserved": bool(abs(F.sum() - total_in) <= 1e-9 * (abs(total_in) + 1.0))}
    big = [r for r in fronts if r["staircase"] == "dense" and r["fm"] == 2048][0]
    print(json.dumps({
        "metric": "numerical-factorization GFLOP/s", "value": big["gflops"], "unit": "GFLOP/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": big["device_ms"], "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "micro: single synthetic fronts (SURVEY.md 8d), value = the dense 2048x3072 front "
                               "through the qr_front seam (device time of its kernels); not the headline workload"},
        "fronts": fronts, "assembly": asm}))
    return 0


DEFAULT_WORKLOAD = {1: "xenon1_colamd_standin", 2: "xenon1_standin", 4: "sme3dc_standin", 8: "c5_standin"}
# the BASELINE matrices that are absent from the reference checkout (.MISSING_LARGE_BLOBS) are read from
# $STMMQR_DATA_DIR when somebody put them there; otherwise the labelled stand-in fixture runs
REAL_FILE_OF = {"xenon1_colamd_standin": "xenon1.mtx", "sme3dc_standin": "sme3Dc.mtx", "c5_standin": "3D_51448_3D.mtx"}
DRIVER_ORDERINGS = {"default": 7, "colamd": 2}        # qrtest.c:155-169; AMD / METIS / NESDIS are third-party packages of the reference


def matrix_workload(pkg, path, ordering_name):
    """--matrix F.mtx: the driver's flow on a file (qrtest.c:112-169) with this library alone -- reader, the driver's default
    tolerance 20 (m + n) eps max-column-norm (qrtest.c:135-142), singletons + COLAMD + symbolic analysis on the host -- and a
    fixture-shaped dict for the numeric factorization that is then timed: the matrix handed to qr_factorize (Y when singletons
    were removed, SparseQR.c:349,371), tol, ntol = its column count, the qr_symbolic."""
    if ordering_name not in DRIVER_ORDERINGS:
        raise SystemExit(f"--ordering {ordering_name}: only {sorted(DRIVER_ORDERINGS)} are computed by this library (AMD / METIS / NESDIS are "
                         "third-party packages of the reference; run stmmqr_qrtest --reflib for those)")
    t0 = time.perf_counter()
    m, n, Ap, Ai, Ax = pkg.read_matrix_market(path)
    t_read = time.perf_counter() - t0
    cn = np.sqrt(np.add.reduceat(Ax * Ax, Ap[:-1][np.diff(Ap) > 0])) if len(Ax) else np.zeros(1)
    mx = float(cn.max(initial=0.0)) or 1.0
    tol = 20.0 * (m + n) * np.finfo(np.float64).eps * mx
    t0 = time.perf_counter()
    sq = pkg.SparseQR(m, n, Ap, Ai, Ax, ordering=DRIVER_ORDERINGS[ordering_name], tol=tol, relax=pkg.relax_for_qr(n, len(Ax)),
                      symbolic_only=True)
    t_sym = time.perf_counter() - t0
    sym = sq.symbolic()
    info = sq.info
    Y = sq.Y()
    inA = Y if Y is not None else (Ap, Ai, Ax)
    g = {"sym_" + k: (np.asarray([v]) if np.isscalar(v) else v) for k, v in sym.items() if k != "info"}
    g.update({"in_Ap": np.ascontiguousarray(inA[0]), "in_Ai": np.ascontiguousarray(inA[1]), "in_Ax": np.ascontiguousarray(inA[2]),
              "in_m": np.asarray([sym["m"]]), "in_n": np.asarray([sym["n"]]), "in_tol": np.asarray([tol]),
              "in_ntol": np.asarray([sym["n"]]), "ordering": np.asarray([DRIVER_ORDERINGS[ordering_name]]),
              "A_m": np.asarray([m]), "A_n": np.asarray([n]), "A_p": Ap, "A_i": Ai, "A_x": Ax})
    meta = {"file": str(path), "read_ms": t_read * 1e3, "own_symbolic_ms": t_sym * 1e3, "n1rows": int(info["n1rows"]),
            "n1cols": int(info["n1cols"]), "flop_bound": float(info["flop_bound"])}
    sq.close()
    return g, meta


def spawn_ranks(args):
    """--gpus N without a launcher: start the N ranks ourselves (torch.distributed.run, one process per GPU) BEFORE
    anything in this process touches the GPU, relay their output, exit with their code."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.call(cmd, env=env)


def _failure_line(args, world, why):
    """the contract's ONE JSON line also when the run did not finish: value null, the reason in `error` (never a hang, never silence)"""
    return json.dumps({"metric": "numerical-factorization GFLOP/s", "value": None, "unit": "GFLOP/s", "n_gpus": world,
                       "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True,
                       "scaling": "strong" if (world > 1 and (args.mode or "sharded") == "sharded") else "weak", "vs_baseline": None,
                       "dtype": "f64", "data": "synthetic", "config": {"workload": args.workload or args.matrix}, "error": why})


def _install_guards(args, rank, world):
    """N > 1: (i) a rank that is terminated by the launcher because ANOTHER rank failed (torch.distributed.run sends SIGTERM to the
    survivors) still prints the line on rank 0; (ii) a watchdog ends a run that makes no progress (a lost message, a rank that
    never arrived) after STMMQR_BENCH_DEADLINE seconds (default 1500) with the line and a non-zero exit instead of hanging the
    node.  The multi-GPU path has never run on hardware (one-GPU build box): its first contact must fail loudly, not hang."""
    import signal
    import threading
    state = {"done": False}

    def bail(why, code):
        if state["done"]:
            return
        state["done"] = True
        if rank == 0:
            print(_failure_line(args, world, why), flush=True)
        os._exit(code)

    if world > 1:
        signal.signal(signal.SIGTERM, lambda sig, frm: bail("terminated by the launcher (another rank failed)", 143))
        deadline = float(os.environ.get("STMMQR_BENCH_DEADLINE", "1500"))
        t = threading.Timer(deadline, lambda: bail(f"no result after {deadline:.0f} s (deadline of bench.py: a rank or a message is missing)", 124))
        t.daemon = True
        t.start()
    return state


DUMP_LIMIT_BYTES = 64 << 20       # --dump-outputs: all files together
DUMP_ARRAY_CAP = 1 << 19          # entries kept of any array but the packed R+H (4 MB each)
DUMP_STACK_CAP = 1 << 22          # entries kept of the packed R+H (32 MB)


def _stratified(a, k, seed):
    """k entries of `a`, one from each of k equal strata at an offset drawn from a fixed seed: the same positions for the same
    length in every run, spread over the whole array.  The whole array when it has at most k entries."""
    if a.size <= k:
        return a
    edges = (np.arange(k + 1, dtype=np.int64) * a.size) // k
    off = (np.random.default_rng(seed).random(k) * np.diff(edges)).astype(np.int64)
    return a[edges[:-1] + off]


def dump_outputs(ddir, plan, S):
    """--dump-outputs: the factors the last timed step left in HBM, as a caller downloads them (the reference's qr_numeric:
    packed R+H, HTau, the integer arrays, rank), written as DIR/<name>.npy in float64 (integers are exact there).  Arrays longer
    than DUMP_ARRAY_CAP are fixed stratified samples; the packed R+H (1.2 GB on the default workload) is a sample of what room
    is left under DUMP_LIMIT_BYTES, plus the sum of squares of every front's block of it (free of the row signs of R)."""
    N = plan.download()
    nf, rh = S.nf, int(N.rh_total)
    stack = N.Stack[:rh]
    order = np.asarray(S.Post[:nf], np.int64)                     # the blocks lie in the stack in postorder
    starts = N.Rblock_off[order]
    ends = np.append(starts[1:], rh)
    front_sumsq = np.zeros(nf)
    for f, a, b in zip(order, starts, ends):
        front_sumsq[f] = np.dot(stack[a:b], stack[a:b])
    arrays = {"info": np.array([N.rank, N.rank1, N.maxfrank, N.maxfm, rh]),
              "HTau": N.HTau[:S.rjsize], "HStair": N.HStair[:S.rjsize], "Rdead": N.Rdead[:S.n], "HPinv": N.HPinv[:S.m],
              "Hii": N.Hii[:S.hisize], "Hm": N.Hm[:nf], "Hr": N.Hr[:nf], "Rblock_off": N.Rblock_off[:nf],
              "R_H_front_sumsq": front_sumsq}
    out = {k: _stratified(np.asarray(v, np.float64), DUMP_ARRAY_CAP, seed) for seed, (k, v) in enumerate(arrays.items())}
    used = sum(a.nbytes + 4096 for a in out.values()) + 4096      # (4 KB per file: the .npy header, generously)
    out["R_H_stack_sample"] = _stratified(np.asarray(stack, np.float64), min(DUMP_STACK_CAP, (DUMP_LIMIT_BYTES - used) // 8), 99)
    d = Path(ddir)
    d.mkdir(parents=True, exist_ok=True)
    for k, a in out.items():
        np.save(d / f"{k}.npy", np.ascontiguousarray(a))
    print(f"[bench] --dump-outputs: {len(out)} arrays, {sum(a.nbytes for a in out.values()) / 2**20:.1f} MB -> {d}",
          file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default=None,
                    help="fixture name or 'micro'; default by --gpus: 1 the xenon1 stand-in in the driver's default (COLAMD) "
                         "ordering, 2 the METIS-ordered xenon1 stand-in, 4 the sme3Dc stand-in, 8 the configs[4] stand-in at full size "
                         "(n = 52 022; c5mid_standin / c5mini_standin are the same structure at n = 27 000 / 8000)")
    ap.add_argument("--matrix", default=None,
                    help="a Matrix Market file instead of a fixture: reader -> singletons + COLAMD + symbolic analysis of this library -> "
                         "timed numeric factorization; CPU leg = the compiled reference on the same file")
    ap.add_argument("--ordering", default="default", help="with --matrix: default | colamd (qrtest's third argument absent / 1)")
    ap.add_argument("--full", action="store_true",
                    help="also the detail pass (roofline), the f1 block, the drop-in seam, the large-front block and the CPU baseline")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the factors of the last timed step as DIR/<name>.npy (float64, at most 64 MB in all)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--big-front-cols", type=int, default=None)
    ap.add_argument("--panel-algo", type=int, default=None)
    ap.add_argument("--lookahead", type=int, default=None)
    ap.add_argument("--no-large-front", dest="large_front", action="store_false",
                    help="with --full: skip the un-headlined large-front block (c5mid / c5 stand-ins, ~15 s) of the default N = 1 line")
    ap.add_argument("--tall-min", type=int, default=None)
    ap.add_argument("--fused-update", type=int, default=None)
    ap.add_argument("--use-graph", type=int, default=None)
    ap.add_argument("--pair-update", type=int, default=None)
    ap.add_argument("--mode", choices=["replicas", "sharded"], default=None,
                    help="N>1: sharded (default) = ONE matrix, subtrees on the ranks, contribution blocks up a tree of joins "
                         "over RCCL point-to-point (strong scaling); replicas = every rank factorizes its own matrix (weak)")
    ap.add_argument("--spread", type=int, default=1,
                    help="sharded mode: 1 (default) = the heavy top fronts are SHARED by the ranks of their group (panels in turn, "
                         "every rank updates its own 32-column blocks: sharded.spread_partition); 0 = subtrees only")
    args = ap.parse_args()
    if args.dump_outputs and (args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.workload == "micro"):
        ap.error("--dump-outputs: one process (--gpus 1) on a matrix workload only")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    guard = _install_guards(args, rank, world)
    try:
        return _run(args, torch, rank, world, local, guard)
    except BaseException as e:                       # (SystemExit of argparse etc. included: the line comes first)
        if world > 1 and not guard["done"] and not isinstance(e, SystemExit):
            guard["done"] = True
            import traceback
            traceback.print_exc()
            if rank == 0:
                print(_failure_line(args, world, f"rank 0: {type(e).__name__}: {e}"), flush=True)
            os._exit(1)                              # (no destructors of a half-initialised process group: they can hang)
        raise


def _run(args, torch, rank, world, local, guard):
    # STMMQR_BENCH_REHEARSAL=1 (a one-GPU box): every rank on device 0, gloo, contribution blocks through the host -- the
    # whole multi-process protocol (spawn, rendezvous, partition, phases, exchange, timing) without RCCL / a second GPU
    rehearsal = world > 1 and os.environ.get("STMMQR_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local = 0
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        to = datetime.timedelta(seconds=float(os.environ.get("STMMQR_BENCH_PG_TIMEOUT", "600")))
        if rehearsal:
            dist.init_process_group(backend="gloo", timeout=to)
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local), timeout=to)
    if world > 1 and os.environ.get("STMMQR_BENCH_FAIL_RANK") == str(rank):        # (tests: one rank dies after the rendezvous)
        raise RuntimeError("injected failure of this rank (STMMQR_BENCH_FAIL_RANK)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if args.mode is None:
        args.mode = "sharded" if world > 1 else "replicas"
    if args.workload is None:
        args.workload = DEFAULT_WORKLOAD.get(world, "xenon1_standin")

    from stmmqr_testlib import Symbolic, load_golden, scalar
    pkg = importlib.import_module(PKG)
    if args.big_front_cols:
        pkg.set_options(big_front_cols=args.big_front_cols)
    if args.panel_algo is not None:
        pkg.set_options(panel_algo=args.panel_algo)
    if args.lookahead is not None:
        pkg.set_options(lookahead=args.lookahead)
    if args.pair_update is not None:
        pkg.set_options(pair_update=args.pair_update)
    if args.fused_update is not None:
        pkg.set_options(fused_update=args.fused_update)
    if args.use_graph is not None:
        pkg.set_options(use_graph=args.use_graph)
    if args.tall_min is not None:
        pkg.set_options(tall_min_rows=args.tall_min)
    name = args.workload
    if name == "micro":
        return run_micro(pkg, args)
    mtx_path, mtx_meta = args.matrix, None
    ddir = os.environ.get("STMMQR_DATA_DIR")
    if mtx_path is None and ddir and name in REAL_FILE_OF and (Path(ddir) / REAL_FILE_OF[name]).exists():
        mtx_path = str(Path(ddir) / REAL_FILE_OF[name])       # the real BASELINE matrix instead of its stand-in
    if mtx_path is not None:
        if not Path(mtx_path).exists() and ddir and (Path(ddir) / mtx_path).exists():
            mtx_path = str(Path(ddir) / mtx_path)
        g, mtx_meta = matrix_workload(pkg, mtx_path, args.ordering)
        name = Path(mtx_path).stem
    else:
        g = load_golden(name)
    S = Symbolic(g)
    sym = {**S.sc, **{k: v for k, v in S.arr.items() if v is not None}}
    tol, ntol = scalar(g, "in_tol"), int(scalar(g, "in_ntol"))

    plan = pkg.HipQR(sym, device=local)
    plan.set_pattern(g["in_Ap"], g["in_Ai"])
    Ax = torch.from_numpy(np.ascontiguousarray(g["in_Ax"])).to(dev)      # values resident in HBM
    torch.cuda.synchronize()

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    st = None
    sharded = args.mode == "sharded" and world > 1
    crit = None
    if sharded:
        sh = importlib.import_module(PKG + ".sharded")
        # the panel loop of shared fronts: native (C++ loop, RCCL point-to-point on a comm stream) unless STMMQR_NATIVE_LOOP=0 or RCCL
        # cannot be set up -- then the step-by-step loop over torch.distributed, which moves the same bytes
        native, native_note = None, "python loop over torch.distributed"
        if not rehearsal and os.environ.get("STMMQR_NATIVE_LOOP", "1") != "0":
            try:
                native = pkg.RcclTransport(dist, dev)
                native_note = ("native phase loop (stmmqr_factorize_phases: subtree exchange as device-packed messages, shared-front panel loop, "
                               "gather), RCCL ncclSend / ncclRecv")
            except Exception as e:                      # noqa: BLE001 (every rank takes the same branch: the id broadcast is collective)
                print(f"[bench] rank {rank}: RCCL transport not available ({e}); python loop", file=sys.stderr, flush=True)
        ok = torch.tensor([1 if native is not None else 0], dtype=torch.int64, device=dev if not rehearsal else "cpu")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            native, native_note = None, "python loop over torch.distributed"
        comm = sh.Comm(dist, None if rehearsal else dev, native=native)
        owner0, phase0 = sh.partition(sym, world)
        crit_sub = sh.critical_path_flops(sym, owner0, phase0, world)
        if args.spread:
            # (a shared front never takes the pair update, so its bits are those of ONE device with --pair-update 0)
            owner, phase, span = sh.spread_partition(sym, world)
        else:
            owner, phase, span = owner0, phase0, None
        crit = sh.critical_path_flops(sym, owner, phase, world, span)
        o_all, p_all, s_all = sh.spread_partition(sym, world, min_step_flops=0)   # (the flop model without the latency threshold)
        crit_all = sh.critical_path_flops(sym, o_all, p_all, world, s_all)
        shard_plan = sh.ShardPlan(plan, sym, owner, phase, comm, span)   # groups + edge lists once, outside the timed region

        def step():
            return sh.factorize_sharded(plan, sym, None, tol, ntol, comm, device_ptr=Ax.data_ptr(), shard_plan=shard_plan)[0]
    else:
        def step():
            return plan.factorize(None, tol, ntol, device_ptr=Ax.data_ptr())
    for _ in range(args.warmup):
        st = step()
    barrier()
    t0 = time.perf_counter()
    dev_ms, retries = 0.0, 0
    for _ in range(args.steps):
        st = step()
        dev_ms += st["ms_total"]
        retries += int(st.get("retries", 0))
    barrier()
    wall = time.perf_counter() - t0
    st_rank = None
    if world == 1:
        st_rank = plan.result_sizes()[1]
    if world > 1:
        t = torch.tensor([wall, st["flops"]], device=dev, dtype=torch.float64)
        tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone(); dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        wall = float(tmax[0].item())
        total_flops = float(tsum[1].item())          # replicas: world x flops; sharded: the shards add up to one matrix
    else:
        total_flops = st["flops"]
    # (a fixture carries the reference's own count; for a file the device's count stands and the CPU leg's must equal it)
    flops = scalar(g, "flopcount") if "flopcount" in g else (total_flops if (sharded or world == 1) else total_flops / world)
    assert int(round(total_flops)) == int(round(flops if (sharded or world == 1) else world * flops)), (total_flops, flops)
    # a step that silently ran twice (a bounded panel wait ran out and the factorization was repeated with one-workgroup
    # panels) is not a measurement
    assert retries == 0, f"{retries} factorization(s) of the timed region were repeated after a panel-wait timeout"
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, plan, S)

    # One extra, un-timed factorization with an event pair around every launch of a category (panel / update / assembly /
    # pack), recorded on the plan's stream with NO synchronisation in between: the schedule runs exactly as in the timed
    # region, and the pairs give each kernel family's own time (kernel-only: what rocprofv3 --kernel-trace --stats sums).
    det, step_rows = None, []
    if rank == 0 and args.full:        # (the detail pass feeds rank 0's roofline object only)
        if sharded:
            plan.set_groups(np.zeros(S.nf, np.int32))
        # (STMMQR_DUMPSTEPS: the library writes one line per timeline step of a detail pass -- the tallest panel of the step and the
        #  time of its panel / update launches -- which is what the latency roofline of the panel kernels below is made of)
        with tempfile.TemporaryDirectory() as td:
            dump = os.path.join(td, "steps.txt")
            os.environ["STMMQR_DUMPSTEPS"] = dump
            try:
                det = plan.factorize(None, tol, ntol, device_ptr=Ax.data_ptr(), detail=True)
            finally:
                os.environ.pop("STMMQR_DUMPSTEPS", None)
            try:
                for line in open(dump):
                    t = line.split()
                    kv = dict(zip(t[1::2], t[2::2]))
                    step_rows.append((int(kv["n_act"]), int(kv["maxrows"]), int(kv["nca_use"]), float(kv["panel_us"]), float(kv["upd_us"])))
            except Exception:
                step_rows = []
    if rank == 0:
        value = total_flops * args.steps / wall * 1e-9
    roof = None
    if rank == 0 and args.full:
        # Algorithmic work: the reference's flop count (FLOP_COUNT, :1571) splits into the dlarfb flops handed to the
        # trailing update (4 * rows * cols * reflectors per panel: stats.flops_update) and the rest, which the panel kernels
        # do (dlarfg + in-panel dlarf + T).  Update bytes: 2 reads + 1 write of every trailing entry per panel = 24 B per
        # (row, col); flops_update counts 4 flops per (live column, row below its diagonal, trailing col), i.e. <= 4*32 per
        # (row, col): a lower bound on the bytes.
        ms_panel, ms_upd = max(det["ms_panel"] + det["ms_small"], 1e-9), max(det["ms_update"], 1e-9)
        panel_flops = max(flops - det["flops_update"], 0.0)
        panel_tf = panel_flops / ms_panel * 1e-9
        upd_tf = det["flops_update"] / ms_upd * 1e-9
        # (fronts with the pair / quad update sweep the trailing columns once per TWO / FOUR panels: 12 / 6 B per (row, col) and panel
        #  there -- the bytes of THIS implementation, not the 24 of a panel-by-panel update)
        sweep_bytes = 6.0 if pkg.get_options()["pair_update"] == 4 else 12.0
        upd_bytes = ((det["flops_update"] - det["flops_update_pair"]) * 24.0 + det["flops_update_pair"] * sweep_bytes) / (4.0 * 32.0)
        upd_gbs = upd_bytes / ms_upd * 1e-6
        pmc, pmc_file = {}, None
        for cand in sorted((ROOT / "profiles").glob(f"r*_{name}_pmc_fetch_write_per_kernel.json")) or \
                sorted((ROOT / "profiles").glob("r*_pmc_fetch_write_per_kernel.json")):
            try:
                pmc, pmc_file = json.loads(cand.read_text()), cand
            except Exception:
                pass
        pmc_ok = bool(pmc) and pmc_file is not None and (name in pmc_file.name or (name == "xenon1_standin" and "standin" not in pmc_file.name.replace("_pmc", "")))

        def pmc_traffic(kernels):
            """HBM bytes per launch from the committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (KB units; separate
            passes; FETCH_SIZE corrected for the gfx950 half-counting, see FETCH_CORRECTION)"""
            tot, calls = 0.0, 0
            for k in kernels:
                e = pmc.get(k, {})
                if "FETCH_SIZE" in e and "WRITE_SIZE" in e:
                    tot += (e["FETCH_SIZE"]["sum_kb"] * FETCH_CORRECTION + e["WRITE_SIZE"]["sum_kb"]) * 1024.0
                    calls += e["FETCH_SIZE"]["calls"]
            return (tot / calls) if calls and pmc_ok else None

        def pmc_per_factorization(kernels):
            """HBM bytes of these kernels per factorization in the committed PMC passes (k_amax runs once per factorization)"""
            nfac = pmc.get("k_amax", {}).get("FETCH_SIZE", {}).get("calls", 0)
            tot = 0.0
            for k in kernels:
                e = pmc.get(k, {})
                if "FETCH_SIZE" in e and "WRITE_SIZE" in e:
                    tot += (e["FETCH_SIZE"]["sum_kb"] * FETCH_CORRECTION + e["WRITE_SIZE"]["sum_kb"]) * 1024.0
            return (tot / nfac) if nfac and pmc_ok else None

        npl, nul = max(det["npanel_launch"], 1), max(det["nupdate_launch"], 1)
        panel_obj = {"bound": "mfma", "kernel": "k_panel (k_panel_pc in the timed schedule: the same workgroups + k_upd_c riders) / k_panel_ca (+ k_front_wg): Householder panels; fp64 vector = matrix peak on gfx950",
                     "achieved": panel_tf, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": panel_tf / PEAK_FP64_MFMA_TFLOPS,
                     "ms": ms_panel, "launch_groups": det["npanel_launch"], "avg_us_per_step": ms_panel / npl * 1e3,
                     "traffic": pmc_traffic(["k_panel", "k_panel_ca"]),
                     "traffic_note": "per launch of k_panel / k_panel_ca alone; k_panel_pc's bytes are its riders' (update_kernels)",
                     "note": "latency-bound: a serial chain of Householder columns (DESIGN.md 4-5)"}
        upd_obj = {"bound": "hbm", "kernel": "k_upd_w + k_upd_c (in the timed schedule: k_upd_b0w = T + block 0 + k_upd_w riders, k_upd_c riders of k_panel_pc) / k_update / k_upd_wq + k_upd_cq (dlarfb on v_mfma_f64_16x16x4_f64)", "achieved": upd_gbs,
                   "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": upd_gbs / PEAK_HBM_GBS, "ms": ms_upd,
                   "launch_groups": det["nupdate_launch"], "avg_us_per_step": ms_upd / nul * 1e3,
                   "mfma_tflops": upd_tf, "mfma_frac": upd_tf / PEAK_FP64_MFMA_TFLOPS,
                   "traffic": pmc_traffic(["k_upd_w", "k_upd_c", "k_upd_b0w", "k_update", "k_upd_w2", "k_upd_c2", "k_upd_wq", "k_upd_cq"]),
                   # (the launches that carry update work in the timed schedule, k_panel_pc's riders included: its own panel bytes are
                   #  ~1 % of it)
                   "traffic_per_factorization": pmc_per_factorization(["k_upd_w", "k_upd_c", "k_upd_b0w", "k_panel_pc", "k_update", "k_upd_w2",
                                                                       "k_upd_y2", "k_upd_c2", "k_upd_wq", "k_upd_yq", "k_upd_cq"]),
                   "algorithmic_bytes_per_factorization": upd_bytes}
        # Latency roofline of the panel kernels ("small-front panel QR -> LDS / latency-bound").  A panel is a chain of 32
        # dependent Householder column steps; what bounds a column step is not flops or bytes but its chain of dependent
        # instructions.  Floors per column, from the guide's cycle constants and the 12 cycles per dependent fp64 VALU instruction
        # measured on this chain (DESIGN.md 4b has the count instruction by instruction), at 2.4 GHz:
        #   column pipeline (dev_tall_group: 13 + 3 exchange-adds, one LDS round trip + s_barrier, dlarfg's rsq / rcp Newton chains,
        #   the dot-product and rank-1 FMAs of 4-8 rows x 4-8 columns per thread)                          0.45 us
        #   wave panel (dev_wave_panel: the same without LDS, barrier and second reduction stage)           0.33 us
        #   Gram-based panel (k_panel_ca: the chain runs on the 32 x 32 Gram matrix in one wave, + the panel's Gram reduction and
        #   B := B M application, ~14 us, spread over its 32 columns)                                        0.60 us
        # A step's class is its tallest panel's kernel (estimated rows: > 4096 Gram-based, <= 512 wave, else the pipeline); its panel
        # time is the event pair around the step's panel launches in the detail pass (no riders there); 32 columns per step.
        LAT_FLOOR = {"column_pipeline": 0.45, "wave_panel": 0.33, "gram_panel": 0.60}
        lat = {}
        for n_act, rows, nca, pus, uus in step_rows:
            if n_act <= 0 or pus <= 0:
                continue
            cls = "gram_panel" if (nca > 0 and rows > 4096) else "wave_panel" if rows <= 512 else "column_pipeline"
            e = lat.setdefault(cls, {"steps": 0, "us": 0.0})
            e["steps"] += 1
            e["us"] += pus
        for cls, e in lat.items():
            e["columns_on_the_chain"] = 32 * e["steps"]
            e["achieved_us_per_column"] = e["us"] / e["columns_on_the_chain"]
            e["latency_floor_us_per_column"] = LAT_FLOOR[cls]
            e["frac_of_latency_floor"] = LAT_FLOOR[cls] / e["achieved_us_per_column"]
        if lat:
            top = max(lat, key=lambda k: lat[k]["us"])
            panel_obj["latency"] = lat
            panel_obj["latency_bound"] = {"kernel_class": top, **{k: lat[top][k] for k in ("latency_floor_us_per_column", "achieved_us_per_column",
                                                                                         "frac_of_latency_floor")},
                                          "note": "floor = dependent-instruction chain of one Householder column step (bench.py, DESIGN.md 4b); "
                                                  "achieved = panel launch time of the steps this class bounds / 32 columns, hand-offs between "
                                                  "column groups included"}
            panel_obj["latency_floor_us_per_column"] = lat[top]["latency_floor_us_per_column"]
            panel_obj["achieved_us_per_column"] = lat[top]["achieved_us_per_column"]
            panel_obj["frac_of_latency_floor"] = lat[top]["frac_of_latency_floor"]
        roof = dict(panel_obj if ms_panel >= ms_upd else upd_obj)
        roof["dominant_by"] = "HIP-event pairs around every launch of the family, no syncs in between (detail pass)"
        roof["panel_kernels"] = panel_obj
        roof["update_kernels"] = upd_obj
        roof["traffic_source"] = (str(pmc_file.relative_to(ROOT)) + f"; FETCH_SIZE x {FETCH_CORRECTION:.3f} (gfx950 half-counting, "
                                  "calibrated on k_rh_copy / k_cpack)") if pmc_ok else None
        # (from the TIMED steps -- value itself --, not from the detail pass, whose event pairs make it ~15 % slower)
        roof["whole_factorization"] = {"bound": "mfma", "achieved": value * 1e-3 / max(world if not sharded else 1, 1),
                                       "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                                       "frac": value * 1e-3 / max(world if not sharded else 1, 1) / PEAK_FP64_MFMA_TFLOPS,
                                       "note": "flops of one factorization / ms_per_step of the timed region, per GPU"}
        roof["assembly"] = {"bound": "hbm", "achieved": det["bytes_assemble"] / max(det["ms_assemble"], 1e-9) * 1e-6,
                            "peak": PEAK_HBM_GBS, "unit": "GB/s",
                            "frac": det["bytes_assemble"] / max(det["ms_assemble"], 1e-9) * 1e-6 / PEAK_HBM_GBS}
        roof["ms"] = {k: det[k] for k in ("ms_total", "ms_assemble", "ms_panel", "ms_small", "ms_update", "ms_pack")}
    if rank == 0:
        oname = ORDERING_NAMES.get(int(g["ordering"][0]), str(int(g["ordering"][0]))) if "ordering" in g else "unknown"
        standin_of = {"xenon1": "xenon1.mtx", "sme3dc": "sme3Dc.mtx", "c5mid": "3D_51448_3D.mtx (structure only, n = 27 000)", "c5mini": "3D_51448_3D.mtx (structure only, n = 8000)",
                      "c5_": "3D_51448_3D.mtx (SURVEY 8d generator at full size, n = 52 022)"}
        sof = next((v for k, v in standin_of.items() if name.startswith(k)), None)
        wl = (f"{name}: m={S.m} n={S.n} nnz={S.anz} fronts={S.nf} flops/step={flops:.4g}, ordering {oname}" +
              (f" (stand-in for {sof}, absent from the reference checkout)" if "standin" in name and sof else "") +
              (f" (Matrix Market file {mtx_meta['file']}: {mtx_meta['n1cols']} column singletons removed first, own reader + COLAMD + "
               f"symbolic analysis)" if mtx_meta else ""))
        out = {
            "metric": "numerical-factorization GFLOP/s", "value": value, "unit": "GFLOP/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": wall / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong" if sharded else "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": wl,
                       "inputs": "values resident in HBM, factors left in HBM",
                       "parallelism": ((f"subtree-sharded x{world}: tree of joins, contribution blocks device-to-device over RCCL "
                                        f"point-to-point" + ("; heavy top fronts shared by their rank group (panels in turn, 32-column "
                                                             "blocks of the trailing matrix per rank)" if args.spread else "")
                                        if sharded else f"replica x{world}") +
                                       (" -- REHEARSAL: all ranks on ONE GPU, gloo, blocks through the host (not a measurement)"
                                        if rehearsal else "")),
                       "flops_per_step": flops, "device_ms_per_step": dev_ms / args.steps, "launches_per_step": st["nlaunch"],
                       "levels": st["nlevels"], "timeline_steps": st["nsteps"], "retries": retries,
                       "device_bytes": (det or st).get("device_bytes", 0.0)},
            **({"roofline": roof} if roof is not None else {}),
        }
        if crit is not None:
            # model bound of the strong-scaling speed-up: whole tree's flop bound / flop bound on the critical path (per phase
            # the heaviest rank; a shared front = its panel chain + 1/R of its updates).  A MODEL: no multi-GPU hardware run of
            # this path was possible on the one-GPU build box; message and launch latency per panel step are not in it.
            out["config"]["critical_path_flop_share"] = crit[0] / max(crit[1], 1.0)
            out["config"]["strong_scaling_bound"] = crit[1] / max(crit[0], 1.0)
            out["config"]["strong_scaling_bound_subtrees_only"] = crit_sub[1] / max(crit_sub[0], 1.0)
            out["config"]["shared_fronts"] = 0 if span is None else int((np.asarray(span) > 1).sum())
            out["config"]["shared_front_loop"] = native_note
            out["config"]["hardware_scaling_note"] = ("no multi-GPU node was available to the build: this line is the FIRST hardware run of the "
                                                      "RCCL path unless parallelism says REHEARSAL")
            # ... and if every heavy top front were shared regardless of the per-step latency threshold of spread_partition
            out["config"]["strong_scaling_bound_all_heavy_fronts_shared"] = crit_all[1] / max(crit_all[0], 1.0)
        if mtx_meta:
            out["config"]["matrix_file"] = mtx_meta
        # SURVEY 8 (f1), outside the timed region: Q'b and the least-squares solve on the factors still resident in HBM
        # (wall time including the copies of the vectors), with the residual the reference's driver prints
        try:
            if args.full and not sharded:
                from stmmqr_testlib import csc_matvec
                Ap_, Ai_, Ax_ = g["in_Ap"], g["in_Ai"], g["in_Ax"]
                xt = np.arange(S.n, dtype=np.float64)
                b = csc_matvec(S.m, Ap_, Ai_, Ax_, xt)
                plan.qmult(0, b)
                t0 = time.perf_counter(); plan.qmult(0, b); t1 = time.perf_counter()
                xs = plan.solve(b); t2 = time.perf_counter()
                res = float(np.linalg.norm(csc_matvec(S.m, Ap_, Ai_, Ax_, xs) - b) /
                            (np.linalg.norm(Ax_) * np.linalg.norm(xs) + np.linalg.norm(b)))
                out["f1_resident_factors"] = {"qmult_qtx_ms": (t1 - t0) * 1e3, "solve_ms": (t2 - t1) * 1e3, "residual": res}
                # a block of 32 right-hand sides through the same passes (batched: DESIGN.md 6b); column 0 is b
                B32 = np.column_stack([b] + [np.roll(b, 7 * (j + 1)) for j in range(31)])
                plan.qmult(0, B32.copy()); xs32 = plan.solve(B32)
                t3 = time.perf_counter(); plan.qmult(0, B32.copy()); t4 = time.perf_counter()
                xs32 = plan.solve(B32); t5 = time.perf_counter()
                out["f1_resident_factors"].update({"qmult_qtx_32rhs_ms": (t4 - t3) * 1e3, "solve_32rhs_ms": (t5 - t4) * 1e3,
                                                   "rhs32_over_rhs1": [(t4 - t3) / max(t1 - t0, 1e-9), (t5 - t4) / max(t2 - t1, 1e-9)],
                                                   "rhs32_column0_equals_single": bool(np.array_equal(np.asarray(xs32)[:, 0], np.asarray(xs).ravel()))})
        except Exception as e:  # rank-deficient inputs: the device solve refuses them
            out["f1_resident_factors"] = {"error": str(e)}
        # Outside `value`: what the drop-in seam adds around the device time -- ONE call of the exported qr_factorize
        # (SparseQR.h:127-135) with host arrays in and a host qr_numeric out: plan build, H2D of the values, the
        # factorization, D2H of the packed R+H, host allocation -- the interval the reference's "Factorize time" brackets
        # (SparseQR.c:346-377).  And the own symbolic phase: stmmqr_analyze on this matrix with its permutation.
        try:
            if args.full and world == 1:
                # the exported qr_factorize itself (reference structs in, qr_numeric out), twice: the first call builds the plan,
                # the second finds it in the seam's cache (same qr_symbolic, same pattern) -- what a refactorization costs
                plan.close()                                        # (this process's bench plan: its HBM goes back first)
                plan = None
                seam = []
                for _ in range(6):
                    t0 = time.perf_counter()
                    Nq = pkg.qr_factorize_seam(sym, g["in_Ap"], g["in_Ai"], g["in_Ax"], tol, ntol)
                    seam.append((time.perf_counter() - t0) * 1e3)
                    mb = Nq.rh_total * 8e-6
                    assert Nq.rank == st_rank, (Nq.rank, st_rank)
                    Nq.close()
                pkg.plan_cache_clear()
                out["dropin_seam_ms"] = seam[0]
                out["dropin_seam_cached_ms"] = sorted(seam[1:])[len(seam[1:]) // 2]      # median of the five later calls
                out["dropin_seam_calls_ms"] = seam
                out["dropin_seam_note"] = ("one call of the exported qr_factorize (plan + H2D + factorization + host qr_numeric + D2H of %.0f MB of "
                                          "packed R+H): first call builds the plan, later calls with an equal qr_symbolic reuse it (seam cache); "
                                          "not part of `value`" % mb)
                Qf = g["sym_Qfill"] if "sym_Qfill" in g and len(g["sym_Qfill"]) else None
                t0 = time.perf_counter()
                pkg.analyze(S.m, S.n, g["in_Ap"], g["in_Ai"], Qf, bool(S.do_rank_detection), None)
                out["own_symbolic_ms"] = (time.perf_counter() - t0) * 1e3
        except Exception as e:
            out["dropin_seam_error"] = str(e)
        # The large-front class (BASELINE configs[4]'s structure: one dense root front carries the flops, the quad update on the matrix
        # cores), un-headlined and outside `value`: the same library, the full-size stand-in and its n = 27 000 sibling, three / two
        # timed factorizations each after one warm-up, plus one detail pass for the update kernels' own share of the MFMA peak.
        if args.full and world == 1 and args.large_front and name == DEFAULT_WORKLOAD.get(1) and mtx_path is None:
            lf = {}
            for wl_name, nsteps in (("c5mid_standin", 3), ("c5_standin", 2)):
                try:
                    if plan is not None:
                        plan.close(); plan = None
                    g2 = load_golden(wl_name)
                    S2 = Symbolic(g2)
                    sym2 = {**S2.sc, **{k: v for k, v in S2.arr.items() if v is not None}}
                    tol2, ntol2 = scalar(g2, "in_tol"), int(scalar(g2, "in_ntol"))
                    p2 = pkg.HipQR(sym2, device=local)
                    p2.set_pattern(g2["in_Ap"], g2["in_Ai"])
                    Ax2 = torch.from_numpy(np.ascontiguousarray(g2["in_Ax"])).to(dev)
                    p2.factorize(None, tol2, ntol2, device_ptr=Ax2.data_ptr())
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rt = 0
                    for _ in range(nsteps):
                        s2 = p2.factorize(None, tol2, ntol2, device_ptr=Ax2.data_ptr())
                        rt += int(s2.get("retries", 0))
                    torch.cuda.synchronize()
                    ms2 = (time.perf_counter() - t0) / nsteps * 1e3
                    d2 = p2.factorize(None, tol2, ntol2, device_ptr=Ax2.data_ptr(), detail=True)
                    fl2 = float(scalar(g2, "flopcount"))
                    assert int(round(s2["flops"])) == int(round(fl2)), (s2["flops"], fl2)
                    lf[wl_name] = {"ms_per_step": ms2, "steps": nsteps, "tflops": fl2 / ms2 * 1e-9, "frac_of_fp64_mfma_peak": fl2 / ms2 * 1e-9 / PEAK_FP64_MFMA_TFLOPS,
                                   "update_kernels_mfma_frac": d2["flops_update"] / max(d2["ms_update"], 1e-9) * 1e-9 / PEAK_FP64_MFMA_TFLOPS,
                                   "update_kernels_ms": d2["ms_update"], "panel_kernels_ms": d2["ms_panel"] + d2["ms_small"], "retries": rt,
                                   "flops_per_step": fl2, "n": int(S2.n), "device_bytes": d2.get("device_bytes", 0.0)}
                    p2.close()
                    del Ax2
                except Exception as e:      # noqa: BLE001 (the headline line must come out whatever happens here)
                    lf[wl_name] = {"error": str(e)[:300]}
            out["large_front"] = lf
        if args.full and not args.no_cpu and world == 1:     # (the CPU baseline is reported at N = 1 only)
            cb = cpu_baseline(name, g, mtx_path=mtx_path, flops=flops)
            if mtx_path is not None and cb.get("kind") == "reference":
                fl_ref = [l for l in cb.get("legs", []) if l.get("mode", "").startswith("serial") and "value" in l]
                if fl_ref:      # the reference's own flop count on the same file must be the device's
                    cb["flops_match_device"] = bool(int(round(fl_ref[0]["flops"])) == int(round(flops)))
            out["cpu_baseline"] = cb
        print(json.dumps(out))
    guard["done"] = True                                # (the line is out: a late SIGTERM / deadline prints nothing more)
    if plan is not None:
        plan.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
