// stmmqr_knobs.h -- every STMMQR_* environment variable libstmmqr_hip.so reads: ONE row each with its name, type, reading rule,
// the moment it is read, its default and what it does.  Plain C++17: nothing of HIP, nothing of the library (a host compiler
// builds it alone: tests/test_knobs_cpu.py).  Diagnosis, tests and experiments only -- none of them is needed to use the library.
//
// The moment is part of the behaviour: tests change these variables between two factorizations of one process and expect the
// next call to see the new value.
//   PROCESS  once per process, at the first use (knobs::once<K_...>())
//   PLAN     when a plan is created (build_plan)
//   SCHED    at every build of a schedule (BuildKnobs::read where a schedule is about to be built: sched::Inputs::k; the plan's sched_gen covers them)
//   RUN      at every run of a schedule (RunKnobs::read at the top of stm_run_schedule; RunKnobs::key is what a captured hipGraph is
//            keyed by: a RUN row is a field of RunKnobs, so the run cannot read a knob that the key forgets)
//   CALL     at every call of the function that uses it
// Reading rules (the call sites apply none of their own):
//   PLAIN    unset: the default; set: the number (atol / atof).  A FLAG is on when that number is not 0 -- "unset means on" is a
//            default of 1, "set and not 0" a default of 0
//   PRESENT  on when the variable is set at all, whatever its text
//   MIN0, MIN1   the number, raised to 0 / 1
//   POSITIVE a number that is not positive reads as the default
//   BOOLEAN  set: 1 when the number is not 0, else 0; unset: the default (-1: the library decides)
// (stmmqr_qrtest, a program of its own, reads STMMQR_REFERENCE_LIB / STMMQR_QRTEST_VERBOSE; the name of the RCCL library,
//  STMMQR_RCCL_LIB, is looked up where it is loaded: stmmqr_multi.cpp.)
#pragma once
#include <cstdlib>
#include <cstring>

namespace knobs {

enum Type { INT, REAL, FLAG, PATH };
enum Rule { PLAIN, PRESENT, MIN0, MIN1, POSITIVE, BOOLEAN };
enum When { PROCESS, PLAN, SCHED, RUN, CALL };

// X(NAME, field, C type of the field, type, rule, moment, default, what it does)      (field: of BuildKnobs / RunKnobs)
#define STM_KNOBS_PROCESS(X)                                                                                                        \
    X(PART_GRAIN, part_grain, long, INT, PLAIN, PROCESS, 2048, "entries per workgroup of the assembly / packing launches (16384 until round 5 -- 2048: epb1 5.81 -> 5.60 ms, default 93.3 -> 92.9)") \
    X(PART_CAP, part_cap, long, INT, PLAIN, PROCESS, 4096, "... and the most workgroups a front gets in them")                      \
    X(RSPW, rspw, int, INT, PLAIN, PROCESS, 0, "row slabs per rider workgroup of the panel launches (0: chosen per launch)")        \
    X(RSPW_W, rspw_w, int, INT, POSITIVE, PROCESS, 2, "row slabs per rider workgroup of the T + block 0 launch")                    \
    X(B0_ONE, b0_one, int, INT, PLAIN, PROCESS, 1, "T + block 0 of a riding step: 1 k_upd_b0w, 0 k_upd_f with its two meeting points") \
    X(ANYORDER, anyorder, int, INT, PLAIN, PROCESS, 0, "k_upd_w riders take their tiles in any order (measurements)")              \
    X(RHS_BATCH, rhs_batch, int, INT, MIN1, PROCESS, 32, "right-hand sides per pass of the resident-factor operations (1: one vector after the other)")
#define STM_KNOBS_PLAN(X)                                                                                                           \
    X(RH_EST_SCALE, rh_est_scale, double, REAL, PLAIN, PLAN, 1.0, "factor on the estimate that sizes the R+H arena (tests shrink it to drive the overflow path); every rebuild of the schedule keeps it") \
    X(QBIG_MIN, qbig_min, long, INT, PLAIN, PLAN, 1L << 20, "entries of a front from which Q-apply / back substitution split its rows over workgroups") \
    X(RTBIG_MIN, rtbig_min, long, INT, PLAIN, PLAN, 1L << 62, "entries of a front from which the R' pass of the minimum-norm solve splits its columns over workgroups; by default only the fronts that one workgroup cannot hold (whether fronts that fit are faster split is unmeasured: the knob is there to tune that, and 1 lets tests send every front through the split kernels)")
#define STM_KNOBS_SCHED(X)                                                                                                          \
    X(TUNE, tune, int, INT, PLAIN, SCHED, 0, "measurement sweeps of the update kernels (also read by every qr_front call)")         \
    X(CA_MIN, ca_min, int, INT, PLAIN, SCHED, 4096, "rows from which panel_algo 0 takes the Gram-based panel (= STM_CA_MIN_ROWS)")  \
    X(RECYCLE, recycle, int, INT, PLAIN, SCHED, 1, "slab recycling of whole-tree plans: 0 never, 2 always, 1 when the slabs of all fronts reach 256 MB (BuildKnobs::recycles)") \
    X(SCHED, sched, int, INT, PLAIN, SCHED, 0, "step order: 1 level-synchronous, 2 as soon as possible, 3 envelope rule, 0 chosen per front group") \
    X(PAIR_MIN, pair_min, long, INT, PLAIN, SCHED, 16384, "estimated rows from which a front takes the pair / quad update (options.pair_update)") \
    X(EARLY_END, early_end, bool, FLAG, PLAIN, SCHED, 1, "a front is scheduled up to the panel where it is expected to run out of rows (0: every panel a step)") \
    X(EARLY_SLACK, early_slack, int, INT, PLAIN, SCHED, 0, "... plus this many panels")                                             \
    X(RIDE, ride, double, REAL, PLAIN, SCHED, 1.0, "envelope rule: factor on the height a riding front may have")            \
    X(KEEP_FRONTS, keep_fronts, int, INT, PLAIN, SCHED, -1, "slab recycling: how many of the largest fronts keep their slab (0..3, larger reads as 3; -1: the planner chooses) -- tests force the set that the download packs on the fly")
#define STM_KNOBS_RUN(X)                                                                                                            \
    X(LA_MIN, la_min, long, INT, PLAIN, RUN, 2500, "look-ahead: tiles (256 x 32) of update beyond block 0 from which a step goes to the side stream (two cross-stream hand-offs, ~25 us)") \
    X(LA_MIN_FUSED, la_min_fused, long, INT, PLAIN, RUN, 1500, "... where T + block 0 is one fused launch")                         \
    X(LA_FUSED_ROWS, la_fused_rows, int, INT, PLAIN, RUN, 5120, "expected panel rows up to which an offloaded step fuses T + block 0 (0: never)") \
    X(LA_MAXPWG, la_maxpwg, long, INT, PLAIN, RUN, 48, "the most panel workgroups an offloaded step may have")                      \
    X(LA_SYSFENCE, la_sysfence, bool, FLAG, PLAIN, RUN, 0, "look-ahead events with the default system-scope fence")                 \
    X(SIDE_RESERVE, side_reserve, long, INT, MIN0, RUN, 32, "compute units the side stream leaves alone (its CU mask: made once per device and process) = half the k_upd_f workgroups surely resident") \
    X(PASSENGERS, passengers, bool, FLAG, PLAIN, RUN, 1, "passenger launches (options.lookahead 2)")                                \
    X(PASS_MAXWG, pass_maxwg, long, INT, PLAIN, RUN, 384, "the most workgroups the T + block 0 launch of a riding step may have")    \
    X(PASS_ROWS, pass_rows, int, INT, PLAIN, RUN, 16384, "expected panel rows up to which a step rides")                            \
    X(PASS_K, pass_k, double, REAL, PLAIN, RUN, 1e30, "riders stay off a panel launch when their tiles exceed this times its microseconds") \
    X(PASS_TILES, pass_tiles, long, INT, PLAIN, RUN, 1L << 40, "... or this many tiles (measured: riding always wins -- 2000: 123 ms, 3000: 117, never: 109.9 on the default workload)") \
    X(PASS_ABL, pass_abl, int, INT, PLAIN, RUN, 0, "timing-only ablations (WRONG results): 1 no k_upd_w riders, 2 no k_upd_c riders, 4 riders as launches of their own, 8 ... behind an empty panel launch") \
    X(CA_RIDERS, ca_riders, bool, FLAG, PLAIN, RUN, 1, "riders on the Gram-based panel launch")                                     \
    X(DBG, dbg, int, INT, PLAIN, RUN, 0, "bit mask (stmmqr_kernels.h); also read wherever a DevCtx is made")
#define STM_KNOBS_CALL(X)                                                                                                           \
    X(QT4, qt4, bool, FLAG, PLAIN, CALL, 1, "grouped split Q-apply (0: the per-panel launches)")                                    \
    X(LIVE_PANELS, live_panels, bool, FLAG, PLAIN, CALL, 1, "Q-apply / back substitution visit only the panels that can hold a reflector") \
    X(RESIDENT_CACHE, resident_cache, int, INT, BOOLEAN, CALL, -1, "recycled slabs: the scratch holds every front in front form (1) or one tree level (0); unset: by free memory") \
    X(NULL_SLAB, null_slab, long, INT, MIN1, CALL, 2048, "rows of the null-space basis N per slab of the Gram matrix N'N and of N'X: a workgroup per (tile, slab), the partial sums added in slab order (read when N is built and at every projection)") \
    X(CHUNK, chunk, int, INT, PLAIN, CALL, 1, "fronts per panel launch with STMMQR_DBG bit 9")                                      \
    X(DOWNLOAD_WIN, download_win, long, INT, POSITIVE, CALL, 32L << 20, "doubles per window of stmmqr_plan_download on a plan that recycles its slabs (256 MB; tests shrink it to put window edges where they want them)") \
    X(PLAN_CACHE, plan_cache, int, INT, MIN0, CALL, 1, "plans the drop-in seam keeps (0: no cache)")                                \
    X(SEAM_EARLY_ALLOC, seam_early_alloc, int, INT, PLAIN, CALL, 1, "the seam populates the returned stack beside the factorization: 0 never, 1 for cached plans, 2 for first calls too") \
    X(SEAM_TIMING, seam_timing, bool, FLAG, PRESENT, CALL, 0, "the seam prints where a call spent its time")                        \
    X(MEMDUMP, memdump, bool, FLAG, PRESENT, CALL, 0, "device memory by purpose, printed per factorization")                        \
    X(DUMPLV, dumplv, bool, FLAG, PRESENT, CALL, 0, "no hipGraph replay (diagnosis runs)")                                          \
    X(DBG_EARLY, dbg_early, bool, FLAG, PRESENT, CALL, 0, "one line per front that outlived its cut schedule")                      \
    X(TIMELINE, timeline, bool, FLAG, PRESENT, CALL, 0, "with STMMQR_DBG bit 5 on a STAMPS build: the timeline of the last panel 1") \
    X(DUMPSTEPS, dumpsteps, const char *, PATH, PLAIN, CALL, 0, "file: one line per timeline step of a detail run with what ran and how long")
#define STM_KNOBS(X) STM_KNOBS_PROCESS(X) STM_KNOBS_PLAN(X) STM_KNOBS_SCHED(X) STM_KNOBS_RUN(X) STM_KNOBS_CALL(X)

enum Id {
#define X(NAME, ...) K_##NAME,
    STM_KNOBS(X)
#undef X
    K_COUNT
};

struct Row { const char *name; Type type; Rule rule; When when; double dflt; const char *doc; };
constexpr Row TABLE[K_COUNT] = {
#define X(NAME, field, ctype, type, rule, when, dflt, doc) {"STMMQR_" #NAME, type, rule, when, (double)(dflt), doc},
    STM_KNOBS(X)
#undef X
};

inline const char *text(Id id) { return getenv(TABLE[id].name); }       // (a PATH: the file name, or nullptr)

// the value of a row under its reading rule (integers are exact in a double far beyond any value here)
inline double value(Id id)
{
    const Row &r = TABLE[id];
    const char *s = text(id);
    if (r.rule == PRESENT) return s ? 1.0 : 0.0;
    if (!s) return r.dflt;
    const double v = (r.type == REAL) ? atof(s) : (double)atol(s);
    switch (r.rule) {
        case MIN0: return v < 0 ? 0.0 : v;
        case MIN1: return v < 1 ? 1.0 : v;
        case POSITIVE: return v > 0 ? v : r.dflt;
        case BOOLEAN: return v != 0 ? 1.0 : 0.0;
        default: return v;
    }
}
inline long num(Id id) { return (long)value(id); }
inline bool on(Id id) { return value(id) != 0; }
// a PROCESS row: the first call fixes the value for the process
template <Id id> inline long once()
{
    static const long v = num(id);
    return v;
}

inline unsigned long long fold(unsigned long long h, unsigned long long v) { return (h ^ v) * 1099511628211ULL; }      // FNV-1a step
inline unsigned long long fold(unsigned long long h, double v)
{
    unsigned long long b;
    v += 0.0;
    memcpy(&b, &v, sizeof b);
    return fold(h, b);
}

// what a build of the schedule (sched::build, stmmqr_sched.h) reads of the environment: read once by its caller
struct BuildKnobs {
#define X(NAME, field, ctype, ...) ctype field;
    STM_KNOBS_SCHED(X)
#undef X
    static BuildKnobs read()
    {
        BuildKnobs k;
#define X(NAME, field, ctype, ...) k.field = (ctype)value(K_##NAME);
        STM_KNOBS_SCHED(X)
#undef X
        return k;
    }
    // STMMQR_RECYCLE's three modes, for a whole-tree plan whose fronts' slabs hold `slabs` doubles (below 256 MB the three extra
    // launches per step cost more than the memory is worth: epb1 holds 70 MB either way and took 7.4 -> 7.7 ms)
    bool recycles(long long slabs) const { return recycle == 2 || (recycle == 1 && slabs >= (32LL << 20)); }
};

// what stm_run_schedule reads of the environment, once at its top -- and, folded, the environment's part of the hipGraph key
struct RunKnobs {
#define X(NAME, field, ctype, ...) ctype field;
    STM_KNOBS_RUN(X)
#undef X
    static RunKnobs read()
    {
        RunKnobs k;
#define X(NAME, field, ctype, ...) k.field = (ctype)value(K_##NAME);
        STM_KNOBS_RUN(X)
#undef X
        return k;
    }
    unsigned long long key() const
    {
        unsigned long long h = 1469598103934665603ULL;
#define X(NAME, field, ...) h = fold(h, (double)field);
        STM_KNOBS_RUN(X)
#undef X
        return h;
    }
};

// the text of every knob read when a plan or its schedule is built, folded into h (the plan cache of the drop-in seam: a plan
// built under other values is another plan).  PROCESS rows never change once the first plan exists.
inline unsigned long long fold_plan_knobs(unsigned long long h)
{
    for (int i = 0; i < K_COUNT; i++) {
        const char *s = (TABLE[i].when == PLAN || TABLE[i].when == SCHED) ? getenv(TABLE[i].name) : nullptr;
        if (!s) continue;
        h = fold(h, (unsigned long long)(i + 1));
        for (; *s; s++) h = fold(h, (unsigned long long)(unsigned char)*s);
    }
    return h;
}

}  // namespace knobs
