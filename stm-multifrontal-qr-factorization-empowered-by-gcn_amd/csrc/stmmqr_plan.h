// stmmqr_plan.h -- the plan object and the helpers shared by the host translation units of libstmmqr_hip.so (local to the library):
//   stmmqr_host.cpp      globals, options, device set-up and the side stream, device alloc / copy / free, shutdown
//   stmmqr_planbuild.cpp the symbolic plan (build_plan), the pattern of A, plan create / destroy, stmmqr_plan_set_groups; the ONE
//                        place where a schedule goes into the plan and onto the device (stm_install_schedule), the arenas
//   stmmqr_factorize.cpp the factorization driver: begin / group / finish / the whole call, around the pure recovery policy of
//                        stmmqr_recover.h; its diagnostic prints in stmmqr_diag.cpp
//   stmmqr_download.cpp  the factors out of the plan in the reference's layout (stmmqr_plan_download)
//   stmmqr_schedule.cpp  the pure planner (stmmqr_sched.h: no plan, no HIP call, no global): the symbolic sizes of the fronts, and
//                        sched::build -- arena offsets, the timeline allocator, the step timeline of every front group -- which
//                        returns the value stmmqr_plan::sch holds
//   stmmqr_run.cpp       the step scheduler (stm_run_schedule: one step, serial, look-ahead, passengers), the pack pass
//   stmmqr_multi.cpp     contribution blocks / panels in and out of a plan, shared fronts, the RCCL transport
//   stmmqr_rfactor.cpp   Q-apply and triangular solves on the resident factors; with stmmqr_rcond.cpp (products with R,
//                        condition estimate), stmmqr_rsparse.cpp / stmmqr_hsparse.cpp (R / H out as a sparse matrix), stmmqr_rcov.cpp (selected inverse), stmmqr_seminormal.cpp (products with A, seminormal
//                        solves) and the pure stmmqr_restables.cpp: stmmqr_resident.h
//   stmmqr_seam.cpp      the drop-in seam qr_factorize with the reference's structs, its plan cache
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <mutex>
#include <thread>
#include <vector>
#ifdef __linux__
#include <sys/mman.h>
#endif
#include <dlfcn.h>

#include "../../include/stmmqr_hip.h"
#include "stmmqr_device.h"
#include "stmmqr_kernels.h"
#include "stmmqr_internal.h"
#include "stmmqr_knobs.h"
#include "stmmqr_recover.h"
#include "stmmqr_sched.h"              // (Step, sched::Schedule: the pure planner)


extern thread_local std::string g_err;
extern stmmqr_options g_opt;
extern size_t g_chunk[4];

// offsets inside the reference's sparse_common for the stock LP64 build; verified against the real header
// by tests/test_abi_layout.py where /root/reference is present.
extern stm_common_layout g_layout;

int fail(int code, const std::string &msg);

#define HIPCHK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return fail(e_ == hipErrorOutOfMemory ? STMMQR_ERR_OUT_OF_MEMORY : STMMQR_ERR_DEVICE,        \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                              \
    } while (0)
#define LCHK(expr)                                                                                        \
    do {                                                                                                  \
        int e_ = (expr);                                                                                  \
        if (e_ != 0) return fail(STMMQR_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString((hipError_t)e_)); \
    } while (0)

#define PASS(expr) do { int e_ = (expr); if (e_ != 0) return e_; } while (0)      // (the callee has said why)

inline double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    int alloc(size_t count)
    {
        release();
        n = count;
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; n = 0; return (int)e; }
        return 0;
    }
    int upload(const std::vector<T> &h, hipStream_t st)
    {
        int e = alloc(h.size());
        if (e) return e;
        if (!h.empty()) return (int)hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
    ~DevBuf() { release(); }
};

// What k_spmv reads of a sparse matrix A besides its values: the column form (cp, ci) for A'x and a row form (rp; per entry its
// column rj and the position rq of its value in A's storage) for A x.  Built on the host by stm_row_form (stmmqr_internal.h).
struct AIndexDev { DevBuf<int> cp, ci, rp, rj, rq; };

#include "stmmqr_resident.h"          // (ResidentState: needs DevBuf)

struct stmmqr_plan {
    int device = 0;
    hipStream_t stream = nullptr;
    // look-ahead: the panel chain runs on `stream` (high priority), everything that does not feed the next panel on `side`
    hipStream_t side = nullptr;                               // (the device's shared side stream: side_stream_for)
    std::vector<hipEvent_t> ev_main, ev_prep, ev_side;        // one of each per timeline step (no timing)
    hipEvent_t ev[8] = {};
    // detail timing: one event pair per launch category and level step, recorded on the plan's stream WITHOUT any
    // synchronisation (the schedule runs exactly as in the timed region); the pairs are read after the final sync
    struct EvPair { hipEvent_t a, b; int cat, step; };
    std::vector<EvPair> evpairs;
    size_t evused = 0;
    long m = 0, n = 0, anz = 0, nf = 0, maxfn = 0, rjsize = 0, hisize = 0;
    int do_rank = 1;
    int keep_h = 1;                                    // QRsym->keepH: 0 = the packed blocks hold R only (qr_rhpack's keepH = 0 layout);
                                                       //  no Q-apply, one group only (stmmqr_plan_set_groups refuses)
    std::vector<long> Sp, Sj, Qfill, PLinv, Sleft, Child, Childp, Super, Rp, Rj, Post, Hip, Fm;
    bool has_qfill = false;
    // ---- what the planner reads (sched::Inputs): the grouping, the symbolic estimates, the recovery state
    std::vector<int> group;                    // per front: phase on this device, -1 = elsewhere
    std::vector<char> shared;                  // per front: STMMQR_GROUP_SHARED -- alone in its group, driven step by step
                                               //  (stmmqr_factorize_step), its trailing column blocks shared with other plans
    long maxstack = 0;                   // QRsym->maxstack (0: unknown)
    long long rh_est_total = 0;          // all packed R+H blocks if no pivot column dies (symbolic; exact for full-rank input)
    std::vector<long long> rh_est_front; // ... per front (keepH = 0: the arena holds those of the fronts that do not keep their slab)
    double rh_est_scale = 1.0;           // ... times STMMQR_RH_EST_SCALE, read once when the plan is created (tests shrink the estimate)
    recover::State rec;                  // what the planner reads of earlier failures (arena growth, full schedule), the last finish's outcome
    // ---- what the planner builds: the fronts (sch.fs) and everything a rebuild of the schedule replaces, as ONE value.  Written by
    // stm_install_schedule alone (stmmqr_planbuild.cpp), which also bumps sched_gen; everyone else reads it
    sched::Schedule sch;
    long sched_gen = 0;                  // schedule generation: what the resident tables and a captured graph were built from
    long long tpanels = 0;               // panels of all fronts: one kept T each (Q-apply on the resident factors)
    bool pattern_set = false;
    double bytes_assemble_idx = 0;       // index bytes of the assembly (symbolic part of SURVEY 8d formula)

    DevBuf<FrontSym> d_fs;
    DevBuf<FrontNum> d_fnum;
    DevBuf<double> d_F, d_C, d_T, d_Gp, d_Tall, d_Sx, d_Ax, d_Tau, d_RH, d_Wp, d_Wp2;
    DevBuf<int> d_tslot, d_Sp, d_Sjrel, d_Sj0, d_Sleft, d_Child, d_Rjrel, d_Stair, d_Hii, d_Cmap, d_Cursor,
        d_lists, d_smap;
    DevBuf<long long> d_Rhoff;
    DevBuf<long long> d_wlists;
    DevBuf<double> d_Ypend;                    // -Y of the pair-update fronts, by absolute column block (DevCtx::Ypend)
    DevBuf<long long> d_ypoff;                 // [nf] offsets into it (-1: not a pair-update front)
    DevBuf<double> d_msg;                // subtree exchange: message buffers (stmmqr_factorize_exchange, grown on demand)
    DevBuf<int> d_wcnt, d_wcnt2;         // per column block of the update workspaces: slab tickets (zero between launches)
    DevBuf<int> d_wflag, d_wflag2;       // ... fused update: step + 1 once W2 of the column block is in its slot
    DevBuf<int> d_abort;                 // [1] a bounded wait ran out, [2] a front outlived its cut schedule, [3] a refused message
    size_t wcnt_n = 1;
    DevBuf<long long> d_Rboff, d_total;
    DevBuf<long long> d_rhtop, d_fin;    // slab recycling: {bump pointer, overflow word}; Post-order offsets of the packed blocks
    DevBuf<char> d_kept;
    DevBuf<double> d_bounce;             // download window
    DevBuf<unsigned long long> d_dbg, d_amax;
    DevBuf<double> d_sig;                           // {sg, 1/sg}: magnitude guard of the panel kernels
    DevBuf<char> d_Rdead;
    // products with A on the device (stmmqr_plan_spmv, the seminormal solve): built at the first such call after set_pattern (stm_ensure_a_index)
    AIndexDev a_idx;
    std::vector<int> h_smap;                    // host copy of d_smap (what those forms are built from)
    bool a_index_ready = false;

    // results of the last factorization
    bool factored = false, begun = false, first_group = true;
    bool serial_panels = false;          // recovery: every panel by ONE workgroup (no inter-workgroup waits at all)
    long long rh_total = 0;
    long rank = 0;
    std::vector<FrontNum> h_fnum;
    ResidentState res;                   // everything the operations on the resident factors keep (stmmqr_resident.h)
    // options.use_graph: the captured schedule of group 0, and what it was captured under -- everything that travels in the kernel
    // arguments or decides what is launched (ensure_graph compares keys; stm_install_schedule clears the capture)
    struct Graph {
        struct Key {
            double tol = 0; int ntol = 0, dbg = 0; unsigned long long opt = 0; long gen = -1;
            bool operator==(const Key &o) const { return tol == o.tol && ntol == o.ntol && dbg == o.dbg && opt == o.opt && gen == o.gen; }
        } key;
        hipGraphExec_t exec = nullptr;
        long nlaunch = 0;                          // launches of one replay (host statistics)
        void clear() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; nlaunch = 0; }
    } graph;
    double last_tol = 0;
    long last_ntol = 0;
    stmmqr_stats stats = {};

    // device memory held right now: the buffers of the factorization and the index of A; of the resident-factor operations only the
    // recycling scratch, the carried solve's view and the null-space basis with its Cholesky factor.  Their maps, work vectors, staging and T4 buffers (the rest of `res`) are not
    // counted: stats.device_bytes reports this number, the footprint of the factorization
    double device_bytes() const
    {
        double b = 0;
        auto add = [&](const auto &buf) { b += (double)buf.n * sizeof(*buf.p); };
        add(d_fs); add(d_fnum); add(d_F); add(d_C); add(d_T); add(d_Gp); add(d_Tall); add(d_Sx); add(d_Ax); add(d_Tau); add(d_RH);
        add(d_Wp); add(d_Wp2); add(d_tslot); add(d_Sp); add(d_Sjrel); add(d_Sj0); add(d_Sleft); add(d_Child); add(d_Rjrel);
        add(d_Stair); add(d_Hii); add(d_Cmap); add(d_Cursor); add(d_lists); add(d_smap); add(d_Rhoff); add(d_wlists);
        add(d_wcnt); add(d_wcnt2); add(d_wflag); add(d_wflag2); add(d_Rboff); add(d_Rdead); add(d_Ypend); add(d_ypoff);
        add(d_rhtop); add(d_fin); add(d_kept); add(res.sched.d_scr); add(d_bounce); add(res.sched.d_fs_scr);
        add(a_idx.cp); add(a_idx.ci); add(a_idx.rp); add(a_idx.rj); add(a_idx.rq);
        add(res.call.d_fs_car); add(res.call.d_fnum_car); add(res.call.d_carlist); add(res.call.d_carN);
        add(res.fact.null.d_N); add(res.fact.null.d_L); add(res.fact.null.d_Ld); add(res.fact.null.d_jd);
        return b;
    }
    DevCtx ctx() const { return ctx((int)knobs::num(knobs::K_DBG)); }
    DevCtx ctx(int dbg) const                                     // (dbg: STMMQR_DBG as the caller has read it)
    {
        DevCtx c;
        c.fs = d_fs.p; c.fnum = d_fnum.p; c.Farena = d_F.p; c.Carena = d_C.p; c.Tws = d_T.p; c.tslot = d_tslot.p;
        c.Tall = d_Tall.p;
        c.Gp = d_Gp.p; c.gp_slabs = sch.gp_slabs; c.sig = d_sig.p; c.panel_algo = serial_panels ? 1 : sch.plan_algo; c.ca_min_rows = sch.ca_min;
        c.Sx = d_Sx.p; c.Sp = d_Sp.p; c.Sjrel = d_Sjrel.p; c.Sj0 = d_Sj0.p; c.Sleft = d_Sleft.p;
        c.Child = d_Child.p; c.Rjrel = d_Rjrel.p; c.Stair = d_Stair.p; c.Tau = d_Tau.p; c.Hii = d_Hii.p;
        c.Rdead = d_Rdead.p; c.Cmap = d_Cmap.p; c.Cursor = d_Cursor.p; c.Rhoff = d_Rhoff.p; c.Rboff = d_Rboff.p;
        c.tol = last_tol; c.ntol = (int)last_ntol;
        c.dbg = dbg;
        c.sweep = sch.sweep;
        c.tune = sch.tune;                                            // (env STMMQR_TUNE when the schedule was built)
        c.Ypend = d_Ypend.p; c.ypoff = d_ypoff.p;
        c.rh_top = sch.recycle ? d_rhtop.p : nullptr; c.rh_cap = sch.rh_cap;
        if (serial_panels) c.dbg = (c.dbg & ~(2048 | 4096)) | 256;   // the one-workgroup LDS / in-place panel for every panel
        c.tall_min = sch.tall_min;
        c.cbskip = 0;
        c.dbgbuf = d_dbg.p;
        c.abort = d_abort.p;
        return c;
    }
    ~stmmqr_plan()
    {
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto &q : evpairs) { if (q.a) (void)hipEventDestroy(q.a); if (q.b) (void)hipEventDestroy(q.b); }
        graph.clear();
        for (auto *v : {&ev_main, &ev_prep, &ev_side})
            for (auto &e : *v)
                if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// One piece of one timeline step (stmmqr_factorize_step): what = STMMQR_STEP_* bits; the update takes the column blocks
// cb_first, cb_first + cb_stride, ... (at most cb_count of them when cb_count >= 0) of the step's fronts.
struct StepReq { int step, what, cb_first, cb_stride, cb_count; };
// scheduler (stmmqr_run.cpp) and plan (stmmqr_planbuild.cpp) entry points used by the other host translation units
int stm_ensure_arenas(stmmqr_plan &P);                                 // (stmmqr_planbuild.cpp)
int stm_run_schedule(stmmqr_plan &P, bool detail, int grp, const StepReq *req);
int stm_run_pack(stmmqr_plan &P, bool &overflow);
int stm_ensure_la_events(stmmqr_plan &P, size_t nsteps, const knobs::RunKnobs &k);
int stm_ensure_device(int device);
hipStream_t stm_side_stream_for(int device);                       // (stmmqr_host.cpp)
void stm_destroy_side_streams();
// stmmqr_planbuild.cpp
int stm_set_pattern(stmmqr_plan &P, const stm_long *Ap, const stm_long *Ai);
int stm_ensure_a_index(stmmqr_plan &P);
// the diagnostic prints of stmmqr_factorize_finish, in the order it calls them (stmmqr_diag.cpp)
void stm_diag_early_fronts(const stmmqr_plan &P);
void stm_diag_dump_steps(const stmmqr_plan &P, const std::vector<float> &pair_ms);
int stm_diag_panel_timeline(const stmmqr_plan &P, int dbg);
int stm_diag_block0_launch(const stmmqr_plan &P, int dbg);
int stm_diag_pipeline_counters(const stmmqr_plan &P, int dbg);
void stm_diag_memdump(const stmmqr_plan &P);
extern "C" int stm_check_c_slot(const stmmqr_plan &P, stm_long f, long long csize, const char *what);     // (defined inside the C ABI block)
