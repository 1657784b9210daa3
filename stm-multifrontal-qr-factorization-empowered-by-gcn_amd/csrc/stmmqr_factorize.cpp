// stmmqr_factorize.cpp -- the factorization driver: the phased interface begin -> factorize_group(g) ... -> finish, and
// stmmqr_factorize_device = all of it with its own recovery.  What a pass can end as and what each driver does about it is the pure
// policy of stmmqr_recover.h (P.rec); this file asks it and carries out the answer.  The steps themselves are run by stmmqr_run.cpp.
//
// There is NO CPU fallback in this file: every numeric operation is a kernel of the stmmqr_*.hip translation units.
#include "stmmqr_plan.h"

using recover::Action;
using recover::Outcome;

namespace {

// ------------------------------------------------------------------------------------------------
// the level-batched schedule (device resident inputs -> device resident factors)
// ------------------------------------------------------------------------------------------------
// State every factorization starts from (issued by stmmqr_factorize_begin, BEFORE any stmmqr_plan_import_front of the
// phased interface: an imported front's fm / rank / cm must survive until its parent assembles it).
int reset_factorization(stmmqr_plan &P)
{
    hipStream_t st = P.stream;
    LCHK(stm_ensure_arenas(P));
    // (with slab recycling every front's slab is zeroed when the front starts: k_zero_slabs in prep)
    if (!P.sch.recycle) HIPCHK(hipMemsetAsync(P.d_F.p, 0, (size_t)P.sch.farena * sizeof(double), st));
    HIPCHK(hipMemsetAsync(P.d_rhtop.p, 0, 2 * sizeof(long long), st));
    HIPCHK(hipMemsetAsync(P.d_Rdead.p, 0, (size_t)std::max(1L, P.n), st));
    HIPCHK(hipMemsetAsync(P.d_fnum.p, 0, (size_t)std::max(1L, P.nf) * sizeof(FrontNum), st));
    // (tickets are back at zero after every launch unless a wait ran out; the flags carry step numbers)
    HIPCHK(hipMemsetAsync(P.d_wcnt.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wcnt2.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wflag.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wflag2.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_abort.p, 0, 4 * sizeof(int), st));
    LCHK(stm_launch_sigma(P.d_Ax.p, (int)P.anz, P.d_amax.p, P.d_sig.p, st));
    LCHK(stm_launch_gather_sx(P.d_Ax.p, P.d_smap.p, P.d_Sx.p, (int)P.anz, st));
    P.stats.nlaunch += 6;
    return 0;
}

// Recovery of ONE group of the phased interface after a bounded panel wait ran out in it: everything its fronts wrote is
// put back to the state reset_factorization left (fronts of other groups and imported fronts are not touched).
int reset_group(stmmqr_plan &P, int grp)
{
    hipStream_t st = P.stream;
    const FrontNum zero = FrontNum();
    for (long f = 0; f < P.nf; f++) {
        if (P.group[f] != grp) continue;
        const FrontSym &s = P.sch.fs[f];
        HIPCHK(hipMemsetAsync(P.d_F.p + s.foff, 0, (size_t)s.ld * (size_t)s.fn * sizeof(double), st));
        HIPCHK(hipMemcpyAsync(P.d_fnum.p + f, &zero, sizeof zero, hipMemcpyHostToDevice, st));
        if (s.fp > 0) HIPCHK(hipMemsetAsync(P.d_Rdead.p + s.col1, 0, (size_t)s.fp, st));
    }
    HIPCHK(hipMemsetAsync(P.d_wcnt.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wcnt2.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wflag.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wflag2.p, 0, P.wcnt_n * sizeof(int), st));
    // abort[0..1] only: [3], a refused message of the subtree exchange, stays, and [2] goes back to what the groups before this one
    // left (recover::after_group: a front of an EARLIER group that outlived its cut schedule must still be reported at finish, while a
    // front of this group that the wait left unfinished is not such a front -- the rerun raises [2] again if it is one)
    HIPCHK(hipMemsetAsync(P.d_abort.p, 0, 2 * sizeof(int), st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(P.d_abort.p + 2), P.rec.abort2_before, 1, st));
    // slab recycling: a recycling plan holds the whole tree in this one group, and the aborted attempt has staged packed blocks behind
    // the arena's bump pointer; the rerun stages every block again, so the pointer (and the overflow word) go back to zero -- otherwise
    // the second set lands behind the first and overflows an arena that holds the estimate + 12.5 %
    if (P.sch.recycle) HIPCHK(hipMemsetAsync(P.d_rhtop.p, 0, 2 * sizeof(long long), st));
    HIPCHK(hipStreamSynchronize(st));                       // (`zero` lives on this stack frame)
    return 0;
}

// The schedule rebuilt on the plan's own grouping from P.rec (the full schedule, a larger arena, the cut one on or off): what every
// REBUILD of the recovery policy comes to.  P.group holds the group ids only; the shared fronts get their STMMQR_GROUP_SHARED bit
// back, or stmmqr_plan_set_groups would take them for fronts of this rank alone.  (A failed finish leaves P.begun set.)
int rebuild_schedule(stmmqr_plan &P)
{
    P.begun = false;
    std::vector<int> grp(P.group.begin(), P.group.end());
    for (size_t f = 0; f < grp.size(); f++) if (f < P.shared.size() && P.shared[f]) grp[f] |= STMMQR_GROUP_SHARED;
    return stmmqr_plan_set_groups(&P, grp.data());
}

int factorize_begin(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai, const double *Ax, int ax_on_device, double tol,
                    stm_long ntol, bool whole_call)
{
    if (!plan || !Ax) return fail(STMMQR_ERR_INVALID, "null plan / values");
    stmmqr_plan &P = *plan;
    HIPCHK(hipSetDevice(P.device));
    if (Ap && Ai) PASS(stm_set_pattern(P, Ap, Ai));
    if (!P.pattern_set) return fail(STMMQR_ERR_INVALID, "pattern of A was never given");
    if (!P.keep_h)
        for (long f = 0; f < P.nf; f++)
            if (P.group[f] != 0) return fail(STMMQR_ERR_INVALID, "a plan without H (keepH = 0) takes one group only");
    // phased use (begin / group / finish by the caller) has no loop around the factorization: what the last finish asked of the
    // schedule happens here (the whole call has acted on it in its own loop)
    if (!whole_call && recover::at_phased_begin(P.rec, P.sch.early_end, P.sch.recycle) == Action::REBUILD) PASS(rebuild_schedule(P));
    P.rec.last = Outcome::DONE;
    const double host_ms_plan = P.stats.ms_host;
    P.stats = stmmqr_stats();
    P.stats.ms_host = host_ms_plan;
    P.factored = false;
    P.res.new_factorization();
    P.evused = 0;
    P.begun = true;
    P.first_group = true;
    P.rec.abort2_before = 0;                                   // (reset_factorization clears abort[])
    if (!P.do_rank) tol = -1;                                  // SparseQR_factorize.c:285-289
    P.last_tol = tol; P.last_ntol = ntol;
    hipStream_t st = P.stream;
    HIPCHK(hipEventRecord(P.ev[0], st));
    if (P.anz > 0) {
        HIPCHK(hipMemcpyAsync(P.d_Ax.p, Ax, (size_t)P.anz * sizeof(double),
                              ax_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipEventRecord(P.ev[1], st));
    return reset_factorization(P);
}

// The step schedule of group 0 as a hipGraph, captured once per plan and per everything that travels in the kernel arguments or
// decides what is launched: (tol, ntol, debug mask), the schedule generation (set_groups rebuilds the lists and may move the
// workspaces) and the run-time options.  On return P.graph.exec is the graph to launch and the host statistics of one run of the
// schedule are added (by the capture itself, or from what the capture counted).
int ensure_graph(stmmqr_plan &P)
{
    const DevCtx c = P.ctx();
    // (everything stm_run_schedule reads at capture time and that decides WHAT is launched or travels in the kernel arguments:
    //  the knobs of the environment as the very struct it reads them into, the run-time options incl. pair_update, STMMQR_TUNE)
    const knobs::RunKnobs rk = knobs::RunKnobs::read();
    unsigned long long optkey = rk.key();
    for (long long v : {(long long)g_opt.lookahead, (long long)g_opt.split_update, (long long)g_opt.fused_update, (long long)g_opt.pair_update,
                        (long long)P.serial_panels, (long long)c.tune, (long long)P.keep_h})
        optkey = knobs::fold(optkey, (unsigned long long)v);
    const stmmqr_plan::Graph::Key key{c.tol, c.ntol, c.dbg, optkey, P.sched_gen};
    if (P.graph.exec && P.graph.key == key) {
        // (the statistics stm_run_schedule accumulates on the host)
        P.stats.nlaunch += P.graph.nlaunch;
        P.stats.nlevels += (long)P.sch.glevels[0].size();
        P.stats.nsteps += (long)P.sch.gsteps[0].size();
        return 0;
    }
    P.graph.clear();
    // everything stm_run_schedule creates lazily is created BEFORE the capture: the device's side stream (device
    // properties, a CU-masked stream, an atexit handler) and the per-step events of the look-ahead
    if (g_opt.lookahead && !P.serial_panels && P.sch.gsteps[0].size() > 1) {
        if (!P.side) P.side = stm_side_stream_for(P.device);
        PASS(stm_ensure_la_events(P, P.sch.gsteps[0].size(), rk));
    }
    const long nl0 = P.stats.nlaunch;
    hipGraph_t gph = nullptr;
    // the side stream is shared by the plans of a device: captures are serialised against each other (a plan that
    // factorizes without a graph while another one captures is the caller's to avoid, as for any shared stream)
    static std::mutex capture_mu;
    std::lock_guard<std::mutex> lock(capture_mu);
    HIPCHK(hipStreamBeginCapture(P.stream, hipStreamCaptureModeThreadLocal));
    const int e = stm_run_schedule(P, false, 0, nullptr);
    const hipError_t ce = hipStreamEndCapture(P.stream, &gph);
    if (e) { if (gph) (void)hipGraphDestroy(gph); return e; }
    HIPCHK(ce);
    HIPCHK(hipGraphInstantiate(&P.graph.exec, gph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(gph);
    P.graph.key = key;
    P.graph.nlaunch = P.stats.nlaunch - nl0;
    return 0;
}

int factorize_group(stmmqr_plan *plan, int group, int detail, bool whole_call)
{
    if (!plan || !plan->begun) return fail(STMMQR_ERR_INVALID, "stmmqr_factorize_begin was not called");
    stmmqr_plan &P = *plan;
    HIPCHK(hipSetDevice(P.device));
    const bool recoverable = recover::group_retry_applies(whole_call, P.serial_panels);
    const bool graph_ok = g_opt.use_graph && !detail && group == 0 && P.first_group && !knobs::on(knobs::K_DUMPLV);
    int e = 0;
    if (graph_ok) {
        PASS(ensure_graph(P));
        HIPCHK(hipGraphLaunch(P.graph.exec, P.stream));
    } else
        e = stm_run_schedule(P, detail != 0, group, nullptr);
    // Phased use (begin / group / finish called by the host: the sharded path): a bounded panel wait that ran out is found
    // HERE and the group is run again with one-workgroup panels (no inter-workgroup waits), exactly as
    // stmmqr_factorize_device does for the whole factorization -- the other groups and the imported fronts are not touched.
    if (!e && recoverable) {
        // (eight bytes: the kernels raise abort[1] beside the front's own perr -- not a copy of every FrontNum per phase -- and
        //  abort[2], which the host keeps as it stands after every group that needs no rerun)
        int flags[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(flags, P.d_abort.p + 1, 2 * sizeof(int), hipMemcpyDeviceToHost, P.stream));
        HIPCHK(hipStreamSynchronize(P.stream));
        if (recover::after_group(P.rec, flags[0] != 0, flags[1])) {
            if (g_opt.verbose) fprintf(stderr, "[stmmqr_hip] a panel wait ran out in group %d: running it again with one-workgroup panels\n", group);
            P.stats.retries++;
            e = reset_group(P, group);
            P.serial_panels = true;
            if (!e) e = stm_run_schedule(P, detail != 0, group, nullptr);
            P.serial_panels = false;
            if (!e) {
                int abort2 = 0;
                HIPCHK(hipMemcpyAsync(&abort2, P.d_abort.p + 2, sizeof(int), hipMemcpyDeviceToHost, P.stream));
                HIPCHK(hipStreamSynchronize(P.stream));
                recover::after_group_rerun(P.rec, abort2);
            }
        }
    }
    P.first_group = false;
    return e;
}

// ---- the steps of stmmqr_factorize_finish ----
// What the pass ended as, from the four facts on the device: abort[1..3], the fronts' own perr (the per-front numeric summary comes
// to the host here: flops, ranks, and which panel chain gave up waiting) and the pack's overflow word.
int read_outcome(stmmqr_plan &P, bool overflow, Outcome &o)
{
    int hard[3] = {0, 0, 0};                                  // abort[1]: a bounded wait ran out; [2]: a front outlived its schedule; [3]: a refused message
    HIPCHK(hipMemcpyAsync(hard, P.d_abort.p + 1, 3 * sizeof(int), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    P.h_fnum.resize((size_t)std::max(1L, P.nf));
    if (P.nf > 0)
        HIPCHK(hipMemcpy(P.h_fnum.data(), P.d_fnum.p, (size_t)P.nf * sizeof(FrontNum), hipMemcpyDeviceToHost));
    bool perr = hard[0] != 0;
    for (long f = 0; f < P.nf; f++)
        if (P.group[f] >= 0) perr = perr || P.h_fnum[f].perr;          // (< 0: factorized elsewhere)
    o = recover::classify(hard[2] != 0, perr, hard[1] != 0, overflow);
    return 0;
}

// A failed pass: the plan notes it (the next begin, the whole call's loop or stmmqr_plan_set_early_end act on it) and the caller
// gets the error.  P.begun stays set.  (evused: its only reader is a finish that succeeds, and begin zeroes it before the next one.)
int report_failure(stmmqr_plan &P, Outcome o)
{
    recover::record(P.rec, o);
    P.evused = 0;
    switch (o) {
        case Outcome::REFUSED_MESSAGE:
            return fail(STMMQR_ERR_DEVICE, "a contribution block received from another rank does not fit its front's symbolic bounds");
        case Outcome::WAIT_RAN_OUT:
            return fail(STMMQR_ERR_DEVICE, "a panel workgroup gave up waiting for its neighbours (device shared with another job?)");
        case Outcome::OUTLIVED_SCHEDULE:
            // (rank-deficient fronts: more rows reached a front than the full-rank estimate its schedule was cut to)
            return fail(STMMQR_ERR_RESCHEDULE, "a front was not finished by its last scheduled panel (the schedule is rebuilt with every panel)");
        default:
            return fail(STMMQR_ERR_OUT_OF_MEMORY, "the packed factors exceed the R+H arena of the slab recycling");
    }
}

// stats.ms_*: the plan's fixed events and, of a detail run, one event pair per launch category and step
int times_from_events(stmmqr_plan &P)
{
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, P.ev[0], P.ev[1])); P.stats.ms_h2d = ms;
    HIPCHK(hipEventElapsedTime(&ms, P.ev[1], P.ev[5])); P.stats.ms_total = ms;
    HIPCHK(hipEventElapsedTime(&ms, P.ev[4], P.ev[5])); P.stats.ms_pack += ms;
    std::vector<float> pair_ms(P.evused, 0.f);
    for (size_t q = 0; q < P.evused; q++) {
        float &t = pair_ms[q];
        HIPCHK(hipEventElapsedTime(&t, P.evpairs[q].a, P.evpairs[q].b));
        switch (P.evpairs[q].cat) {
            case 0: P.stats.ms_assemble += t; break;
            case 1: P.stats.ms_front += t; P.stats.ms_small += t; break;
            case 2: P.stats.ms_front += t; P.stats.ms_panel += t; P.stats.npanel_launch++; break;
            case 3: P.stats.ms_front += t; P.stats.ms_update += t; P.stats.nupdate_launch++; break;
            default: P.stats.ms_pack += t; break;
        }
    }
    stm_diag_dump_steps(P, pair_ms);
    P.evused = 0;
    return 0;
}

// rank, flops and the byte counts of the roofline, summed over the fronts this plan factorized
void sums_over_fronts(stmmqr_plan &P)
{
    double flops = 0, bytes_asm = 0, bytes_pack = 0, fl_upd = 0, fl_upd_pair = 0;
    long rank = 0;
    for (long f = 0; f < P.nf; f++) {
        if (P.group[f] < 0) continue;                  // factorized elsewhere
        const FrontNum &nm = P.h_fnum[f];
        const FrontSym &s = P.sch.fs[f];
        flops += nm.flops;
        fl_upd += nm.flops_upd;
        if ((size_t)f < P.sch.pair_front.size() && P.sch.pair_front[f]) fl_upd_pair += nm.flops_upd;
        rank += nm.rank;
        const double cn = s.fn - s.fp, cm = nm.cm;
        const double csize = cm * (cm + 1) / 2 + cm * (cn - cm);
        bytes_asm += 8.0 * ((double)nm.fm * s.fn) + 8.0 * csize;   // F first write + child C read (as a child)
        bytes_pack += 16.0 * (csize + (double)nm.rsize);
    }
    bytes_asm += 8.0 * (double)P.anz + P.bytes_assemble_idx;
    P.rank = rank;
    P.stats.flops = flops;
    P.stats.flops_update = fl_upd;
    P.stats.flops_update_pair = fl_upd_pair;
    P.stats.bytes_assemble = bytes_asm;
    P.stats.bytes_pack = bytes_pack;
    P.stats.device_bytes = P.device_bytes();
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int stmmqr_factorize_begin(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                           int ax_on_device, double tol, stm_long ntol)
{
    return factorize_begin(plan, Ap, Ai, Ax, ax_on_device, tol, ntol, false);
}

int stmmqr_factorize_group(stmmqr_plan *plan, int group, int detail) { return factorize_group(plan, group, detail, false); }

int stmmqr_factorize_finish(stmmqr_plan *plan, stmmqr_stats *stats)
{
    if (!plan || !plan->begun) return fail(STMMQR_ERR_INVALID, "stmmqr_factorize_begin was not called");
    stmmqr_plan &P = *plan;
    HIPCHK(hipSetDevice(P.device));
    HIPCHK(hipEventRecord(P.ev[4], P.stream));
    bool overflow = false;
    PASS(stm_run_pack(P, overflow));
    HIPCHK(hipEventRecord(P.ev[5], P.stream));
    Outcome o = Outcome::DONE;
    PASS(read_outcome(P, overflow, o));
    stm_diag_early_fronts(P);
    if (o != Outcome::DONE) return report_failure(P, o);
    PASS(times_from_events(P));
    sums_over_fronts(P);
    const int dbg = (int)knobs::num(knobs::K_DBG);
    PASS(stm_diag_panel_timeline(P, dbg));
    PASS(stm_diag_block0_launch(P, dbg));
    PASS(stm_diag_pipeline_counters(P, dbg));
    stm_diag_memdump(P);
    P.factored = true;
    P.begun = false;
    if (stats) *stats = P.stats;
    return 0;
}

int stmmqr_factorize_device(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                            int ax_on_device, double tol, stm_long ntol, stmmqr_stats *stats)
{
    if (!plan) return fail(STMMQR_ERR_INVALID, "null plan");
    const bool detail = g_opt.verbose >= 2 || (stats && stats->nlaunch == -1);
    // The multi-workgroup panel kernels wait for each other inside a launch (bounded).  Should such a wait ever run out
    // (the workgroups of a launch are not guaranteed to run together: a GPU shared with another job), the factorization is
    // not lost: it is run once more with every panel factorized by ONE workgroup (dev_panel: no inter-workgroup wait
    // anywhere), slower but independent of co-residency.  An arena that overflowed or a cut schedule that a front outlived is
    // rebuilt and both attempts start over (recover::after_pass; it ends: stmmqr_recover.h).
    recover::WholeCall w;
    for (;;) {
        plan->serial_panels = w.serial;
        int e = factorize_begin(plan, Ap, Ai, Ax, ax_on_device, tol, ntol, true);
        if (!e) plan->stats.retries = w.retries();               // (visible in stmmqr_stats: bench.py asserts 0)
        if (!e) plan->stats.reschedules = w.reschedules;
        for (int g = 0; g < (int)plan->sch.glevels.size() && !e; g++) e = factorize_group(plan, g, detail, true);
        Outcome o = Outcome::DONE;
        if (!e && (e = stmmqr_factorize_finish(plan, stats)) != 0) o = plan->rec.last;
        const Action a = recover::after_pass(plan->rec, w, o, plan->sch.recycle);
        plan->serial_panels = false;                 // (also before a rebuild, which reads it nowhere: the next pass sets it anew)
        if (a == Action::RETURN) return e;
        if (g_opt.verbose) {
            if (o == Outcome::ARENA_OVERFLOW)
                // sized from the full-rank estimate -> once more with the hard bound (QRsym->maxstack); at the hard bound (never seen) ->
                // once more with every front in a slab of its own and the packed blocks placed at the end, as sharded plans always run
                fprintf(stderr, "[stmmqr_hip] R+H arena overflow: factorizing again %s\n", plan->rec.overflowed ? "without slab recycling" : "with the arena at its hard bound");
            else if (o == Outcome::OUTLIVED_SCHEDULE)
                fprintf(stderr, "[stmmqr_hip] a front outlived its schedule (rank-deficient fronts): factorizing again on the full schedule\n");
            else
                fprintf(stderr, "[stmmqr_hip] a panel wait ran out: factorizing again with one-workgroup panels\n");
        }
        if (a == Action::REBUILD) PASS(rebuild_schedule(*plan));
        else if (stats && detail) stats->nlaunch = -1;
        Ap = nullptr; Ai = nullptr;                  // (the pattern is set; begin uploads / copies the values again)
    }
}

int stmmqr_plan_set_early_end(stmmqr_plan *plan, int mode)
{
    if (!plan) return fail(STMMQR_ERR_INVALID, "null plan");
    stmmqr_plan &P = *plan;
    if (!recover::set_early_end(P.rec, P.begun, mode))
        return fail(STMMQR_ERR_INVALID, "stmmqr_plan_set_early_end between factorize_begin and factorize_finish");
    return rebuild_schedule(P);
}

int stmmqr_factorize_arrays(const stmmqr_symbolic_view *sym, const stm_long *Ap, const stm_long *Ai,
                            const double *Ax, double tol, stm_long ntol, double *Stack, stm_long stack_cap,
                            stm_long *Rblock_off, char *Rdead, stm_long *HStair, double *HTau, stm_long *Hii,
                            stm_long *HPinv, stm_long *Hm, stm_long *Hr, stm_long *scalars, stmmqr_stats *stats)
{
    int st = 0;
    stmmqr_plan *P = stmmqr_plan_create(sym, -1, &st);
    if (!P) return st;
    st = stmmqr_factorize_device(P, Ap, Ai, Ax, 0, tol, ntol, stats);
    if (!st && Stack && P->rh_total > stack_cap) st = fail(STMMQR_ERR_INVALID, "Stack buffer too small");
    if (!st) st = stmmqr_plan_download(P, Stack, Rblock_off, Rdead, HStair, HTau, Hii, HPinv, Hm, Hr, scalars, stats);
    stmmqr_plan_destroy(P);
    return st;
}

}  // extern "C"
