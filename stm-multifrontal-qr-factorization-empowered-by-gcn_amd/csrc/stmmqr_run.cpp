// stmmqr_run.cpp -- the step scheduler: runs the timeline of one front group (stmmqr_schedule.cpp built it) as kernel launches,
// and the pack pass that ends a factorization.  Device resident inputs -> device resident factors.
//
// Reference counterpart (paths relative to the reference's STMMQR directory): qr_kernel's per-front loop + qr_multithreads,
// src/qr/SparseQR_factorize.c:791-985, SparseQR_multithreads.c:14-115 (tree parallelism re-cast as step-batched launches on a
// HIP stream: the fronts in flight at a step are independent, so a step = a few batched kernel launches; no blocking waits
// inside workers, cf. SURVEY.md 3.3 deadlock note).
//
// One Run object holds what the launches of a run share; four drivers walk the steps:
//   run_request     one piece of one step (stmmqr_factorize_step: StepReq)
//   run_serial      every step in order on the plan's stream
//   run_lookahead   options.lookahead = 1: the update beyond block 0, the packing and the next assembly on the side stream
//   run_passengers  options.lookahead = 2 (default): one stream, the update beyond block 0 rides on the chain's own launches
// Every kernel does exactly what it does in the serial order: same bits every way.
#include "stmmqr_plan.h"

namespace {

// detail timing: each category is bracketed with an event pair from the pool; no host synchronisation here
enum { CAT_ASM = 0, CAT_SMALL = 1, CAT_PANEL = 2, CAT_UPD = 3, CAT_CPK = 4 };

// the riders of a pending step Q as the panel / update launchers take them: the k_upd_c launch of its update beyond block 0
#define RIDERS_OF(Q) L0 + (Q).act_off, L0 + (Q).plist_off, (Q).n_norm, 1, (Q).maxcb - 1, (Q).maxsl, P.d_Wp2.p, P.d_wlists.p + (Q).wp_off

struct Run {
    stmmqr_plan &P;
    const bool detail;
    const int grp;
    const knobs::RunKnobs k = knobs::RunKnobs::read();
    hipStream_t st = P.stream;
    DevCtx c = P.ctx(k.dbg);
    const int *L0 = P.d_lists.p;
    const std::vector<Step> &SV = P.sch.gsteps[grp];
    long nlaunch = 0;
    int cur_step = 0;
    const Step *pend = nullptr;                                // passengers: the step whose k_upd_c beyond block 0 is still due

    const int *act(const Step &S) const { return L0 + S.act_off; }
    const int *pl(const Step &S) const { return L0 + S.plist_off; }
    const FrontSym &front(const Step &S, int i) const { return P.sch.fs[P.sch.lists[S.act_off + i]]; }
    int panel(const Step &S, int i) const { return P.sch.lists[S.plist_off + i]; }
    // the epoch of a step's hand-offs through global memory (k_upd_f, k_upd_b0w): the step number of the group
    int epoch(const Step &S) const { return (int)(&S - SV.data()) + 1 + grp * (1 << 20); }
    // tiles (256 x 32) of the update beyond block 0 of the step's normal fronts (expected rows, not the bound)
    long tiles_beyond_b0(const Step &S) const
    {
        long tiles = 0;
        for (int i = 0; i < S.n_norm; i++) {
            const int ncb = stm_upd_ncb(front(S, i), panel(S, i));
            if (ncb > 1) tiles += (long)(ncb - 1) * ((stm_panel_rows_est(front(S, i), panel(S, i)) + STM_UPD_SLAB - 1) / STM_UPD_SLAB);
        }
        return tiles;
    }
    // workgroups of the step's fused T + block 0 launch: two per row slab, counted with the row BOUND of every front (a rank-
    // deficient front can have more rows than its estimate).  They wait for each other (bounded): all must be resident at once.
    long fused_wgs(const Step &S) const
    {
        long wgs = 0;
        for (int i = 0; i < S.n_norm; i++) wgs += 2L * stm_upd_nsl(front(S, i));
        return wgs;
    }
    // the rows the tallest panel of the step is expected to reach (not the bound)
    int panel_rows_max(const Step &S) const
    {
        int rows = 0;
        for (int i = 0; i < S.n_act; i++) rows = std::max(rows, stm_panel_rows_est(front(S, i), panel(S, i)));
        return rows;
    }
    bool packs(const Step &S) const { return S.n_cpk > 0 || (P.sch.recycle && S.n_rhp > 0); }

    template <class F> int timed(int cat, F &&fn)
    {
        if (!detail) return fn();
        if (P.evused == P.evpairs.size()) {
            stmmqr_plan::EvPair q = {nullptr, nullptr, 0, 0};
            HIPCHK(hipEventCreate(&q.a));
            HIPCHK(hipEventCreate(&q.b));
            P.evpairs.push_back(q);
        }
        stmmqr_plan::EvPair &q = P.evpairs[P.evused++];
        q.cat = cat;
        q.step = cur_step;
        HIPCHK(hipEventRecord(q.a, st));
        PASS(fn());
        HIPCHK(hipEventRecord(q.b, st));
        return 0;
    }

    // prep(t): set up + assemble the fronts that start at step t, factorize the small ones among them (whole, one launch)
    int prep(const Step &S, hipStream_t q)
    {
        const int *starting = L0 + S.start_off;
        if (S.n_start > 0) {
            PASS(timed(CAT_ASM, [&]() -> int {
                if (P.sch.recycle) { LCHK(stm_launch_zero_slabs(c, starting, S.n_start, S.asm_maxparts, q)); nlaunch++; }
                LCHK(stm_launch_setup(c, starting, S.n_start, q));
                LCHK(stm_launch_assemble(c, starting, L0 + S.asm_parts_off, S.n_start, S.asm_maxparts, q));
                return 0;
            }));
            nlaunch += 2;
        }
        if (S.n_small > 0) {
            PASS(timed(CAT_SMALL, [&]() -> int {
                LCHK(stm_launch_front_wg(c, starting, S.n_small, S.lds_small, q));
                return 0;
            }));
            nlaunch++;
        }
        return 0;
    }

    // which kernel takes a panel is a property of the front (stm_use_ca); a step with both kinds gets both launches (each
    // kernel skips the other's fronts).  A front with trailing columns leaves T to its update (dev_tall_group /
    // k_panel_ca), one at its last panel to k_cpack.
    int panels(const Step &S)
    {
        return timed(CAT_PANEL, [&]() -> int {
            if (S.nca_use && !P.serial_panels) { LCHK(stm_launch_panel_ca(c, act(S), pl(S), S.n_act, S.nca, 1, st)); nlaunch++; }
            if (S.npipe_use || P.serial_panels) {
                const int lds = (P.serial_panels || (c.dbg & (64 | 256))) ? S.lds_big : S.lds_plan;
                LCHK(stm_launch_panel(c, act(S), pl(S), S.n_act, S.nsub, 1, lds, st));
                nlaunch++;
            }
            return 0;
        });
    }

    // trailing update of the column blocks [cb0, cb0 + ncb) of every front in flight (block 0 = the columns of its next
    // panel); gram: the T factors the panel kernels left to the update are built in this launch (row-parallel form; the
    // one-workgroup form builds T in every workgroup)
    int update(const Step &S, int cb0, int ncb, bool gram, double *Wp, hipStream_t q)
    {
        const bool split = S.split && g_opt.split_update;
        const bool whole = (cb0 == 0 && gram);                 // the step's whole update: the pair-update classes too
        const bool pairs = whole && S.n_sweep() > 0;
        if (S.n_norm <= 0 || (ncb <= 0 && !(gram && split))) {
            if (!pairs) return 0;
        }
        const int *act = this->act(S), *pl = this->pl(S);
        const bool main_ws = (Wp == P.d_Wp.p);
        int *wcnt = main_ws ? P.d_wcnt.p : P.d_wcnt2.p;
        const long long *wl = P.d_wlists.p + S.wp_off;
        return timed(CAT_UPD, [&]() -> int {
            if (S.n_norm > 0 && (ncb > 0 || (gram && split))) {
                if (split && g_opt.fused_update && S.maxsl <= 256 && !P.serial_panels && c.cbskip == 0) {
                    // one launch: C is read and written once (k_upd_f)
                    LCHK(stm_launch_update_fused(c, act, pl, S.n_norm, cb0, ncb, S.maxsl, Wp, wl, wcnt,
                                                 main_ws ? P.d_wflag.p : P.d_wflag2.p, epoch(S), gram ? 1 : 0, q));
                    nlaunch++;
                } else if (split) {
                    LCHK(stm_launch_update_split(c, act, pl, S.n_norm, cb0, ncb, S.maxsl, Wp, wl, wcnt, gram ? 1 : 0, q));
                    nlaunch += 2;
                } else {
                    LCHK(stm_launch_update(c, act, pl, S.n_norm, cb0, ncb, q));
                    nlaunch++;
                }
            }
            if (pairs) {
                // panel r of a sweep of w: column blocks 0 .. w-1-r (the columns of the next panels), T by the Gram block; after the
                // last one the w panels at once on everything beyond
                int o = S.n_norm;
                for (int r = 0; r < P.sch.sweep; r++) {
                    const int n = S.n_pk[r];
                    if (n <= 0) continue;
                    LCHK(stm_launch_update_split(c, act + o, pl + o, n, 0, P.sch.sweep - r, S.maxsl_pk[r], Wp, wl + o, wcnt, 1, q));
                    nlaunch += 2;
                    if (r == P.sch.sweep - 1) {
                        if (c.dbg & 65536)                     // tests: the sweep launches by front, with the front's own column blocks
                            for (int i = 0; i < n; i++)
                                fprintf(stderr, "[sweep launch] w %d step %d front %d panel %d ncbp %d nslf %d (launch: ncbp %d maxsl %d)\n", P.sch.sweep,
                                        cur_step, P.sch.lists[S.act_off + o + i], panel(S, o + i), stm_upd_ncb(front(S, o + i), panel(S, o + i)) - 1,
                                        stm_upd_nsl(front(S, o + i)), S.maxcbp_po, S.maxsl_pk[r]);
                        if (P.sch.sweep == 4) LCHK(stm_launch_update_quad(c, act + o, pl + o, n, S.maxcbp_po, S.maxsl_pk[r], Wp, wl + o, wcnt, q));
                        else LCHK(stm_launch_update_pair(c, act + o, pl + o, n, S.maxcbp_po, S.maxsl_pk[r], Wp, wl + o, wcnt, q));
                        nlaunch += 3;
                    }
                    o += n;
                }
            }
            return 0;
        });
    }

    // T and block 0 of a step's update in ONE launch (k_upd_f: the slab workgroups of the block meet through global memory; the
    // Gram block of the same launch builds T) -- the look-ahead chain panel(t) -> block 0 -> panel(t+1) then has one launch between
    // two panels instead of three (T, k_upd_w, k_upd_c).  Same bits as the other forms.
    int update_b0_fused(const Step &S, hipStream_t q)
    {
        nlaunch++;
        return timed(CAT_UPD, [&]() -> int {
            LCHK(stm_launch_update_fused(c, act(S), pl(S), S.n_norm, 0, 1, S.maxsl, P.d_Wp.p, P.d_wlists.p + S.wp_off, P.d_wcnt.p, P.d_wflag.p,
                                         epoch(S), 1, q));
            return 0;
        });
    }

    int post(const Step &S, hipStream_t q)
    {
        if (!packs(S)) return 0;
        return timed(CAT_CPK, [&]() -> int {
            if (S.n_cpk > 0) { LCHK(stm_launch_cpack(c, L0 + S.cpk_off, L0 + S.cpk_parts_off, S.n_cpk, S.cpk_maxparts, q)); nlaunch++; }
            if (P.sch.recycle && S.n_rhp > 0) {
                // slab recycling: the packed R+H blocks of the fronts that are finished now go to the arena (sizes and places on the
                // device: k_rh_count bumps the arena's pointer); their slabs are free from the next step on
                if (P.keep_h) {
                    LCHK(stm_launch_rh_count(c, L0 + S.rhp_off, S.n_rhp, q));
                    LCHK(stm_launch_rh_copy(c, L0 + S.rhp_off, L0 + S.rhp_parts_off, S.n_rhp, S.rhp_maxparts, P.d_RH.p, q));
                } else {
                    LCHK(stm_launch_r_count(c, L0 + S.rhp_off, S.n_rhp, q));
                    LCHK(stm_launch_r_copy(c, L0 + S.rhp_off, L0 + S.rhp_parts_off, S.n_rhp, S.rhp_maxparts, P.d_RH.p, q));
                }
                nlaunch += 2;
            }
            return 0;
        });
    }

    // ---- one requested step ---------------------------------------------------------------------------------------------------
    int run_request(const StepReq &req)
    {
        if (req.step < 0 || req.step >= (int)SV.size()) return fail(STMMQR_ERR_INVALID, "no such step in the group");
        const Step &S = SV[(size_t)req.step];
        cur_step = req.step;
        int e = 0;
        if (req.what & STMMQR_STEP_PREP) e = prep(S, st);
        if (!e && (req.what & STMMQR_STEP_PANEL) && S.n_act > 0) e = panels(S);
        if (!e && (req.what & (STMMQR_STEP_UPDATE | STMMQR_STEP_GRAM)) && S.n_act > 0) {
            if (S.n_sweep() > 0) return fail(STMMQR_ERR_INVALID, "pair-update fronts cannot be stepped (mark the front STMMQR_GROUP_SHARED)");
            int nmine = 0;
            if ((req.what & STMMQR_STEP_UPDATE) && req.cb_first >= 0 && req.cb_first < S.maxcb)
                nmine = (S.maxcb - req.cb_first + c.cbskip) / (1 + c.cbskip);
            if (req.cb_count >= 0) nmine = std::min(nmine, req.cb_count);
            e = update(S, std::max(0, req.cb_first), nmine, (req.what & STMMQR_STEP_GRAM) != 0, P.d_Wp.p, st);
        }
        if (!e && (req.what & STMMQR_STEP_POST)) e = post(S, st);
        P.stats.nlaunch += nlaunch;
        return e;
    }

    // ---- the serial order -----------------------------------------------------------------------------------------------------
    int run_serial()
    {
        for (const Step &S : SV) {
            cur_step = (int)(&S - SV.data());
            PASS(prep(S, st));
            if (S.n_act > 0) PASS(panels(S));
            if (S.n_act > 0) PASS(update(S, 0, S.maxcb, true, P.d_Wp.p, st));
            PASS(post(S, st));
        }
        return 0;
    }

    // ---- look-ahead on the side stream ----------------------------------------------------------------------------------------
    // T + block 0 of an offloaded step in ONE launch (update_b0_fused) where the step's panels are expected to reach at most
    // STMMQR_LA_FUSED_ROWS rows: one launch between two panels of the chain instead of three, and look-ahead then pays from
    // STMMQR_LA_MIN_FUSED tiles.  Measured: sme3Dc stand-in 87.2 -> 84.3 ms, default workload 121.4 -> 119.4-120.9; on the 7818-row
    // fronts of c5mini (31 slabs) the fused launch is the slower one (43.5 -> 48.9 ms).
    // Forward progress of that launch: what is guaranteed while the side stream fills the rest of the GPU are the reserved
    // compute units, two k_upd_f workgroups each (248 VGPRs).
    bool b0_fused(const Step &S) const
    {
        if (k.la_fused_rows <= 0 || !S.split || !g_opt.split_update || S.maxsl > 256 || S.n_sweep() > 0 || c.cbskip != 0) return false;
        return fused_wgs(S) <= 2 * k.side_reserve && panel_rows_max(S) <= k.la_fused_rows;
    }

    // a step goes to the side stream when the update beyond block 0 is worth two cross-stream hand-offs (STMMQR_LA_MIN) and when
    // the panel workgroups of the step fit the compute units the side stream leaves alone (a wide step fills the GPU with panel
    // workgroups by itself: STMMQR_LA_MAXPWG)
    bool worth_it(const Step &S) const
    {
        long pwg = 0;
        for (int i = 0; i < S.n_act; i++)
            pwg += stm_use_ca(front(S, i), panel(S, i), P.sch.plan_algo, P.sch.ca_min) ? stm_ca_slabs(front(S, i)) : stm_tall_launches(front(S, i), panel(S, i), P.sch.tall_min);
        return S.n_sweep() == 0 &&                                  // (pair-update steps stay on one stream)
               tiles_beyond_b0(S) >= (b0_fused(S) ? std::min(k.la_min, k.la_min_fused) : k.la_min) && pwg <= k.la_maxpwg;
    }

    bool any_step_worth_it() const
    {
        for (const Step &S : SV)
            if (S.n_act > 0 && S.maxcb > 1 && worth_it(S)) return true;
        return false;
    }

    // Look-ahead of depth one.  The chain  panel(t) -> update of block 0 (the next panel's columns) -> panel(t+1)
    // stays on the plan's stream; the rest of the update of step t, the packing of the fronts that ended at t and the
    // preparation of those that start at t+1 run beside it on the side stream:
    //   main:  [wait prep(t)]  panel(t)  T(t)  record main(t)  [wait side(t-1)]  update block 0
    //   side:  wait main(t)    pack(t)   prep(t+1)  record prep(t+1)   update blocks 1..  record side(t)
    // (side(t) needs the panel and its T only, not block 0: the side stream runs its updates back to back while the
    //  main stream alternates block 0 and the next panel.)
    int run_lookahead()
    {
        const size_t ns = SV.size();
        PASS(stm_ensure_la_events(P, ns, k));
        hipStream_t sd = P.side;
        long side_ev = -1;                                     // last side event the main stream has not waited for
        bool prep_on_side = false;                             // prep(t) was issued on the side stream during step t-1
        auto join_side = [&]() -> int {
            if (side_ev >= 0) { HIPCHK(hipStreamWaitEvent(st, P.ev_side[side_ev], 0)); side_ev = -1; }
            return 0;
        };
        for (size_t t = 0; t < ns; t++) {
            const Step &S = SV[t];
            if (prep_on_side) HIPCHK(hipStreamWaitEvent(st, P.ev_prep[t], 0));
            else {
                // (what a starting front assembles may have been packed on the side stream)
                if (S.n_start > 0) PASS(join_side());
                PASS(prep(S, st));
            }
            prep_on_side = false;
            if (S.n_act > 0) PASS(panels(S));
            // (early end: a front may end at a panel with trailing columns; its step is packed after the whole update)
            const bool offload = S.n_act > 0 && S.maxcb > 1 && worth_it(S) && !(P.sch.early_end && packs(S));
            if (!offload) {
                if (S.n_act > 0) {
                    PASS(join_side());
                    PASS(update(S, 0, S.maxcb, true, P.d_Wp.p, st));
                }
                PASS(post(S, st));
                continue;
            }
            if (b0_fused(S)) {
                PASS(join_side());
                PASS(update_b0_fused(S, st));                                                // T + block 0
                HIPCHK(hipEventRecord(P.ev_main[t], st));
            } else {
                PASS(update(S, 0, 0, true, P.d_Wp.p, st));                                   // T
                HIPCHK(hipEventRecord(P.ev_main[t], st));
                PASS(join_side());
                PASS(update(S, 0, 1, false, P.d_Wp.p, st));                                  // block 0
            }
            HIPCHK(hipStreamWaitEvent(sd, P.ev_main[t], 0));
            PASS(post(S, sd));
            if (t + 1 < ns && SV[t + 1].n_start > 0) {
                PASS(prep(SV[t + 1], sd));
                HIPCHK(hipEventRecord(P.ev_prep[t + 1], sd));
                prep_on_side = true;
            }
            PASS(update(S, 1, S.maxcb - 1, false, P.d_Wp2.p, sd));
            HIPCHK(hipEventRecord(P.ev_side[t], sd));
            side_ev = (long)t;
        }
        return join_side();                                        // join: the caller continues on `stream`
    }

    // ---- passenger launches ---------------------------------------------------------------------------------------------------
    // ONE stream, no events.  The chain stays  panel(t) -> T(t) + block 0 (one fused launch) -> panel(t+1); the two launches of the
    // update beyond block 0 ride on the chain's launches as extra workgroups behind the chain's own (k_upd_w of step t behind
    // T + block 0 of step t, k_upd_c of step t behind the panels of step t+1: stmmqr_*.hip, "Passenger launches").  A step takes
    // part when its update is the row-parallel form and every workgroup of its fused launch is resident at once (they wait for each
    // other, bounded: two per CU); any other step runs in the serial order after the riders of the step before it.

    // the riders that are due, as a launch of their own
    int flush_alone()
    {
        if (!pend) return 0;
        const Step &Q = *pend;
        pend = nullptr;
        LCHK(stm_launch_update_c(c, RIDERS_OF(Q), st));
        nlaunch++;
        return 0;
    }

    // the panels of step S, the riders of the step before behind them where a launch can take them
    int passenger_panels(const Step &S)
    {
        const int abl = k.pass_abl;
        if (S.nca_use && !S.npipe_use && pend && !(abl & 6) && k.ca_riders) {
            // (every panel of the step is Gram-based: the riders of the step before take THAT launch)
            const Step &Q = *pend;
            pend = nullptr;
            LCHK(stm_launch_panel_ca_pc(c, act(S), pl(S), S.n_act, S.nca, 1, RIDERS_OF(Q), st));
            nlaunch++;
        } else if (S.nca_use) { LCHK(stm_launch_panel_ca(c, act(S), pl(S), S.n_act, S.nca, 1, st)); nlaunch++; }
        if (!S.npipe_use) return flush_alone();
        const int lds = (c.dbg & (64 | 256)) ? S.lds_big : S.lds_plan;
        if (pend && (abl & 2)) pend = nullptr;
        if (pend) {
            // a rider has its CU to itself (the panel launch's registers and LDS): 2-3 x the time of k_upd_c's own launch
            // per tile.  Beyond pass_tiles tiles (a wide step of the lower tree levels) the riders would outlast any panel.
            const long tiles = tiles_beyond_b0(*pend);
            // (the panel launch they would ride on: ~25 us up to 512 rows, ~48 us up to 4096, ~72 us beyond)
            const int prow = panel_rows_max(S);
            const double panel_us = prow <= 512 ? 25.0 : prow <= 4096 ? 48.0 : 72.0;
            if (tiles > k.pass_tiles || (double)tiles > k.pass_k * panel_us) PASS(flush_alone());
        }
        if (pend && (abl & 4)) return passenger_panels_ablated(S, lds);
        if (pend) {
            const Step &Q = *pend;
            pend = nullptr;
            LCHK(stm_launch_panel_pc(c, act(S), pl(S), S.n_act, S.nsub, 1, lds, RIDERS_OF(Q), st));
        } else
            LCHK(stm_launch_panel(c, act(S), pl(S), S.n_act, S.nsub, 1, lds, st));
        nlaunch++;
        return 0;
    }

    // STMMQR_PASS_ABL & 4 (measurement): the riders as launches of their own, same order; & 8: behind an empty panel launch
    int passenger_panels_ablated(const Step &S, int lds)
    {
        LCHK(stm_launch_panel(c, act(S), pl(S), S.n_act, S.nsub, 1, lds, st));
        if (k.pass_abl & 8) {
            const Step &Q = *pend;
            pend = nullptr;
            LCHK(stm_launch_panel_pc(c, act(S), pl(S), -1, S.nsub, 1, lds, RIDERS_OF(Q), st));
        }
        PASS(flush_alone());
        nlaunch++;
        return 0;
    }

    // (pass_rows: 5120 until the riders of a step before Gram-based panels got a launch to ride on (k_panel_ca_pc) -- beyond
    //  ~5000 rows the one-launch block 0 is the slower form of T + block 0, but the riders no longer cost a launch of their
    //  own on the chain: c5mini 41.1 -> 37.0 ms, default 91.4 -> 90.9 at 8192 ... unlimited; 16384 = where the pair-update
    //  fronts begin, which never ride)
    bool rides(const Step &S) const
    {
        return S.split && S.n_sweep() == 0 && S.n_norm > 0 && S.maxcb > 1 && S.maxsl <= 256 && fused_wgs(S) <= k.pass_maxwg &&
               panel_rows_max(S) <= k.pass_rows && !g_opt.fused_update;
    }

    // T + block 0 of a riding step, its k_upd_w beyond block 0 behind them
    int passenger_block0(const Step &S)
    {
        const int abl = k.pass_abl;
        const long long *wl = P.d_wlists.p + S.wp_off;
        if (abl & 4) {
            LCHK(stm_launch_update_fw(c, act(S), pl(S), S.n_norm, 1, S.maxsl, P.d_Wp.p, wl, P.d_wcnt.p, P.d_wflag.p, epoch(S), P.d_Wp2.p, P.d_wcnt2.p, st));
            LCHK(stm_launch_update_w(c, act(S), pl(S), S.n_norm, 1, S.maxcb - 1, S.maxsl, P.d_Wp2.p, wl, P.d_wcnt2.p, st));
        } else
            LCHK(stm_launch_update_fw(c, act(S), pl(S), S.n_norm, (abl & 1) ? 1 : S.maxcb, S.maxsl, P.d_Wp.p, wl, P.d_wcnt.p, P.d_wflag.p, epoch(S),
                                      P.d_Wp2.p, P.d_wcnt2.p, st));
        nlaunch++;
        return 0;
    }

    int run_passengers()
    {
        for (const Step &S : SV) {
            cur_step = (int)(&S - SV.data());
            PASS(prep(S, st));
            if (S.n_act > 0) {
                PASS(passenger_panels(S));
                if (rides(S)) {
                    PASS(passenger_block0(S));
                    pend = &S;
                } else
                    PASS(update(S, 0, S.maxcb, true, P.d_Wp.p, st));
            }
            // (a front that ends at a panel with trailing columns -- FrontSym::nsched -- is packed only after the riders of that update)
            if (pend && P.sch.early_end && packs(S)) PASS(flush_alone());
            PASS(post(S, st));
        }
        return flush_alone();
    }
};

#undef RIDERS_OF

}  // namespace

// Events of the look-ahead schedule order two streams of ONE device: no timing, and no system-scope fence when they are recorded
// (the host never inspects them; the kernels' own agent-scope release / acquire at their boundaries is what the other stream needs).
// STMMQR_LA_SYSFENCE=1 brings the default (system-scope) events back.  One of each kind per timeline step, created before the
// run that needs them (and before a capture: nothing is created inside one).
int stm_ensure_la_events(stmmqr_plan &P, size_t nsteps, const knobs::RunKnobs &k)
{
    const unsigned flags = hipEventDisableTiming | (k.la_sysfence ? 0u : (unsigned)hipEventDisableSystemFence);
    for (auto *v : {&P.ev_main, &P.ev_prep, &P.ev_side})
        while (v->size() < nsteps + 1) {
            hipEvent_t ev = nullptr;
            HIPCHK(hipEventCreateWithFlags(&ev, flags));
            v->push_back(ev);
        }
    return 0;
}

int stm_run_schedule(stmmqr_plan &P, bool detail, int grp, const StepReq *req)
{
    if (grp < 0 || grp >= (int)P.sch.gsteps.size()) return fail(STMMQR_ERR_INVALID, "no such front group");
    Run R{P, detail, grp};
    if (req) {
        R.c.cbskip = std::max(1, req->cb_stride) - 1;
        return R.run_request(*req);
    }
    // Passenger launches take the steps when nothing asks for the serial order; look-ahead needs some step whose update is
    // worth the side stream -- small matrices never touch it.
    const bool pass = g_opt.lookahead >= 2 && !detail && !P.serial_panels && R.c.cbskip == 0 && g_opt.split_update && !(R.c.dbg & 512) &&
                      R.k.passengers;
    const bool la = g_opt.lookahead && !pass && !detail && !P.serial_panels && R.SV.size() > 1 && R.any_step_worth_it();
    PASS(pass ? R.run_passengers() : la ? R.run_lookahead() : R.run_serial());
    P.stats.nlaunch += R.nlaunch;
    P.stats.nlevels += (long)P.sch.glevels[grp].size();
    P.stats.nsteps += (long)P.sch.gsteps[grp].size();
    return 0;
}

// The end of a factorization: sizes and places of the packed R+H blocks in the reference's layout.
// overflow: the slab recycling's arena did not hold every packed block (k_cpack staged nothing past it); the caller decides what
// that means (stmmqr_factorize_finish: a schedule or wait failure explains it, otherwise the arena grows)
int stm_run_pack(stmmqr_plan &P, bool &overflow)
{
    overflow = false;
    hipStream_t st = P.stream;
    const DevCtx c = P.ctx();
    const int *L0 = P.d_lists.p;
    if (P.sch.recycle) {
        // the blocks were staged front by front (Run::post); what is left are the kept fronts' column offsets, the
        // reference's layout of all blocks (Post order: d_fin, used by the download) and the check that the arena held everything
        std::vector<int> kl;
        for (long f = 0; f < P.nf; f++) if (P.sch.kept[(size_t)f]) kl.push_back((int)f);
        if (!kl.empty()) {
            DevBuf<int> d_kl;
            LCHK(d_kl.upload(kl, st));
            DevCtx ck = c;
            ck.rh_top = nullptr;                                  // (no place in the arena: packed on the fly by the download)
            LCHK(P.keep_h ? stm_launch_rh_count(ck, d_kl.p, (int)kl.size(), st) : stm_launch_r_count(ck, d_kl.p, (int)kl.size(), st));
            HIPCHK(hipStreamSynchronize(st));
        }
        LCHK(stm_launch_rh_scan(c, L0 + P.sch.post_off, (int)P.nf, P.d_total.p, P.d_fin.p, st));
        long long total = 0, top[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(&total, P.d_total.p, sizeof(long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(top, P.d_rhtop.p, 2 * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        P.rh_total = total;
        P.stats.nlaunch += 2;
        overflow = (top[1] != 0);
        return 0;
    }
    LCHK(P.keep_h ? stm_launch_rh_count(c, L0 + P.sch.own_off, P.sch.n_own, st) : stm_launch_r_count(c, L0 + P.sch.own_off, P.sch.n_own, st));
    LCHK(stm_launch_rh_scan(c, L0 + P.sch.post_off, (int)P.nf, P.d_total.p, P.d_Rboff.p, st));
    long long total = 0;
    HIPCHK(hipMemcpyAsync(&total, P.d_total.p, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    P.rh_total = total;
    if ((size_t)total > P.d_RH.n) LCHK(P.d_RH.alloc((size_t)(total + total / 64 + 1024)));   // (a little room: a refactorization with other dead columns)
    if (P.keep_h) LCHK(stm_launch_rh_copy(c, L0 + P.sch.own_off, L0 + P.sch.rh_parts_off, P.sch.n_own, P.sch.rh_maxparts, P.d_RH.p, st));
    else LCHK(stm_launch_r_copy(c, L0 + P.sch.own_off, L0 + P.sch.rh_parts_off, P.sch.n_own, P.sch.rh_maxparts, P.d_RH.p, st));
    P.stats.nlaunch += 3;
    return 0;
}
