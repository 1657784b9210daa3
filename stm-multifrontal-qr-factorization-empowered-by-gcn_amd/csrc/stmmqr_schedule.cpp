// stmmqr_schedule.cpp -- the planner (stmmqr_sched.h): the symbolic sizes of the fronts, and sched::build -- arenas, the timeline
// allocator of the slab recycling, the step timeline of every front group.  Everything here is symbolic and pure: values in, a value
// out; stm_install_schedule (stmmqr_planbuild.cpp) puts it into a plan, stmmqr_run.cpp runs it.
//
// level schedule.  in.group[f] = g >= 0: front f is factorized here in phase g; -1: not on this device (its
// contribution block is imported).  For every group the fronts are bucketed by tree level (leaves = 0, counted
// inside the group), small ones first, large ones by decreasing panel count.
#include "stmmqr_sched.h"

#include <algorithm>

static_assert(STM_CA_MIN_ROWS == 4096, "the default of STMMQR_CA_MIN (stmmqr_knobs.h) is the kernels' STM_CA_MIN_ROWS");

namespace sched {

// ---- per-front symbolic sizes -----------------------------------------------------------
int front_syms(const Symbolic &v, Fronts &out, std::string &msg)
{
    const long nf = v.nf;
    std::vector<long> parent(nf, -1);
    for (long f = 0; f < nf; f++)
        for (long q = v.Childp[f]; q < v.Childp[f + 1]; q++) parent[v.Child[q]] = f;

    // upper bound on the rows of every front: taken from the analysis when given (QRsym->Fm, worst case when
    // rank detection is on: SparseQR_analyze.c:461-471), otherwise recomputed with the same recurrence
    out.Fm.assign(nf, 0);
    if (v.Fm) {
        for (long f = 0; f < nf; f++) out.Fm[f] = v.Fm[f];
    } else {
        std::vector<long> cmub(nf, 0);
        for (long kf = 0; kf < nf; kf++) {
            const long f = v.Post[kf];
            const long fp = v.Super[f + 1] - v.Super[f], fn = v.Rp[f + 1] - v.Rp[f];
            long fm = v.Sleft[v.Super[f + 1]] - v.Sleft[v.Super[f]];
            for (long q = v.Childp[f]; q < v.Childp[f + 1]; q++) fm += cmub[v.Child[q]];
            out.Fm[f] = fm;
            const long cn = fn - fp;
            cmub[f] = v.do_rank ? std::min(fm, cn) : std::min(std::max(fm - std::min(fm, fp), 0L), cn);
        }
    }

    // the row count every front will have if no pivot column dies (exact for full-rank input): used only to plan the
    // number of panel launches (stm_tall_panel); the kernels cope with any actual row count
    std::vector<long> &fmest = out.fm_est, &cmest = out.cm_est;
    fmest.assign(nf, 0); cmest.assign(nf, 0);
    for (long kf = 0; kf < nf; kf++) {
        const long f = v.Post[kf];
        const long fp = v.Super[f + 1] - v.Super[f], fn = v.Rp[f + 1] - v.Rp[f];
        long fe = v.Sleft[v.Super[f + 1]] - v.Sleft[v.Super[f]];
        for (long q = v.Childp[f]; q < v.Childp[f + 1]; q++) fe += cmest[v.Child[q]];
        fmest[f] = std::min(fe, out.Fm[f]);
        cmest[f] = std::min(std::max(fe - std::min(fe, fp), 0L), fn - fp);
    }

    out.fs.assign(nf, FrontSym());
    long long tpan_total = 0;
    for (long kf = 0; kf < nf; kf++) {
        const long f = v.Post[kf];
        FrontSym &s = out.fs[f];
        const long fp = v.Super[f + 1] - v.Super[f], fn = v.Rp[f + 1] - v.Rp[f];
        const long fm = out.Fm[f];
        // (front-local offsets are 64-bit on the device: row + column * ld; rows and columns themselves are int32)
        if (fm * fn >= (1L << 36)) { msg = "a single front exceeds 2^36 entries"; return 1; }
        s.fn = (int)fn; s.fp = (int)fp; s.col1 = (int)v.Super[f]; s.rp = (int)v.Rp[f]; s.hip = (int)v.Hip[f];
        s.child0 = (int)v.Childp[f]; s.child1 = (int)v.Childp[f + 1];
        s.srow0 = (int)v.Sleft[v.Super[f]]; s.srow1 = (int)v.Sleft[v.Super[f + 1]];
        s.fm_ub = (int)fm;
        s.fm_est = (int)fmest[f];
        s.ld = (int)std::max(2L, (fm + 1) & ~1L);
        s.npanels = (int)((fn + STM_NB - 1) / STM_NB);
        s.tpan = (int)tpan_total;
        tpan_total += s.npanels;
        // Q-apply: fronts with this many entries or more are split over workgroups (k_qbig_*); STMMQR_QBIG_MIN
        // overrides the threshold (tests send small fronts through that path).  2 M entries until round 4; with the grouped launches
        // (k_qbig_step4) smaller fronts pay too, at 256 KB of T4 per four panels -- default workload, threshold: Q'b / solve ms,
        // GB of T4: 2 M 13.1 / 20.6, 0.31; 1 M 12.5 / 20.0, 0.39; 256 K 11.9 / 19.5, 0.61; 128 K 11.6 / 19.2, 0.81.  1 M.
        // ... and, whatever its entry count, a front that one workgroup cannot hold in LDS: a tall thin one (16 363 rows at 40
        // columns) or a short wide one whose columns are all pivotal (10 921 of them) -- the split kernels have no such limit
        const bool over_lds = stm_lds_qapply(fm, fn) > STM_RES_LDS_MAX || stm_lds_rsolve(fp, fn) > STM_RES_LDS_MAX;
        s.qbig = ((fm * fn >= v.qbig_min || over_lds) && fn >= 1) ? 1 : 0;
        // R' x = b: the one-workgroup kernel keeps the front's u and x in LDS (6 550 columns of a square-ish front, 10 890 of a
        // short wide one); a front beyond that is split over its columns (k_rtbig_*) by the pass that knows how, rt_pass in mode RT_SPLIT.
        // STMMQR_RTBIG_MIN splits smaller ones too
        s.rtbig = (stm_lds_rtsolve(fp, fm, fn) > STM_RES_LDS_MAX || fm * fn >= v.rtbig_min) ? 1 : 0;
        s.parent = (int)parent[f];
        s.foff = 0; s.coff = 0;                                    // (they belong to a schedule: Planner::assign_arenas)
    }
    out.tpanels = tpan_total;
    return 0;
}

// ---- size of every packed R+H block if no pivot column dies (exact for full-rank input): the symbolic staircase of the front
// (qr_fsize: rows of S by leftmost column + the children's contribution rows, whose leftmost columns are the columns of their
// C) run through qr_front's row bookkeeping (:1434-1609) and qr_rhpack's column lengths (:1691-1784).  Sizes the R+H arena of
// the slab recycling (with a margin; QRsym->maxstack is the hard bound the arena falls back to) ----
void rh_estimate(const Symbolic &v, const std::vector<int> &Rjrel, Fronts &out)
{
    const long nf = v.nf;
    out.rh_est_total = 0;
    out.rh_est_front.assign((size_t)std::max(1L, nf), 0);
    std::vector<long> stair;
    for (long kf = 0; kf < nf; kf++) {
        const long f = v.Post[kf];
        const long fp = out.fs[f].fp, fn = out.fs[f].fn, fm = out.fm_est[f];
        stair.assign((size_t)fn + 1, 0);
        for (long j = 0; j < fp; j++) stair[(size_t)j] = v.Sleft[v.Super[f] + j + 1] - v.Sleft[v.Super[f] + j];
        for (long q = v.Childp[f]; q < v.Childp[f + 1]; q++) {
            const long c = v.Child[q];
            const long fpc = v.Super[c + 1] - v.Super[c], pc = v.Rp[c] + fpc;
            for (long i = 0; i < out.cm_est[c]; i++) stair[(size_t)Rjrel[(size_t)(pc + i)]]++;
        }
        long run = 0;
        for (long j = 0; j < fn; j++) { run += stair[(size_t)j]; stair[(size_t)j] = run; }       // rows with leftmost column <= j
        long g = 0, rm = 0;
        long long sz = 0;
        for (long k = 0; k < fn; k++) {
            long t;
            if (g >= fm) t = (k < fp) ? 0 : fm;                       // rows ran out
            else { t = std::min(fm, std::max(g + 1, stair[(size_t)k])); g++; }
            if (!v.keep_h) { if (k < fp && t > 0 && rm < fm) rm++; sz += rm; continue; }   // (R only: rm rows per column)
            if (k < fp) { if (t > 0) rm++; sz += (t > 0) ? t : rm; }
            else { const long h = std::min(rm + (k - fp) + 1, fm); sz += rm + std::max(t - h, 0L); }
        }
        out.rh_est_total += sz;
        out.rh_est_front[(size_t)f] = sz;
    }
}

// the timeline allocator of the slab recycling (stmmqr_sched.h says what it does)
long long timeline_first_fit(std::vector<TlObj> &objs, long long base, int nstep)
{
    std::vector<std::vector<int>> at0((size_t)nstep + 1), at1((size_t)nstep + 2);
    for (size_t i = 0; i < objs.size(); i++) {
        objs[i].size = (objs[i].size + 1) & ~1LL;
        if (objs[i].size <= 0) { *objs[i].out = base; continue; }
        at0[(size_t)objs[i].t0].push_back((int)i);
        at1[(size_t)objs[i].t1 + 1].push_back((int)i);
    }
    std::vector<std::pair<long long, long long>> freeb;            // (offset, size), sorted by offset, never adjacent
    long long top = base;
    auto release = [&](long long off, long long sz) {
        size_t i = (size_t)(std::lower_bound(freeb.begin(), freeb.end(), std::make_pair(off, 0LL)) - freeb.begin());
        freeb.insert(freeb.begin() + (long)i, {off, sz});
        if (i + 1 < freeb.size() && freeb[i].first + freeb[i].second == freeb[i + 1].first) {
            freeb[i].second += freeb[i + 1].second;
            freeb.erase(freeb.begin() + (long)i + 1);
        }
        if (i > 0 && freeb[i - 1].first + freeb[i - 1].second == freeb[i].first) {
            freeb[i - 1].second += freeb[i].second;
            freeb.erase(freeb.begin() + (long)i);
        }
        if (!freeb.empty() && freeb.back().first + freeb.back().second == top) {      // (no free block ever touches the top)
            top = freeb.back().first;
            freeb.pop_back();
        }
    };
    long long peak = base;
    for (int t = 0; t <= nstep; t++) {
        for (int i : at1[(size_t)t]) release(*objs[(size_t)i].out, objs[(size_t)i].size);
        if (t == nstep) break;
        std::vector<int> &now = at0[(size_t)t];
        std::stable_sort(now.begin(), now.end(), [&](int a, int b) { return objs[(size_t)a].size > objs[(size_t)b].size; });
        for (int i : now) {
            const long long sz = objs[(size_t)i].size;
            long long at = -1;
            for (auto it = freeb.begin(); it != freeb.end(); ++it)
                if (it->second >= sz) {
                    at = it->first;
                    if (it->second == sz) freeb.erase(it);
                    else { it->first += sz; it->second -= sz; }
                    break;
                }
            if (at < 0) { at = top; top = at + sz; }             // nothing fits: the arena grows
            *objs[(size_t)i].out = at;
            peak = std::max(peak, top);
        }
    }
    return peak;
}

namespace {

const int LDS_CAP_DOUBLES = STM_LDS_CAP_DOUBLES;   // 128 KiB of dynamic LDS for the staged (sub-)panel, k_panel
const int LDS_CAP_SMALL = 15360;          // 120 KiB in k_front_wg (it carries 8 KiB more static LDS)

// the step timeline of one group while it is being built
struct Timeline {
    int nlev = 0, nstep = 0;
    bool use_level = false;                                    // the level-synchronous order was chosen
    std::vector<int> level, start, end;                        // per front: tree level, first step, one past its last step
    // panel_at[t] = the (big front, panel) pairs of step t; small_at[t] = the small fronts factorized at step t
    std::vector<std::vector<std::pair<int, int>>> panel_at;
    std::vector<std::vector<int>> small_at, starting, ending;  // ... the fronts that start at t / are packed at the end of t
};

// sched::build: the phases below, called in sequence.  The order of what they append to out.lists and
// out.wlists is part of the plan: offsets into both are baked into every Step.
struct Planner {
    const Inputs &in;
    Schedule out;
    const knobs::BuildKnobs &k = in.k;
    const long nf = in.nf;
    int ngroups = 1;
    bool whole = false;          // ONE group holds every front and none is shared

    bool shared(long f) const { return (size_t)f < in.shared.size() && in.shared[(size_t)f]; }
    bool is_big(int f) const { return sched::is_big(out.fs[f], in.opt.big_front_cols); }
    // Pair update (k_upd_w2 / k_upd_c2): a property of the front alone -- it changes the rounding of the front's
    // trailing updates, and results must not depend on the schedule.  Fronts whose update is bandwidth bound: many rows.
    bool is_pair(int f) const
    {
        const FrontSym &s = out.fs[f];
        if (shared(f)) return false;                              // (the pair update has no column-block stride)
        return in.opt.pair_update && is_big(f) && s.fm_est >= k.pair_min && s.npanels >= 4;
    }
    int steps_of(int f) const { return is_big(f) ? out.fs[f].nsched : 1; }
    // workgroups a front gets in the assembly / packing launches for `work` entries
    int work_parts(long work) const { return (int)std::min(in.part_cap, std::max(1L, (work + in.part_grain - 1) / in.part_grain)); }
    // ... in the copy of its packed R+H block (a wave per column; 64 left the 17.6 GB copy of a 50 000-column front at 0.5 TB/s)
    static int rh_parts(const FrontSym &s) { return std::min(256, std::max(1, s.fn / 16)); }

    void begin()
    {
        out.fs = in.fs;
        out.tune = k.tune;
        out.tall_min = in.opt.tall_min_rows;
        out.plan_algo = in.opt.panel_algo;
        out.ca_min = k.ca_min;
        for (long f = 0; f < nf; f++) ngroups = std::max(ngroups, in.group[f] + 1);
        whole = (ngroups == 1) && nf > 0;
        for (long f = 0; f < nf && whole; f++) whole = (in.group[f] == 0) && !shared(f);
    }

    // Offsets of the fronts (F arena) and of the packed contribution blocks (C arena) for the groups: a front gets room
    // in F when it is factorized here (group >= 0), a contribution block when its front is factorized here or arrives here
    // (stmmqr_plan_import_front: a child of one of this plan's fronts).  One rank of a sharded run holds its subtrees and the
    // fronts above them that it owns or shares, not the whole tree.  (Every front keeps its F until the factors are packed at the
    // end of the factorization: stmmqr_factorize_finish.  A plan that recycles gets other offsets: recycling_layout.)
    void assign_arenas()
    {
        long long foff = 0, coff = 0;
        std::vector<char> needc((size_t)std::max(1L, in.nf), 0);
        out.c_slot.assign((size_t)std::max(1L, in.nf), 0);
        for (long f = 0; f < in.nf; f++) {
            if (in.group[f] < 0) continue;
            needc[(size_t)f] = 1;
            for (long q = in.Childp[f]; q < in.Childp[f + 1]; q++) needc[(size_t)in.Child[q]] = 1;
        }
        for (long kf = 0; kf < in.nf; kf++) {
            const long f = in.Post[kf];
            FrontSym &s = out.fs[f];
            s.foff = 0; s.coff = 0;
            if (in.group[f] >= 0) {
                s.foff = foff;
                foff += (long long)s.ld * s.fn;
            }
            if (needc[(size_t)f]) {
                const long cn = s.fn - s.fp, fm = s.fm_ub;
                const long cm = in.do_rank ? std::min(fm, cn) : std::min(std::max(fm - std::min(fm, (long)s.fp), 0L), cn);
                s.coff = coff;
                out.c_slot[(size_t)f] = (long long)cm * (cm + 1) / 2 + (long long)cm * (cn - cm);
                coff += out.c_slot[(size_t)f];
                coff = (coff + 1) & ~1LL;
            }
        }
        out.has_c.swap(needc);
        out.farena = std::max(1LL, foff); out.carena = std::max(1LL, coff);
    }

    // slab recycling: plans that hold the whole tree in one group (STMMQR_RECYCLE=0: every front keeps its slab, as sharded
    // plans do); a plan whose last factorization overflowed the R+H arena stays without it
    void decide_recycle()
    {
        long long slabs = 0;
        for (long f = 0; f < nf; f++) slabs += (long long)out.fs[f].ld * out.fs[f].fn;
        out.recycle = whole && !in.overflowed && k.recycles(slabs);
    }

    void mark_pair_fronts()
    {
        out.sweep = (in.opt.pair_update == 4) ? 4 : 2;
        out.pair_front.assign(std::max(1L, nf), 0);
        for (long f = 0; f < nf; f++) out.pair_front[f] = (in.group[f] >= 0 && is_pair((int)f)) ? 1 : 0;
        out.ypoff.assign(std::max(1L, nf), -1);
        out.yp_doubles = 0;
        for (long f = 0; f < nf; f++)
            if (out.pair_front[f]) {
                out.ypoff[f] = out.yp_doubles;
                out.yp_doubles += (long long)((out.fs[f].fn + 31) / 32) * (out.sweep * STM_NB * 32);
            }
    }

    void clear_lists()
    {
        out.tslot.assign(std::max(1L, nf), 0);
        out.glevels.assign(ngroups, std::vector<Level>());
        out.gsteps.assign(ngroups, std::vector<Step>());
        out.lists.clear();
        out.wlists.clear();
        out.tslots = 1;
        out.gp_slabs = 1;
        out.wp_doubles = 0;
        out.wp2_doubles = 0;
    }

    // ---- how many panels of a front get a step (FrontSym::nsched).  A front of fm rows and fn > fm columns runs out of rows at
    // column fm: the panel that holds that column finalises every column behind it (dev_panel: "no rows left") and the panels after
    // it have nothing to do -- yet each was a step of the timeline, and the parent could not start before the last of them: 446 of the
    // 1249 steps on the critical path of the default workload (8000 of its 15 313 panels), 40 of epb1's 132.  fm is only known on
    // the device, but fm_est -- the rows if no pivot column dies -- is exact for a full-rank matrix: a plan that holds the whole tree
    // schedules floor(min(fm_est, fn) / 32) + 1 panels per front.  Should a front NOT be finished by its last scheduled panel
    // (pivot columns died below it: more rows reach it than estimated), k_cpack's extra workgroup raises abort[2] and the
    // factorization is run again on the full schedule, which the plan then keeps (in.full_schedule; stats.retries counts it).
    // STMMQR_EARLY_END=0: every panel a step, as before. ----
    void cut_fronts()
    {
        const bool early = (whole || in.early_phased) && !in.full_schedule && k.early_end;
        for (long f = 0; f < nf; f++) {
            FrontSym &s = out.fs[f];
            s.nsched = s.npanels;
            if (early && is_big((int)f) && !is_pair((int)f) && in.group[f] >= 0 && !shared(f))
                s.nsched = std::min(s.npanels, std::min(s.fm_est, s.fn) / STM_NB + 1 + k.early_slack);
        }
        out.early_end = early;
    }

    // ---- tree levels (leaves = 0, counted inside the group): the order of the solves and of Q; the first and last step of every
    // front as soon as possible and level by level, and which of the two orders the group takes ----
    void levels(int grp, Timeline &T)
    {
        std::vector<int> &level = T.level, &start = T.start, &end = T.end;
        level.assign(nf, -1); start.assign(nf, 0); end.assign(nf, 0);
        int nlev = 0, nstep = 0;
        for (long kf = 0; kf < nf; kf++) {
            const long f = in.Post[kf];
            if (in.group[f] != grp) continue;
            int lv = 0, t0 = 0;
            for (long q = in.Childp[f]; q < in.Childp[f + 1]; q++) {
                const long ch = in.Child[q];
                if (in.group[ch] != grp) continue;              // (earlier phase or imported: already there)
                lv = std::max(lv, level[ch] + 1);
                t0 = std::max(t0, end[ch]);
            }
            level[f] = lv;
            nlev = std::max(nlev, lv + 1);
            start[f] = t0;
            end[f] = t0 + steps_of((int)f);
            nstep = std::max(nstep, end[f]);
        }
        // the level-synchronous schedule: every front of a tree level starts when the level below has finished
        std::vector<int> lstart(nf, 0), lend(nf, 0);
        int nstep_level = 0;
        {
            std::vector<int> lvl_end(nlev + 1, 0);
            for (int lv = 0; lv < nlev; lv++) {
                int e1 = lvl_end[lv];
                for (long kf = 0; kf < nf; kf++) {
                    const long f = in.Post[kf];
                    if (in.group[f] != grp || level[f] != lv) continue;
                    lstart[f] = lvl_end[lv];
                    lend[f] = lstart[f] + steps_of((int)f);
                    e1 = std::max(e1, lend[f]);
                }
                lvl_end[lv + 1] = e1;
            }
            nstep_level = lvl_end[nlev];
        }
        // Which order (STMMQR_SCHED unset): the envelope rule reaches the minimum number of steps (nstep here) but its steps
        // are ~10-15 % longer than those of the level-synchronous order (a launch lasts as long as its slowest front and
        // rows are only a proxy for that; measured) -- it is taken when it removes more than a fifth of the steps.
        // (Round 5: with the update beyond block 0 riding on the chain's launches and the fronts ending where they run out of rows, the
        //  envelope order wins wherever it removes steps at all -- default workload 803 against 985 steps: 94.4 against 106.3 ms, sme3Dc
        //  stand-in 541 / 637: 65.9 / 71.3, xenon1-METIS 406 / 436: 43.9 / 45.0, epb1 96 / 124: 6.3 / 7.6; a tie in steps goes to the
        //  level-synchronous order: c5mini 250 / 250: 42.3 / 42.6.)
        T.use_level = k.sched == 1 || (k.sched == 0 && 100L * nstep > 97L * nstep_level);
        if (T.use_level) {
            start = lstart; end = lend;
            nstep = nstep_level;
        }
        T.nlev = nlev; T.nstep = nstep;
        std::vector<std::vector<int>> byl(nlev);
        for (long kf = 0; kf < nf; kf++)
            if (in.group[in.Post[kf]] == grp) byl[level[in.Post[kf]]].push_back((int)in.Post[kf]);
        std::vector<Level> &LV = out.glevels[grp];
        LV.assign(nlev, Level());
        for (int lv = 0; lv < nlev; lv++) {
            Level &L = LV[lv];
            std::vector<int> small, big;
            for (int f : byl[lv]) (is_big(f) ? big : small).push_back(f);
            std::stable_sort(big.begin(), big.end(), [&](int a, int b) { return out.fs[a].npanels > out.fs[b].npanels; });
            L.all_off = (int)out.lists.size();
            L.n_small = (int)small.size(); L.n_big = (int)big.size(); L.n_all = L.n_small + L.n_big;
            out.lists.insert(out.lists.end(), small.begin(), small.end());
            out.lists.insert(out.lists.end(), big.begin(), big.end());
        }
    }

    // ---- the step timeline: what runs at every step under the three policies ----
    // The envelope rule: every step runs the fronts on the longest remaining path (counted in panels up to the root); any other
    // front that is ready or in flight rides along if its panel is no taller than theirs -- a launch lasts as long
    // as its tallest panel and is configured for it (LDS, column groups), so shorter panels are free while a taller
    // one would make the step of the critical fronts longer.  The minimum number of steps, the cheapest envelope.
    void order_steps(int grp, Timeline &T)
    {
        auto &panel_at = T.panel_at;
        auto &small_at = T.small_at;
        if (T.use_level || k.sched == 2) {
            panel_at.assign(T.nstep, {});
            small_at.assign(T.nstep, {});
            for (long kf = 0; kf < nf; kf++) {
                const int f = (int)in.Post[kf];
                if (in.group[f] != grp) continue;
                if (!is_big(f)) { small_at[T.start[f]].push_back(f); continue; }
                for (int q = 0; q < out.fs[f].nsched; q++) panel_at[T.start[f] + q].push_back({f, q});
            }
            return;
        }
        std::vector<int> parent_in(nf, -1), pend(nf, 0), tails(nf, 0);
        for (long f = 0; f < nf; f++) {
            if (in.group[f] != grp) continue;
            for (long q = in.Childp[f]; q < in.Childp[f + 1]; q++)
                if (in.group[in.Child[q]] == grp) { parent_in[in.Child[q]] = (int)f; pend[f]++; }
        }
        for (long kf = nf; kf-- > 0;) {
            const long f = in.Post[kf];
            if (in.group[f] != grp) continue;
            tails[f] = steps_of((int)f) + (parent_in[f] >= 0 ? tails[parent_in[f]] : 0);
        }
        std::vector<int> ready;
        for (long kf = 0; kf < nf; kf++)
            if (in.group[in.Post[kf]] == grp && pend[in.Post[kf]] == 0) ready.push_back((int)in.Post[kf]);
        struct Fly { int f, p; };
        std::vector<Fly> fly;                                 // big fronts ready or in flight, with their next panel
        while (!ready.empty() || !fly.empty()) {
            std::vector<int> newly, smalls;
            for (int f : ready) {
                if (is_big(f)) fly.push_back({f, 0});
                else smalls.push_back(f);
            }
            panel_at.push_back({});
            small_at.push_back(smalls);
            auto finish = [&](int f) {
                const int pf = parent_in[f];
                if (pf >= 0 && --pend[pf] == 0) newly.push_back(pf);
            };
            if (!fly.empty()) {
                auto rem = [&](const Fly &e) { return tails[e.f] - e.p; };
                auto rows = [&](const Fly &e) { return stm_panel_rows_est(out.fs[e.f], e.p); };
                int rl = 0, env = 0;
                for (const Fly &e : fly) rl = std::max(rl, rem(e));
                for (const Fly &e : fly)
                    if (rem(e) == rl) env = std::max(env, rows(e));
                std::vector<Fly> keep;
                for (Fly &e : fly) {
                    if (rem(e) == rl || rows(e) <= k.ride * env) {
                        panel_at.back().push_back({e.f, e.p});
                        if (++e.p >= out.fs[e.f].nsched) { finish(e.f); continue; }
                    }
                    keep.push_back(e);
                }
                fly.swap(keep);
            }
            for (int f : smalls) finish(f);
            ready.swap(newly);
        }
        T.nstep = (int)panel_at.size();
    }

    // ---- the steps themselves: per step the fronts that start, the fronts in flight with their panel and workspace slices, the
    // launch shapes, and the fronts that are packed at its end ----
    void emit_steps(int grp, Timeline &T)
    {
        const int nstep = T.nstep;
        auto &starting = T.starting;
        auto &ending = T.ending;
        starting.assign(nstep, {}); ending.assign(nstep, {});
        std::vector<int> pan_now(nf, 0);                          // the panel a front in flight is at, per step
        for (int t = 0; t < nstep; t++) {
            for (int f : T.small_at[t]) starting[t].push_back(f);
            for (const auto &fp : T.panel_at[t]) {
                if (fp.second == 0) starting[t].push_back(fp.first);
                if (fp.second == out.fs[fp.first].nsched - 1) ending[t].push_back(fp.first);
            }
        }
        // The packing of finished fronts is batched: k_cpack runs at the last step before some front STARTS (only an
        // assembly reads a packed block) or at the end of the group -- one launch per tree level in the level-synchronous
        // order instead of one per step in which a front happens to end.  (T / Gram slots are released at the flush:
        // k_cpack's extra workgroup may still write the T of the front's last panel.)
        for (int t = 0, carry_from = -1; t < nstep; t++) {
            const bool flush = (t + 1 == nstep) || !starting[t + 1].empty();
            if (carry_from >= 0 && carry_from != t) {
                ending[t].insert(ending[t].begin(), ending[carry_from].begin(), ending[carry_from].end());
                ending[carry_from].clear();
            }
            carry_from = (flush || ending[t].empty()) ? -1 : t;
            if (!flush && !ending[t].empty()) carry_from = t;
        }
        std::vector<Step> &SV = out.gsteps[grp];
        SV.assign(nstep, Step());
        std::vector<int> active, freeslots;                   // big fronts in flight; released T / Gram slots
        int nslots = 0;
        for (int t = 0; t < nstep; t++) {
            Step &S = SV[t];
            std::vector<int> small, big;
            for (int f : starting[t]) (is_big(f) ? big : small).push_back(f);
            S.start_off = (int)out.lists.size();
            S.n_small = (int)small.size(); S.n_start = (int)(small.size() + big.size());
            out.lists.insert(out.lists.end(), small.begin(), small.end());
            out.lists.insert(out.lists.end(), big.begin(), big.end());
            S.asm_parts_off = (int)out.lists.size();
            long maxfm_small = 0;
            for (int i = 0; i < S.n_start; i++) {
                const FrontSym &s = out.fs[out.lists[S.start_off + i]];
                const int parts = work_parts((long)s.fm_ub * s.fn);
                out.lists.push_back(parts);
                S.asm_maxparts = std::max(S.asm_maxparts, parts);
                if (i < S.n_small) maxfm_small = std::max(maxfm_small, (long)s.fm_ub);
            }
            // (rows padded as dev_panel pads them, so that a whole panel fits whenever the cap allows: the sub-panel width
            //  of a front -- and with it the rounding -- must not depend on which other fronts share its step)
            S.lds_small = (int)std::min((long)LDS_CAP_SMALL, (((maxfm_small + 63) & ~63L) | 1) * STM_NB + 64);
            // (the wave-pipelined panels of k_front_wg: an image of 32 x 128 rows, and dev_gram_T's 4 x 768 doubles of scratch)
            if (S.n_small > 0) S.lds_small = std::max(S.lds_small, STM_NB * 128 + 64);
            // T / Gram-partial slots: a slot is held from the step a front starts to the step it ends
            for (int f : big) {
                if (!freeslots.empty()) { out.tslot[f] = freeslots.back(); freeslots.pop_back(); }
                else out.tslot[f] = nslots++;
            }
            active.clear();
            for (const auto &fp : T.panel_at[t]) { active.push_back(fp.first); pan_now[fp.first] = fp.second; }
            // heaviest update first (the order inside a launch does not change any result); classes: see Step
            auto work_at = [&](int f) { return (long)stm_upd_ncb(out.fs[f], pan_now[f]) * stm_upd_nsl(out.fs[f]); };
            auto cls = [&](int f) { return !is_pair(f) ? 0 : 1 + pan_now[f] % out.sweep; };
            std::stable_sort(active.begin(), active.end(), [&](int a, int b) {
                return cls(a) != cls(b) ? cls(a) < cls(b) : work_at(a) > work_at(b);
            });
            S.act_off = (int)out.lists.size();
            S.n_act = (int)active.size();
            out.lists.insert(out.lists.end(), active.begin(), active.end());
            S.plist_off = (int)out.lists.size();
            for (int f : active) out.lists.push_back(pan_now[f]);
            S.wp_off = (int)out.wlists.size();
            long long wp = 0, ncbsum = 0;
            long maxfm_big = 0;
            for (int f : active) {
                const FrontSym &s = out.fs[f];
                const int p = pan_now[f];
                const int ncb = stm_upd_ncb(s, p), nsl = stm_upd_nsl(s);
                const bool ca = stm_use_ca(s, p, in.opt.panel_algo, out.ca_min), tall = stm_tall_panel(s, p, out.tall_min);
                out.wlists.push_back(wp);
                // (+1: Gram block.  Pair-update fronts: two blocks per partial, at most stm_pair_slots partials per column block in the
                //  sweep of an odd panel -- a workgroup takes up to four slabs --, and the panel-by-panel updates of the next panels'
                //  columns use the first 2 + 1 column blocks with the full slab count)
                //  (quad update: four blocks per partial, three Gram blocks, 4 + 1 column blocks in the panel-by-panel updates)
                if (is_pair(f))
                    wp += std::max((long long)(ncb + out.sweep - 1) * (out.sweep == 4 ? stm_quad_slots(nsl, out.tune) : stm_pair_slots(nsl, out.tune)) *
                                       (out.sweep * STM_NB * 32),
                                   (out.sweep + 1LL) * nsl * (STM_NB * 32));
                else
                    wp += (long long)(ncb + 1) * nsl * (STM_NB * 32);
                const int c = cls(f);
                if (c == 0) {
                    S.n_norm++;
                    ncbsum += ncb;
                    S.maxcb = std::max(S.maxcb, ncb);
                    S.maxsl = std::max(S.maxsl, nsl);
                } else {
                    S.n_pk[c - 1]++;
                    S.maxsl_pk[c - 1] = std::max(S.maxsl_pk[c - 1], nsl);
                    if (c == out.sweep) S.maxcbp_po = std::max(S.maxcbp_po, ncb - 1);
                }
                S.nsub = std::max(S.nsub, stm_tall_launches(s, p, out.tall_min));
                S.nca = std::max(S.nca, stm_ca_slabs(s));
                (ca ? S.nca_use : S.npipe_use)++;
                out.gp_slabs = std::max(out.gp_slabs, stm_ca_slabs(s));
                maxfm_big = std::max(maxfm_big, (long)s.fm_ub);
                if (!tall && !ca) S.lds_plan = std::max(S.lds_plan, stm_front_lds(s));
                // a short panel of the pipeline is taken by one workgroup with the panel's image in LDS (dev_wave_panel)
                if (tall && !ca) S.lds_plan = std::max(S.lds_plan, STM_NB * STM_WP_ROWS);
            }
            S.lds_big = (int)std::min((long)LDS_CAP_DOUBLES, (((maxfm_big + 63) & ~63L) | 1) * STM_NB + 64);
            // row-parallel update when it pays: >= 3 slabs, or so many column blocks in the launch that the one-workgroup
            // form's redundant T (every column-block workgroup builds it) costs throughput (T is built once per front
            // by k_upd_w).  Either form gives the same bits.
            S.split = (S.maxsl >= 3 || ncbsum >= 512) ? 1 : 0;
            out.wp_doubles = std::max(out.wp_doubles, wp);
            if (S.n_sweep() == 0) out.wp2_doubles = std::max(out.wp2_doubles, wp);
            // fronts at their last panel: packed at the end of the step, slot released for the next
            S.cpk_off = (int)out.lists.size();
            S.n_cpk = (int)ending[t].size();
            out.lists.insert(out.lists.end(), ending[t].begin(), ending[t].end());
            S.cpk_parts_off = (int)out.lists.size();
            for (int f : ending[t]) {
                const FrontSym &s = out.fs[f];
                const long cn = s.fn - s.fp;
                const int parts = work_parts(cn * std::min((long)s.fm_ub, cn));
                out.lists.push_back(parts);
                S.cpk_maxparts = std::max(S.cpk_maxparts, parts);
                freeslots.push_back(out.tslot[f]);
            }
        }
        out.tslots = std::max(out.tslots, nslots);
    }

    // Front and contribution-block offsets of a plan that holds the whole tree in ONE group, from the step timeline of that group
    // (out.f_t0 / f_t1 / c_t1, filled by Planner::recycling_layout).  `kept` fronts sit at the bottom of the front arena for good.
    // Returns {front arena, contribution arena} in doubles.
    std::pair<long long, long long> timeline_offsets(const std::vector<char> &kept, int nstep, bool apply)
    {
            std::vector<long long> foff((size_t)std::max(1L, nf), 0), coff((size_t)std::max(1L, nf), 0);
        long long base = 0;
        for (long f = 0; f < nf; f++)
            if (kept[(size_t)f]) { foff[(size_t)f] = base; base += (long long)out.fs[f].ld * out.fs[f].fn; }
        std::vector<TlObj> fo, co;
        for (long f = 0; f < nf; f++) {
            const FrontSym &s = out.fs[f];
            if (!kept[(size_t)f]) fo.push_back({(long long)s.ld * s.fn, out.f_t0[f], out.f_t1[f], &foff[(size_t)f]});
            const long cn = s.fn - s.fp, fm = s.fm_ub;
            const long cm = in.do_rank ? std::min(fm, cn) : std::min(std::max(fm - std::min(fm, (long)s.fp), 0L), cn);
            const long long csz = (long long)cm * (cm + 1) / 2 + (long long)cm * (cn - cm);
            if (apply) out.c_slot[(size_t)f] = csz;
            co.push_back({csz, out.f_t1[f], std::max(out.f_t1[f], out.c_t1[f]), &coff[(size_t)f]});
        }
        const long long fpeak = timeline_first_fit(fo, base, nstep), cpeak = timeline_first_fit(co, 0, nstep);
        if (apply)
            for (long f = 0; f < nf; f++) { out.fs[f].foff = foff[(size_t)f]; out.fs[f].coff = coff[(size_t)f]; }
        return {std::max(1LL, fpeak), std::max(1LL, cpeak)};
    }

    // ---- slab recycling: lifetimes of the slabs and contribution blocks on this timeline, the fronts that keep their slab,
    // the offsets, and per step the fronts whose packed R+H block is staged at its end ----
    void recycling_layout(int grp, const Timeline &T)
    {
        const int nstep = T.nstep;
        std::vector<Step> &SV = out.gsteps[grp];
        const std::vector<Level> &LV = out.glevels[grp];
        auto slab = [&](long f) { return (long long)out.fs[f].ld * out.fs[f].fn; };
        out.f_t0.assign((size_t)std::max(1L, nf), 0); out.f_t1.assign((size_t)std::max(1L, nf), 0); out.c_t1.assign((size_t)std::max(1L, nf), 0);
        for (int t = 0; t < nstep; t++) {
            for (int f : T.starting[t]) { out.f_t0[(size_t)f] = t; if (!is_big(f)) out.f_t1[(size_t)f] = t; }
            for (int f : T.ending[t]) out.f_t1[(size_t)f] = t;
        }
        for (long f = 0; f < nf; f++) {
            const int par = out.fs[f].parent;
            out.c_t1[(size_t)f] = (par >= 0) ? out.f_t0[(size_t)par] : out.f_t1[(size_t)f];
        }
        // which fronts keep their slab: none, or the 1-3 largest -- whatever makes fronts + contribution blocks + R+H arena
        // smallest (the arena holds min(maxstack, all recycled slabs) doubles: the reference's bound for all of R+H)
        std::vector<int> bysize((size_t)nf);
        for (long f = 0; f < nf; f++) bysize[(size_t)f] = (int)f;
        std::stable_sort(bysize.begin(), bysize.end(), [&](int a, int b) { return slab(a) > slab(b); });
        // R only (keepH = 0): the arena holds the estimated R of the fronts that do not keep their slab (+ 12.5 %); a kept
        // front's R is packed on the fly by the download and never enters it
        auto staged_est = [&](const std::vector<char> &kp) -> long long {
            double e = 0;
            for (long f = 0; f < nf; f++) if (!kp[(size_t)f]) e += (double)in.rh_est_front[(size_t)f];
            const long long est = (long long)(e * in.rh_est_scale);
            return est + est / 8 + 4096;
        };
        // the hard bound of the arena when the fronts in kp keep their slab
        auto hard_cap = [&](const std::vector<char> &kp) -> long long {
            long long rec = 0;
            for (long f = 0; f < nf; f++) if (!kp[(size_t)f]) rec += slab(f);
            return (in.maxstack > 0) ? std::min((long long)in.maxstack, rec) : rec;
        };
        long long best = -1;
        int bestk = 0;
        // (STMMQR_KEEP_FRONTS: tests force how many keep it; everything after the choice runs on the forced set)
        const int forced = (k.keep_fronts >= 0) ? (int)std::min<long>(std::min(k.keep_fronts, 3), nf) : -1;
        if (forced >= 0) bestk = forced;
        for (int q = 0; forced < 0 && q <= std::min(3L, nf); q++) {
            std::vector<char> kp((size_t)std::max(1L, nf), 0);
            for (int i = 0; i < q; i++) kp[(size_t)bysize[(size_t)i]] = 1;
            const auto pk = timeline_offsets(kp, nstep, false);
            long long cap = hard_cap(kp);
            if (!in.keep_h && !in.rh_grow) cap = std::min(cap, staged_est(kp));     // (R only: the arena follows the packed R)
            const long long tot = pk.first + pk.second + cap;
            if (best < 0 || tot < best - best / 50) { best = tot; bestk = q; }      // (a kept front must buy at least 2 %)
        }
        out.kept.assign((size_t)std::max(1L, nf), 0);
        for (int i = 0; i < bestk; i++) out.kept[(size_t)bysize[(size_t)i]] = 1;
        out.rh_cap = std::max(1LL, hard_cap(out.kept));
        // (the estimate + 12.5 % where that is less: dead columns move rows into later fronts and can make the factors
        //  larger than the full-rank pattern says; an arena that overflows is regrown to the hard bound and the factorization
        //  repeated once -- stats.retries says so)
        if (!in.rh_grow && !in.keep_h) out.rh_cap = std::max(1LL, std::min(out.rh_cap, staged_est(out.kept)));
        else if (!in.rh_grow && in.rh_est_total > 0) {
            // (in.rh_est_scale: tests shrink the estimate to drive the overflow path)
            const long long est = (long long)((double)in.rh_est_total * in.rh_est_scale);
            out.rh_cap = std::max(1LL, std::min(out.rh_cap, est + est / 8 + 4096));
        }
        const auto pk = timeline_offsets(out.kept, nstep, true);
        out.farena = pk.first; out.carena = pk.second;
        out.has_c.assign((size_t)std::max(1L, nf), 1);
        for (int t = 0; t < nstep; t++) {
            Step &S = SV[t];
            std::vector<int> rhp;
            for (int f : T.starting[t]) if (!is_big(f) && !out.kept[(size_t)f]) rhp.push_back(f);
            for (int f : T.ending[t]) if (!out.kept[(size_t)f]) rhp.push_back(f);
            S.rhp_off = (int)out.lists.size();
            S.n_rhp = (int)rhp.size();
            out.lists.insert(out.lists.end(), rhp.begin(), rhp.end());
            S.rhp_parts_off = (int)out.lists.size();
            for (int f : rhp) {
                const int parts = rh_parts(out.fs[f]);
                out.lists.push_back(parts);
                S.rhp_maxparts = std::max(S.rhp_maxparts, parts);
            }
        }
        // scratch of the resident-factor operations: every tree level in front form, one level at a time
        out.fs_scr = out.fs;
        out.scr_doubles = 1;
        for (size_t l = 0; l < LV.size(); l++) {
            long long o = 0;
            for (int q = 0; q < LV[l].n_all; q++) {
                const int f = out.lists[(size_t)(LV[l].all_off + q)];
                if (out.kept[(size_t)f]) continue;
                out.fs_scr[(size_t)f].foff = o;
                o += slab(f);
            }
            out.scr_doubles = std::max(out.scr_doubles, o);
        }
    }

    // fronts factorized on this device, in Post order, + their R+H copy parts; then ALL fronts in Post order
    void tail_lists()
    {
        out.own_off = (int)out.lists.size();
        out.n_own = 0;
        for (long kf = 0; kf < nf; kf++)
            if (in.group[in.Post[kf]] >= 0) { out.lists.push_back((int)in.Post[kf]); out.n_own++; }
        out.rh_parts_off = (int)out.lists.size();
        out.rh_maxparts = 1;
        for (long kf = 0; kf < nf; kf++) {
            if (in.group[in.Post[kf]] < 0) continue;
            const int parts = rh_parts(out.fs[in.Post[kf]]);
            out.lists.push_back(parts);
            out.rh_maxparts = std::max(out.rh_maxparts, parts);
        }
        out.post_off = (int)out.lists.size();
        for (long kf = 0; kf < nf; kf++) out.lists.push_back((int)in.Post[kf]);
        if (out.lists.empty()) out.lists.push_back(0);
        if (out.wlists.empty()) out.wlists.push_back(0);
    }
};

}  // namespace

Schedule build(const Inputs &in)
{
    Planner B{in, Schedule()};
    B.begin();
    B.assign_arenas();
    B.decide_recycle();
    B.mark_pair_fronts();
    B.clear_lists();
    B.cut_fronts();
    for (int grp = 0; grp < B.ngroups; grp++) {
        Timeline T;
        B.levels(grp, T);
        B.order_steps(grp, T);
        B.emit_steps(grp, T);
        if (B.out.recycle && grp == 0) B.recycling_layout(grp, T);
    }
    B.tail_lists();
    return std::move(B.out);
}

}  // namespace sched
