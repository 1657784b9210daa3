// stmmqr_sched.h -- the planner as a pure unit: the symbolic sizes of the fronts and the schedule of a grouping, built as VALUES from
// plain vectors and numbers.  No HIP call, no device buffer, no plan, no process global (stmmqr_device.h, stmmqr_knobs.h,
// stmmqr_recover.h and the standard library only), so tests/schedule_selftest.cpp runs it under ASan + UBSan without a GPU.  The one
// place that moves a Schedule into a plan and onto the device is stm_install_schedule (stmmqr_planbuild.cpp).
#pragma once
#include <string>
#include <vector>

#include "stmmqr_device.h"
#include "stmmqr_knobs.h"
#include "stmmqr_recover.h"

// One step of the factorization timeline.  Every front starts at the step after the last of its children has finished
// (a small front takes one step, a big one a step per panel), so a front deep in a short branch does not wait for the
// tallest front of its tree level: at every step the launches cover all the big fronts that are in flight, each at its
// own panel.  Everything here is symbolic (lists built once per schedule).
struct Step {
    int start_off = 0, n_start = 0, n_small = 0;      // fronts starting here (small first, then big): set up + assembled
    int asm_parts_off = 0, asm_maxparts = 1, lds_small = 0;
    int act_off = 0, plist_off = 0, n_act = 0;        // big fronts in flight + the panel each is at
    int wp_off = 0;                                   // (index into wlists) their slices of the update workspace
    int nsub = 1, nca = 1, nca_use = 0, npipe_use = 0, maxcb = 0, maxsl = 0, split = 0;
    int lds_big = 0;       // dynamic LDS of the panel launch when every front may take the one-workgroup panel (recovery, tests)
    int lds_plan = 0;      // ... when only the fronts planned for it do (the pipeline groups need the update's LDS only)
    // the fronts in flight are listed in three classes: [0, n_norm) every panel's update on all trailing columns;
    // then the sweep fronts (is_pair; w = 2 or 4 panels per sweep, Schedule::sweep) by panel number mod w: class r updates the
    // column blocks 0 .. w-1-r only (the columns of the next panels), the last class then applies the w last panels at once to
    // everything beyond
    int n_norm = 0, n_pk[4] = {0, 0, 0, 0};
    int maxsl_pk[4] = {0, 0, 0, 0}, maxcbp_po = 0;
    int n_sweep() const { return n_pk[0] + n_pk[1] + n_pk[2] + n_pk[3]; }
    int cpk_off = 0, cpk_parts_off = 0, n_cpk = 0, cpk_maxparts = 1;   // big fronts whose last panel runs here
    // slab recycling: the fronts whose packed R+H block is staged at the end of this step (the small fronts that started here and
    // the big fronts packed here, kept fronts excluded) + copy parts
    int rhp_off = 0, rhp_parts_off = 0, n_rhp = 0, rhp_maxparts = 1;
};

namespace sched {

// ---- the symbolic sizes of the fronts (the pure half of build_plan) -------------------------------------------------------------
// The analysis as the plan holds it; Fm: QRsym->Fm or nullptr (recomputed with the same recurrence); qbig_min / rtbig_min: the PLAN
// knobs STMMQR_QBIG_MIN / STMMQR_RTBIG_MIN as the caller has read them.
struct Symbolic {
    long nf;
    const std::vector<long> &Sleft, &Super, &Rp, &Hip, &Child, &Childp, &Post;
    const long *Fm;
    int do_rank, keep_h;
    long qbig_min, rtbig_min;
};
struct Fronts {
    std::vector<long> Fm;                // upper bound on the rows of every front
    std::vector<long> fm_est, cm_est;    // rows of every front / of its contribution block if no pivot column dies
    std::vector<FrontSym> fs;            // foff = coff = 0, nsched = 0: they belong to a schedule (build)
    long long tpanels = 0;               // panels of all fronts
    long long rh_est_total = 0;          // all packed R+H blocks if no pivot column dies (exact for full-rank input)
    std::vector<long long> rh_est_front; // ... per front
};
// Fm, the row estimates, FrontSym, tpanels.  Returns 0, or 1 (a front is too large for the device's indices) with the text for the
// caller's `fail`
int front_syms(const Symbolic &v, Fronts &out, std::string &msg);
// rh_est_total / rh_est_front of `out` (after front_syms).  Rjrel: child column -> parent column, per slot of Rj
void rh_estimate(const Symbolic &v, const std::vector<int> &Rjrel, Fronts &out);

// ---- the schedule of a grouping ---------------------------------------------------------------------------------------------------
// what the planner reads of stmmqr_options, as they are when the schedule is built
struct Options { int big_front_cols, pair_update, tall_min_rows, panel_algo; };

// a large front: a step per panel on the timeline, the panel / update kernels; the others are factorized by one workgroup in one step
inline bool is_big(const FrontSym &s, int big_front_cols) { return s.fn >= big_front_cols && s.fm_ub >= 64; }

struct Inputs {
    long nf;
    const std::vector<long> &Post, &Child, &Childp;                // the tree
    const std::vector<FrontSym> &fs;                               // (foff / coff / nsched are not read)
    int do_rank, keep_h;
    long maxstack;                                                 // QRsym->maxstack (0: unknown)
    long long rh_est_total;
    const std::vector<long long> &rh_est_front;
    double rh_est_scale;
    const std::vector<int> &group;                                 // per front: phase on this device, -1 = elsewhere
    const std::vector<char> &shared;                               // per front (may be empty: none): alone in its group, driven step by step
    Options opt;
    knobs::BuildKnobs k;
    long part_grain, part_cap;                                     // the PROCESS knobs STMMQR_PART_GRAIN / STMMQR_PART_CAP
    // of recover::State
    bool overflowed;
    int rh_grow;
    bool full_schedule, early_phased;
};

// Everything a (re)build of the schedule replaces, and nothing else.
struct Schedule {
    std::vector<FrontSym> fs;                  // the fronts, with foff / coff / nsched of this schedule
    std::vector<std::vector<Level>> glevels;   // [group][level]
    std::vector<std::vector<Step>> gsteps;     // [group][step]
    std::vector<int> lists;                    // what every offset of Level and Step points into (d_lists)
    std::vector<long long> wlists;             // ... Step::wp_off (d_wlists)
    std::vector<int> tslot;                    // per big front: its T / Gram slot (d_tslot)
    int tslots = 1;
    int gp_slabs = 1;                          // Gram-based panel: max slab workgroups of a front
    long long wp_doubles = 0;                  // workspace of the row-parallel update (partial W blocks)
    long long wp2_doubles = 0;                 // ... of the side stream's copy: steps with pair-update fronts never go there
    std::vector<char> pair_front;              // per front: takes the pair / quad update
    int sweep = 2;                             // panels per sweep of those fronts: 2 (k_upd_w2 / y2 / c2) or 4 (k_upd_wq / yq / cq)
    std::vector<long long> ypoff;              // [nf] offsets into Ypend (-1: not a pair-update front)
    long long yp_doubles = 0;
    // arenas
    long long farena = 0, carena = 0;
    std::vector<char> has_c;                   // per front: its packed contribution block has a slot in the C arena of this plan
                                               //  (the front is factorized here, or it is a child of one that is)
    std::vector<long long> c_slot;             // ... and the size of that slot in doubles (the symbolic bound of csize)
    // ---- slab recycling (the reference's stack discipline, SparseQR_factorize.c:405-422,925-933, re-cast for a timeline of steps):
    // a front's slab lives from the step it starts to the step its contribution block is packed and its R+H block staged into the
    // R+H arena; a contribution block from there to the step its parent starts.  Offsets are assigned by an address-ordered
    // first-fit over that timeline, all symbolic.  Fronts in `kept` keep their slab (never staged: their packed block is produced on
    // the fly when the factors are downloaded) -- chosen where that makes the peak smaller (a root front that IS most of the
    // factors).  Only plans that hold the whole tree in one group recycle (sharded plans: every front keeps its slab).
    bool recycle = false;
    std::vector<char> kept;                    // per front
    std::vector<int> f_t0, f_t1, c_t1;         // slab: [f_t0, f_t1]; contribution block: [f_t1, c_t1]  (steps of group 0)
    long long rh_cap = 0;                      // capacity of the R+H arena (doubles)
    std::vector<FrontSym> fs_scr;              // scratch of the resident-factor operations: FrontSym with foff into it,
    long long scr_doubles = 0;                 //  and the doubles of its widest tree level
    // the tail of lists: the fronts factorized here in Post order + their R+H copy parts; all fronts in Post order
    int own_off = 0, n_own = 0, post_off = 0, rh_parts_off = 0, rh_maxparts = 1;
    bool early_end = false;                    // the schedule of group 0 stops every front at the panel where it is expected to run out of rows
    int ca_min = STM_CA_MIN_ROWS;              // STMMQR_CA_MIN when the schedule was built
    int plan_algo = 0;                         // options.panel_algo ...
    int tall_min = STM_TALL_MIN;               // options.tall_min_rows ...
    int tune = 0;                              // STMMQR_TUNE ... (measurement sweeps)
};

Schedule build(const Inputs &in);

// ---- timeline allocator (slab recycling) ----------------------------------------------------------------------------------
// Objects with a size and a lifetime [t0, t1] in steps; an address may be given to another object from step t1 + 1 on.  Objects
// are placed in order of their first step (larger first inside a step) at the lowest address that holds them (address-ordered
// first fit, free blocks coalesced).  Returns the peak address.  Everything is symbolic, so the offsets are part of the schedule.
struct TlObj { long long size; int t0, t1; long long *out; };
long long timeline_first_fit(std::vector<TlObj> &objs, long long base, int nstep);

}  // namespace sched
