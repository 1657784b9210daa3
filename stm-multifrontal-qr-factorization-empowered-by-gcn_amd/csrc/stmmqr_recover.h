// stmmqr_recover.h -- what a factorization pass can end as, and what each driver does about it: the recovery policy of
// stmmqr_factorize.cpp as plain functions of (state, outcome, who drives).  Pure: no HIP header, no plan, no device buffer
// (tests/recover_selftest.cpp walks it without a GPU; DESIGN.md 1d has the same table in words).
//
// The device honours two preconditions, and the termination of the whole-call loop rests on them:
//   (P1) no OUTLIVED_SCHEDULE on a full schedule: only a schedule cut at the fronts' expected last panels can be outlived, and the
//        planner cuts none once State::full_schedule is set;
//   (P2) no ARENA_OVERFLOW on a plan that does not recycle its slabs: only the recycling's R+H arena has a bump pointer to overflow,
//        and the planner gives none to a plan whose State::overflowed is set.
#pragma once

namespace recover {

// How a pass (begin .. finish) ended, as stmmqr_factorize_finish reads it from the device.
enum class Outcome {
    DONE,
    REFUSED_MESSAGE,      // abort[3]: a contribution block received from another rank does not fit its front's symbolic bounds
    WAIT_RAN_OUT,         // abort[1] or a front's perr: a bounded inter-workgroup wait of a panel kernel ran out
    OUTLIVED_SCHEDULE,    // abort[2]: a front had rows left at its last scheduled panel (cut schedule, rank-deficient fronts)
    ARENA_OVERFLOW        // the packed factors did not fit the R+H arena of the slab recycling
};

// The causes, most specific first.  A wait that ran out leaves its front unfinished, so it also looks like a front that outlived its
// schedule: that is the wait's failure.  Either leaves fronts that packed what they held when they stopped, which may not fit the
// recycled arena: that overflow is theirs, not the arena's.
inline Outcome classify(bool refused_message, bool wait_ran_out, bool outlived, bool overflow)
{
    if (refused_message) return Outcome::REFUSED_MESSAGE;
    if (wait_ran_out) return Outcome::WAIT_RAN_OUT;
    if (outlived) return Outcome::OUTLIVED_SCHEDULE;
    if (overflow) return Outcome::ARENA_OVERFLOW;
    return Outcome::DONE;
}

// The recovery state of a plan.  The planner reads the first four when it builds a schedule (stmmqr_schedule.cpp); they change
// here only, and take effect at the next rebuild of the schedule.
struct State {
    int rh_grow = 0;                     // 0: the R+H arena is sized from the full-rank estimate; 1: from the hard bounds (it overflowed once)
    bool overflowed = false;             // a factorization did not fit the arena at its hard bound: this plan does not recycle
    bool full_schedule = false;          // a cut schedule did not hold once, or the caller took it back: every panel is scheduled from now on
    bool early_phased = false;           // the caller of the phased interface asked for the cut schedule (stmmqr_plan_set_early_end)
    Outcome last = Outcome::DONE;        // of the last finish; DONE again once begin or a transition has acted on it
    int abort2_before = 0;               // phased use: abort[2] as the groups run so far left it (a rerun group starts from it)
};

// finish: the outcome is noted, and an arena that overflowed is larger at the next rebuild (the hard bound, then no recycling).
inline void record(State &s, Outcome o)
{
    s.last = o;
    if (o != Outcome::ARENA_OVERFLOW) return;
    if (!s.rh_grow) s.rh_grow = 1;
    else s.overflowed = true;
}

enum class Action {
    RETURN,               // finish's result (success or its error) goes to the caller
    RERUN_SERIAL,         // same schedule, every panel by one workgroup (no inter-workgroup wait anywhere)
    REBUILD               // rebuild the schedule from the state and start over (the parallel attempt first)
};

// ---- stmmqr_factorize_device: the whole call recovers the whole factorization itself -------------------------------------------
struct WholeCall {
    bool serial = false;                 // this pass runs one-workgroup panels
    int arena_retries = 0, reschedules = 0;
    int retries() const { return (serial ? 1 : 0) + arena_retries; }     // stats.retries of the pass about to run
};

// `o`: what the pass ended as (DONE also stands for an error that finish did not classify: it goes up); `recycles`: the plan recycles
// its slabs.  An overflow that belongs to a wait or an outlived schedule never reaches here as ARENA_OVERFLOW (classify).
inline Action after_pass(State &s, WholeCall &w, Outcome o, bool recycles)
{
    if (o == Outcome::ARENA_OVERFLOW && recycles) {              // (record() has grown the arena)
        s.last = Outcome::DONE;
        w.arena_retries++;
        w.serial = false;
        return Action::REBUILD;
    }
    if (o == Outcome::OUTLIVED_SCHEDULE) {
        s.last = Outcome::DONE;
        s.full_schedule = true;
        w.reschedules++;
        w.serial = false;
        return Action::REBUILD;
    }
    if (o == Outcome::WAIT_RAN_OUT && !w.serial) {
        w.serial = true;
        return Action::RERUN_SERIAL;
    }
    w.serial = false;
    return Action::RETURN;
}

// ---- the phased interface (begin / group ... / finish by the caller): no loop around the factorization ---------------------------
// At stmmqr_factorize_begin, before anything is reset.  `cut_in_force`: the schedule of group 0 is a cut one; `recycles` as above.
// REBUILD or RETURN (= go on with the schedule as it is).  After a wait nothing: the group's own rerun has handled it.
inline Action at_phased_begin(State &s, bool cut_in_force, bool recycles)
{
    // a cut schedule needs the whole call's rerun when a front outlives it: a phased caller gets it only by asking (early_phased)
    // and loses it when a finish said OUTLIVED
    const bool to_full = (cut_in_force && !s.early_phased) || s.last == Outcome::OUTLIVED_SCHEDULE;
    // the last finish did not fit the arena: a caller that simply tries again gets the larger one instead of the same failure
    const bool regrow = s.last == Outcome::ARENA_OVERFLOW && recycles;
    if (to_full) s.full_schedule = true;
    if (to_full || regrow) s.last = Outcome::DONE;
    return (to_full || regrow) ? Action::REBUILD : Action::RETURN;
}

// stmmqr_plan_set_early_end(mode): refused between begin and finish -- `begun` stays set after a failed finish -- unless that
// finish said OUTLIVED (the caller's own recovery: every rank goes back to the full schedule).  true: allowed, rebuild.
inline bool set_early_end(State &s, bool begun, int mode)
{
    if (begun && s.last != Outcome::OUTLIVED_SCHEDULE) return false;
    s.last = Outcome::DONE;
    s.early_phased = (mode != 0);
    s.full_schedule = (mode == 0);
    return true;
}

// The group retry of the phased interface: a wait that ran out in a group is found after that group, which is run again with
// one-workgroup panels.  Not inside the whole call (it reruns everything) nor when the panels are serial already.
inline bool group_retry_applies(bool whole_call, bool serial_panels) { return !whole_call && !serial_panels; }

// abort[2] is one word for all groups, and a group that a wait left unfinished raises it for fronts that are merely unfinished.  So
// the verdict of the groups that needed no rerun is kept, a rerun group starts from it (State::abort2_before goes back into
// abort[2]) and raises it again if one of its fronts does outlive the schedule.  true: run the group again.
inline bool after_group(State &s, bool wait_ran_out, int abort2)
{
    if (!wait_ran_out) s.abort2_before = abort2;
    return wait_ran_out;
}
inline void after_group_rerun(State &s, int abort2) { s.abort2_before = abort2; }

}  // namespace recover
