// Stand-alone check of csrc/stmmqr_recover.h (tests/test_recover_cpu.py builds it with g++ under ASan + UBSan): the recovery policy
// of the factorization driver walked without a GPU -- the classification of a finished pass, the whole call's loop, the phased
// caller's begin, stmmqr_plan_set_early_end, the group retry's abort[2] rule, and that the whole call always ends.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "stmmqr_recover.h"

using namespace recover;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static bool same_persistent(const State &a, const State &b)
{
    return a.rh_grow == b.rh_grow && a.overflowed == b.overflowed && a.full_schedule == b.full_schedule && a.early_phased == b.early_phased;
}

// What the device and the planner do around the policy, as far as the policy can see it: the plan recycles its slabs unless it was
// created without recycling or State::overflowed is set, its schedule is cut unless the knob is off or State::full_schedule is set
// -- both as of the last REBUILD, which is when the planner reads the state.
struct Model {
    bool recycles0, cut0;
    State s;
    WholeCall w;
    bool recycles, cut;
    int rebuilds = 0;
    Model(bool r, bool c) : recycles0(r), cut0(c), recycles(r), cut(c) {}
    void rebuild() { recycles = recycles0 && !s.overflowed; cut = cut0 && !s.full_schedule; rebuilds++; }
    // one pass of stmmqr_factorize_device ending as `o`: begin, finish, the policy, the rebuild
    Action pass(Outcome o)
    {
        s.last = Outcome::DONE;                          // (begin)
        if (o != Outcome::DONE) record(s, o);            // (finish)
        const Action a = after_pass(s, w, o, recycles);
        if (a == Action::REBUILD) rebuild();
        return a;
    }
};

static void check_classification()
{
    // all 16 combinations of the four facts: a refused message first, then the wait, then the schedule, then the arena
    for (int m = 0; m < 16; m++) {
        const bool refused = m & 1, wait = m & 2, outlived = m & 4, overflow = m & 8;
        const Outcome want = refused ? Outcome::REFUSED_MESSAGE : wait ? Outcome::WAIT_RAN_OUT : outlived ? Outcome::OUTLIVED_SCHEDULE
                           : overflow ? Outcome::ARENA_OVERFLOW : Outcome::DONE;
        CHECK(classify(refused, wait, outlived, overflow) == want, "facts %d", m);
    }
    // (spelled out: a wait that ran out also looks like an outlived schedule and may overflow the arena, and wins over both)
    CHECK(classify(false, true, true, true) == Outcome::WAIT_RAN_OUT, "wait + outlived + overflow");
    CHECK(classify(false, false, true, true) == Outcome::OUTLIVED_SCHEDULE, "outlived + overflow");
    CHECK(classify(false, false, false, false) == Outcome::DONE, "nothing");
}

static void check_whole_call()
{
    {   // overflow -> hard bound -> overflow -> no recycling -> done; both attempts again each time
        Model M(true, true);
        CHECK(M.w.retries() == 0 && M.w.reschedules == 0, "first pass");
        CHECK(M.pass(Outcome::ARENA_OVERFLOW) == Action::REBUILD, "first overflow");
        CHECK(M.s.rh_grow == 1 && !M.s.overflowed && M.recycles && M.s.last == Outcome::DONE, "the arena at its hard bound");
        CHECK(!M.w.serial && M.w.retries() == 1 && M.w.reschedules == 0, "retries %d", M.w.retries());
        CHECK(M.pass(Outcome::ARENA_OVERFLOW) == Action::REBUILD, "second overflow");
        CHECK(M.s.rh_grow == 1 && M.s.overflowed && !M.recycles, "no recycling");
        CHECK(!M.w.serial && M.w.retries() == 2, "retries %d", M.w.retries());
        CHECK(M.pass(Outcome::DONE) == Action::RETURN && M.w.retries() == 2 && !M.s.full_schedule && M.rebuilds == 2, "done");
    }
    {   // an overflow on the serial attempt: the arena grows, and the parallel attempt comes first again
        Model M(true, true);
        CHECK(M.pass(Outcome::WAIT_RAN_OUT) == Action::RERUN_SERIAL && M.w.serial, "wait");
        CHECK(M.pass(Outcome::ARENA_OVERFLOW) == Action::REBUILD && !M.w.serial && M.w.retries() == 1 && M.s.rh_grow == 1, "overflow of the serial attempt");
    }
    {   // outlived -> the full schedule, one reschedule, no retry
        Model M(true, true);
        CHECK(M.pass(Outcome::OUTLIVED_SCHEDULE) == Action::REBUILD, "outlived");
        CHECK(M.s.full_schedule && !M.cut && M.s.rh_grow == 0 && !M.s.overflowed && M.s.last == Outcome::DONE, "the full schedule");
        CHECK(M.w.reschedules == 1 && M.w.retries() == 0 && !M.w.serial, "one reschedule");
        CHECK(M.pass(Outcome::DONE) == Action::RETURN && M.w.reschedules == 1 && M.w.retries() == 0 && M.rebuilds == 1, "done");
    }
    {   // wait -> serial -> success, retries == 1, same schedule
        Model M(true, true);
        const State before = M.s;
        CHECK(M.pass(Outcome::WAIT_RAN_OUT) == Action::RERUN_SERIAL, "wait on the parallel attempt");
        CHECK(M.w.serial && M.w.retries() == 1 && M.w.reschedules == 0 && M.rebuilds == 0 && same_persistent(M.s, before), "serial rerun");
        CHECK(M.pass(Outcome::DONE) == Action::RETURN && M.rebuilds == 0 && same_persistent(M.s, before), "done");
        CHECK(!M.w.serial, "the plan is left with parallel panels");
    }
    {   // wait on the serial attempt -> the error goes up
        Model M(true, true);
        const State before = M.s;
        CHECK(M.pass(Outcome::WAIT_RAN_OUT) == Action::RERUN_SERIAL, "wait on the parallel attempt");
        CHECK(M.pass(Outcome::WAIT_RAN_OUT) == Action::RETURN, "wait on the serial attempt");
        CHECK(M.s.last == Outcome::WAIT_RAN_OUT && M.rebuilds == 0 && same_persistent(M.s, before) && !M.w.serial, "nothing else changes");
    }
    {   // wait with abort[2] and the overflow word set together -> the serial retry only
        Model M(true, true);
        const State before = M.s;
        CHECK(M.pass(classify(false, true, true, true)) == Action::RERUN_SERIAL, "wait + outlived + overflow");
        CHECK(M.s.rh_grow == 0 && !M.s.overflowed && !M.s.full_schedule && same_persistent(M.s, before) && M.rebuilds == 0, "rh_grow and full_schedule untouched");
        CHECK(M.w.retries() == 1 && M.w.reschedules == 0, "one retry");
    }
    {   // an overflow that belongs to an outlived schedule does not grow the arena
        Model M(true, true);
        CHECK(M.pass(classify(false, false, true, true)) == Action::REBUILD && M.s.full_schedule && M.s.rh_grow == 0 && M.w.reschedules == 1 && M.w.retries() == 0,
              "outlived + overflow");
    }
    {   // a refused message -> nothing changes, on either attempt
        Model M(true, true);
        const State before = M.s;
        CHECK(M.pass(Outcome::REFUSED_MESSAGE) == Action::RETURN && same_persistent(M.s, before) && M.rebuilds == 0 && !M.w.serial && M.w.retries() == 0, "refused");
        Model N(true, true);
        N.pass(Outcome::WAIT_RAN_OUT);
        CHECK(N.pass(Outcome::REFUSED_MESSAGE) == Action::RETURN && same_persistent(N.s, before) && N.rebuilds == 0 && !N.w.serial, "refused on the serial attempt");
    }
    {   // an error that finish did not classify (DONE stands for it) goes up and leaves the plan with parallel panels
        Model M(true, true);
        M.pass(Outcome::WAIT_RAN_OUT);
        CHECK(M.pass(Outcome::DONE) == Action::RETURN && !M.w.serial, "done / unclassified");
    }
}

// ---- termination ----
// Every REBUILD flips exactly one of rh_grow (0 -> 1), overflowed and full_schedule, none of which ever flips back: at most
// 2 * recycles0 + cut0 rebuilds, because under (P2) a plan that never recycled sees no overflow, after `overflowed` the planner
// stops recycling, and under (P1) nothing is outlived once full_schedule is set or where the schedule was never cut.  Between two
// rebuilds, and after the last, there are at most two passes: the parallel attempt, and the serial one if a wait ran out (a second
// wait goes up); the pass that causes a rebuild may be either.  So at most 2 * (1 + 2 * recycles0 + cut0) passes, 8 at the most,
// and the sequence (wait, overflow) (wait, overflow) (wait, outlived) (wait, wait) reaches it.
static int deepest;
static void walk(const Model &M, int depth, int bound)
{
    static const Outcome all[] = {Outcome::DONE, Outcome::REFUSED_MESSAGE, Outcome::WAIT_RAN_OUT, Outcome::OUTLIVED_SCHEDULE, Outcome::ARENA_OVERFLOW};
    for (Outcome o : all) {
        if (o == Outcome::OUTLIVED_SCHEDULE && !M.cut) continue;          // (P1)
        if (o == Outcome::ARENA_OVERFLOW && !M.recycles) continue;        // (P2)
        Model N = M;
        const Action a = N.pass(o);
        deepest = std::max(deepest, depth + 1);
        if (a == Action::RETURN) continue;
        if (depth + 1 >= bound) { CHECK(false, "the whole call goes on after %d passes", depth + 1); continue; }
        walk(N, depth + 1, bound);
    }
}
static void check_termination()
{
    for (int r = 0; r < 2; r++)
        for (int c = 0; c < 2; c++) {
            const int bound = 2 * (1 + 2 * r + c);
            deepest = 0;
            walk(Model(r != 0, c != 0), 0, bound);
            CHECK(deepest == bound, "recycles %d cut %d: %d passes at the most, bound %d", r, c, deepest, bound);
        }
}

static void check_phased_begin()
{
    const Outcome all[] = {Outcome::DONE, Outcome::REFUSED_MESSAGE, Outcome::WAIT_RAN_OUT, Outcome::OUTLIVED_SCHEDULE, Outcome::ARENA_OVERFLOW};
    // a caller that asked for the cut schedule, on a recycling plan
    for (Outcome o : all) {
        State s;
        s.early_phased = true;
        record(s, o);
        const State before = s;
        const Action a = at_phased_begin(s, /*cut_in_force*/ true, /*recycles*/ true);
        const bool rebuild = o == Outcome::OUTLIVED_SCHEDULE || o == Outcome::ARENA_OVERFLOW;
        CHECK((a == Action::REBUILD) == rebuild, "outcome %d", (int)o);
        CHECK(s.full_schedule == (o == Outcome::OUTLIVED_SCHEDULE), "outcome %d: full_schedule", (int)o);
        CHECK(s.rh_grow == before.rh_grow && s.overflowed == before.overflowed && s.early_phased, "outcome %d: begin grows nothing itself", (int)o);
        CHECK(s.rh_grow == (o == Outcome::ARENA_OVERFLOW ? 1 : 0), "outcome %d: finish has grown the arena", (int)o);
        if (rebuild) CHECK(s.last == Outcome::DONE, "outcome %d: acted on", (int)o);
        // the same begin again: nothing more to do (the schedule is full now, or the arena larger)
        CHECK(at_phased_begin(s, /*cut_in_force*/ !s.full_schedule, true) == Action::RETURN || !rebuild, "outcome %d: twice", (int)o);
    }
    {   // a cut schedule in force that the caller never asked for (a fresh whole-tree plan): the full schedule, whatever the last outcome
        for (Outcome o : all) {
            State s;
            record(s, o);
            CHECK(at_phased_begin(s, true, true) == Action::REBUILD && s.full_schedule && s.last == Outcome::DONE, "outcome %d", (int)o);
            CHECK(at_phased_begin(s, false, true) == Action::RETURN, "outcome %d: once", (int)o);
        }
    }
    {   // overflow on a plan that does not recycle (a sharded plan never reports one: (P2)): no rebuild
        State s;
        record(s, Outcome::ARENA_OVERFLOW);
        CHECK(at_phased_begin(s, false, false) == Action::RETURN && !s.full_schedule, "no recycling, no rebuild");
    }
    {   // overflow twice: hard bound, then no recycling
        State s;
        record(s, Outcome::ARENA_OVERFLOW);
        CHECK(at_phased_begin(s, false, true) == Action::REBUILD && s.rh_grow == 1 && !s.overflowed, "hard bound");
        record(s, Outcome::ARENA_OVERFLOW);
        CHECK(at_phased_begin(s, false, true) == Action::REBUILD && s.rh_grow == 1 && s.overflowed, "no recycling");
    }
    {   // after a wait: nothing, and the full schedule is not forced on a caller who asked for the cut one
        State s;
        s.early_phased = true;
        record(s, Outcome::WAIT_RAN_OUT);
        CHECK(at_phased_begin(s, true, true) == Action::RETURN && !s.full_schedule && s.rh_grow == 0, "wait");
    }
}

// A phased finish fails, and the caller goes on with the whole call on the same plan without a begin of its own in between.  The
// whole call's begin starts from DONE like every begin: its loop acts on its own passes only, and the next phased begin sees the
// whole call's last outcome.  (With one flag per failure, the phased failure's flag outlived the whole call.)
static void check_phased_failure_then_whole_call()
{
    {   // phased: outlived.  Whole call: a wait on the parallel attempt is a wait (serial rerun, no reschedule), then done.
        Model M(true, true);
        M.s.early_phased = true;
        record(M.s, Outcome::OUTLIVED_SCHEDULE);
        const State before = M.s;
        CHECK(M.pass(Outcome::WAIT_RAN_OUT) == Action::RERUN_SERIAL && M.w.reschedules == 0 && M.rebuilds == 0, "the wait is the whole call's own");
        CHECK(M.pass(Outcome::DONE) == Action::RETURN && M.s.last == Outcome::DONE && same_persistent(M.s, before), "done");
        // the next phased begin: the cut schedule the caller asked for held in the whole call, and stays
        CHECK(at_phased_begin(M.s, true, true) == Action::RETURN && !M.s.full_schedule, "no full schedule forced by the old failure");
        // ... and stmmqr_plan_set_early_end is judged by the whole call's finish (which cleared `begun`), not by the old one
        CHECK(set_early_end(M.s, false, 1), "allowed");
    }
    {   // phased: overflow (finish has grown the arena).  Whole call: done on the old schedule.  The growth is kept for the next
        // rebuild, but no begin rebuilds for it
        Model M(true, false);
        record(M.s, Outcome::ARENA_OVERFLOW);
        CHECK(M.pass(Outcome::DONE) == Action::RETURN && M.rebuilds == 0 && M.w.retries() == 0, "done");
        CHECK(M.s.rh_grow == 1 && !M.s.overflowed && M.s.last == Outcome::DONE, "the growth is kept");
        CHECK(at_phased_begin(M.s, false, true) == Action::RETURN, "nothing left to act on");
    }
    {   // phased: overflow.  Whole call: its own overflow is the second one of the plan
        Model M(true, false);
        record(M.s, Outcome::ARENA_OVERFLOW);
        CHECK(M.pass(Outcome::ARENA_OVERFLOW) == Action::REBUILD && M.s.overflowed && !M.recycles && M.w.retries() == 1, "no recycling");
    }
    {   // phased: a wait that the group retry could not cure.  Whole call: an error finish did not classify goes up as it is
        Model M(true, true);
        record(M.s, Outcome::WAIT_RAN_OUT);
        CHECK(M.pass(Outcome::DONE) == Action::RETURN && !M.w.serial && M.s.last == Outcome::DONE, "not taken for a wait of this pass");
    }
}

static void check_set_early_end()
{
    const Outcome all[] = {Outcome::DONE, Outcome::REFUSED_MESSAGE, Outcome::WAIT_RAN_OUT, Outcome::OUTLIVED_SCHEDULE, Outcome::ARENA_OVERFLOW};
    for (int mode = 0; mode < 2; mode++) {
        {   // outside begin .. finish: allowed
            State s;
            CHECK(set_early_end(s, false, mode) && s.early_phased == (mode != 0) && s.full_schedule == (mode == 0), "mode %d", mode);
        }
        for (Outcome o : all) {
            // between begin and finish (last == DONE: no finish yet), or after a failed finish, which leaves `begun` set
            State s;
            s.early_phased = true;
            if (o != Outcome::DONE) record(s, o);
            const State before = s;
            const bool ok = set_early_end(s, true, mode);
            CHECK(ok == (o == Outcome::OUTLIVED_SCHEDULE), "mode %d after outcome %d", mode, (int)o);
            if (ok) CHECK(s.last == Outcome::DONE && s.early_phased == (mode != 0) && s.full_schedule == (mode == 0), "mode %d: set", mode);
            else CHECK(same_persistent(s, before) && s.last == before.last, "mode %d after outcome %d: a refused call changes nothing", mode, (int)o);
        }
    }
    {   // mode 1 takes back a full schedule that an outlived one had forced
        State s;
        s.full_schedule = true;
        CHECK(set_early_end(s, false, 1) && !s.full_schedule && s.early_phased, "cut again");
        CHECK(at_phased_begin(s, true, true) == Action::RETURN, "the caller asked for it");
    }
}

static void check_group_retry()
{
    CHECK(group_retry_applies(false, false), "phased, parallel panels");
    CHECK(!group_retry_applies(true, false) && !group_retry_applies(false, true) && !group_retry_applies(true, true), "not in the whole call, not with serial panels");
    State s;
    // group 0 ends clean with abort[2] raised (a front of it outlived the schedule): kept
    CHECK(!after_group(s, false, 1) && s.abort2_before == 1, "group 0");
    // group 1: the wait ran out, abort[2] says 7 for its unfinished fronts: rerun, and the rerun starts from group 0's verdict
    CHECK(after_group(s, true, 7) && s.abort2_before == 1, "group 1, first run");
    after_group_rerun(s, 1);
    CHECK(s.abort2_before == 1, "group 1, rerun");
    // a fresh pass where only the rerun raises it
    State t;
    CHECK(!after_group(t, false, 0) && t.abort2_before == 0, "group 0");
    CHECK(after_group(t, true, 1) && t.abort2_before == 0, "group 1: the wait's own abort[2] is not a verdict");
    after_group_rerun(t, 1);
    CHECK(t.abort2_before == 1, "group 1's rerun does outlive the schedule");
}

int main()
{
    check_classification();
    check_whole_call();
    check_termination();
    check_phased_begin();
    check_phased_failure_then_whole_call();
    check_set_early_end();
    check_group_retry();
    printf("recover_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
