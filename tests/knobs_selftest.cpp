// Stand-alone check of csrc/stmmqr_knobs.h (tests/test_knobs_cpu.py builds it with g++ under ASan + UBSan): the table's defaults,
// overrides and reading rules, and the hipGraph key of RunKnobs.  It loops over the table, so a new row is covered as it stands.
#include <cstdio>
#include <string>

#include "stmmqr_knobs.h"

using namespace knobs;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void clear_all() { for (int i = 0; i < K_COUNT; i++) unsetenv(TABLE[i].name); }

// a text whose value under the row's rule differs from what the row reads when unset, and that value
static std::string other(const Row &r, double *want)
{
    if (r.rule == PRESENT) { *want = 1; return "0"; }              // (set at all, whatever the text)
    if (r.type == REAL) { *want = 2.5; return "2.5"; }
    if (r.type == FLAG) { *want = r.dflt != 0 ? 0 : 1; return r.dflt != 0 ? "0" : "1"; }
    if (r.rule == BOOLEAN) { *want = 0; return "0"; }
    *want = r.dflt + 3;                                            // (positive for every rule that clamps)
    return std::to_string((long)(r.dflt + 3));
}

int main()
{
    clear_all();
    for (int i = 0; i < K_COUNT; i++) {
        const Row &r = TABLE[i];
        CHECK(strncmp(r.name, "STMMQR_", 7) == 0 && r.doc && r.doc[0], "%s", r.name);
        for (int j = 0; j < i; j++) CHECK(strcmp(r.name, TABLE[j].name) != 0, "%s is listed twice", r.name);
        if (r.type == PATH) { CHECK(text((Id)i) == nullptr, "%s", r.name); continue; }
        CHECK(value((Id)i) == (r.rule == PRESENT ? 0.0 : r.dflt), "%s unset reads %g", r.name, value((Id)i));
    }
    for (int i = 0; i < K_COUNT; i++) {
        const Row &r = TABLE[i];
        if (r.type == PATH) {
            setenv(r.name, "/tmp/steps.txt", 1);
            CHECK(text((Id)i) && strcmp(text((Id)i), "/tmp/steps.txt") == 0, "%s", r.name);
        } else {
            double want = 0;
            const std::string s = other(r, &want);
            setenv(r.name, s.c_str(), 1);
            CHECK(value((Id)i) == want, "%s=%s reads %g, not %g", r.name, s.c_str(), value((Id)i), want);
            CHECK(num((Id)i) == (long)want && on((Id)i) == (want != 0), "%s=%s", r.name, s.c_str());
        }
        unsetenv(r.name);
    }
    // the reading rules
    CHECK(on(K_PASSENGERS) && RunKnobs::read().passengers, "unset means on");
    setenv("STMMQR_PASSENGERS", "0", 1);
    CHECK(!on(K_PASSENGERS) && !RunKnobs::read().passengers, "PASSENGERS=0 is off");
    setenv("STMMQR_PASSENGERS", "2", 1);
    CHECK(on(K_PASSENGERS), "PASSENGERS=2 is on");
    CHECK(on(K_CA_RIDERS) && on(K_QT4) && on(K_LIVE_PANELS) && !on(K_LA_SYSFENCE), "flag defaults");
    CHECK(BuildKnobs::read().early_end, "unset means on");
    setenv("STMMQR_EARLY_END", "0", 1);
    CHECK(!BuildKnobs::read().early_end, "EARLY_END=0 is off");
    setenv("STMMQR_SIDE_RESERVE", "-5", 1);
    CHECK(num(K_SIDE_RESERVE) == 0 && RunKnobs::read().side_reserve == 0, "SIDE_RESERVE=-5 reads %ld", num(K_SIDE_RESERVE));
    setenv("STMMQR_SIDE_RESERVE", "40", 1);
    CHECK(RunKnobs::read().side_reserve == 40, "SIDE_RESERVE=40");
    setenv("STMMQR_RSPW_W", "0", 1);
    CHECK(num(K_RSPW_W) == 2, "a non-positive RSPW_W reads as the default");
    setenv("STMMQR_RHS_BATCH", "0", 1);
    CHECK(num(K_RHS_BATCH) == 1, "RHS_BATCH is at least 1");
    setenv("STMMQR_PLAN_CACHE", "-3", 1);
    CHECK(num(K_PLAN_CACHE) == 0, "PLAN_CACHE is at least 0");
    CHECK(num(K_RESIDENT_CACHE) == -1, "RESIDENT_CACHE unset: the library decides");
    setenv("STMMQR_RESIDENT_CACHE", "7", 1);
    CHECK(num(K_RESIDENT_CACHE) == 1, "RESIDENT_CACHE=7 is on");
    CHECK(!on(K_MEMDUMP), "MEMDUMP unset");
    setenv("STMMQR_MEMDUMP", "", 1);
    CHECK(on(K_MEMDUMP), "MEMDUMP set to the empty text is on");
    clear_all();
    // the window of the download and the forced kept set
    CHECK(num(K_DOWNLOAD_WIN) == (32L << 20), "DOWNLOAD_WIN unset reads %ld", num(K_DOWNLOAD_WIN));
    for (const char *s : {"0", "-5", "text"}) {
        setenv("STMMQR_DOWNLOAD_WIN", s, 1);
        CHECK(num(K_DOWNLOAD_WIN) == (32L << 20), "DOWNLOAD_WIN=%s reads %ld, not the default", s, num(K_DOWNLOAD_WIN));
    }
    setenv("STMMQR_DOWNLOAD_WIN", "4096", 1);
    CHECK(num(K_DOWNLOAD_WIN) == 4096, "DOWNLOAD_WIN=4096 reads %ld", num(K_DOWNLOAD_WIN));
    CHECK(TABLE[K_DOWNLOAD_WIN].when == CALL && TABLE[K_DOWNLOAD_WIN].rule == POSITIVE, "DOWNLOAD_WIN: read at every download");
    CHECK(num(K_KEEP_FRONTS) == -1 && BuildKnobs::read().keep_fronts == -1, "KEEP_FRONTS unset: the planner chooses");
    setenv("STMMQR_KEEP_FRONTS", "0", 1);
    CHECK(num(K_KEEP_FRONTS) == 0 && BuildKnobs::read().keep_fronts == 0, "KEEP_FRONTS=0 reads %ld", num(K_KEEP_FRONTS));
    CHECK(TABLE[K_KEEP_FRONTS].when == SCHED && TABLE[K_KEEP_FRONTS].rule == PLAIN, "KEEP_FRONTS: read when a schedule is built");
    {
        // neither row is in the key of a captured graph
        clear_all();
        const unsigned long long k0 = RunKnobs::read().key();
        setenv("STMMQR_DOWNLOAD_WIN", "4096", 1); setenv("STMMQR_KEEP_FRONTS", "2", 1);
        CHECK(RunKnobs::read().key() == k0, "DOWNLOAD_WIN / KEEP_FRONTS move the key of the captured graph");
    }
    clear_all();
    const long long small = 1 << 20, large = 32LL << 20;
    CHECK(!BuildKnobs::read().recycles(small) && BuildKnobs::read().recycles(large), "RECYCLE unset: by size");
    setenv("STMMQR_RECYCLE", "1", 1);
    CHECK(!BuildKnobs::read().recycles(small) && BuildKnobs::read().recycles(large), "RECYCLE=1: by size");
    setenv("STMMQR_RECYCLE", "2", 1);
    CHECK(BuildKnobs::read().recycles(small), "RECYCLE=2: always");
    setenv("STMMQR_RECYCLE", "0", 1);
    CHECK(!BuildKnobs::read().recycles(large), "RECYCLE=0: never");
    setenv("STMMQR_RECYCLE", "3", 1);
    CHECK(!BuildKnobs::read().recycles(large), "RECYCLE=3: no mode");
    clear_all();
    setenv("STMMQR_LA_MIN", "7", 1); setenv("STMMQR_PASS_K", "0.5", 1); setenv("STMMQR_PAIR_MIN", "9", 1);
    CHECK(RunKnobs::read().la_min == 7 && RunKnobs::read().pass_k == 0.5 && BuildKnobs::read().pair_min == 9, "fields follow their rows");
    // once<>: the first call fixes the value
    setenv("STMMQR_PART_GRAIN", "512", 1);
    CHECK(once<K_PART_GRAIN>() == 512, "first read");
    setenv("STMMQR_PART_GRAIN", "1024", 1);
    CHECK(once<K_PART_GRAIN>() == 512 && num(K_PART_GRAIN) == 1024, "once per process");
    // the hipGraph key: equal for equal environments, another one after every RUN knob
    clear_all();
    const unsigned long long key0 = RunKnobs::read().key(), plan0 = fold_plan_knobs(1);
    CHECK(key0 == RunKnobs::read().key(), "two reads of one environment");
    int nrun = 0;
    for (int i = 0; i < K_COUNT; i++) {
        const Row &r = TABLE[i];
        if (r.type == PATH) continue;
        double want = 0;
        const std::string s = other(r, &want);
        setenv(r.name, s.c_str(), 1);
        const unsigned long long key = RunKnobs::read().key();
        if (r.when == RUN) { nrun++; CHECK(key != key0, "%s=%s leaves the key of the captured graph as it was", r.name, s.c_str()); }
        else CHECK(key == key0, "%s is no RUN knob but moves the key", r.name);
        CHECK(key == RunKnobs::read().key(), "%s=%s: two reads", r.name, s.c_str());
        CHECK((fold_plan_knobs(1) != plan0) == (r.when == PLAN || r.when == SCHED), "%s and the plan cache", r.name);
        unsetenv(r.name);
        CHECK(RunKnobs::read().key() == key0, "%s unset again", r.name);
    }
    CHECK(nrun >= 14, "%d RUN rows", nrun);
    printf("knobs: %d rows, %d run knobs, %d failures\n", (int)K_COUNT, nrun, failures);
    return failures ? 1 : 0;
}
