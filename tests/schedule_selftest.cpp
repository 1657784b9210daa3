// Stand-alone check of the pure planner, csrc/stmmqr_schedule.cpp (tests/test_schedule_cpu.py builds both with g++ under ASan + UBSan):
// schedules built as values from hand-written trees and, given as files on the command line, from the symbolic analyses of golden
// fixtures -- under every grouping and setting that sends the builder down another path -- and checked for what the step scheduler and the
// kernels rely on.  No GPU, no plan.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <string>

#include "stmmqr_sched.h"

using namespace sched;

static int failures = 0;
static std::string ctx;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures < 40) { printf("FAILED %s:%d [%s]  %s  ", __FILE__, __LINE__, ctx.c_str(), #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- a symbolic analysis: what the plan keeps of one ------------------------------------------------------------------------------
struct Tree {
    std::string name;
    long nf = 0, n = 0, maxstack = 0;
    int do_rank = 1, keep_h = 1;
    std::vector<long> Sleft, Super, Rp, Hip, Child, Childp, Post, Fm, Rj;     // Fm empty: recomputed
    Fronts F;
};

// Hand-written: fronts numbered in postorder; front f has fp[f] pivotal columns, rows[f] rows of S in each of them and cn[f] further
// columns: the first cn[f] of its ancestors' pivotal columns, the parent's first (so a child's columns are columns of its parent as
// long as cn[child] <= fp[parent] + cn[parent]).
static Tree make_tree(const char *name, const std::vector<int> &parent, const std::vector<int> &fp, const std::vector<int> &cn, const std::vector<int> &rows)
{
    Tree T;
    T.name = name;
    const long nf = T.nf = (long)parent.size();
    T.Super.assign(nf + 1, 0);
    for (long f = 0; f < nf; f++) T.Super[f + 1] = T.Super[f] + fp[f];
    T.n = T.Super[nf];
    T.Sleft.assign(T.n + 2, 0);
    for (long f = 0; f < nf; f++)
        for (long j = T.Super[f]; j < T.Super[f + 1]; j++) T.Sleft[j + 1] = T.Sleft[j] + rows[f];
    T.Sleft[T.n + 1] = T.Sleft[T.n];
    T.Rp.assign(nf + 1, 0);
    for (long f = 0; f < nf; f++) {
        T.Rp[f] = (long)T.Rj.size();
        for (long j = T.Super[f]; j < T.Super[f + 1]; j++) T.Rj.push_back(j);
        int left = cn[f];
        for (int a = parent[f]; a >= 0 && left > 0; a = parent[a])
            for (long j = T.Super[a]; j < T.Super[a + 1] && left > 0; j++, left--) T.Rj.push_back(j);
        if (left > 0) { printf("tree %s: front %ld wants more columns than its ancestors have\n", name, f); exit(2); }
    }
    T.Rp[nf] = (long)T.Rj.size();
    T.Childp.assign(nf + 2, 0);
    for (long f = 0; f < nf; f++) if (parent[f] >= 0) T.Childp[parent[f] + 1]++;
    for (long f = 0; f < nf; f++) T.Childp[f + 1] += T.Childp[f];
    T.Childp[nf + 1] = T.Childp[nf];
    T.Child.assign(nf + 1, 0);
    std::vector<long> at(T.Childp.begin(), T.Childp.end());
    for (long f = 0; f < nf; f++) if (parent[f] >= 0) T.Child[at[parent[f]]++] = f;
    T.Post.resize(nf);
    for (long f = 0; f < nf; f++) T.Post[f] = f;
    T.Hip.assign(nf + 1, 0);
    return T;
}

// "key count v v v ..." records, as tests/test_schedule_cpu.py writes them from a golden .npz
static Tree read_tree(const char *path)
{
    Tree T;
    std::ifstream in(path);
    std::string key;
    long cnt;
    std::map<std::string, std::vector<long>> rec;
    while (in >> key >> cnt) {
        if (key == "name") { in >> T.name; continue; }
        std::vector<long> &v = rec[key];
        v.resize((size_t)cnt);
        for (long &x : v) in >> x;
    }
    if (!in.eof() || rec.count("nf") == 0) { printf("cannot read %s\n", path); exit(2); }
    T.nf = rec["nf"][0]; T.n = rec["n"][0]; T.maxstack = rec["maxstack"][0]; T.do_rank = (int)rec["do_rank"][0]; T.keep_h = (int)rec["keep_h"][0];
    T.Sleft = rec["Sleft"]; T.Super = rec["Super"]; T.Rp = rec["Rp"]; T.Hip = rec["Hip"]; T.Child = rec["Child"]; T.Childp = rec["Childp"];
    T.Post = rec["Post"]; T.Fm = rec["Fm"]; T.Rj = rec["Rj"];
    T.Post.resize((size_t)T.nf);
    return T;
}

// the pure half of build_plan: sizes, then the estimate of the packed factors from the relative indices (child column -> parent column)
static void analyse(Tree &T)
{
    const Symbolic sv{T.nf, T.Sleft, T.Super, T.Rp, T.Hip, T.Child, T.Childp, T.Post, T.Fm.empty() ? nullptr : T.Fm.data(), T.do_rank, T.keep_h, 1L << 20, 1L << 62};
    std::string msg;
    ctx = T.name;
    CHECK(front_syms(sv, T.F, msg) == 0, "%s", msg.c_str());
    std::vector<int> Rjrel(std::max<size_t>(1, T.Rj.size()), 0), Fmap((size_t)std::max(1L, T.n), -1);
    for (long f = 0; f < T.nf; f++) {
        for (long j = T.Rp[f]; j < T.Rp[f + 1]; j++) Fmap[(size_t)T.Rj[j]] = (int)(j - T.Rp[f]);
        for (long q = T.Childp[f]; q < T.Childp[f + 1]; q++) {
            const long c = T.Child[q], pc = T.Rp[c] + (T.Super[c + 1] - T.Super[c]);
            for (long j = pc; j < T.Rp[c + 1]; j++) {
                Rjrel[(size_t)j] = Fmap[(size_t)T.Rj[j]];
                CHECK(Rjrel[(size_t)j] >= 0 && T.Rj[T.Rp[f] + Rjrel[(size_t)j]] == T.Rj[j], "front %ld: column %ld of child %ld is none of its columns", f, T.Rj[j], c);
            }
        }
    }
    rh_estimate(sv, Rjrel, T.F);
    long long tot = 0, pan = 0;
    for (long f = 0; f < T.nf; f++) {
        const FrontSym &s = T.F.fs[f];
        tot += T.F.rh_est_front[f];
        pan += s.npanels;
        CHECK(s.fn == T.Rp[f + 1] - T.Rp[f] && s.fp == T.Super[f + 1] - T.Super[f] && s.fm_ub == T.F.Fm[f] && s.fm_est <= s.fm_ub && s.ld >= s.fm_ub && s.ld % 2 == 0,
              "front %ld: fn %d fp %d fm_ub %d fm_est %d ld %d", f, s.fn, s.fp, s.fm_ub, s.fm_est, s.ld);
        CHECK(T.F.rh_est_front[f] >= 0 && T.F.rh_est_front[f] <= (long long)s.fm_ub * s.fn, "front %ld: estimate %lld of a %d x %d front", f, T.F.rh_est_front[f], s.fm_ub, s.fn);
    }
    CHECK(tot == T.F.rh_est_total && pan == T.F.tpanels, "totals %lld / %lld, %lld / %lld", tot, T.F.rh_est_total, pan, T.F.tpanels);
}

// ---- one configuration ------------------------------------------------------------------------------------------------------------------
struct Config {
    std::string name;
    std::vector<int> group;
    std::vector<char> shared;
    Options opt{64, 4, STM_TALL_MIN, 0};                 // the library's defaults
    knobs::BuildKnobs k = knobs::BuildKnobs::read();     // (the test runs with no STMMQR_* variable set: the table's defaults)
    bool full_schedule = false, early_phased = false;
};

static Schedule build_for(const Tree &T, const Config &c)
{
    const Inputs in{T.nf, T.Post, T.Child, T.Childp, T.F.fs, T.do_rank, T.keep_h, T.maxstack, T.F.rh_est_total, T.F.rh_est_front, 1.0, c.group, c.shared,
                    c.opt, c.k, 2048, 4096, false, 0, c.full_schedule, c.early_phased};
    return build(in);
}

template <class V> static bool same_bytes(const std::vector<V> &a, const std::vector<V> &b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}
static bool same(const Schedule &a, const Schedule &b)
{
    bool e = same_bytes(a.fs, b.fs) && same_bytes(a.fs_scr, b.fs_scr) && a.lists == b.lists && a.wlists == b.wlists && a.tslot == b.tslot && a.pair_front == b.pair_front &&
             a.ypoff == b.ypoff && a.has_c == b.has_c && a.c_slot == b.c_slot && a.kept == b.kept && a.f_t0 == b.f_t0 && a.f_t1 == b.f_t1 && a.c_t1 == b.c_t1 &&
             a.glevels.size() == b.glevels.size() && a.gsteps.size() == b.gsteps.size();
    for (size_t g = 0; e && g < a.gsteps.size(); g++) e = same_bytes(a.glevels[g], b.glevels[g]) && same_bytes(a.gsteps[g], b.gsteps[g]);
    const long long sa[] = {a.tslots, a.gp_slabs, a.wp_doubles, a.wp2_doubles, a.sweep, a.yp_doubles, a.farena, a.carena, a.recycle, a.rh_cap, a.scr_doubles, a.own_off,
                            a.n_own, a.post_off, a.rh_parts_off, a.rh_maxparts, a.early_end, a.ca_min, a.plan_algo, a.tall_min, a.tune};
    const long long sb[] = {b.tslots, b.gp_slabs, b.wp_doubles, b.wp2_doubles, b.sweep, b.yp_doubles, b.farena, b.carena, b.recycle, b.rh_cap, b.scr_doubles, b.own_off,
                            b.n_own, b.post_off, b.rh_parts_off, b.rh_maxparts, b.early_end, b.ca_min, b.plan_algo, b.tall_min, b.tune};
    return e && memcmp(sa, sb, sizeof sa) == 0;
}

struct Range { long long a, b; int t0, t1; long f; };      // addresses [a, b) while steps [t0, t1]
// no two ranges that are alive in a common step share an address; all inside [0, cap)
static void check_disjoint(std::vector<Range> R, long long cap, const char *what)
{
    std::sort(R.begin(), R.end(), [](const Range &x, const Range &y) { return x.a < y.a; });
    for (size_t i = 0; i < R.size(); i++) {
        CHECK(R[i].a >= 0 && R[i].b <= cap, "%s of front %ld: [%lld, %lld) outside %lld", what, R[i].f, R[i].a, R[i].b, cap);
        for (size_t j = i + 1; j < R.size() && R[j].a < R[i].b; j++)
            CHECK(R[j].t0 > R[i].t1 || R[i].t0 > R[j].t1, "%s of fronts %ld and %ld overlap: [%lld, %lld) steps %d-%d, [%lld, %lld) steps %d-%d", what, R[i].f, R[j].f,
                  R[i].a, R[i].b, R[i].t0, R[i].t1, R[j].a, R[j].b, R[j].t0, R[j].t1);
    }
}

static void check_schedule(const Tree &T, const Config &c)
{
    ctx = T.name + " / " + c.name;
    const int failed_before = failures;
    const Schedule S = build_for(T, c);
    CHECK(same(S, build_for(T, c)), "two builds from the same inputs differ");
    const long nf = T.nf;
    const size_t NL = S.lists.size();
    auto big = [&](long f) { return is_big(S.fs[f], c.opt.big_front_cols); };
    auto sharedf = [&](long f) { return (size_t)f < c.shared.size() && c.shared[(size_t)f]; };
    auto slab = [&](long f) { return (long long)S.fs[f].ld * S.fs[f].fn; };
    // a front's slice of the update workspace at panel p: (column blocks + the Gram block) x slabs of 32 x 32 partial sums; the sweep
    // fronts w blocks per partial at the stride of stm_pair_slots / stm_quad_slots, or the panel-by-panel updates' w + 1 column blocks
    auto slice = [&](long f, int p) {
        const long long ncb = stm_upd_ncb(S.fs[f], p), nsl = stm_upd_nsl(S.fs[f]), w = S.sweep;
        if (!S.pair_front[f]) return (ncb + 1) * nsl * (STM_NB * 32);
        return std::max((ncb + w - 1) * (w == 4 ? stm_quad_slots((int)nsl, S.tune) : stm_pair_slots((int)nsl, S.tune)) * (w * STM_NB * 32), (w + 1) * nsl * (STM_NB * 32));
    };
    int ngroups = 1;
    for (long f = 0; f < nf; f++) ngroups = std::max(ngroups, c.group[f] + 1);
    CHECK((int)S.gsteps.size() == ngroups && (int)S.glevels.size() == ngroups, "%zu step lists, %zu level lists for %d groups", S.gsteps.size(), S.glevels.size(), ngroups);
    if ((int)S.gsteps.size() != ngroups || (int)S.glevels.size() != ngroups) return;
    CHECK(S.fs.size() == (size_t)nf && S.tslot.size() >= (size_t)nf && S.c_slot.size() >= (size_t)nf && S.has_c.size() >= (size_t)nf, "per-front arrays are short");

    // ---- every front of a group starts exactly once, in that group; its panels 0 .. nsched-1 appear once each, in order, at increasing steps
    // (the envelope rule may let a front sit out a step); what it is packed (small: the step it runs in) ----
    std::vector<int> start(nf, -1), packed(nf, -1), next_panel(nf, 0), last_step(nf, -1), in_level(nf, 0);
    for (int g = 0; g < ngroups; g++) {
        for (const Level &L : S.glevels[g]) {
            CHECK(L.all_off >= 0 && L.n_all >= 0 && (size_t)L.all_off + (size_t)L.n_all <= NL && L.n_all == L.n_small + L.n_big, "level list [%d, +%d) of %zu", L.all_off, L.n_all, NL);
            for (int q = 0; q < L.n_all && (size_t)(L.all_off + q) < NL; q++) {
                const int f = S.lists[(size_t)(L.all_off + q)];
                CHECK(f >= 0 && f < nf && c.group[f] == g && big(f) == (q >= L.n_small), "level of group %d lists front %d", g, f);
                if (f >= 0 && f < nf) in_level[f]++;
            }
        }
        const std::vector<Step> &SV = S.gsteps[g];
        for (int t = 0; t < (int)SV.size(); t++) {
            const Step &s = SV[(size_t)t];
            auto inside = [&](int off, int cnt) { return off >= 0 && cnt >= 0 && (size_t)off + (size_t)cnt <= NL; };
            CHECK(inside(s.start_off, s.n_start) && inside(s.asm_parts_off, s.n_start) && inside(s.act_off, s.n_act) && inside(s.plist_off, s.n_act) &&
                      inside(s.cpk_off, s.n_cpk) && inside(s.cpk_parts_off, s.n_cpk) && s.wp_off >= 0 && (size_t)s.wp_off + (size_t)s.n_act <= S.wlists.size() &&
                      (!S.recycle || (inside(s.rhp_off, s.n_rhp) && inside(s.rhp_parts_off, s.n_rhp))) && s.n_small <= s.n_start &&
                      s.n_norm + s.n_sweep() == s.n_act,
                  "group %d step %d: a list of the step leaves lists (%zu) / wlists (%zu)", g, t, NL, S.wlists.size());
            if (failures != failed_before) return;
            for (int i = 0; i < s.n_start; i++) {
                const int f = S.lists[(size_t)(s.start_off + i)];
                CHECK(f >= 0 && f < nf && c.group[f] == g && start[f] < 0 && big(f) == (i >= s.n_small), "group %d step %d starts front %d (group %d, started at %d)", g, t, f,
                      f >= 0 && f < nf ? c.group[f] : -9, f >= 0 && f < nf ? start[f] : -9);
                if (f < 0 || f >= nf) continue;
                start[f] = t;
                if (!big(f)) packed[f] = t;
                const int parts = S.lists[(size_t)(s.asm_parts_off + i)];
                CHECK(parts >= 1 && parts <= s.asm_maxparts && parts <= 4096, "front %d: %d assembly parts (max %d)", f, parts, s.asm_maxparts);
            }
            std::set<int> slots;
            long long wp_end = 0;
            for (int i = 0; i < s.n_act; i++) {
                const int f = S.lists[(size_t)(s.act_off + i)], p = S.lists[(size_t)(s.plist_off + i)];
                CHECK(f >= 0 && f < nf && big(f) && c.group[f] == g, "group %d step %d: front %d in flight", g, t, f);
                if (f < 0 || f >= nf) continue;
                CHECK(p == next_panel[f] && last_step[f] < t && start[f] >= 0 && start[f] == (p == 0 ? t : start[f]), "front %d: panel %d at step %d (next %d, last step %d, start %d)", f, p,
                      t, next_panel[f], last_step[f], start[f]);
                next_panel[f] = p + 1; last_step[f] = t;
                CHECK(S.tslot[f] >= 0 && S.tslot[f] < S.tslots && slots.insert(S.tslot[f]).second, "front %d: T slot %d of %d taken twice in step %d", f, S.tslot[f], S.tslots, t);
                const long long w = S.wlists[(size_t)(s.wp_off + i)];
                CHECK(w >= wp_end && w <= S.wp_doubles, "front %d: workspace slice at %lld (previous ends %lld, all %lld)", f, w, wp_end, S.wp_doubles);
                wp_end = w + slice(f, p);
                CHECK(stm_ca_slabs(S.fs[f]) <= S.gp_slabs, "front %d: %d Gram slabs, %d planned", f, stm_ca_slabs(S.fs[f]), S.gp_slabs);
            }
            CHECK(wp_end <= S.wp_doubles, "step %d: the update workspace ends at %lld of %lld", t, wp_end, S.wp_doubles);
            for (int i = 0; i < s.n_cpk; i++) {
                const int f = S.lists[(size_t)(s.cpk_off + i)];
                CHECK(f >= 0 && f < nf && big(f) && c.group[f] == g && packed[f] < 0 && next_panel[f] == S.fs[f].nsched, "group %d step %d packs front %d (panel %d of %d)", g, t, f,
                      f >= 0 && f < nf ? next_panel[f] : -9, f >= 0 && f < nf ? S.fs[f].nsched : -9);
                if (f >= 0 && f < nf) packed[f] = t;
            }
        }
    }
    for (long f = 0; f < nf; f++) {
        const FrontSym &s = S.fs[f];
        if (c.group[f] < 0) { CHECK(start[f] < 0 && in_level[f] == 0, "front %ld is elsewhere and starts at step %d", f, start[f]); continue; }
        CHECK(start[f] >= 0 && packed[f] >= start[f] && in_level[f] == 1, "front %ld of group %d: start %d, packed %d, in %d level lists", f, c.group[f], start[f], packed[f], in_level[f]);
        CHECK(s.nsched >= 1 || !big(f), "front %ld: nsched %d", f, s.nsched);
        CHECK(s.nsched <= s.npanels && (!big(f) || next_panel[f] == s.nsched), "front %ld: %d panels ran, nsched %d of %d", f, next_panel[f], s.nsched, s.npanels);
        if (c.full_schedule || !S.early_end) CHECK(s.nsched == s.npanels, "front %ld: nsched %d of %d on a full schedule", f, s.nsched, s.npanels);
        if (sharedf(f) || S.pair_front[f]) CHECK(s.nsched == s.npanels, "front %ld (shared / sweeps): nsched %d of %d", f, s.nsched, s.npanels);
        // ---- a front starts after every child of the same group has been packed ----
        for (long q = T.Childp[f]; q < T.Childp[f + 1]; q++) {
            const long ch = T.Child[q];
            if (c.group[ch] == c.group[f]) CHECK(packed[ch] >= 0 && packed[ch] < start[f], "front %ld starts at %d, its child %ld is packed at %d", f, start[f], ch, packed[ch]);
        }
    }
    // ---- fronts in flight at the same time (from the start to the step that packs them: the slot goes back at the flush) have different T slots ----
    for (long f = 0; f < nf; f++)
        for (long h = f + 1; h < nf; h++)
            if (c.group[f] >= 0 && c.group[f] == c.group[h] && big(f) && big(h) && S.tslot[f] == S.tslot[h])
                CHECK(packed[f] < start[h] || packed[h] < start[f], "fronts %ld (steps %d-%d) and %ld (%d-%d) share T slot %d", f, start[f], packed[f], h, start[h], packed[h], S.tslot[f]);
    // ---- the tail of lists ----
    CHECK(S.own_off >= 0 && S.n_own >= 0 && (size_t)S.own_off + (size_t)S.n_own <= NL && S.rh_parts_off >= 0 && (size_t)S.rh_parts_off + (size_t)S.n_own <= NL && S.post_off >= 0 &&
              (size_t)S.post_off + (size_t)nf <= NL, "own [%d, +%d), parts at %d, post at %d of %zu", S.own_off, S.n_own, S.rh_parts_off, S.post_off, NL);
    if (failures != failed_before) return;
    long owned = 0;
    for (long f = 0; f < nf; f++) owned += c.group[f] >= 0;
    CHECK(S.n_own == owned, "%d owned fronts listed, %ld in the groups", S.n_own, owned);
    for (int i = 0; i < S.n_own; i++) {
        const int f = S.lists[(size_t)(S.own_off + i)], parts = S.lists[(size_t)(S.rh_parts_off + i)];
        CHECK(f >= 0 && f < nf && c.group[f] >= 0 && parts >= 1 && parts <= S.rh_maxparts, "owned list: front %d, %d parts", f, parts);
    }
    for (long kf = 0; kf < nf; kf++) CHECK(S.lists[(size_t)(S.post_off + kf)] == T.Post[kf], "post list [%ld]", kf);

    // ---- the arenas ----
    bool whole = ngroups == 1 && nf > 0;
    for (long f = 0; f < nf && whole; f++) whole = c.group[f] == 0 && !sharedf(f);
    CHECK(S.recycle == (whole && c.k.recycles([&] { long long a = 0; for (long f = 0; f < nf; f++) a += slab(f); return a; }())), "recycle %d on a %s plan", (int)S.recycle, whole ? "whole-tree" : "partial");
    auto csize = [&](long f) {
        const FrontSym &s = S.fs[f];
        const long cn = s.fn - s.fp, fm = s.fm_ub;
        const long cm = T.do_rank ? std::min(fm, cn) : std::min(std::max(fm - std::min(fm, (long)s.fp), 0L), cn);
        return (long long)cm * (cm + 1) / 2 + (long long)cm * (cn - cm);
    };
    std::vector<Range> FR, CR;
    if (!S.recycle) {
        // every owned front its slab, every front that is owned or a child of an owned one its slot, for the whole factorization
        for (long f = 0; f < nf; f++) {
            bool needc = c.group[f] >= 0;
            if (S.fs[f].parent >= 0 && c.group[S.fs[f].parent] >= 0) needc = true;
            CHECK((bool)S.has_c[f] == needc, "front %ld: has_c %d", f, (int)S.has_c[f]);
            if (c.group[f] >= 0 && slab(f) > 0) FR.push_back({S.fs[f].foff, S.fs[f].foff + slab(f), 0, 0, f});
            if (S.has_c[f]) {
                CHECK(S.c_slot[f] == csize(f), "front %ld: slot of %lld, bound %lld", f, S.c_slot[f], csize(f));
                if (S.c_slot[f] > 0) CR.push_back({S.fs[f].coff, S.fs[f].coff + S.c_slot[f], 0, 0, f});
            }
        }
    } else {
        // slabs over [f_t0, f_t1], contribution blocks over [f_t1, c_t1]; a kept front is never given away
        const int nstep = (int)S.gsteps[0].size();
        long long rec = 0;
        int nkept = 0, nrhp = 0;
        for (const Step &s : S.gsteps[0]) {
            nrhp += s.n_rhp;
            for (int i = 0; i < s.n_rhp; i++) {
                const int f = S.lists[(size_t)(s.rhp_off + i)], parts = S.lists[(size_t)(s.rhp_parts_off + i)];
                CHECK(f >= 0 && f < nf && !S.kept[f] && packed[f] == (int)(&s - S.gsteps[0].data()) && parts >= 1 && parts <= s.rhp_maxparts, "staging list: front %d, %d parts", f, parts);
            }
        }
        for (long f = 0; f < nf; f++) {
            CHECK(S.f_t0[f] == start[f] && S.f_t1[f] == packed[f] && S.c_t1[f] == (S.fs[f].parent >= 0 ? start[S.fs[f].parent] : packed[f]), "front %ld: lifetimes %d %d %d", f, S.f_t0[f],
                  S.f_t1[f], S.c_t1[f]);
            CHECK(S.has_c[f] && S.c_slot[f] == csize(f), "front %ld: slot of %lld, bound %lld", f, S.c_slot[f], csize(f));
            nkept += S.kept[f] ? 1 : 0;
            if (!S.kept[f]) rec += slab(f);
            if (slab(f) > 0) FR.push_back({S.fs[f].foff, S.fs[f].foff + slab(f), S.kept[f] ? 0 : S.f_t0[f], S.kept[f] ? nstep : S.f_t1[f], f});
            if (S.c_slot[f] > 0) CR.push_back({S.fs[f].coff, S.fs[f].coff + S.c_slot[f], S.f_t1[f], std::max(S.f_t1[f], S.c_t1[f]), f});
        }
        CHECK(nrhp == nf - nkept, "%d fronts staged, %ld not kept", nrhp, nf - nkept);
        CHECK(S.rh_cap >= 1 && S.rh_cap <= std::max(1LL, rec), "R+H arena of %lld, recycled slabs %lld", S.rh_cap, rec);
        // ---- the forced kept set is the q largest slabs ----
        if (c.k.keep_fronts >= 0) {
            long long least_kept = -1, most_free = -1;
            for (long f = 0; f < nf; f++) {
                if (S.kept[f]) least_kept = least_kept < 0 ? slab(f) : std::min(least_kept, slab(f));
                else most_free = std::max(most_free, slab(f));
            }
            CHECK(nkept == (int)std::min<long>(std::min(c.k.keep_fronts, 3), nf) && (nkept == 0 || least_kept >= most_free), "%d kept (asked %d), smallest kept %lld, largest free %lld", nkept,
                  c.k.keep_fronts, least_kept, most_free);
        } else
            CHECK(nkept <= 3, "%d kept", nkept);
        // the scratch of the resident-factor operations: the fronts of a level side by side
        long long widest = 1;
        for (const Level &L : S.glevels[0]) {
            std::vector<Range> LR;
            for (int q = 0; q < L.n_all; q++) {
                const int f = S.lists[(size_t)(L.all_off + q)];
                if (!S.kept[f] && slab(f) > 0) LR.push_back({S.fs_scr[f].foff, S.fs_scr[f].foff + slab(f), 0, 0, f});
            }
            check_disjoint(LR, S.scr_doubles, "scratch slab");
            for (const Range &r : LR) widest = std::max(widest, r.b);
        }
        CHECK(widest == S.scr_doubles, "scratch of %lld, widest level %lld", S.scr_doubles, widest);
    }
    check_disjoint(FR, S.farena, "slab");
    check_disjoint(CR, S.carena, "contribution block");

    // ---- sweeps ----
    CHECK(S.sweep == (c.opt.pair_update == 4 ? 4 : 2), "sweep %d", S.sweep);
    long long yp = 0;
    for (long f = 0; f < nf; f++) {
        const bool pair = c.opt.pair_update && c.group[f] >= 0 && !sharedf(f) && big(f) && S.fs[f].fm_est >= c.k.pair_min && S.fs[f].npanels >= 4;
        CHECK((bool)S.pair_front[f] == pair && (S.ypoff[f] >= 0) == pair, "front %ld: pair_front %d, ypoff %lld", f, (int)S.pair_front[f], S.ypoff[f]);
        if (pair) { CHECK(S.ypoff[f] == yp, "front %ld: ypoff %lld, expected %lld", f, S.ypoff[f], yp); yp += (long long)((S.fs[f].fn + 31) / 32) * (S.sweep * STM_NB * 32); }
    }
    CHECK(yp == S.yp_doubles, "Ypend of %lld, fronts need %lld", S.yp_doubles, yp);
}

// ---- the configurations of one tree --------------------------------------------------------------------------------------------------
static void mark_subtree(const Tree &T, long root, int g, std::vector<int> &group)
{
    group[root] = g;
    for (long q = T.Childp[root]; q < T.Childp[root + 1]; q++) mark_subtree(T, T.Child[q], g, group);
}

static void run_tree(Tree &T)
{
    analyse(T);
    if (failures) return;
    const long nf = T.nf;
    Config base;
    base.group.assign((size_t)nf, 0);
    std::vector<Config> cs;
    auto add = [&](const char *name, Config c) { c.name = name; cs.push_back(c); };
    add("one group", base);
    { Config c = base; c.k.early_end = false; add("early_end off", c); }
    { Config c = base; c.full_schedule = true; add("full_schedule", c); }
    { Config c = base; c.k.sched = 1; add("level order", c); }
    { Config c = base; c.k.sched = 2; add("as soon as possible", c); }
    { Config c = base; c.k.recycle = 0; add("recycle 0", c); }
    for (int q = -1; q <= 3; q++) { Config c = base; c.k.recycle = 2; c.k.keep_fronts = q; add(("recycle 2, keep_fronts " + std::to_string(q)).c_str(), c); }
    for (int pu : {0, 1, 4}) { Config c = base; c.opt.pair_update = pu; c.opt.big_front_cols = 16; c.k.pair_min = 1; c.k.recycle = pu == 1 ? 2 : 1; add(("pair_update " + std::to_string(pu)).c_str(), c); }
    // two and three groups cut by subtree (below the last root, the first front with two children or more: the subtrees of its first children)
    long root = -1;
    for (long f = 0; f < nf; f++) if (T.F.fs[f].parent < 0) root = f;
    std::vector<long> heads;
    long hub = -1;
    for (long h = root; heads.size() < 3 && h >= 0;) {
        // (walk down the widest chain until a front has two children or more)
        const long nch = T.Childp[h + 1] - T.Childp[h];
        if (nch >= 2) { hub = h; for (long q = T.Childp[h]; q < T.Childp[h + 1] && heads.size() < 3; q++) heads.push_back(T.Child[q]); break; }
        if (nch == 0) break;
        h = T.Child[T.Childp[h]];
    }
    for (size_t ng = 2; ng <= 3 && ng <= heads.size() + 1; ng++) {
        // groups 0 .. ng-2: a subtree each; group ng-1: their parent alone (its other children are elsewhere); the rest: -1
        Config c = base;
        c.group.assign((size_t)nf, -1);
        for (size_t g = 0; g + 1 < ng; g++) mark_subtree(T, heads[g], (int)g, c.group);
        c.group[hub] = (int)ng - 1;
        add((std::to_string(ng) + " groups by subtree").c_str(), c);
        c.early_phased = true;
        add((std::to_string(ng) + " groups by subtree, early_phased").c_str(), c);
    }
    if (is_big(T.F.fs[root], base.opt.big_front_cols) && nf > 1) {
        Config c = base;
        c.group[root] = 1;
        c.shared.assign((size_t)nf, 0);
        c.shared[(size_t)root] = 1;
        add("one shared root", c);
    }
    for (const Config &c : cs) {
        const int before = failures;
        check_schedule(T, c);
        if (failures != before) return;
    }
    printf("%-16s %5ld fronts, %2zu configurations\n", T.name.c_str(), nf, cs.size());
}

// the allocator alone: pseudo-random lifetimes, no two objects alive together share an address, the peak is what the placements reach
static void check_first_fit()
{
    ctx = "timeline_first_fit";
    unsigned long long rng = 12345;
    auto next = [&](int mod) { rng = rng * 6364136223846793005ULL + 1442695040888963407ULL; return (int)((rng >> 33) % (unsigned)mod); };
    for (int trial = 0; trial < 20; trial++) {
        const int nstep = 1 + next(30), nobj = 1 + next(60);
        std::vector<long long> off((size_t)nobj, -1);
        std::vector<TlObj> objs;
        for (int i = 0; i < nobj; i++) {
            const int t0 = next(nstep), t1 = t0 + next(nstep - t0);
            objs.push_back({(long long)next(5) * next(100), t0, t1, &off[(size_t)i]});
        }
        const long long base = 2 * next(10), peak = timeline_first_fit(objs, base, nstep);
        std::vector<Range> R;
        long long top = base;
        for (int i = 0; i < nobj; i++) {
            CHECK(off[(size_t)i] >= base && objs[(size_t)i].size % 2 == 0, "object %d at %lld (base %lld), size %lld", i, off[(size_t)i], base, objs[(size_t)i].size);
            if (objs[(size_t)i].size > 0) { R.push_back({off[(size_t)i], off[(size_t)i] + objs[(size_t)i].size, objs[(size_t)i].t0, objs[(size_t)i].t1, i}); top = std::max(top, R.back().b); }
        }
        check_disjoint(R, peak, "object");
        CHECK(top == peak, "peak %lld, highest object ends at %lld", peak, top);
    }
}

int main(int argc, char **argv)
{
    check_first_fit();
    // a chain of big and small fronts; a star: eleven leaves under one root; a three-level arrow with one big root (ten small leaves, three
    // middle fronts, the root 40 panels wide); a forest of three trees (a chain, a single front, a small star)
    std::vector<Tree> trees;
    trees.push_back(make_tree("chain", {1, 2, 3, 4, -1}, {40, 8, 100, 30, 200}, {60, 100, 90, 150, 0}, {3, 2, 2, 1, 1}));
    {
        std::vector<int> par(12, 11), fp(12, 20), cn(12, 70), rows(12, 3);
        par[11] = -1; fp[11] = 300; cn[11] = 0; rows[11] = 1; fp[3] = 90; cn[3] = 200; rows[3] = 4;
        trees.push_back(make_tree("star", par, fp, cn, rows));
    }
    {
        std::vector<int> par, fp, cn, rows;
        for (int i = 0; i < 10; i++) { par.push_back(10 + i % 3); fp.push_back(6 + i); cn.push_back(30 + 2 * i); rows.push_back(2); }
        for (int i = 0; i < 3; i++) { par.push_back(13); fp.push_back(70 + 30 * i); cn.push_back(400); rows.push_back(1 + i); }
        par.push_back(-1); fp.push_back(1280); cn.push_back(0); rows.push_back(1);
        trees.push_back(make_tree("arrow", par, fp, cn, rows));
    }
    trees.push_back(make_tree("forest", {1, 2, -1, -1, 7, 7, 7, -1}, {30, 70, 130, 50, 10, 80, 12, 90}, {100, 90, 0, 0, 40, 60, 20, 0}, {2, 1, 1, 2, 3, 2, 2, 1}));
    for (Tree &T : trees) run_tree(T);
    for (int i = 1; i < argc; i++) { Tree T = read_tree(argv[i]); run_tree(T); }
    printf("%d trees, %d failures\n", (int)trees.size() + argc - 1, failures);
    return failures ? 1 : 0;
}
