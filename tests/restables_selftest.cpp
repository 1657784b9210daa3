// Stand-alone check of csrc/stmmqr_restables.cpp (tests/test_restables_cpu.py builds both with g++ under ASan + UBSan): the index
// arithmetic of the resident-factor operations on hand-written trees, against values written out here or recomputed by brute force.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>

#include "stmmqr_restables.h"

using namespace restab;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static FrontSym front(int fn, int fp, int col1, int rp, int fm_ub, int qbig = 0, int rtbig = 0)
{
    FrontSym s;
    memset(&s, 0, sizeof(s));
    s.fn = fn; s.fp = fp; s.col1 = col1; s.rp = rp; s.fm_ub = fm_ub; s.ld = fm_ub + (fm_ub & 1); s.npanels = (fn + STM_NB - 1) / STM_NB;
    s.qbig = qbig; s.rtbig = rtbig; s.parent = -1;
    return s;
}
static FrontNum numeric(int fm, int rank)
{
    FrontNum nm;
    memset(&nm, 0, sizeof(nm));
    nm.fm = fm; nm.rank = rank;
    return nm;
}
static Level level(int off, int n) { Level l; l.all_off = off; l.n_all = n; return l; }

// ---- tree 1: sizes only.  Level 0: a small front, a split front (7 panels, 3 row slabs), a split front without rows; level 1: a
// rank-deficient front split both ways; level 2: a small front that the R' pass splits.  The level lists start at lists[2].
static const int QT4 = 1000;             // (stm_qt4_doubles() of the kernels: any step will do)
static std::vector<FrontSym> fs1 = {front(40, 10, 0, 0, 50), front(200, 100, 10, 40, 1200, 1), front(70, 30, 110, 240, 0, 1),
                                    front(300, 150, 140, 310, 160, 1, 1), front(20, 20, 290, 610, 30, 0, 1)};
static std::vector<Level> lv1 = {level(2, 3), level(5, 1), level(6, 1)};
static std::vector<int> lists1 = {-7, -7, 0, 1, 2, 3, 4};

static void check_level_tables()
{
    const LevelTables T = level_tables(fs1, lv1, lists1, QT4);
    size_t nq = 0, nr = 0, nt4 = 0;
    long long xf = 1, dq = 1, wq = 1, lc = 1;
    for (size_t l = 0; l < lv1.size(); l++) {
        int qa = 0, qa_all = 0, rs = 0, rt = 0, rt_small = 0;
        long long xo = 0, dqo = 0, wo = 0, lco = 0;
        CHECK(T.qbig[l].off == (int)nq && T.rtbig[l].off == (int)nr && T.qbig[l].t4i_off == (int)nt4, "level %zu: the ranges do not follow each other", l);
        int q_seen = 0, r_seen = 0;
        for (int q = 0; q < lv1[l].n_all; q++) {
            const int f = lists1[(size_t)(lv1[l].all_off + q)];
            const FrontSym &s = fs1[(size_t)f];
            qa_all = std::max(qa_all, (int)stm_lds_qapply(s.fm_ub, s.fn));
            rt = std::max(rt, (int)stm_lds_rtsolve(s.fp, s.fm_ub, s.fn));
            if (!s.qbig) { qa = std::max(qa, (int)stm_lds_qapply(s.fm_ub, s.fn)); rs = std::max(rs, (int)stm_lds_rsolve(s.fp, s.fn)); }
            if (!s.rtbig) rt_small = std::max(rt_small, (int)stm_lds_rtsolve(s.fp, s.fm_ub, s.fn));
            if (s.rtbig) {
                const RtDesc &d = T.rtb[nr + (size_t)r_seen++];
                CHECK(d.f == f && d.lcoff == lco, "front %d: RtDesc {%d, %d}", f, d.f, d.lcoff);
                lco += s.fp;
            }
            if (s.qbig) {
                const QbDesc &d = T.qb[nq + (size_t)q_seen];
                const int nslab = (s.fm_ub + STM_QB_ROWS - 1) / STM_QB_ROWS, ngr = (s.npanels + 3) / 4;
                CHECK(d.f == f && d.xoff == xo && d.dqoff == dqo && d.wqoff == wo && d.nslab == nslab && d.np_live == s.npanels, "front %d: QbDesc", f);
                CHECK(T.t4fronts[nq + (size_t)q_seen] == f && T.qbt4off[nq + (size_t)q_seen] == (long long)nt4 * QT4, "front %d: T4 offset", f);
                for (int g = 0; g < ngr; g++, nt4++)
                    CHECK(T.t4items[nt4].f == f && T.t4items[nt4].g == g && T.t4items[nt4].off == (long long)nt4 * QT4 &&
                          T.t4items[nt4].dqo == T.t4dqo[nq + (size_t)q_seen], "front %d: T4 item %d", f, g);
                xo += s.fm_ub; dqo += s.fn; wo += 2LL * nslab * STM_NB;
                q_seen++;
            }
        }
        CHECK(T.lds_qa[l] == qa && T.lds_qa_all[l] == qa_all && T.lds_rs[l] == rs && T.lds_rt[l] == rt && T.rtbig[l].lds_small == rt_small,
              "level %zu: LDS maxima %d %d %d %d %d", l, T.lds_qa[l], T.lds_qa_all[l], T.lds_rs[l], T.lds_rt[l], T.rtbig[l].lds_small);
        CHECK(T.qbig[l].n == q_seen && T.rtbig[l].n == r_seen && T.qbig[l].t4i_n == (int)nt4 - T.qbig[l].t4i_off, "level %zu: counts", l);
        nq += (size_t)q_seen; nr += (size_t)r_seen;
        xf = std::max(xf, xo); dq = std::max(dq, dqo); wq = std::max(wq, wo); lc = std::max(lc, lco);
    }
    CHECK(T.qb.size() == nq && T.rtb.size() == nr && T.t4items.size() == nt4, "the level ranges do not cover the descriptor arrays");
    CHECK(nq == 3 && nr == 2 && nt4 == 2 + 1 + 3, "%zu split fronts, %zu rtbig fronts, %zu T4 items", nq, nr, nt4);
    CHECK(T.xf_doubles == xf && T.dq_ints == dq && T.wq_doubles == wq && T.wq4_doubles == 4 * wq && T.rtlc_ints == lc &&
          T.t4_doubles == (long long)nt4 * QT4 && T.dq4_ints == 200 + 70 + 300, "buffer sizes");
    CHECK(T.qbig[0].max_np == 7 && T.qbig[0].max_nslab == 3 && T.qbig[0].max_fm == 1200 && T.qbig[0].max_rsteps == 4, "level 0 maxima");
    CHECK(T.rtbig[1].max_steps == 5 && T.rtbig[1].max_nslab == 3 && T.rtbig[2].max_steps == 1 && T.rtbig[2].max_nslab == 1, "rtbig maxima");
    const LevelTables E = level_tables(fs1, {level(2, 1)}, lists1, QT4);           // no split front at all
    CHECK(E.qb.size() == 1 && E.rtb.empty() && E.t4items.empty() && E.xf_doubles == 1 && E.rtlc_ints == 1, "the tree without split fronts");
}

static void check_live_counts()
{
    LevelTables T = level_tables(fs1, lv1, lists1, QT4);
    // front 1: every row live; front 2: no row; front 3: rank 100 < fp 150, fm 140 > rank: min(300, 140 + 50) = 190 columns -> 6 panels
    const std::vector<FrontNum> nm = {numeric(45, 10), numeric(1100, 100), numeric(0, 0), numeric(140, 100), numeric(25, 20)};
    LiveCounts L;
    CHECK(live_counts(T, fs1, nm, true, L), "the first count changes np_live");
    CHECK(T.qb[0].np_live == 7 && T.qb[1].np_live == 0 && T.qb[2].np_live == 6, "np_live %d %d %d", T.qb[0].np_live, T.qb[1].np_live, T.qb[2].np_live);
    CHECK(L.np == std::vector<int>({7, 6, 0}) && L.rsteps == std::vector<int>({4, 4, 0}) && L.rtsteps == std::vector<int>({0, 4, 1}), "live maxima");
    CHECK(!live_counts(T, fs1, nm, true, L), "the second count of the same factorization changes nothing");
    CHECK(live_counts(T, fs1, nm, false, L), "every panel again: changed");
    CHECK(T.qb[0].np_live == 7 && T.qb[1].np_live == 3 && T.qb[2].np_live == 10, "flag off: every front its npanels");
    CHECK(L.np == std::vector<int>({7, 10, 0}) && L.rsteps == std::vector<int>({T.qbig[0].max_rsteps, T.qbig[1].max_rsteps, 0}) &&
          L.rtsteps == std::vector<int>({0, T.rtbig[1].max_steps, T.rtbig[2].max_steps}), "flag off: the symbolic maxima");
    std::vector<FrontNum> capped = nm;
    capped[3] = numeric(400, 150);                                           // more live columns than the front has panels for
    live_counts(T, fs1, capped, true, L);
    CHECK(T.qb[2].np_live == 10, "np_live is capped at npanels: %d", T.qb[2].np_live);
}

// ---- tree 2: [A B] with 6 columns of A and 2 of B, 12 rows of which 2 are empty.  Fronts 0 and 1 are leaves (front 1 is
// rank-deficient), front 2 is their parent and holds B's first column as its last pivot, front 3 (the root) holds the other.
static std::vector<FrontSym> fs2 = {front(4, 2, 0, 0, 3), front(5, 2, 2, 4, 4), front(4, 3, 4, 9, 6), front(1, 1, 7, 13, 2)};
static std::vector<Level> lv2 = {level(0, 2), level(2, 1), level(3, 1)};
static std::vector<int> lists2 = {0, 1, 2, 3};
static std::vector<long> Super2 = {0, 2, 4, 7, 8}, Rj2 = {0, 1, 4, 6, 2, 3, 4, 5, 7, 4, 5, 6, 7, 7};
static const long N2 = 8, NCOL2 = 6, M2 = 12;

static void check_row_map()
{
    std::vector<long> Sleft(N2 + 2, 0), Hip = {0, 3, 7, 13, 15};
    Sleft[N2] = 10; Sleft[N2 + 1] = M2;                                       // rows 10 and 11 are empty
    const std::vector<int> Hii = {0, 1, 2, 3, 4, 5, 6, 7, 2, 4, 8, 5, 6, 9, 8};
    const std::vector<FrontNum> nm = {numeric(3, 2), numeric(4, 1), numeric(6, 3), numeric(2, 1)};
    std::vector<int> W, rb;
    row_map(Sleft, Hip, Hii, fs2, nm, M2, N2, W, rb);
    std::vector<int> sorted(W);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 0; i < M2; i++) CHECK(sorted[(size_t)i] == i, "Wmap is no permutation of the rows");
    int row = 0, run = 0;
    for (size_t f = 0; f < fs2.size(); f++) {                                   // the rows of R, front by front
        CHECK(rb[f] == run, "rowbase[%zu] = %d", f, rb[f]);
        for (int i = 0; i < nm[f].rank; i++, row++) CHECK(W[(size_t)Hii[(size_t)Hip[f] + (size_t)i]] == row, "front %zu, row %d of R", f, i);
        run += nm[f].rank;
    }
    CHECK(row == 7 && W[10] == 11 && W[11] == 10, "the empty rows go last");
}

static void check_rj_transpose()
{
    std::vector<int> cp, slot;
    rj_transpose(Rj2, N2, cp, slot);
    CHECK(cp.size() == (size_t)N2 + 1 && cp[0] == 0 && cp[(size_t)N2] == (int)Rj2.size() && slot.size() == Rj2.size(), "sizes");
    std::set<int> seen;
    for (long j = 0; j < N2; j++)
        for (int p = cp[(size_t)j]; p < cp[(size_t)j + 1]; p++) {
            CHECK(Rj2[(size_t)slot[(size_t)p]] == j, "slot %d is listed under column %ld", slot[(size_t)p], j);
            CHECK(p == cp[(size_t)j] || slot[(size_t)p - 1] < slot[(size_t)p], "column %ld: slots out of order", j);
            seen.insert(slot[(size_t)p]);
        }
    CHECK(seen.size() == Rj2.size(), "every slot once");
    rj_transpose({}, 0, cp, slot);
    CHECK(cp.size() == 1 && slot.size() == 1, "the empty R");
}

static void check_carried_view()
{
    std::vector<FrontSym> vs = fs2;
    std::vector<int> blist, boff;
    carried_view(fs2, lv2, lists2, NCOL2, vs, blist, boff);
    CHECK(blist == std::vector<int>({2, 3}) && boff == std::vector<int>({0, 0, 1, 2}), "the B fronts, level by level");
    for (size_t f = 0; f < fs2.size(); f++) {
        const bool cut = fs2[f].col1 + fs2[f].fp > NCOL2;
        CHECK(vs[f].fp == (cut ? (int)std::max(0L, NCOL2 - fs2[f].col1) : fs2[f].fp), "front %zu: fp %d", f, vs[f].fp);
        FrontSym t = vs[f];
        t.fp = fs2[f].fp;
        CHECK(memcmp(&t, &fs2[f], sizeof(t)) == 0, "front %zu: another field changed", f);
    }
    carried_view(fs2, lv2, lists2, N2, vs, blist, boff);                        // no B column: one unused entry
    CHECK(blist == std::vector<int>({0}) && boff == std::vector<int>({0, 0, 0, 0}), "the view that cuts nothing");
}

static void check_selinv_layout()
{
    const SelInvLayout Y = selinv_layout(fs2, lv2, lists2, Rj2, NCOL2);
    long long z = 0, wmax = 1;
    for (size_t l = 0; l < lv2.size(); l++) {
        long long w = 0;
        int r = 0, c = 0;
        for (int q = 0; q < lv2[l].n_all; q++) {
            const int f = lists2[(size_t)(lv2[l].all_off + q)];
            const FrontSym &s = fs2[(size_t)f];
            const SiDesc &d = Y.sd[(size_t)f];
            const int fp = (int)std::min<long>(s.fp, std::max(0L, NCOL2 - s.col1));
            int cn = 0;
            for (int k = s.fp; k < s.fn && fp == s.fp; k++) cn += Rj2[(size_t)(s.rp + k)] < NCOL2;
            CHECK(d.fp == fp && d.check == (fp == s.fp) && d.cn == cn && d.rmax == std::min(fp, s.fm_ub), "front %d: {%d, %d, %d, %d}", f, d.fp, d.check, d.cn, d.rmax);
            CHECK(d.zoff == z && d.woff == w, "front %d: zoff %lld woff %lld", f, d.zoff, d.woff);
            z += (long long)(d.rmax + d.cn) * (d.rmax + d.cn);
            w += (long long)std::max(d.rmax, 1) * (d.rmax + d.cn);
            r = std::max(r, d.rmax); c = std::max(c, d.cn);
        }
        CHECK(Y.lev_r[l] == r && Y.lev_cn[l] == c, "level %zu maxima", l);
        wmax = std::max(wmax, w);
    }
    CHECK(Y.zall == z && z == 9 + 16 + 4 && Y.wmax == wmax && wmax == 14, "zall %lld wmax %lld", Y.zall, Y.wmax);
    CHECK(Y.sd[0].cn == 1 && Y.sd[1].cn == 2 && !Y.sd[2].check && !Y.sd[3].check && Y.sd[3].fp == 0, "the view of A");
}

static void check_pairs()
{
    CHECK(column_fronts(Super2, 4, NCOL2) == std::vector<int>({0, 0, 1, 1, 2, 2}), "column_fronts");
    const long Q[] = {2, 0, 1, 3, 5, 4, 6, 7};                                 // R's order -> the caller's column
    std::vector<int> trip;
    std::string msg;
    // caller's 3 = R's 3, the diagonal; caller's (2, 5) = R's (0, 4) in both orders; caller's (2, 0) = R's (0, 1): two pivots of front 0
    const long I[] = {3, 2, 5, 2}, J[] = {3, 5, 2, 0};
    CHECK(resolve_pairs(fs2, Super2, Rj2, Q, NCOL2, 4, I, J, trip, msg) == 0 && msg.empty(), "%s", msg.c_str());
    CHECK(trip == std::vector<int>({1, 1, 1, 0, 0, 2, 0, 0, 2, 0, 0, 1}), "triples through Qfill");
    const long I0[] = {0, 4, 2}, J0[] = {4, 0, 5};                                 // no Qfill; front 1's list holds column 5 at 3
    CHECK(resolve_pairs(fs2, Super2, Rj2, nullptr, NCOL2, 3, I0, J0, trip, msg) == 0, "%s", msg.c_str());
    CHECK(trip == std::vector<int>({0, 0, 2, 0, 0, 2, 1, 0, 3}), "triples without Qfill");
    const long Ib[] = {0, 6}, Jb[] = {0, 0};
    CHECK(resolve_pairs(fs2, Super2, Rj2, nullptr, NCOL2, 2, Ib, Jb, trip, msg) != 0, "column 6 is outside A");
    CHECK(msg == "covariance entries: pair 1 = (6, 0) names a column outside 0 .. ncol - 1 = 5", "%s", msg.c_str());
    const long Ic[] = {5}, Jc[] = {0};
    CHECK(resolve_pairs(fs2, Super2, Rj2, nullptr, NCOL2, 1, Ic, Jc, trip, msg) != 0, "columns 0 and 5 share no front");
    CHECK(msg == "covariance entries: pair 0 = columns (5, 0) is outside the pattern of the selected inverse (the later column in R's order "
                 "is no column of the front whose pivots hold the earlier one)", "%s", msg.c_str());
    CHECK(resolve_pairs(fs2, Super2, Rj2, nullptr, NCOL2, 0, nullptr, nullptr, trip, msg) == 0 && trip.empty(), "no pair");
}

int main()
{
    check_level_tables();
    check_live_counts();
    check_row_map();
    check_rj_transpose();
    check_carried_view();
    check_selinv_layout();
    check_pairs();
    printf("restables selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
