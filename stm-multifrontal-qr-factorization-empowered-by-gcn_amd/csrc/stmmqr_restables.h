// stmmqr_restables.h -- the index arithmetic of the resident-factor operations: plain vectors in, plain vectors out.  No HIP call, no
// device buffer, no plan (stmmqr_device.h and the standard library only), so tests/restables_selftest.cpp runs it under ASan + UBSan
// without a GPU.  The callers (stmmqr_rfactor.cpp, stmmqr_rcov.cpp) keep the uploads, the allocations and the launches.
#pragma once
#include <string>
#include <vector>

#include "stmmqr_device.h"

namespace restab {
// per level: the fronts that take the split Q-apply / back substitution (descriptors from `off`), their maxima, their T4 groups
struct QbLevel { int off = 0, n = 0, max_np = 0, max_nslab = 0, max_fm = 0, max_rsteps = 0, t4i_off = 0, t4i_n = 0; };
// per level: the fronts with FrontSym::rtbig (descriptors from `off`), their most blocks of 32 pivot columns and column slabs, and the
// dynamic LDS k_rtsolve needs for the other fronts of the level
struct RtLevel { int off = 0, n = 0, max_steps = 0, max_nslab = 0, lds_small = 0; };
struct T4Item { int f, g; long long off, dqo; };      // (= Qt4ItemHost of stmmqr_kernels.h; stmmqr_rfactor.cpp asserts the layout)

// Of one schedule: the dynamic LDS of every tree level's launches (stm_lds_*; _all: the unblocked kernel takes the split fronts too),
// the descriptors of the split fronts, the bookkeeping of their grouped Q-apply (T4: one item per group of four panels), and the
// sizes of the per-vector buffers (maxima over the levels)
struct LevelTables {
    std::vector<int> lds_qa, lds_qa_all, lds_rs, lds_rt;
    std::vector<QbLevel> qbig;
    std::vector<RtLevel> rtbig;
    std::vector<QbDesc> qb;              // never empty (one unused entry where no front is split); np_live follows the factorization
    std::vector<RtDesc> rtb;
    std::vector<T4Item> t4items;
    std::vector<int> t4fronts;
    std::vector<long long> t4dqo, qbt4off;
    long long t4_doubles = 0, dq4_ints = 0, wq4_doubles = 0, rtlc_ints = 1, xf_doubles = 1, dq_ints = 1, wq_doubles = 1;
};
LevelTables level_tables(const std::vector<FrontSym> &fs, const std::vector<Level> &LV, const std::vector<int> &lists, int qt4_doubles);

// Of one factorization, per level: the panels of a split front that can hold a live reflector and the blocks of live pivot columns.
// A front of fm rows has fm live reflectors at most; they sit in its first fm + (dead pivot columns) columns, and a front has at
// most fp - rank dead pivot columns.  The panels behind that column were launches that did nothing: on the default workload
// 330 launches per Q'b, 177 of them for panels without a reflector (same finding as the factorization's own schedule,
// stmmqr_schedule.cpp "how many panels").  live = false (STMMQR_LIVE_PANELS=0): every panel.
struct LiveCounts { std::vector<int> np, rsteps, rtsteps; };
// -> whether an np_live of T.qb changed (the device copy is stale)
bool live_counts(LevelTables &T, const std::vector<FrontSym> &fs, const std::vector<FrontNum> &fnum, bool live, LiveCounts &L);

// The host half of qr_hpinv for the device: Wmap[S-row id] = position in the permuted row order (same rule as in stmmqr_plan_download),
// and rowbase[f] = the rows of R above front f.  Hii: the row ids of the fronts as the factorization left them (from Hip[f])
void row_map(const std::vector<long> &Sleft, const std::vector<long> &Hip, const std::vector<int> &Hii, const std::vector<FrontSym> &fs,
             const std::vector<FrontNum> &fnum, long m, long n, std::vector<int> &Wmap, std::vector<int> &rowbase);

// The transpose of Rj: column j of R -> the slots p with Rj[p] = j, slot[cp[j] .. cp[j + 1]) in slot order
void rj_transpose(const std::vector<long> &Rj, long n, std::vector<int> &cp, std::vector<int> &slot);

// The view of a factorization of [A B] that ends at column ncol: `vs` (the FrontSym array the kernels read) gets fp cut back to the A
// pivots; blist = the fronts that hold B pivots, level by level (never empty: one unused entry), boff = their offsets per level
void carried_view(const std::vector<FrontSym> &fs, const std::vector<Level> &LV, const std::vector<int> &lists, long ncol,
                  std::vector<FrontSym> &vs, std::vector<int> &blist, std::vector<int> &boff);

// Where every front's block of the selected inverse lies (SiDesc; zoff cumulative over the tree, woff within a level), per level
// the largest rmax and cn, the doubles of all blocks and of the widest level's workspace
struct SelInvLayout {
    std::vector<SiDesc> sd;
    std::vector<int> lev_r, lev_cn;
    long long zall = 0, wmax = 1;
};
SelInvLayout selinv_layout(const std::vector<FrontSym> &fs, const std::vector<Level> &LV, const std::vector<int> &lists,
                           const std::vector<long> &Rj, long ncol);

// colfront[k] = the front where column k (R's order) is pivotal, k < ncol
std::vector<int> column_fronts(const std::vector<long> &Super, long nf, long ncol);
// Pairs (I[p], J[p]) of caller's columns -> trip[3p ..] = (front of the earlier column in R's order, its local column, the local column
// of the later one).  Returns 0, or the error code with the text for the caller's `fail`
int resolve_pairs(const std::vector<FrontSym> &fs, const std::vector<long> &Super, const std::vector<long> &Rj, const long *Qfill, long ncol,
                  long npairs, const long *I, const long *J, std::vector<int> &trip, std::string &msg);

// The null-space basis of R (stmmqr_rnull.cpp).  The live (pc) and the dead (jd) pivot columns among the first rd.size(), in R's column
// order; the row slabs of N -- rows [s h, min(ncol, (s + 1) h)), h = the height asked for, at least 1 and doubled until a launch's
// grid can count the slabs --; the panels of the Cholesky factorization = block rows of the substitutions (32 columns each, the last
// one d - 32 (panels - 1) wide) and the lower tiles of the Gram matrix
void null_split(const std::vector<char> &rd, std::vector<int> &pc, std::vector<int> &jd);
struct NullSlabs { int height, count; };
NullSlabs null_slabs(long ncol, long want);
int null_panels(int d);
int null_panel_width(int d, int p);
long long null_lower_tiles(int d);
}  // namespace restab
