// stmmqr_resident.h -- the state of the operations on the resident factors (stmmqr_plan::res), sorted by how long it lives, and what
// their seven host units share (included by stmmqr_plan.h, after DevBuf):
//   stmmqr_rfactor.cpp     the front form, the row map, the passes over the tree; qmult, rsolve, solve, solve_minnorm, solve_carried
//   stmmqr_rcond.cpp       products with R and R', the condition estimate
//   stmmqr_rsparse.cpp     R out as compressed columns / rows in device memory
//   stmmqr_hsparse.cpp     H, HTau and HPinv out in device memory
//   stmmqr_rnull.cpp       the null-space basis of R, its Gram matrix and Cholesky factor, the minimum-norm projector
//   stmmqr_rcov.cpp        the selected inverse: variances, leverages, covariance entries
//   stmmqr_seminormal.cpp  products with A, the seminormal solves, the minimum-norm forwarder of the SparseQR object
#pragma once
#include <functional>

#include "stmmqr_restables.h"

struct ResidentState {
    // ---- per schedule: follows the level lists of one schedule (stmmqr_plan::sch).  `gen` is the stmmqr_plan::sched_gen the tables and the
    // static maps were built from (ensure_rowmap rebuilds them when the plan's has moved on); rm_gen / rmt_gen the same for the
    // parts that the first product with R / with R' adds.
    struct Schedule {
        long gen = -1, rm_gen = -1, rmt_gen = -1, rjt_gen = -1;   // (rjt_gen: the transpose of Rj alone, ensure_rj_transpose)
        restab::LevelTables T;                          // dynamic LDS per level, split fronts, T4 bookkeeping, buffer sizes
        std::vector<int> rm_rslab, rm_cslab;            // per level the most row slabs (R x) / column slabs (R' y) of a front
        DevBuf<int> d_Rj, d_PLinv, d_Qfill;             // the static integer maps
        DevBuf<int> d_rmcp, d_rmslot;                   // the transpose of Rj (restab::rj_transpose)
        DevBuf<QbDesc> d_qb;                            // T.qb (np_live refreshed per factorization)
        DevBuf<RtDesc> d_rtb;                           // T.rtb
        DevBuf<int> d_Dq, d_Rm;                         // reflector numbering of a level's split fronts / their rows of R (k_rbig_*)
        DevBuf<int> d_rtLc, d_rtRm;                     // live pivot columns of a level's rtbig fronts (T.rtlc_ints) / their counts
        // R as a sparse matrix (stmmqr_rsparse.cpp), made by the first call of a form and kept: per slot of Rj its kept and visited
        // entries (two ints) and its start (64-bit); per row of R the same two counts; a partial sum per 256 items, the four of info
        DevBuf<int> d_rsSlot, d_rsRow;
        DevBuf<long long> d_rsOff, d_rsPart, d_rsInfo;
        // H as a sparse matrix (stmmqr_hsparse.cpp), made by the first call and kept: per slot of Rj its kept and visited entries and
        // its column number in H (three ints) and its start (64-bit); the four of info
        DevBuf<int> d_hsSlot;
        DevBuf<long long> d_hsOff, d_hsInfo;
        // grouped split Q-apply (k_qbig_step4): allocated at the first Q-apply that wants it (t4_tried); t4_ok: there was room
        bool t4_ok = false, t4_tried = false;
        DevBuf<Qt4ItemHost> d_t4items;
        DevBuf<int> d_t4fronts, d_Dq4;
        DevBuf<long long> d_t4dqo, d_qbt4off;
        DevBuf<double> d_T4;
        // slab recycling: the scratch that holds the widest tree level (the schedule's scr_doubles) or, scr_all, every front in front form
        std::vector<FrontSym> fs_scr;                   // FrontSym with foff into that scratch: the schedule's fs_scr or the scr_all layout
                                                        //  (ensure_scratch; kept fronts: their own slab, relative to it)
        bool scr_all = false;
        DevBuf<double> d_scr;
        DevBuf<FrontSym> d_fs_scr;
    } sched;
    // ---- per factorization: void after new_factorization(), made again by the first operation that follows
    struct Factorization {
        bool rowmap_ready = false;                      // d_Wmap, d_rowbase and `live` belong to the factorization held
        bool scr_valid = false;                         // scr_all: the scratch is up to date
        bool t4_valid = false;                          // t4_level_valid belongs to the factorization held
        std::vector<char> t4_level_valid;               // T4 of the level's split fronts is built (per level: with the per-level scratch
                                                        //  only the level at hand is in front form)
        restab::LiveCounts live;
        DevBuf<int> d_Wmap, d_rowbase;                  // restab::row_map
        // the null-space basis of the first `ncol` columns (stmmqr_rnull.cpp): built by the first call that asks for it, found by the
        // later ones with the same ncol; its memory goes back with the factorization
        struct NullSpace {
            bool ready = false;
            long ncol = -1;
            int d = 0, r = 0;                           // dead / live pivot columns among the first ncol
            double nfro = 0.0, lmin = 0.0;              // |N|_F, the smallest diagonal entry of L
            double ms[3] = {0.0, 0.0, 0.0};             // device ms of the build: N, the Gram matrix, the Cholesky factorization
            DevBuf<double> d_N, d_L, d_Ld;              // N (ncol x d), L (d x d: the blocks below the diagonal), its 32 x 32 diagonal blocks
            DevBuf<int> d_jd;                           // the dead columns
            void release() { ready = false; ncol = -1; d = r = 0; d_N.release(); d_L.release(); d_Ld.release(); d_jd.release(); }
        } null;
    } fact;
    // ---- per call: grown on demand, never shrunk
    struct Call {
        int rhs_cap = 1;                                // right-hand sides the per-vector buffers hold (RhsBatch, stmmqr_kernels.h)
        DevBuf<double> d_W, d_Xs, d_Io, d_Xf, d_Wq, d_Wq4, d_U, d_Xr;   // per-vector work buffers
        DevBuf<double> d_Xall, d_Yall;                  // staging of a call's right-hand sides and results
        DevBuf<int> d_err;                              // the kernels' error word (end_resident_op)
        DevBuf<double> d_csB, d_csX, d_csR, d_csZ, d_csY, d_csD, d_csN;   // the seminormal solve's vectors
        DevBuf<double> d_ceA, d_ceB, d_ceY, d_ceV, d_ceS;               // the condition estimate's: two of n, one of m, the attaining
        DevBuf<int> d_cepc;                                             //  vector, the scalars read back; the live pivot columns
        // solve_carried: the view that ends at column n (restab::carried_view; FrontNum with the live A pivots as rank), the fronts
        // that hold B pivots, the residual norms
        DevBuf<FrontSym> d_fs_car;
        DevBuf<FrontNum> d_fnum_car;
        DevBuf<int> d_carlist;
        DevBuf<double> d_carN;
        DevBuf<double> d_nlX, d_nlT, d_nlP, d_nlS;     // the projector's: a batch in R's column order, N'X, its slab partial sums, norms
    } call;
    void new_factorization() { fact.rowmap_ready = fact.scr_valid = fact.t4_valid = false; fact.null.release(); }
};

// ---- what stmmqr_rfactor.cpp gives the other three units ----
struct stmmqr_plan;
// how every entry point starts and ends: the refusal before it looks at its other arguments; the plan's device and the maps of the
// factorization held; the check of the kernels' error word (1 from a front's live pivot count, 2 from a lookup of k_si_leverage,
// 3 + 4 (column + 1) from a pivot of k_null_chol_panel)
int check_factored(const stmmqr_plan *plan);
int begin_resident_op(stmmqr_plan &P);
int end_resident_op(stmmqr_plan &P);
int check_carried_view(const stmmqr_plan &P, long ncol);        // may the plan of [A B] be cut back to a view that ends at column ncol
bool holds_whole_tree(const stmmqr_plan &P);                    // the whole tree in one group, nothing imported or shared
DevCtx res_ctx(stmmqr_plan &P);                                 // the fronts the resident-factor kernels read
std::vector<FrontSym> resident_front_syms(const stmmqr_plan &P);
int level_to_front_form(stmmqr_plan &P, size_t l);
int rhs_batch_max();
// stmmqr_plan_solve with B and X on the host or, on_device, on the device
int plan_solve(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs, int on_device);
int for_each_batch(stmmqr_plan &P, stm_long nrhs, const std::function<int(stm_long, int)> &op);
// staging: rows x cols doubles between a caller's array (leading dimension ld; host, or device with on_device) and a device buffer that
// holds the columns one after the other (grown if needed); stage_out waits for the stream
int grow(DevBuf<double> &d, size_t n);
int copy_cols(double *dst, long ldd, const double *src, long lds, long rows, long cols, hipMemcpyKind kind, hipStream_t st);
int stage_in(DevBuf<double> &d, const double *src, long ld, long rows, long cols, int on_device, hipStream_t st);
int stage_out(const DevBuf<double> &d, double *dst, long ld, long rows, long cols, int on_device, hipStream_t st);
int to_host(void *dst, const void *src, size_t bytes, hipStream_t st);   // bytes from the device on the stream, not waited for (0 bytes: no call)
// count longs as ints: t receives the host copy, which the upload reads until the caller's next synchronize (HIP's code: the caller words it)
int upload_narrowed(DevBuf<int> &d, const long *v, size_t count, std::vector<int> &t, hipStream_t st);
// the passes (stmmqr_rfactor.cpp says what they read and write)
enum RtMode { RT_ONE_WORKGROUP, RT_SPLIT };
int ensure_rt(stmmqr_plan &P, RtMode mode);
int rt_pass(stmmqr_plan &P, int nb, RtMode mode);
int rsolve_vector(stmmqr_plan &P, int nb);
int r_vectors(stmmqr_plan &P, const double *Y, double *X, int nb, bool through_qfill);
int rt_vectors(stmmqr_plan &P, const double *Z, double *Y, int nb, bool through_qfill);
int ensure_rmult(stmmqr_plan &P);
int ensure_rtmult(stmmqr_plan &P);
int ensure_rj_transpose(stmmqr_plan &P);                        // d_rmcp / d_rmslot alone (what ensure_rtmult makes besides its vectors)
int rmult_pass(stmmqr_plan &P, const double *X, double *Y, int nb, int twofold = 0);    // twofold: row sums carried in two doubles
int rtmult_pass(stmmqr_plan &P, const double *Y, double *Z, int nb, int absval = 0);
