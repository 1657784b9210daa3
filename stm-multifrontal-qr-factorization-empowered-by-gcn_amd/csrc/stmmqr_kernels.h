// stmmqr_kernels.h -- kernel argument block and launcher prototypes (host <-> the kernel translation units: stmmqr_kdev.h lists them)
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include "stmmqr_device.h"

// Everything a kernel needs, passed by value.  Pointers are device pointers.
struct DevCtx {
    const FrontSym *fs;        // [nf]
    FrontNum *fnum;            // [nf]
    double *Farena;            // fronts
    double *Carena;            // packed contribution blocks
    double *Tws;               // T factors of the large fronts in flight, [slots][NB*NB]
    const int *tslot;          // [nf] slot in Tws (large fronts only)
    double *Tall;              // [sum of npanels][NB*NB] T of EVERY panel, kept for the Q-apply (nullptr: not kept)
    double *Gp;                // Gram-based panel: per T slot, gp_slabs partial Gram matrices + the M mailbox, NB*NB each
    int gp_slabs;              // max slab workgroups of a front (stm_ca_slabs) over the plan
    const double *sig;         // {sg, 1/sg}: the power-of-two magnitude guard of the panel kernels (stm_larfg_guarded)
    int panel_algo;            // stmmqr_options::panel_algo (stm_use_ca)
    int ca_min_rows;           // ... panels with more estimated rows take the Gram-based kernel (panel_algo 0)
    const double *Sx;          // [anz] values of S = A(P,Q), row form
    const int *Sp;             // [m+1]
    const int *Sjrel;          // [anz] column of each S entry inside its front
    const int *Sj0;            // [m]   leftmost column of each S row
    const int *Sleft;          // [n+2]
    const int *Child;          // [nf+1]
    const int *Rjrel;          // [rjsize] for child c, slot Rp[c]+fp+cj: column of the parent
    int *Stair;                // [rjsize] HStair
    double *Tau;               // [rjsize] HTau
    int *Hii;                  // [hisize]
    char *Rdead;               // [n]
    int *Cmap;                 // [rjsize] for child c, slot Rp[c]+fp+ci: row of the parent
    int *Cursor;               // [rjsize] scratch of k_setup
    long long *Rhoff;          // [rjsize] column offsets inside a packed R+H block
    long long *Rboff;          // [nf] offset of each packed R+H block
    double tol;
    int ntol;
    unsigned long long *dbgbuf; // [64] diagnosis counters (STMMQR_DBG bit 4: phase cycle sums of STAMPS builds, panels by actual rows,
                                //  launched / useful update workgroups, refresh rounds), else unused
    int *abort;                 // set by the first bounded wait of the fused update that runs out: the others give up at once
    int tall_min;              // stmmqr_options::tall_min_rows at plan time (stm_tall_panel)
    int cbskip;                // update launches: workgroup x takes column block cb0 + x * (1 + cbskip) -- 0 everywhere except
                               //  when the trailing columns of a front are shared between plans (stmmqr_factorize_step)
    double *Ypend;             // pair update: -Y (64 x 32 per column block) of every pair-update front, by ABSOLUTE column block (column >> 5):
                               //  written by k_upd_y2, read by k_upd_c2 of the same step
    const long long *ypoff;    // [nf] offset (doubles) of a front's blocks in Ypend (-1: not a pair-update front)
    long long *rh_top;         // slab recycling: {bump pointer of the R+H arena (doubles), overflow word}; nullptr = the packed blocks are
                               //  placed by k_rh_scan at the end (Post order), every front keeps its slab until then
    long long rh_cap;          // ... capacity of that arena (doubles)
    int sweep;                 // panels per sweep of the pair / quad update fronts (2 or 4): their panel-by-panel updates bring that many column blocks
    int tune;                  // env STMMQR_TUNE, measurement sweeps only (0 = the shipped rules): bits 0-3 force 2^(x-1) slabs per
                               //  workgroup of the pair update's kernels
    int dbg;                   // env STMMQR_DBG, ablations / cross-checks only: 1 no in-panel apply (LDS panel path),
                               //  2 no T, 4 no dlarf in the LDS sub-panel, 16/32 phase timers (-DSTMMQR_STAMPS builds),
                               //  64 in-place panel path, 128 no folded norms, 256 no panel pipeline (LDS panels only),
                               //  8192 reflector-by-reflector Q-apply instead of the blocked one,
                               //  512 panel launches in chunks of env STMMQR_CHUNK fronts (default 1),
                               //  2048 column group (dbg >> 20) & 7 of every pipelined panel starts late (tests)
                               //  4096 every column group but the first gives up waiting at once (tests: recovery)
                               //  16384 no wave-pipelined panels (short panels through the multi-workgroup pipeline too)
                               //  32768 timeline of the block-0 role (tests: how many workgroup sets ran it)
                               //  65536 host only: one stderr line per front of every pair / quad sweep launch (tests)
                               //  131072 host only: one stderr line per launch that carries riders (stm_report_rider_launch; tests)
};

// STMMQR_DBG bit 131072: what a launcher of riders decided -- the kernel that hosts them, the riders' fronts, column blocks and
// slabs of the launch, the slabs per rider workgroup and the slab groups.  Host code; no kernel reads the bit.
#define STM_DBG_RIDER_LAUNCH 131072
static inline void stm_report_rider_launch(const DevCtx &c, const char *host, int unfr, int uncb, int umaxsl, int rspw, int uy)
{
    if (c.dbg & STM_DBG_RIDER_LAUNCH)
        fprintf(stderr, "[rider launch] host %s unfr %d uncb %d umaxsl %d rspw %d uy %d\n", host, unfr, uncb, umaxsl, rspw, uy);
}

int stm_configure_kernels(void);       // (stmmqr_panel.hip; calls the other translation units' stm_configure_*)
int stm_update_lds_bytes(void);
int stm_launch_sigma(const double *Ax, int anz, unsigned long long *amaxbits, double *sig, hipStream_t st);
int stm_launch_gather_sx(const double *Ax, const int *smap, double *Sx, int anz, hipStream_t st);
int stm_launch_setup(const DevCtx &c, const int *flist, int nfr, hipStream_t st);
int stm_launch_assemble(const DevCtx &c, const int *flist, const int *nparts, int nfr, int maxparts, hipStream_t st);
int stm_launch_front_wg(const DevCtx &c, const int *flist, int nfr, int lds_doubles, hipStream_t st);
int stm_launch_panel(const DevCtx &c, const int *flist, const int *plist, int nfr, int nsub, int defer_ok, int lds_doubles, hipStream_t st);
int stm_configure_capanel(void);
int stm_launch_panel_ca(const DevCtx &c, const int *flist, const int *plist, int nfr, int nw, int defer_ok, hipStream_t st);
int stm_launch_panel_ca_pc(const DevCtx &c, const int *flist, const int *plist, int nfr, int nw, int defer_ok, const int *uflist,
                           const int *uplist, int unfr, int ucb0, int uncb, int umaxsl, const double *Wp, const long long *uwpoff, hipStream_t st);
int stm_launch_update(const DevCtx &c, const int *flist, const int *plist, int nfr, int cb0, int ncb, hipStream_t st);
int stm_launch_update_fused(const DevCtx &c, const int *flist, const int *plist, int nfr, int cb0, int ncb, int maxsl, double *Wp,
                            const long long *wpoff, int *wcnt, int *wflag, int epoch, int with_gram, hipStream_t st);
// passenger launches (options.lookahead = 2): the update beyond block 0 rides on the chain's own launches
int stm_launch_panel_pc(const DevCtx &c, const int *flist, const int *plist, int nfr, int nsub, int defer_ok, int lds_doubles,
                        const int *uflist, const int *uplist, int unfr, int ucb0, int uncb, int umaxsl, const double *Wp,
                        const long long *uwpoff, hipStream_t st);
int stm_launch_update_fw(const DevCtx &c, const int *flist, const int *plist, int nfr, int ncb, int maxsl, double *Wp,
                         const long long *wpoff, int *wcnt, int *wflag, int epoch, double *Wp2, int *wcnt2, hipStream_t st);
int stm_launch_update_w(const DevCtx &c, const int *flist, const int *plist, int nfr, int cb0, int ncb, int maxsl, double *Wp,
                        const long long *wpoff, int *wcnt, hipStream_t st);
int stm_launch_update_c(const DevCtx &c, const int *flist, const int *plist, int nfr, int cb0, int ncb, int maxsl, const double *Wp,
                        const long long *wpoff, hipStream_t st);
int stm_launch_update_pair(const DevCtx &c, const int *flist, const int *plist, int nfr, int ncbp, int maxsl, double *Wp,
                           const long long *wpoff, int *wcnt, hipStream_t st);
int stm_launch_update_quad(const DevCtx &c, const int *flist, const int *plist, int nfr, int ncbp, int maxsl, double *Wp,
                           const long long *wpoff, int *wcnt, hipStream_t st);
int stm_launch_update_split(const DevCtx &c, const int *flist, const int *plist, int nfr, int cb0, int ncb, int maxsl, double *Wp,
                            const long long *wpoff, int *wcnt, int with_gram, hipStream_t st);
int stm_launch_larft(const DevCtx &c, int f, hipStream_t st);
int stm_launch_update_notrans(const DevCtx &c, int f, int ncb, hipStream_t st);   // qr_larftb seam, QR_QX
int stm_launch_cpack(const DevCtx &c, const int *flist, const int *nparts, int nfr, int maxparts, hipStream_t st);
int stm_launch_rh_count(const DevCtx &c, const int *flist, int nfr, hipStream_t st);
int stm_launch_rh_scan(const DevCtx &c, const int *post, int nf, long long *rh_total, long long *outoff, hipStream_t st);
// slab recycling (stmmqr_schedule.cpp, timeline allocator)
int stm_launch_zero_slabs(const DevCtx &c, const int *flist, int nfr, int maxparts, hipStream_t st);
int stm_launch_rh_unpack(const DevCtx &c, const FrontSym *cs, const int *flist, int nfr, int maxparts, const char *kept, const double *RH,
                         double *scratch, hipStream_t st);
int stm_launch_rh_window(const DevCtx &c, const int *flist, int nfr, int maxparts, const long long *fin, const char *kept, const double *RH,
                         long long w0, long long w1, double *out, hipStream_t st);
int stm_launch_rh_copy(const DevCtx &c, const int *flist, const int *nparts, int nfr, int maxparts, double *RH,
                       hipStream_t st);
// factors without H (keepH = 0: qr_rhpack's R-only layout) and products with A (stmmqr_qless.hip); the block offsets come from
// stm_launch_rh_scan as for R+H
int stm_launch_r_count(const DevCtx &c, const int *flist, int nfr, hipStream_t st);
int stm_launch_r_copy(const DevCtx &c, const int *flist, const int *nparts, int nfr, int maxparts, double *RH, hipStream_t st);
int stm_launch_r_window(const DevCtx &c, const int *flist, int nfr, int maxparts, const long long *fin, const char *kept, const double *RH,
                        long long w0, long long w1, double *out, hipStream_t st);
int stm_launch_rh_zero(const DevCtx &c, const FrontSym *cs, const int *flist, int nfr, int maxparts, const char *kept, double *scratch,
                       hipStream_t st);
int stm_launch_r_unpack(const DevCtx &c, const int *flist, int nfr, int maxparts, const char *kept, const double *RH, const FrontSym *cs,
                        double *scratch, hipStream_t st);
int stm_launch_spmv(int rows, const int *ptr, const int *idx, const int *vpos, const double *Ax, const double *X, long long ldx,
                    const double *B, long long ldb, double *Y, long long ldy, long long nrhs, hipStream_t st);
int stm_launch_colnorm2(long long rows, const double *X, long long ldx, int ncols, double *out, hipStream_t st);
int stm_launch_add_cols(int rows, int ncols, const double *D, long long ldd, double *X, long long ldx, hipStream_t st);
// right-hand sides carried through the factorization (stmmqr_carried.hip): the view of the fronts that hold B columns as pivots
// (live A pivots -> view[f].rank, residual norms of the B columns), and x(n + j0 + r) = -1 in vector r of a batch
int stm_launch_carried_view(const DevCtx &c, const int *flist, int nfr, int n, FrontNum *view, double *resid, hipStream_t st);
int stm_launch_carried_seed(double *X, long long ldx, int n, int j0, int nb, hipStream_t st);
// selected inversion of R'R (stmmqr_selinv.hip): live-column lists and position tables of every front, then the kernels of one tree
// level (gather, [G | S], the two products, the diagonal) -- max_r / max_cn: the largest SiDesc::rmax / cn of the level's fronts
int stm_launch_si_prep(const DevCtx &c, int nf, const SiDesc *sd, int *Lc, int *Pos, int *Rm, int *err, hipStream_t st);
int stm_launch_si_level(const DevCtx &c, const int *flist, int nfr, int max_r, int max_cn, const SiDesc *sd, const int *Rm, const int *Lc,
                        const int *Pos, const int *Rj, const int *Qfill, double *W, double *Z, double *var, hipStream_t st);
// leverages and single entries of the selected inverse (stmmqr_leverage.hip), read from the blocks the level loop above leaves in Z.
// SiView: what the lookups read besides DevCtx::fs -- colfront[k] = the front where column k (R's order, k < ncol) is pivotal
struct SiView { const SiDesc *sd; const int *Pos; const int *Rj; const int *colfront; const double *Z; };
// lev[i] = a_i' Z a_i for the m rows of the caller's matrix: row PLinv[i] of S (Sp, Sj: global columns in R's order, Sx), columns >= ncol
// skipped; *err = 2 if a pair of a row's columns is not in the blocks
int stm_launch_si_leverage(const DevCtx &c, const SiView &v, int m, int ncol, const int *PLinv, const int *Sp, const int *Sj,
                           const double *Sx, double *lev, int *err, hipStream_t st);
// out[p] = the block entry of trip[3 p ..] = (front, local column of the earlier column, local column of the later one)
int stm_launch_si_entries(const DevCtx &c, const SiView &v, int npairs, const int *trip, double *out, hipStream_t st);
// Q-apply / triangular solve on the resident factors
// Several right-hand sides per launch (QR_qmult / QR_solve take blocks of them: qr_panel, SparseQR.c:1591-1706): every kernel of
// these operations takes right-hand side blockIdx.y (or .z) of a BATCH -- the same workgroups, one set per vector, in the same
// launch -- with the per-vector buffers laid out at these strides (doubles).  The launches of one vector are a chain of ~10-25 us
// kernels that leave the GPU nearly empty, so a batch costs little more than one vector.  nb = 1 with zero strides: one vector.
struct RhsBatch { long long w, x, xf, wq, wq4, u; };

int stm_launch_qapply(const DevCtx &c, const int *flist, int nfr, int method, double *W, int lds_bytes, int *err, hipStream_t st);
int stm_launch_qapply_t(const DevCtx &c, const int *flist, int nfr, int method, double *W, int lds_bytes, hipStream_t st, int nb,
                        const RhsBatch &B);
int stm_qt4_doubles(void);
struct Qt4ItemHost { int f, g; long long off, dqo; };     // (= Qt4Item of stmmqr_resident.hip)
int stm_launch_qt4_build(const DevCtx &c, const int *fl, const long long *dqo, int nfronts, const void *items, int nitems, int *Dq4, double *T4all,
                         hipStream_t st);
int stm_launch_qapply_big4(const DevCtx &c, const QbDesc *qd, const long long *t4off, int nq, int max_npanels, int max_nslab, int max_fm,
                           int method, double *W, double *Xf, int *Dq, double *Wq4, const double *T4all, hipStream_t st, int nb,
                           const RhsBatch &B);
int stm_launch_qapply_big(const DevCtx &c, const QbDesc *qd, int nq, int max_npanels, int max_nslab, int max_fm, int method, double *W,
                          double *Xf, int *Dq, double *Wq, hipStream_t st, int nb, const RhsBatch &B);
int stm_launch_rsolve_big(const DevCtx &c, const QbDesc *qd, int nq, int max_steps, int max_nslab, const int *Rj, const double *W,
                          double *X, double *Acc, int *Lc, int *Rm, int *err, hipStream_t st, int nb, const RhsBatch &B);
int stm_launch_rsolve(const DevCtx &c, const int *flist, int nfr, const int *Rj, const double *W, double *X, int lds_bytes,
                      int *err, hipStream_t st, int nb, const RhsBatch &B);
// (skip_rtbig: the fronts with FrontSym::rtbig are left to stm_launch_rtsolve_big -- the pass that splits them; 0: every front)
int stm_launch_rtsolve(const DevCtx &c, const int *flist, int nfr, const double *Bp, double *U, double *Xr, const int *rowbase,
                       int lds_bytes, hipStream_t st, int nb, const RhsBatch &B, int skip_rtbig = 0);
int stm_launch_rtsolve_big(const DevCtx &c, const RtDesc *rd, int nq, int max_steps, int max_nslab, const double *Bp, double *U, double *Xr,
                           const int *rowbase, int *Lc, int *Rm, int *err, hipStream_t st, int nb, const RhsBatch &B);
// products with R and R' on the resident factors (stmmqr_rmult.hip), a tree level per launch.  R x: X in R's column order (stride
// B.x) -> Y in R's row order (stride B.w), max_slab = most row slabs (STM_RM_ROWS) of a front of the level.  R' y: every front's
// column dots into its slots of U (stride B.u; absval: |R| and y = 1, one vector), max_slab = most column slabs (STM_RM_COLS);
// then, once for all levels, z[j] = its slots in slot order (cp / slot: the transpose of Rj)
int stm_launch_rmult(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, const double *X, double *Y,
                     hipStream_t st, int nb, const RhsBatch &B);
// ... the same product with every row's sum carried in two doubles (k_rmult_dd: the residual of the null-space basis' refinement)
int stm_launch_rmult_dd(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, const double *X, double *Y,
                        hipStream_t st, int nb, const RhsBatch &B);
int stm_launch_rtmult_dots(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *rowbase, const double *Y, double *U, int absval,
                           hipStream_t st, int nb, const RhsBatch &B);
int stm_launch_rtmult_gather(const int *cp, const int *slot, const double *U, double *Z, int n, hipStream_t st, int nb, long long su, long long sz);
// the reductions and maps of the condition estimate (stmmqr_rmult.hip: k_ce_reduce / k_ce_map / k_ce_vector list the `what` codes)
int stm_launch_ce_reduce(int what, const double *a, const int *idx, const double *b, int r, double *out, hipStream_t st);
int stm_launch_ce_map(int what, double *a, const int *idx, double *dst, int r, double d, hipStream_t st);
int stm_launch_ce_vector(const double *x, const int *qfill, double *out, int ncol, double d, hipStream_t st);
// R as a sparse matrix in device memory (stmmqr_rsparse.hip), a tree level per launch of the walks.  Columns: count_cols writes every
// slot's kept / visited entries (rows < econ <= m, columns < ncol; max_slab = most column slabs of STM_RM_COLS), item_sums + scan turn
// them into ptr (nitems + 1) and info (4), slot_offsets into every slot's start, fill_cols writes idx / val.  Rows: rows(fill = 0)
// counts per row of R (cnt / vis: m ints each, zeroed by the caller; max_slab = most row slabs of STM_RM_ROWS), item_sums (cp nullptr)
// + scan, rows(fill = 1).  part: one entry per 256 items.  Every offset is 64-bit.
int stm_launch_rs_count_cols(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, int ncol, int econ,
                             int *cnt, int *vis, hipStream_t st);
int stm_launch_rs_fill_cols(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, int ncol, int econ,
                            const long long *off, long long *idx, double *val, hipStream_t st);
int stm_launch_rs_rows(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, int ncol, int econ,
                       int *cnt, int *vis, const long long *ptr, long long *idx, double *val, int fill, hipStream_t st);
int stm_launch_rs_item_sums(const int *cp, const int *slot, const int *cnt, const int *vis, int nitems, long long *ptr, long long *part,
                            hipStream_t st);
int stm_launch_rs_scan(long long *ptr, long long nitems, const long long *part, int nparts, long long rtot, long long *info, hipStream_t st);
int stm_launch_rs_slot_offsets(const int *cp, const int *slot, const int *cnt, const long long *ptr, long long *off, int ncol, hipStream_t st);
// H as a sparse matrix in device memory (stmmqr_hsparse.hip), the level walk of the columns of R on the rows below them.  count writes
// every slot's kept / visited entries and whether it is a column of H (cnt / vis / col: one int per slot of Rj each, the unit diagonal
// counted); scan turns cnt into every slot's start (off) and col into its column number and writes info (4: nh, hnz, visited, m);
// cols writes Hp (nh + 1) and HTau (nh) from them, fill writes Hi / Hx (row ids through Hii and wmap), pinv HPinv[i] = wmap[plinv[i]].
int stm_launch_hs_count(const DevCtx &c, const int *flist, int nfr, int max_slab, int *cnt, int *vis, int *col, hipStream_t st);
int stm_launch_hs_scan(const int *cnt, const int *vis, int *col, long long *off, long long nslots, long long m, long long *info, hipStream_t st);
int stm_launch_hs_cols(const double *Tau, const int *cnt, const int *col, const long long *off, int nslots, const long long *info, long long *Hp,
                       double *HTau, hipStream_t st);
int stm_launch_hs_fill(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *wmap, const long long *off, long long *Hi, double *Hx,
                       hipStream_t st);
int stm_launch_hs_pinv(const int *plinv, const int *wmap, int m, long long *HPinv, hipStream_t st);
// null-space basis of R and the minimum-norm projector (stmmqr_nullspace.hip).  N is ncol x d (ld = ncol, R's column order), G = N'N
// and its Cholesky factor L are d x d (ld = d): the blocks below the diagonal in place, the 32 x 32 diagonal blocks of L in Ld (1024
// doubles each, the identity beyond d).  Every offset into N, G and the partial sums is 64-bit.
//   unit / scatter     a batch of unit vectors e_jd[k0 + v] (X zeroed by the caller); column k0 + v of N = e - (R \ (R e)) of that batch
//   refine             N(live rows, k0 + v) -= x of vector v, x = R \ (R N(:, k0 + v)) with the residual's row sums in two doubles
//   gram               lower 32 x 32 tiles of N'N per row slab into Pt ([tile][slab][1024]), then their sum in slab order into G
//   chol_panel / _update   panel p of the right-looking factorization (columns 32 p ..): nblk = block rows at or below the diagonal
//   nt                 T (d x nb) = N'X by slab partial sums (Pt: [vector][slab][d]) added in slab order
//   llt                T <- (L L')^-1 T, a workgroup per vector
//   sub                X -= N T, a row per thread
//   norm2              out[v] = |A(:, v)|_2^2
int stm_launch_null_unit(const int *jd, int k0, int nb, double *X, long long ldx, hipStream_t st);
int stm_launch_null_scatter(const double *Xs, long long sx, const char *Rdead, const int *jd, int k0, int nb, int ncol, double *N, hipStream_t st);
int stm_launch_null_refine(const double *Xs, long long sx, const char *Rdead, int k0, int nb, int ncol, double *N, hipStream_t st);
int stm_launch_null_gram(const double *N, int ncol, int d, int slab, int nslab, double *Pt, double *G, hipStream_t st);
int stm_launch_null_chol_panel(double *G, double *Ld, int d, int p, int *err, hipStream_t st);
int stm_launch_null_chol_update(double *G, int d, int p, hipStream_t st);
int stm_launch_null_nt(const double *N, int ncol, int d, int slab, int nslab, const double *X, long long ldx, int nb, double *Pt, double *T,
                       hipStream_t st);
int stm_launch_null_llt(const double *L, const double *Ld, int d, double *T, int nb, hipStream_t st);
int stm_launch_null_sub(const double *N, int ncol, int d, const double *T, int nb, double *X, long long ldx, hipStream_t st);
int stm_launch_null_norm2(const double *A, long long lda, int n, int nb, double *out, hipStream_t st);
// the values of [W A; D | W B; 0] of the damped least-squares object and |D x_j|_2 (stmmqr_lsbuild.hip).  ap / ai: A's column pointers
// and row indices as int; val: the augmented values (entry p of column j at p + j, D_jj at ap[j + 1] + j, then the B block of
// (m + n) x nrhs); D [n].  values: w NULL = all 1.  diag: D_jj = sl * d[j] (d NULL: sl; d may be D).  marquardt: D_jj = sl * the clamped
// 2-norm of the built column j.  rhs: in place on the B block, whose rows 0 .. m-1 hold B.  dnorm: out[k] = |D x_k|_2, X n x nrhs.
int stm_launch_lsb_values(long long anz, int n, const int *ap, const int *ai, const double *Ax, const double *w, double *val, hipStream_t st);
int stm_launch_lsb_diag(int n, const int *ap, const double *d, double sl, double *D, double *val, hipStream_t st);
int stm_launch_lsb_marquardt(int n, const int *ap, double sl, double smin, double smax, double *D, double *val, hipStream_t st);
int stm_launch_lsb_rhs(long long m, long long n, int nrhs, const double *w, double *Bv, hipStream_t st);
int stm_launch_lsb_dnorm(int n, int nrhs, const double *D, const double *X, long long ldx, double *out, hipStream_t st);
// the adjoint of the least-squares solve (stmmqr_lsadjoint.hip).  entries: g(i, j) = sum_k rt[i,k] z[j,k] - ut[i,k] x[j,k] over A's
// anz entries (ap / ai: A's int pattern; Axbar[p] = w[ai[p]] * g, w NULL = all 1) and over the n entries of D (row m + j; Dbar[j]);
// entry (i, k) of rt / ut at i * si_r + k * sk_r, entry (j, k) of x / z at j * si_c + k * sk_c; a NULL output is skipped.  kfast:
// out[i * nrhs + k] = in[i + k * ld], nrhs <= STMMQR_LS_MAX_NRHS.  pad: V (na x nb) = [s * src (n x nb, lds); 0], or with unit0 >= 0
// row n + unit0 + k of column k = 1.  bbar: Bbar[i, k] = w[i] * ut[i, k].  wbar: 2 sum_k rt ut / w[i], 0.0 where w[i] == 0.  resid:
// res = xbar - t per column, out[2k] = |res_k|^2, out[2k + 1] = |xbar_k|^2 (out may be NULL).
int stm_launch_lsa_entries(long long anz, int n, long long m, int nrhs, const int *ap, const int *ai, const double *rt, const double *ut,
                           long long si_r, long long sk_r, const double *x, const double *z, long long si_c, long long sk_c,
                           const double *w, double *Axbar, double *Dbar, hipStream_t st);
int stm_launch_lsa_kfast(long long rows, int nrhs, const double *in, long long ld, double *out, hipStream_t st);
int stm_launch_lsa_pad(int n, int na, int nb, const double *src, long long lds, double s, int unit0, double *V, hipStream_t st);
int stm_launch_lsa_bbar(long long m, int nrhs, const double *ut, long long ldu, const double *w, double *Bbar, long long ldbb, hipStream_t st);
int stm_launch_lsa_wbar(long long m, int nrhs, const double *rt, const double *ut, long long ld, const double *w, double *wbar, hipStream_t st);
int stm_launch_lsa_resid(int n, int nb, const double *xbar, long long ldxb, const double *t, long long ldt, double *res, long long ldr,
                         double *out, hipStream_t st);
// robust least squares (stmmqr_lsrobust.hip).  resid: r = b - A x over the row form (rp, rj, rq) with the values Ax.  abs: a = |w0 o r|
// (w0 NULL: |r|).  select: the order statistics of a over mask != 0 (mask NULL: all) -- out[0..3] = 0.5 (lo + hi), lo, hi, the count, on
// the device; sel: stm_lsr_sel_words() words, zeroed by the call.  weights: w = w0 o f(a / sigma) and stat[0..7] = sigma, lo, hi, count,
// sum of rho, rows rejected, rows with f == 1, flags, with sigma = max(med ? mad_factor * med[0] : sigma_given, sigma_min) (med: what
// select wrote); part: stm_lsr_part_doubles(m) doubles.  step: out[0] = max |x - xprev|, out[1] = max |x|.  scale: dst[p] =
// w[idx[p]] * src[p] (idx NULL: w[p]).  fill: dst[p] = v.
long long stm_lsr_sel_words();
long long stm_lsr_part_doubles(long long m);
int stm_launch_lsr_resid(long long m, const int *rp, const int *rj, const int *rq, const double *Ax, const double *x, const double *b,
                         double *r, hipStream_t st);
int stm_launch_lsr_abs(long long m, const double *w0, const double *r, double *a, hipStream_t st);
int stm_launch_lsr_select(long long len, const double *a, const double *mask, unsigned long long *sel, double *out, hipStream_t st);
int stm_launch_lsr_weights(long long m, const double *a, const double *w0, const double *med, double sigma_given, double mad_factor,
                           double sigma_min, int loss, double cc, double *w, double *part, double *stat, hipStream_t st);
int stm_launch_lsr_step(long long n, const double *x, const double *xprev, double *out, hipStream_t st);
int stm_launch_lsr_scale(long long len, const int *idx, const double *w, const double *src, double *dst, hipStream_t st);
int stm_launch_lsr_fill(long long len, double v, double *dst, hipStream_t st);
// k_rf_colnorm (stmmqr_refactor.hip): the largest column 2-norm of the ncol columns ap (64-bit pointers) of Ax, bit for bit the one
// stm_qr_default_tol takes, as the bits of a non-negative double combined into *mx_bits by an atomic maximum (mx_bits leads a block of
// 16 bytes -- the refactorization's head -- which the caller zeroes first); tsrc: NULL, or the storage position of every entry
int stm_launch_rf_colnorm(long long ncol, const long long *ap, const int *tsrc, const double *Ax, unsigned long long *mx_bits, hipStream_t st);
int stm_launch_panel_msg(void *const homes[6], const long long offs[6], const long long bytes[6], void *buf, int out, hipStream_t st);
// subtree exchange: contribution blocks between plans as fixed-size messages, packed / unpacked on the device (stmmqr_pack.hip)
struct StmFrontMsg { long long off, slot; int f, pad; };      // front f at buf + off: [8 | slot | fn - fp] doubles
struct StmFrontMsgs { StmFrontMsg m[16]; };
int stm_launch_front_msg(const DevCtx &c, const StmFrontMsgs &g, int nmsg, long long max_slot, double *buf, int out, hipStream_t st);
int stm_launch_front_cols(const DevCtx &c, int f, int part, int nparts, int nown, long long max_run, double *buf, int out, hipStream_t st);
int stm_launch_perm(const double *in, const int *perm, double *out, int n, int scatter, hipStream_t st, int nb = 1, long long sin = 0,
                    long long sout = 0);
