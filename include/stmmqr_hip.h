/* include/stmmqr_hip.h -- C ABI of libstmmqr_hip.so, the MI355X-native numerical-factorization path
 * for STM-Multifrontal-QR.
 *
 * Drop-in scope: the hot path of the reference, STMMQR/src/qr/SparseQR_factorize.c +
 * SparseQR_multithreads.c (qr_factorize -> qr_kernel -> {qr_fsize, qr_assemble, qr_front, qr_cpack,
 * qr_rhpack} + qr_stranspose2 + qr_hpinv), executed on one gfx950 device.  All entry points are plain
 * C (extern "C", pointers and sizes only).  "Long" below is the reference's Sparse_long = C long
 * (STMMQR/include/SparseBase_config.h:29); all numerics are fp64 (Makefile.option:62).
 *
 * Three groups of symbols:
 *   1. the drop-in seam with the reference's own names and signatures (a maintainer links this library
 *      instead of compiling SparseQR_factorize.c / SparseQR_multithreads.c);
 *   2. the same path on plain arrays (stmmqr_*), used by the Python host side, the tests and bench.py;
 *   3. configuration / introspection.
 *
 * Error convention (reference: SparseQR_factorize.c:329-333,378-383,540-545): nothing throws across
 * this boundary; failures free partial state, return NULL / a negative code and leave
 * cc->status < SPARSE_OK.  A missing or unusable GPU is an error (STMMQR_ERR_DEVICE), never a CPU
 * fallback.
 */
#ifndef STMMQR_HIP_H
#define STMMQR_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef long stm_long;

/* ---- status codes (values of cc->status in the reference: SparseCore.h "SPARSE_OK" family) ---- */
#define STMMQR_OK                0
#define STMMQR_ERR_OUT_OF_MEMORY (-2)   /* SPARSE_OUT_OF_MEMORY */
#define STMMQR_ERR_TOO_LARGE     (-3)   /* SPARSE_TOO_LARGE     */
#define STMMQR_ERR_INVALID       (-4)   /* SPARSE_INVALID       */
#define STMMQR_ERR_DEVICE        (-5)   /* SPARSE_GPU_PROBLEM: no gfx950 device / HIP runtime error */
#define STMMQR_ERR_RESCHEDULE    (-6)   /* stmmqr_factorize_finish: a front still had rows at the last panel the plan scheduled for it
                                           (stmmqr_plan_set_early_end); nothing is lost but this attempt -- factorize again */
#define STMMQR_ERR_STALE         (-7)   /* stmmqr_sparseqr_refactorize: a singleton of the first values has no pivot above the tolerance
                                           under the new ones; the object is unchanged -- make a new one */

/* ================================================================================================
 * Layout-compatible mirrors of the structs that cross the seam
 * ================================================================================================ */

/* sparse_csc  (STMMQR/include/SparseCore.h:514-556) */
typedef struct stm_sparse_csc {
    size_t nrow, ncol, nzmax;
    void *p, *i, *nz, *x, *z;
    int stype, itype, xtype, dtype, sorted, packed;
} stm_sparse_csc;

/* qr_symbolic (STMMQR/include/SparseQR_struct.h:26-137): produced by qr_analyze, borrowed, never modified */
typedef struct stm_qr_symbolic {
    stm_long m, n, anz;
    stm_long *Sp, *Sj, *Qfill, *PLinv, *Sleft;
    stm_long nf, maxfn;
    stm_long *Parent, *Child, *Childp, *Super, *Rp, *Rj, *Post;
    stm_long rjsize, do_rank_detection, maxstack, hisize, keepH;
    stm_long *Hip;
    stm_long ntasks, ns;
    stm_long *TaskChildp, *TaskChild, *TaskStack, *TaskFront, *TaskFrontp, *On_stack, *Stack_maxstack;
    stm_long *Fm, *Cm;
} stm_qr_symbolic;

/* qr_numeric (STMMQR/include/SparseQR_struct.h:145-209): returned, owned by the caller, released by the
 * reference's qr_freenum (SparseQR.c:1225-1272), hence every array is malloc'ed with the sizes stored here
 * and accounted in cc->malloc_count / memory_inuse exactly like SparseCore_malloc does. */
typedef struct stm_qr_numeric {
    double **Rblock;
    double **Stacks;
    stm_long *Stack_size;
    stm_long hisize, n, m, nf, ntasks, ns, maxstack;
    char *Rdead;
    stm_long rank, rank1, maxfrank;
    double norm_E_fro;
    stm_long keepH, rjsize;
    stm_long *HStair;
    double *HTau;
    stm_long *Hii, *HPinv, *Hm, *Hr;
    stm_long maxfm;
} stm_qr_numeric;

/* sparse_common is opaque here: the few fields the path touches are reached through byte offsets.
 * The defaults are the offsets of the stock reference build (LP64); a host that compiles the reference
 * with a different layout passes its own offsetof() values once (INTEGRATION.md shows the stub). */
typedef struct sparse_common_struct stm_sparse_common;
typedef struct stm_common_layout {
    size_t status, malloc_count, memory_usage, memory_inuse, blas_ok;
    size_t SPQR_grain, SPQR_small, SPQR_shrink, SPQR_flopcount, SPQR_flopcount_bound;
} stm_common_layout;
void stmmqr_set_common_layout(const stm_common_layout *layout);
void stmmqr_get_common_layout(stm_common_layout *layout);
/* SparseCore_malloc / SparseCore_free / cc->status through that layout (src/core/SparseCore_common.c:603-655): what a host-side
 * companion of this library hands to code that releases it with the reference's allocator (libstmmqr_hip_api.so does) */
void *stmmqr_cc_malloc(size_t n, size_t size, stm_sparse_common *cc);
void stmmqr_cc_free(size_t n, size_t size, void *p, stm_sparse_common *cc);
void stmmqr_cc_set_status(stm_sparse_common *cc, int code);

/* ================================================================================================
 * 1. Drop-in seam (reference names; prototypes STMMQR/include/SparseQR.h:127-268)
 * ================================================================================================ */

/* SparseQR.h:127-135; call sites SparseQR.c:349 (&A,FALSE,tol,n) and :371 (&Y,TRUE,tol,n2) */
stm_qr_numeric *qr_factorize(stm_sparse_csc **Ahandle, stm_long freeA, double tol, stm_long ntol,
                             stm_qr_symbolic *QRsym, stm_sparse_common *cc);

/* The seam keeps the plan of the last qr_symbolic it factorized (symbolic upload, schedule, workspaces, front arenas: about as
 * expensive to build as one factorization of the BASELINE matrices): a later call with an EQUAL qr_symbolic -- compared by a hash of
 * its scalars and arrays, the options and the plan-time environment -- and the same device reuses it, and skips the value map
 * (qr_stranspose2) too when A's pattern is unchanged.  A cached plan keeps its device memory until stmmqr_plan_cache_clear() /
 * stmmqr_shutdown(); env STMMQR_PLAN_CACHE = 0 turns the cache off, = n keeps the n most recent plans.
 * STMMQR_SEAM_TIMING=1 prints where a call spent its time.  Match: the interval SparseQR.c:346-377 brackets ("Factorize time"). */
void stmmqr_plan_cache_clear(void);
/* releases a qr_numeric returned by qr_factorize with the reference's accounting (= qr_freenum, SparseQR.c:1225-1272), for hosts
 * that link this library without the reference */
void stmmqr_free_numeric(stm_qr_numeric **QRnum, stm_sparse_common *cc);

/* SparseQR.h:137-143 ; globals FCHUNK/SMALL/MINCHUNK/MINCHUNK_RATIO (SparseQR.h:16-19) become library state */
int chunk_getSettings(size_t fchunk, size_t small_, size_t minchunk, size_t minchunk_ratio);

/* Inner seams on HOST buffers (device copies are made inside; used for unit parity).
 * cc may be NULL.  SparseQR.h:145-268. */
void qr_stranspose2(stm_sparse_csc *A, stm_long *Qfill, stm_long *Sp, stm_long *PLinv, double *Sx, stm_long *W);
void qr_hpinv(stm_qr_symbolic *QRsym, stm_qr_numeric *QRnum, stm_long *W);
stm_long qr_fsize(stm_long f, stm_long *Super, stm_long *Rp, stm_long *Rj, stm_long *Sleft, stm_long *Child,
                  stm_long *Childp, stm_long *Cm, stm_long *Fmap, stm_long *Stair);
void qr_assemble(stm_long f, stm_long fm, int keepH, stm_long *Super, stm_long *Rp, stm_long *Rj, stm_long *Sp,
                 stm_long *Sj, stm_long *Sleft, stm_long *Child, stm_long *Childp, double *Sx, stm_long *Fmap,
                 stm_long *Cm, double **Cblock, stm_long *Hr, stm_long *Stair, stm_long *Hii, stm_long *Hip,
                 double *F, stm_long *Cmap);
stm_long qr_csize(stm_long c, stm_long *Rp, stm_long *Cm, stm_long *Super);
stm_long qr_front(stm_long m, stm_long n, stm_long npiv, double tol, stm_long ntol, stm_long fchunk, double *F,
                  stm_long *Stair, char *Rdead, double *Tau, double *W, double *wscale, double *wssq,
                  stm_sparse_common *cc);
stm_long qr_fcsize(stm_long m, stm_long n, stm_long npiv, stm_long g);
stm_long qr_cpack(stm_long m, stm_long n, stm_long npiv, stm_long g, double *F, double *C);
stm_long qr_rhpack(int keepH, stm_long m, stm_long n, stm_long npiv, stm_long *Stair, double *F, double *R,
                   stm_long *p_rm);
void qr_larftb(int method, stm_long m, stm_long n, stm_long k, stm_long ldc, stm_long ldv, double *V,
               double *Tau, double *C, double *W, stm_sparse_common *cc);

/* ================================================================================================
 * 2. The same path on plain arrays
 * ================================================================================================ */

/* symbolic inputs as plain arrays (same meaning as the qr_symbolic fields of the same name) */
typedef struct stmmqr_symbolic_view {
    stm_long m, n, anz, nf, maxfn, rjsize, hisize, do_rank_detection;
    const stm_long *Sp, *Sj, *Qfill, *PLinv, *Sleft;
    const stm_long *Child, *Childp, *Super, *Rp, *Rj, *Post, *Hip, *Fm;
    stm_long maxstack;          /* QRsym->maxstack: the analysis' bound for the reference's one stack, hence for all of R+H; sizes the
                                   R+H arena of the slab recycling.  0 = unknown (the arena then holds all recycled slabs)          */
    stm_long r_only;            /* !QRsym->keepH.  0 (a zero-initialised view): the Householder vectors are kept (R+H blocks), as
                                   always.  1: R only, in qr_rhpack's keepH = 0 layout -- less device memory and a smaller download;
                                   stmmqr_plan_rsolve and the seminormal solve work, everything that needs Q (qmult, solve, H of
                                   export_r) returns STMMQR_ERR_INVALID, and the plan takes one group only (stmmqr_plan_set_groups,
                                   the shared-front and phase entries refuse it) */
} stmmqr_symbolic_view;

/* per-call measurements (all times in milliseconds, HIP events on the library's own stream) */
typedef struct stmmqr_stats {
    double flops;              /* the reference's FLOP_COUNT formula (SparseQR_factorize.c:1571)          */
    double ms_total;           /* upload-excluded device time: gather S .. pack R+H                        */
    double ms_assemble;        /* front_setup + assemble kernels                                            */
    double ms_front;           /* panel + trailing-update + small-front kernels (detail runs)              */
    double ms_pack;            /* R+H count / scan / copy kernels                                           */
    double ms_h2d, ms_d2h;     /* PCIe transfers of A values in, packed factors out                         */
    double ms_host;            /* host-side planning + hpinv                                                */
    double bytes_assemble;     /* algorithmic bytes of the assembly kernels, SURVEY.md 8(d) formula        */
    double bytes_pack;
    double flops_update;       /* flops executed by the MFMA trailing-update kernel (4*m*n*k per block)    */
    double ms_update;          /* time of the MFMA trailing-update launches only                            */
    stm_long nlaunch;          /* kernel launches in the timed region                                       */
    stm_long nlevels;
    /* detail runs only (stats->nlaunch == -1 on entry): HIP-event pairs around every launch of a category, recorded on
       the plan's stream without any synchronisation (the schedule runs as in an untimed call)                       */
    double ms_panel;           /* panel kernels of the large fronts (k_panel / k_panel_ca)                          */
    double ms_small;           /* k_front_wg: whole small fronts                                                    */
    stm_long npanel_launch, nupdate_launch;   /* event pairs behind ms_panel / ms_update (one per timeline step)    */
    stm_long nsteps;           /* steps of the factorization timeline (a big front advances one panel per step)     */
    double flops_update_pair;  /* the part of flops_update on fronts that take the pair update (two panels per sweep:
                                  12 instead of 24 algorithmic bytes per updated entry and panel)                     */
    stm_long retries;          /* times (part of) the factorization was run again with one-workgroup panels because a bounded
                                  inter-workgroup wait of a panel kernel ran out (0 in a healthy run: bench.py asserts it)  */
    double device_bytes;       /* device memory held by the plan when the factorization finished (arenas, factors, workspaces) */
    stm_long reschedules;      /* times the factorization was run again on the FULL schedule because a front still had rows at the
                                  last panel the plan had scheduled for it (the schedule of a whole-tree plan stops every front where
                                  the full-rank row estimate says it runs out of rows; rank-deficient input: once per plan, which
                                  then keeps the full schedule)                                                           */
} stmmqr_stats;

typedef struct stmmqr_plan stmmqr_plan;     /* device-resident symbolic plan + arenas; reusable across calls */

/* Build the device plan from the symbolic analysis (host work + one upload).  Returns NULL on error
 * (*status gets the code).  device < 0 selects the current HIP device.  The front and contribution-block arenas are
 * sized from the fronts the plan factorizes, shares or imports (all of them until stmmqr_plan_set_groups says otherwise)
 * and allocated by the first factorization: STMMQR_ERR_OUT_OF_MEMORY then comes from stmmqr_factorize_begin /
 * stmmqr_factorize_device, and one rank of a sharded run never holds the whole tree. */
stmmqr_plan *stmmqr_plan_create(const stmmqr_symbolic_view *sym, int device, int *status);
void stmmqr_plan_destroy(stmmqr_plan *plan);

/* Give the plan the pattern of A (column pointers / row indices): builds the qr_stranspose2 gather map
 * (SparseQR_factorize.c:755-785) once.  stmmqr_factorize_device does this itself when Ap/Ai are non-NULL. */
int stmmqr_plan_set_pattern(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai);

/* Numeric factorization of A (CSC, Long indices) with a plan.  Results stay resident in HBM inside the plan;
 * stmmqr_plan_download copies them out.  Ax may be a host pointer (uploaded, timed as ms_h2d) or, when
 * ax_on_device != 0, a device pointer. */
int stmmqr_factorize_device(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                            int ax_on_device, double tol, stm_long ntol, stmmqr_stats *stats);

/* The same factorization in phases (multi-GPU): begin (upload values) -> factorize_group(g) for the groups of
 * stmmqr_plan_set_groups in increasing order, with stmmqr_plan_import_front calls in between -> finish (pack). */
int stmmqr_factorize_begin(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                           int ax_on_device, double tol, stm_long ntol);
int stmmqr_factorize_group(stmmqr_plan *plan, int group, int detail);
int stmmqr_factorize_finish(stmmqr_plan *plan, stmmqr_stats *stats);

/* Subtree sharding.  group[f] >= 0: front f is factorized on this device in phase group[f];
 * -1: on another device (its packed contribution block, row ids, fm/rank/cm arrive by import_front before the
 * phase of its parent).  A child must never be in a later phase than its parent. */
int stmmqr_plan_set_groups(stmmqr_plan *plan, const int *group /* [nf] */);
/* info[0..5] = fm, rank, cm, csize, fn, fp of a factorized (or imported) front */
int stmmqr_plan_front_info(stmmqr_plan *plan, stm_long f, stm_long *info);
/* packed contribution block (csize doubles, qr_cpack layout) + cm row ids of front f; C may be a device pointer */
int stmmqr_plan_export_front(stmmqr_plan *plan, stm_long f, double *C, stm_long *rows, int c_on_device);
int stmmqr_plan_import_front(stmmqr_plan *plan, stm_long f, stm_long fm, stm_long rank, stm_long cm, const double *C,
                             const stm_long *rows, int c_on_device);

/* A front SHARED between plans (one plan per device): the reference moves whole contribution blocks between
 * its stacks (SparseQR_factorize.c:1228) and leaves a big front to one thread team; here the trailing matrix of one front is
 * spread over the devices of a group by 32-column blocks.  Every plan of the group marks the front
 *     group[f] = phase | STMMQR_GROUP_SHARED            (alone in its group, one of the large fronts, no pair update)
 * assembles it, and then walks the group's timeline -- one step per 32-column panel -- with stmmqr_factorize_step:
 *     PREP (step 0)                       set up + assemble (every plan: each holds the whole front)
 *     PANEL (step q)                      only the plan that owns panel q (q % nparts == part), then
 *         stmmqr_plan_export_panel        -> the others  stmmqr_plan_import_panel   (columns, T, Tau/Stair/Rdead, progress)
 *     UPDATE|GRAM (step q)                every plan, on its own column blocks: block b of step q holds the columns of panel
 *                                         q + 1 + b, so plan `part` takes cb_first = (part - q - 1) mod nparts, stride nparts
 *                                         (GRAM: build T of the step's panel; once per step and plan, before or with the first
 *                                         UPDATE; cb_count limits the launch, e.g. to block 0 before the next PANEL)
 *     POST (last step)                    pack the contribution block (complete in the owned columns only:
 *                                         stmmqr_plan_export_front_cols / _import_front_cols gather it on one plan)
 * The arithmetic of a column block does not depend on the plan that runs it: same bits as the unshared front with
 * options.pair_update = 0.  After stmmqr_factorize_finish every plan's packed R+H block of the front is valid in the columns
 * of its own panels (stmmqr_plan_front_rhoff gives the column offsets for the merge). */
#define STMMQR_GROUP_SHARED  (1 << 30)
#define STMMQR_STEP_PREP     1
#define STMMQR_STEP_PANEL    2
#define STMMQR_STEP_UPDATE   4
#define STMMQR_STEP_GRAM     8
#define STMMQR_STEP_POST     16
/* steps of a group's timeline (a shared front: its number of panels); -1 = no such group */
int stmmqr_plan_group_steps(stmmqr_plan *plan, int group);
int stmmqr_factorize_step(stmmqr_plan *plan, int group, int step, int what, int cb_first, int cb_stride, int cb_count);
/* one panel message: ndoubles is the same for every panel of the front; buf may be a device pointer (on_device != 0).
 * export returns when the buffer is complete; import is ordered on the plan's stream. */
int stmmqr_plan_panel_doubles(stmmqr_plan *plan, stm_long f, stm_long *ndoubles);
int stmmqr_plan_export_panel(stmmqr_plan *plan, stm_long f, stm_long p, double *buf, int on_device);
int stmmqr_plan_import_panel(stmmqr_plan *plan, stm_long f, stm_long p, const double *buf, int on_device);
/* the columns of the packed contribution block that belong to the panels of `part` (buf == NULL: count only) */
int stmmqr_plan_export_front_cols(stmmqr_plan *plan, stm_long f, int part, int nparts, double *buf, int on_device,
                                  stm_long *ndoubles);
int stmmqr_plan_import_front_cols(stmmqr_plan *plan, stm_long f, int part, int nparts, const double *buf, int on_device);
/* The panel loop of a shared front, native (round 4): ONE call per rank and shared front does what the step-by-step interface
 * above does from a host loop -- PREP, then for every panel the owner's block 0 / PANEL / export / send / rest of its update and
 * the others' posted receive / update / import -- with everything enqueued on the plan's stream and a comm stream ordered by
 * events: no stream synchronisation and no interpreter between two steps; the send of panel t overlaps the owner's update of step
 * t - 1, a receiver posts the receive of panel t before its update of step t - 1.  This rank is tr->rank, the group is the ranks
 * [first_rank, first_rank + nranks).  Returns when the device has finished the front.
 * The transport is a table of callbacks on DEVICE buffers, enqueued on the stream they are given:
 *   stmmqr_rccl_transport_create   RCCL point-to-point (ncclSend / ncclRecv in a group) -- the xGMI path of a multi-GPU node;
 *                                  librccl is loaded at run time; the 128-byte id comes from stmmqr_rccl_unique_id on one rank
 *                                  and reaches the others by any means (bench.py: a torch.distributed broadcast)
 *   a caller's own table           tests play the ranks of a group on ONE GPU this way (tests/test_gpu_sharded.py) */
typedef struct stmmqr_transport {
    void *ctx;
    int (*send)(void *ctx, const void *dev_buf, size_t bytes, int peer, void *hip_stream);
    int (*recv)(void *ctx, void *dev_buf, size_t bytes, int peer, void *hip_stream);
    int (*group_begin)(void *ctx);          /* may be NULL */
    int (*group_end)(void *ctx);            /* may be NULL */
    int rank, size;
} stmmqr_transport;
int stmmqr_factorize_shared_front(stmmqr_plan *plan, int group, stm_long f, int first_rank, int nranks, const stmmqr_transport *tr);
/* The subtree exchange, native (round 5): the contribution blocks that enter a phase from other ranks.  The unit of exchange is the
 * reference's: the packed C block of a child front with its row ids (SparseQR_factorize.c:1228; between the reference's tasks it
 * stays in shared memory).  Block q of the `out` list goes to rank out_peer[q], block q of the `in` list comes from in_peer[q]; for
 * one pair of ranks the fronts appear in the same order on both sides.  A block is ONE message whose size the plan knows (8 doubles
 * of header + the front's symbolic C slot + fn - fp row ids), packed by a kernel that reads the front's state on the device, sent
 * and received on the plan's stream in one transport group, unpacked by a kernel that writes the state
 * stmmqr_plan_import_front would: the host neither waits for the device nor learns (fm, rank, cm).  A message that does not fit the
 * front's symbolic bounds makes the factorization fail (stats.failed at stmmqr_factorize_finish).
 * stmmqr_shared_front_gather: after the panel loop of a shared front, the columns of its contribution block that the other ranks
 * of the group own, collected on the group's first rank (the native form of stmmqr_plan_export/import_front_cols; nothing to do
 * for a root).
 * stmmqr_factorize_phases: everything between stmmqr_factorize_begin and stmmqr_factorize_finish of a sharded factorization as ONE
 * call -- per phase k: the exchange (lists [out_ptr[k], out_ptr[k+1]) / [in_ptr[k], in_ptr[k+1])), then the shared front this rank
 * takes part in (shared_front[k] >= 0: panel loop + gather, group [shared_first[k], + shared_span[k])) or its own fronts of the
 * phase (has_group[k]: stmmqr_factorize_group(plan, k)).  The only host waits left are the eight bytes stmmqr_factorize_group reads
 * after a group. */
int stmmqr_factorize_exchange(stmmqr_plan *plan, stm_long nout, const stm_long *out_front, const int *out_peer, stm_long nin,
                              const stm_long *in_front, const int *in_peer, const stmmqr_transport *tr);
int stmmqr_shared_front_gather(stmmqr_plan *plan, stm_long f, int first_rank, int nranks, const stmmqr_transport *tr);
/* How many panels of a front get a step ("How many panels"): a front of fm rows needs floor(fm / 32) + 1 of its
 * ceil(fn / 32) panels, and fm -- known on the device only -- equals the plan-time estimate unless pivot columns die.
 * stmmqr_factorize_device cuts the schedule of a whole-tree plan there by itself and runs a factorization that outlives it again on
 * the full schedule.  A caller of the phased interface (begin / group / finish: sharded plans) has no such loop around it and gets the
 * full schedule unless it asks: mode 1 = cut schedule, and the CALLER handles STMMQR_ERR_RESCHEDULE from stmmqr_factorize_finish --
 * every rank of a sharded factorization must then factorize again (sharded.factorize_sharded agrees on that with one tiny exchange per
 * factorization); the plan that failed schedules every panel from its next begin on, the others are told by mode 0.
 * Rebuilds the schedule; not between begin and finish (except after that failure).  Shared fronts always keep every panel. */
int stmmqr_plan_set_early_end(stmmqr_plan *plan, int mode);
typedef struct stmmqr_shard_phases {
    int nphase;
    const stm_long *out_ptr, *out_front;    /* [nphase + 1], [out_ptr[nphase]] */
    const int *out_peer;
    const stm_long *in_ptr, *in_front;
    const int *in_peer;
    const stm_long *shared_front;           /* [nphase]: -1 = none */
    const int *shared_first, *shared_span;  /* [nphase] */
    const int *has_group;                   /* [nphase] */
} stmmqr_shard_phases;
int stmmqr_factorize_phases(stmmqr_plan *plan, const stmmqr_shard_phases *ph, const stmmqr_transport *tr);
int stmmqr_device_copy(void *dst, const void *src, size_t bytes, void *hip_stream);   /* D2D, complete on return, after the stream's work */
int stmmqr_rccl_unique_id(char id[128]);
int stmmqr_rccl_transport_create(int world, int rank, const char id[128], stmmqr_transport **out);
void stmmqr_rccl_transport_destroy(stmmqr_transport *tr);
int stmmqr_transport_sendrecv(const stmmqr_transport *tr, const void *sendbuf, size_t sendbytes, int dst, void *recvbuf, size_t recvbytes,
                              int src, void *hip_stream);

/* off[0..fn]: start of each column of front f inside its packed R+H block (after stmmqr_factorize_finish) */
int stmmqr_plan_front_rhoff(stmmqr_plan *plan, stm_long f, stm_long *off);

/* slab recycling: 1 when front f keeps its slab (its packed block is produced on the fly by stmmqr_plan_download), 0 when its block
 * is staged in the R+H arena; -1 for a plan that does not recycle its slabs or a bad f */
int stmmqr_plan_front_kept(const stmmqr_plan *plan, stm_long f);

/* device memory the plan holds right now, in bytes (what stmmqr_stats.device_bytes reports at the end of a factorization) */
double stmmqr_plan_device_bytes(const stmmqr_plan *plan);

/* out[0..1] = the reference's flop count of front f (FLOP_COUNT, SparseQR_factorize.c:1571) and the part of it done by
 * trailing updates: every plan of a shared front counts the whole front, the merge keeps one */
int stmmqr_plan_front_flops(stmmqr_plan *plan, stm_long f, double *out);

/* sizes needed by the caller to allocate the outputs of stmmqr_plan_download */
int stmmqr_plan_result_sizes(const stmmqr_plan *plan, stm_long *rh_total, stm_long *rank);

/* Copy the results of the last stmmqr_factorize_device to host arrays laid out like qr_numeric:
 * Stack[rh_total] holds the packed R+H blocks in Post order (= the single shrunk stack of the reference's
 * serial run), Rblock_off[nf] the offset of each front's block in it.  Any pointer may be NULL. */
int stmmqr_plan_download(stmmqr_plan *plan, double *Stack, stm_long *Rblock_off, char *Rdead, stm_long *HStair,
                         double *HTau, stm_long *Hii, stm_long *HPinv, stm_long *Hm, stm_long *Hr,
                         stm_long *scalars /* [rank, rank1, maxfrank, maxfm] */, stmmqr_stats *stats);

/* one-shot convenience: plan + factorize + download (what qr_factorize does internally) */
int stmmqr_factorize_arrays(const stmmqr_symbolic_view *sym, const stm_long *Ap, const stm_long *Ai,
                            const double *Ax, double tol, stm_long ntol, double *Stack, stm_long stack_cap,
                            stm_long *Rblock_off, char *Rdead, stm_long *HStair, double *HTau, stm_long *Hii,
                            stm_long *HPinv, stm_long *Hm, stm_long *Hr, stm_long *scalars, stmmqr_stats *stats);

/* Q-apply and least-squares solve on the factors that are still resident in HBM after
 * stmmqr_factorize_device -- no download of the packed R+H.
 *   stmmqr_plan_qmult  replaces QR_qmult (STMMQR/include/SparseQR.h:403-409; SparseQR.c:1790-2020) for the methods
 *                      QR_QTX (0: X <- Q'X) and QR_QX (1: X <- Q X) on a dense m x nrhs array, in place.  Row order as in
 *                      the reference: Q'X comes back in the row order of R (HPinv applied), Q X expects it.
 *   stmmqr_plan_solve  replaces QR_solve(QR_RETX_EQUALS_B) (SparseQR.h:411-417; SparseQR.c:2024-2216 + qr_rsolve
 *                      :2218-2517): X = E * R^{-1} * (Q'B)(1:n), the solution the driver's residual check uses
 *                      (qrtest.c:11-53); dead pivot columns get x = 0 (the reference's basic solution).  The singleton
 *                      block R1 of SparseQR() is not part of the plan: it stays with the caller. */
int stmmqr_plan_qmult(stmmqr_plan *plan, int method, double *X, stm_long ldx, stm_long nrhs);
int stmmqr_plan_solve(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs);
/*   stmmqr_plan_qmult also takes the methods QR_XQT (2: X <- X Q') and QR_XQ (3: X <- X Q) of qr_panel (SparseQR.c:1591-1700,
 *                      2040-2075): X is then k x m with ldx >= k and `nrhs` = k.  All vectors cross PCIe in one transfer.
 *   stmmqr_plan_rsolve replaces QR_solve for all four systems (SparseQR_definitions.h:27-30; SparseQR.c:2118-2216,
 *                      qr_rsolve :2218-2517, qr_private_rtsolve :2522): 0 QR_RX_EQUALS_B  X = R\B, 1 QR_RETX_EQUALS_B
 *                      X = E(R\B) -- B is m x nrhs in R's row order (what QR_QTX returns), X n x nrhs --, 2 QR_RTX_EQUALS_B
 *                      X = R'\B, 3 QR_RTX_EQUALS_ETB  X = R'\(E'B) -- B n x nrhs, X m x nrhs (zero beyond the rank). */
int stmmqr_plan_rsolve(stmmqr_plan *plan, int system, const double *B, stm_long ldb, double *X, stm_long ldx,
                       stm_long nrhs);
/* Factors without H (stmmqr_symbolic_view.r_only = 1, QRsym->keepH = 0): stmmqr_plan_rsolve takes all four systems;
 * stmmqr_plan_qmult and stmmqr_plan_solve return STMMQR_ERR_INVALID (the message names keepH) and leave the plan usable.
 *   stmmqr_plan_keep_h           1 / 0: the plan's keepH (-1: null plan).
 *   stmmqr_plan_spmv             Y = A X (trans 0: X n x nrhs, Y m x nrhs) or Y = A' X (trans 1: X m x nrhs, Y n x nrhs) with the
 *                                values of the last factorization and A's pattern as given to it (A's own row and column order).
 *                                on_device: X and Y are device pointers, else host arrays.  Deterministic: every entry is summed
 *                                in index order, no atomics, so column j of a batch equals the single-vector call.
 *   stmmqr_plan_solve_seminormal least squares with R only, by the corrected seminormal equations: x = E R^-1 R^-T E' A'b, then
 *                                `refine` times r = b - A x, x += E R^-1 R^-T E' A'r (B m x nrhs, X n x nrhs; device pointers
 *                                with on_device).  Works on plans with and without H and reads R only.  Dead columns get x = 0
 *                                (the basic solution).  info (may be NULL): the largest |A'r| / (|A|_F (|A|_F |x| + |b|)) over the
 *                                right-hand sides, r = b - A x of the returned x.  Accurate to about cond(A) u only while
 *                                cond(A)^2 u << 1: above cond(A) ~ 1e7 the Q-based stmmqr_plan_solve is the right tool
 *                                (stmmqr_plan_condest below estimates cond(A) from the factors the plan holds).  A front too
 *                                wide for the one-workgroup R' solve gives STMMQR_ERR_TOO_LARGE, as stmmqr_plan_rsolve systems 2-3.
 *                                (stmmqr_plan_solve_minnorm below has no such limit: its R' pass splits such fronts.) */
int stmmqr_plan_keep_h(const stmmqr_plan *plan);
int stmmqr_plan_spmv(stmmqr_plan *plan, int trans, const double *X, stm_long ldx, double *Y, stm_long ldy, stm_long nrhs, int on_device);
int stmmqr_plan_solve_seminormal(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs, int refine,
                                 int on_device, double *info);

/* X (m x nrhs, ldx >= m) = Q * (R' \ B) (permuted != 0: B, n x nrhs, is in R's column order) or Q * (R' \ (E' B)) (permuted == 0):
 * with the plan holding the factorization of M (m x n), the minimum-2-norm solution of the equations M(:, live)' x = b(live);
 * live = the pivot columns that did not die.  Dead columns have no equation (the squeezed R of qr_private_rtsolve).
 * Needs H.  on_device: B and X are device pointers.
 * Everything runs on the device, with no host round trip between the two passes, and the result is in the caller's row order of M
 * (what stmmqr_plan_qmult method 1 returns).  At default settings it is, bit for bit, stmmqr_plan_qmult(1) of stmmqr_plan_rsolve(3 / 2)
 * wherever those accept the tree -- but it never returns STMMQR_ERR_TOO_LARGE for the width of a front: a front that the
 * one-workgroup R' solve cannot hold has its columns split over workgroups (STMMQR_RTBIG_MIN splits smaller ones too).  Refusals
 * (STMMQR_ERR_INVALID, the plan stays usable): nothing factorized, bad pointers or leading dimensions, keepH = 0 (the message names
 * keepH, as stmmqr_plan_qmult's).  nrhs = 0 returns 0 and writes nothing. */
int stmmqr_plan_solve_minnorm(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs,
                              int permuted, int on_device);

/* Products with R itself on the resident factors.  R is the whole rank x n factor, dead pivot columns included (they keep the rows
 * above them): the matrix of A E = Q R, so stmmqr_plan_qmult(1, .) of the result of trans = 0 reproduces A x.
 *   trans = 0: X is n x nrhs (ldx >= n), Y is m x nrhs (ldy >= m) in R's row order -- what stmmqr_plan_qmult method 0 returns and
 *              method 1 takes.  Y = R X (permuted != 0: X is in R's column order) or R (E' X) (permuted == 0: X is in the caller's
 *              column order and is gathered through Qfill).  Rows beyond the rank are written as zero.
 *   trans = 1: X is m x nrhs, rows beyond the rank are not read; Y is n x nrhs.  Y = R' X or E (R' X).
 * Reads R only: plans with and without H, and no limit on the width or height of a front.  on_device: X and Y are device pointers.
 * Deterministic: every entry is summed in an order fixed by the front it belongs to -- no atomics (R' X adds every front's column
 * dots in the order of the fronts) -- so column j of a batch carries the bits of the one-vector call, host and device output carry
 * the same bits, and so do plans with and without H.  Batches of STMMQR_RHS_BATCH vectors share one pass.  trans = 0 allocates
 * nothing beyond the caller's vectors; the index and the slot array the transposed product needs (the transpose of Rj, one double
 * per entry of Rj and vector of a batch) are made at the first call with trans = 1; a plan that never calls this allocates nothing for it.
 * Refusals (STMMQR_ERR_INVALID, the plan stays usable): nothing factorized, trans not 0 or 1, bad pointers or leading dimensions.
 * nrhs = 0 returns 0 and writes nothing. */
int stmmqr_plan_rmult(stmmqr_plan *plan, int trans, const double *X, stm_long ldx, double *Y, stm_long ldy, stm_long nrhs, int permuted,
                      int on_device);

/* The condition number of the held factorization, estimated on the device.  R_live = R over its live pivot columns (rank x rank, upper
 * triangular); since A E = Q R, cond(R_live) = cond(A(:, live)) in the 2-norm, and within a factor sqrt(m) of it in the 1-norm.
 *   kind = 1: the one-norm, the convention of LAPACK's dtrcon / dlacn2.  |R_live|_1 is exact (column sums on the device);
 *             |R_live^-1|_1 is Hager's estimate in Higham's form: from x = 1/r at most five rounds of y = R \ x, xi = sign(y),
 *             z = R' \ xi, x = e_j at the first largest |z_j|, until |z|_inf <= z'x, the arg-max repeats or the estimate stops
 *             growing; then the safeguard vector x_i = (-1)^i (1 + i / (r - 1)) with estimate 2 |R \ x|_1 / (3 r); the larger of
 *             the two.  Cost: out[3] rounds, each a solve with R and one with R', plus one solve with R (typically 2-3 rounds).
 *   kind = 2: the two-norm.  `iters` steps (iters <= 0: 8) of the power iteration on R'R for |R_live|_2 and of the same iteration
 *             on its inverse (a solve with R' and one with R per step) for |R_live^-1|_2 = 1 / |R_live v|_2 of its last iterate v;
 *             both start from the safeguard vector, normalised.  Cost: iters solve pairs and 2 iters + 1 products with R.
 * Both kinds are LOWER bounds of the condition number: every quantity is |M x| / |x| of some x.  Expect 0.7 .. 1 of the true
 * one-norm condition, and 0.9 .. 1 of the two-norm condition after 8 steps (measured: DESIGN.md 6k).  All vectors stay on the
 * device; the host reads a few scalars per round.
 *   out[0] the condition estimate = out[1] * out[2]     out[1] the norm of R_live     out[2] the estimated norm of its inverse
 *   out[3] kind 1: the rounds entered -- every round is a solve with R, and every round but possibly the last (the one that stops
 *          because the estimate did not grow, or the fifth) a solve with R' as well; the safeguard's one solve with R is not counted.
 *          kind 2: the solve pairs of the inverse iteration whose result became the iterate (iters, unless a zero or non-finite
 *          norm ended it early)
 *   out[4] r = the number of live pivot columns     out[5] kind     out[6..7] 0
 *   r = 0: condition 1, norms 0, nothing is launched.
 *   v non-NULL [ncol]: an approximate null vector in the caller's column order, zero on dead columns, of unit norm of the kind.
 *   kind 1: R_live^-1 x / |R_live^-1 x|_1 of the x that attained the estimate, so |R_live v|_1 = 1 / out[2] (MATLAB's
 *   [c, v] = condest(A)); kind 2: the last iterate of the inverse iteration, |R_live v|_2 = 1 / out[2].  It lets a caller verify
 *   the estimate without trusting the iteration.
 *   ncol < the columns of the plan: the plan holds [A B] as stmmqr_plan_solve_carried expects it (the same messages) and the
 *   trailing columns take no part.  on_device: out and v are device pointers.
 * Reads R only: plans with and without H, fronts of any width (the R' solves are those of stmmqr_plan_solve_minnorm).  Its vectors
 * are made at the first call.  STMMQR_ERR_INVALID (the message says why; the plan stays usable): null plan or nothing factorized, out
 * NULL, ncol out of range, kind not 1 or 2, the carried conditions not met for ncol < n, or a plan that does not hold the whole tree. */
int stmmqr_plan_condest(stmmqr_plan *plan, stm_long ncol, int kind, int iters, double *out /* [8] */, double *v /* [ncol] or NULL */,
                        int on_device);

/* Minimum-norm least squares on rank-deficient factors.  Every solve above returns the BASIC solution: x = 0 on the columns whose
 * pivot died.  With pc the r live and jd the d dead pivot columns among the first ncol (R's column order), R11 = R(:, pc) and
 * R12 = R(:, jd):
 *     W = R11^-1 R12,   N = [-W on pc; I on jd]  (ncol x d),   R N = 0,
 * so |A E N(:, k)|_2 <= tol + rounding (only what the rank test dropped), and the minimum-norm least-squares solution is
 *     x_min = (I - N G^-1 N') x_basic,   G = N'N = I + W'W = L L'   (what lsqminnorm, spqr_cod or a pseudo-inverse return).
 * N, G and L live on the device and belong to the factorization held: the first call with a given ncol builds them (N a batch of
 * STMMQR_RHS_BATCH dead columns per pass over the tree: a unit vector through the product with R, then the back substitution, and one
 * step of refinement on a residual R N whose row sums are carried in two doubles, which takes the error of N from eps cond(R11) to
 * eps (1 + eps cond(R11)^2); G by
 * 32 x 32 tiles over row slabs of STMMQR_NULL_SLAB rows on the matrix cores; L by a right-looking blocked Cholesky factorization),
 * later calls find them, the next factorization releases them.  While held, stmmqr_plan_device_bytes counts their
 * 8 (ncol d + d^2 + 1024 ceil(d / 32)) + 4 d bytes.  The projector is applied twice (one pass leaves |N'x| / (|N| |x|) near
 * |W|_2 u, the second brings it to u).  The error of x_min is governed by cond(R11) max(1, |W|_2) u, not by cond(G).
 *   stmmqr_plan_nullspace        *ndead = d.  N non-NULL (ldn >= ncol): receives N, ncol x d column-major; column k belongs to the k-th
 *                                dead column in R's column order: exactly 1.0 on that column, exactly 0.0 on the other dead columns,
 *                                -W(:, k) on the live ones.  permuted == 0: the rows are in the caller's column order (scattered
 *                                through Qfill); permuted != 0: in R's column order.  N NULL: only *ndead is written, nothing is built.
 *   stmmqr_plan_project_minnorm  X (ncol x nrhs, ldx >= ncol, in place) <- (I - N G^-1 N')^2 X; permuted as above.  info ([8], host,
 *                                may be NULL): [0] d; [1] the largest |N'x_out|_2 / (|N|_F |x_in|_2) over the right-hand sides, measured
 *                                on the device after the second pass (0 where x_in = 0); [2] |N|_F; [3] the smallest diagonal entry
 *                                of L (>= 1 in exact arithmetic); [4] 1 if this call built N and L, 0 if it found them; [5..7] 0.
 *   stmmqr_plan_solve_lsminnorm  stmmqr_plan_solve followed by the projector: B m x nrhs, X n x nrhs.  Needs H (keepH = 0: refused with
 *                                stmmqr_plan_solve's message); the other two read R only and work on plans with and without H.
 * ncol < the columns of the plan: the plan holds [A B] as stmmqr_plan_solve_carried expects it (the same messages) and the trailing
 * columns take no part.  d = 0: *ndead = 0, X comes back bit for bit, nothing is launched and nothing is allocated.  nrhs = 0 returns
 * 0 and writes nothing.  on_device: N, X and B are device pointers.
 * Deterministic: no atomics, every sum in an order fixed by (ncol, d, the slab height) alone, so column j of a batch carries the bits
 * of the one-vector call, host and device output, two calls, and plans with and without H carry the same bits.
 * STMMQR_ERR_INVALID (the message says why; the plan stays usable): null plan or nothing factorized, bad pointers or leading
 * dimensions, ncol out of range, the carried conditions not met for ncol < n, a plan that does not hold the whole tree, or a pivot
 * of the Cholesky factorization that is not positive and finite (only a non-finite W can do that; the message names the pivot).
 * STMMQR_ERR_OUT_OF_MEMORY: no room for N, G and the partial sums; whatever was allocated is released and the plan stays usable.
 * Measured on an MI355X, largest ratio to the bounds of tests/test_gpu_nullspace.py over the committed fixtures:
 * |R N(:, k)| 1.4e-3 of its bound, |A E N(:, k)| 0.81 of tol + that bound (reorientation_8), |N - N_ref| / |N_ref| <= 1.8e-15, and
 * 1.3e-12 on lns_3937 (cond(R11) 8.3e12; 1e-8 without the refinement step); after the second pass |N'x| / (|N|_F |x|) <= 3.3e-17
 * against the device's own N and 3.5e-3 of 8 (d + 2) eps at most against the long double N_ref.  Whole path against a dense SVD
 * solution: 2.3e-15 (small fixtures), 2.3e-12 (dwt_992).
 * Times: cvxqp3 (n = 17500, d = 458) N 418 ms, Gram 0.43 ms, Cholesky 0.55 ms, one projection 1.24 ms (32 vectors: 1.50 ms) next to
 * 8.8 ms of one stmmqr_plan_solve; lns_3937 (n = 3908, d = 2086) 222 / 0.87 / 2.87 ms, 7.9 ms (8.4 ms), solve 3.0 ms.
 * Out of scope: a stmmqr_sparseqr_* entry point.  The singleton block R1 of that object lives on the host and is no part of the
 * plan (as for the variances); the stmmqr_ls object below removes no singletons and is the home of this feature. */
int stmmqr_plan_nullspace(stmmqr_plan *plan, stm_long ncol, stm_long *ndead, double *N, stm_long ldn, int permuted, int on_device);
int stmmqr_plan_project_minnorm(stmmqr_plan *plan, stm_long ncol, double *X, stm_long ldx, stm_long nrhs, int permuted, int on_device,
                                double *info /* [8] or NULL, host */);
int stmmqr_plan_solve_lsminnorm(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs, int on_device,
                                double *info);
/* ms [3]: device milliseconds of the last build of the basis the plan holds -- N, the Gram matrix, the Cholesky factorization
 * (STMMQR_ERR_INVALID if it holds none). */
int stmmqr_plan_nullspace_times(const stmmqr_plan *plan, double *ms);

/* Least squares with the right-hand sides carried through the factorization: the plan holds a factorization of the m x (n + nrhs)
 * matrix [A B] made with ntol = n (the columns of B are never rank-tested), whose Qfill is the identity on the last nrhs columns.
 * The reflectors reached B as trailing columns, so C = Q'B sits in the last nrhs columns of R and no Q is needed:
 *   X (n x nrhs, ldx >= n) = E R11^-1 C, C = R(rows of the live columns among the first n, n + j); dead columns among the first n get
 *   x = 0 (the basic solution, as stmmqr_plan_solve); resid[j] (may be NULL) = the 2-norm of column n + j of R below those rows
 *   = |b_j - A x_j|_2, 0 where no such rows exist (square full-rank A).
 * Reads R only: plans with and without H.  No diagonal entry of the B block is a divisor: b = 0 and b in range(A) give finite results.
 * Batches of STMMQR_RHS_BATCH right-hand sides share one pass over the tree.  on_device: X and resid are device pointers.
 * STMMQR_ERR_INVALID (the message says why; the plan stays usable): nothing factorized, the last factorization's ntol is not
 * n = (columns of the plan) - nrhs, or a B column is permuted.  A host that runs the reference's qr_analyze on [A B] and calls
 * qr_factorize(..., ntol = n) can use it on the seam's cached plan. */
int stmmqr_plan_solve_carried(stmmqr_plan *plan, stm_long nrhs, double *X, stm_long ldx, double *resid, int on_device);

/* Variances of a least-squares fit.  var[j], j < ncol (the caller's column order) = diag(((A E)_live' (A E)_live)^-1), the unscaled
 * variances of the basic least-squares solution; (A E)_live holds the columns with Rdead == 0.  Dead columns get 0, as the solves give
 * x = 0 there.  The variance of x_j is var[j] * |b - A x|^2 / (m - rank).
 * The selected inverse of R'R (Takahashi / Erisman-Tinney) is built front by front from the root to the leaves with dense triangular
 * solves and matrix products on the fronts held in HBM.  Reads R only: plans with and without H.  No limit on the width of a front.
 *   ncol = the number of columns of the plan: all of them.
 *   ncol < that: the plan holds [A B] as stmmqr_plan_solve_carried expects it (ntol = ncol, Qfill the identity on the trailing
 *   columns: the same messages), and the trailing columns take no part.
 *   on_device: var is a device pointer.
 * Device memory of the call alone, released before it returns (stmmqr_plan_device_bytes does not change): the blocks of the
 * selected inverse, sum over the fronts of (min(fp, fm_ub) + fn - fp)^2 doubles, the widest tree level's R11^-1 [I | R12] and two
 * index tables of the size of Rj.  No room for them: STMMQR_ERR_OUT_OF_MEMORY, the plan stays usable.
 * STMMQR_ERR_INVALID (the message says why; the plan stays usable): null plan or nothing factorized, var NULL, ncol out of range, the
 * carried conditions not met for ncol < n, or a plan that does not hold the whole tree (stmmqr_plan_set_groups, imported or shared
 * fronts).
 * Accuracy: the recurrence forms entries of (R'R)^-1, whose condition is cond(A)^2, so an entry carries an error of about
 * u cond(A)^2 times the largest one -- as the normal equations would.  Up to cond(A) ~ 1e7 every variance has digits to spare
 * (measured: DESIGN.md 6h); on lns_3937 (cond ~ 1e11) 45 of 1822 variances are off by more than 1e-3 relative and four are negative.
 * There |stmmqr_plan_rsolve(system 3, e_j)|^2 gives column j to u cond(A), one column at a time.  stmmqr_plan_condest below tells
 * which side of that threshold the held factorization is on.
 * Entries off the diagonal and the leverages of the rows come from the same blocks: stmmqr_plan_covariance_entries and
 * stmmqr_plan_leverage below.  Out of scope: entries outside the pattern of the selected inverse, and a stmmqr_sparseqr_* entry (the
 * singleton block R1 lives on the host and is no part of the plan; the stmmqr_ls object removes no singletons and is the home of
 * this feature). */
int stmmqr_plan_covariance_diag(stmmqr_plan *plan, stm_long ncol, double *var, int on_device);

/* Leverages of a least-squares fit.  With Z = ((A E)_live' (A E)_live)^-1 as above and a_i = row i of the factorized matrix
 * restricted to its first ncol columns (the values of the last factorization), lev[i] = a_i' Z a_i for i < m in the caller's row
 * order: the diagonal of the orthogonal projector onto the span of the live columns (the hat matrix), 0 <= lev[i] <= 1 and
 * sum_i lev[i] = the number of live columns.  Dead columns take no part; an empty row gives 0.
 * The selected inversion of stmmqr_plan_covariance_diag is run once and its blocks are read while they are resident: a row of A makes
 * its columns a clique of A'A, so every Z(j, k) the row needs lies in the block of the front where the earlier of the two columns is
 * pivotal.  No solve with R' is made and there is no limit on the width of a front.  A row costs nnz(row)^2 lookups on one
 * wavefront: a matrix with a dense row of tens of thousands of entries is slow here.
 *   var non-NULL [ncol]: receives exactly what stmmqr_plan_covariance_diag(plan, ncol, var, on_device) writes (the same bits), from the
 *   same inversion.  on_device: lev and var are device pointers.
 * Needs the pattern of A (stmmqr_factorize_device was given Ap / Ai once): otherwise STMMQR_ERR_INVALID, "pattern of A was never
 * given".  lev NULL: STMMQR_ERR_INVALID.  Every other refusal, the messages and the memory behaviour are those of
 * stmmqr_plan_covariance_diag; the call's own tables (S's row pointers and column indices, one int per column) are released before it
 * returns as well.  Accuracy: as the variances, an error of about u cond(A)^2 (measured: DESIGN.md 6i).
 * The same bits from two calls, from plans with and without H, and for host and device output. */
int stmmqr_plan_leverage(stmmqr_plan *plan, stm_long ncol, double *lev /* [m] */, double *var /* [ncol] or NULL */, int on_device);

/* Entries of the inverse: out[p] = Z(I[p], J[p]), p < npairs, with Z as above and the column indices in the caller's column order
 * (0 <= I[p], J[p] < ncol).  I and J are host arrays; on_device: out is a device pointer.
 * A pair is in the pattern of the selected inverse when its columns are equal, or when the later one in R's column order is a column
 * of the front whose pivots hold the earlier one (two columns that share a row of A always are).  This is decided on the host from the
 * symbolic analysis before anything is allocated or launched: the first pair outside the pattern gives STMMQR_ERR_INVALID with a
 * message that names p and the two columns, out is not written and the plan stays usable.
 * An in-pattern pair with a dead column gives exactly 0; (i, j) and (j, i) give the same bits; (j, j) gives the bits of var[j].
 * npairs < 0, or npairs > 0 with out, I or J NULL: STMMQR_ERR_INVALID.  Every other refusal, the messages and the memory behaviour
 * are those of stmmqr_plan_covariance_diag.  The correlation of x_i and x_j is Z(i, j) / sqrt(Z(i, i) Z(j, j)). */
int stmmqr_plan_covariance_entries(stmmqr_plan *plan, stm_long ncol, stm_long npairs, const stm_long *I, const stm_long *J,
                                   double *out /* [npairs] */, int on_device);

/* dense single-front kernels on host buffers (inner seams without the cc argument) */
stm_long stmmqr_front(stm_long m, stm_long n, stm_long npiv, double tol, stm_long ntol, double *F,
                      stm_long *Stair, char *Rdead, double *Tau, double *flops);
int stmmqr_larftb_qtx(stm_long m, stm_long n, stm_long k, stm_long ldc, stm_long ldv, const double *V,
                      const double *Tau, double *C);
/* qr_larftb with a return code, all four methods (0 QR_QTX, 1 QR_QX: C is m x n and V m x k; 2 QR_XQT, 3 QR_XQ: C is m x n
 * and V n x k; SparseQR_factorize.c:1851-1904).  The reference-named export qr_larftb calls this and turns a failure into
 * cc->status < 0 + stmmqr_last_error(), never into a silent return. */
int stmmqr_larftb(int method, stm_long m, stm_long n, stm_long k, stm_long ldc, stm_long ldv, const double *V,
                  const double *Tau, double *C);
/* device time (ms, HIP events) of the kernels of the last qr_front / stmmqr_front / qr_assemble seam call on this
 * thread's device, -1 if none: the seams take host buffers, so their wall time is dominated by the copies; the kernel
 * micro-benchmarks of SURVEY.md 8(d) (bench.py --workload micro) read this instead */
double stmmqr_last_seam_ms(void);

/* ================================================================================================
 * 3. Configuration / introspection
 * ================================================================================================ */
/* Defaults: {32, 64, 0, 0, 0, 1, 0, 1, 0, 1}.  (Two options of round 3 were removed in round 4 with the kernels behind them, both
 * measured slower at every setting: mid_front_cols = whole mid-size fronts in one workgroup, pair_update = 2 = the single-sweep pair
 * update; profiles/EXPERIMENTS.md.)   Read when a plan is created (or a seam is called); the numerical results do not
 * depend on them beyond rounding.
 * Environment (diagnosis, tests and experiments only): every STMMQR_* variable the library reads is one row of the table in
 * csrc/stmmqr_knobs.h, with its default, its reading rule and the moment it is read.  Those a caller may reasonably set:
 * STMMQR_PLAN_CACHE (plans the drop-in seam keeps; 0 turns the cache off) and STMMQR_SEAM_TIMING=1 (section 1); STMMQR_RECYCLE
 * (slab recycling: 0 never, 2 always; unset: by the size of the fronts); STMMQR_EARLY_END=0 (every panel of every front a step of
 * the timeline; default: a front is scheduled up to the panel where the full-rank row estimate says it runs out of rows,
 * DESIGN.md 4); STMMQR_PASSENGERS=0 (passenger launches off); STMMQR_RHS_BATCH (right-hand sides per pass of the resident-factor
 * operations); STMMQR_RESIDENT_CACHE (recycled slabs: every front in front form at once, 1, or level by level, 0); STMMQR_MEMDUMP=1
 * (device memory by purpose); STMMQR_DUMPSTEPS=file (detail runs: one line per step with what ran and how long); STMMQR_DBG (bit
 * mask, csrc/stmmqr_kernels.h; of general use: 16 diagnosis counters printed by stmmqr_factorize_finish -- panels by actual rows,
 * launched / useful update workgroups, refresh rounds --, 16384 no wave-pipelined panels: every short panel through the
 * multi-workgroup pipeline).  For tests of the download under slab recycling: STMMQR_DOWNLOAD_WIN (doubles per window of
 * stmmqr_plan_download, read at every download; default 32 << 20 = 256 MB) and STMMQR_KEEP_FRONTS (0..3: that many of the largest
 * fronts keep their slab, instead of the planner's choice; stmmqr_plan_front_kept tells which).  The Python package adds STMMQR_NATIVE_PHASES=0 and STMMQR_EARLY_END_SHARDED=0 (sharded.py: the
 * Python phase loop; the full schedule on sharded plans). */
typedef struct stmmqr_options {
    int panel_width;        /* Householder panel width on device (<= 32); reference FCHUNK = 32                    */
    int big_front_cols;     /* fronts with fn >= this use the multi-workgroup panel/update path                     */
    int verbose;
    int use_graph;          /* replay the level schedule as a hipGraph (captured per plan and tol); 0: no gain measured */
    int panel_algo;         /* panel of the large fronts: 1 the column pipeline (one workgroup reduction per column),
                               2 the Gram-based panel (one Gram matrix per panel, any height), 0 (default) by the panel's
                               estimated rows: Gram-based above STMMQR_CA_MIN, the column pipeline below -- whose
                               panels of at most 512 actual rows are taken by ONE workgroup, a wave per 4 columns     */
    int split_update;       /* row-parallel (2-launch) trailing update for fronts of >= 3 row slabs (1)             */
    int tall_min_rows;      /* panels with more rows than this run as a pipeline of column groups (plan time; 0)    */
    int lookahead;          /* 2 (default since round 5): one stream, the trailing update beyond the next panel's columns rides
                               on the chain's own launches as extra workgroups (passenger launches); 1: that update, the
                               packing of finished fronts and the assembly of the next ones run on a second stream beside
                               the panel chain; 0: one stream, serial order.  Same bits every way.                     */
    int fused_update;       /* 0 (default): the row-parallel trailing update is two launches (k_upd_w, k_upd_c);
                               1: ONE launch that keeps its tiles of C in registers between V'C and the application
                               (C read once, written once per panel).  Same bits either way; measured 1.1x - 2.5x slower
                               on MI355X (the slab workgroups of a column block idle while one of them adds the partial
                               sums: DESIGN.md 5), kept as an experiment.  ONE exception to "0 = two launches": an offloaded
                               look-ahead step applies T + column block 0 in one fused launch when every workgroup of that launch
                               fits the compute units the side stream leaves alone (counted with the fronts' row BOUNDS) and the
                               panels are expected to reach at most STMMQR_LA_FUSED_ROWS rows (0 turns it off).            */
    int pair_update;        /* fronts of STMMQR_PAIR_MIN rows apply the block reflectors of several consecutive panels in ONE sweep over
                               the columns beyond the next panel (their update is bound by what a sweep moves per MFMA):
                               4 (default): four panels per sweep (k_upd_wq / k_upd_yq / k_upd_cq: 0.75 passes over the trailing
                               matrix per panel; round 4: configs[4] stand-in 4127 -> 3640 ms against pairs);
                               1: two panels per sweep (k_upd_w2 / k_upd_y2 / k_upd_c2: 1.5 passes; the round-2/3 form);
                               0: every front panel by panel (3 passes).  A property of the front (plan time); it changes
                               rounding only.  (A single-sweep form of the pair, 16 instead of 24 bytes per entry and pair, was
                               built in round 3, measured slower at one wave per SIMD and removed in round 4:
                               profiles/EXPERIMENTS.md.)                                                                    */
} stmmqr_options;
void stmmqr_get_options(stmmqr_options *opt);
void stmmqr_set_options(const stmmqr_options *opt);

/* ---- the driver's Matrix Market reader ------------------------------------------------------------
 * SparseCore_read_matrix (STMMQR/src/core/SparseCore_read_write.c:982) as test/qrtest.c:112 calls it (prefer = 1): a
 * coordinate file (real / integer / pattern; general / symmetric / hermitian / skew-symmetric, or without a banner) is
 * returned as an UNSYMMETRIC CSC with both triangles, duplicates summed, columns sorted, explicit zeros kept.
 * Ap (ncol+1), Ai, Ax are malloc'ed: release with stmmqr_free.  Returns 0 or a negative STMMQR_ERR_* code
 * (stmmqr_mm_last_error() has the text); dense ("array") and complex files are refused as the driver refuses them. */
int stmmqr_read_matrix_market(const char *path, stm_long *nrow, stm_long *ncol, stm_long *nnz, stm_long **Ap,
                              stm_long **Ai, double **Ax);
const char *stmmqr_mm_last_error(void);
void stmmqr_free(void *p);

/* ---- own symbolic phase ---------------------------------------------------------------------------
 * stmmqr_analyze replaces qr_analyze (STMMQR/include/SparseQR.h; src/qr/SparseQR_analyze.c:20-700) as SparseQR() calls it
 * (SparseQR.c:338 ordering GIVEN with Q1fill, :360 FIXED on Y): the supernodal analysis of A(:,Q)'A(:,Q) (elimination
 * tree, column counts, relaxed supernodes: SparseChol_analyze_p2 / SparseChol_super_symbolic2), the frontal tree and its
 * weighted post-order, S = A(P,Q) in row form, front sizes, staircases, flop and stack bounds.  A: CSC pattern (m x n,
 * Long indices; values are not needed).  Quser: the fill-reducing column permutation (NULL = natural order).
 * relax: supernode amalgamation knobs (NULL = the library defaults 4/16/48, 0.8/0.1/0.05; stmmqr_relax_for_qr gives what
 * the driver's Relaxfactor_setting(n, nnz, RELAX_FOR_QR) sets, SparseCore_common.c:1172-1203, qrtest.c:153).
 * The result is bit-identical to the reference's qr_symbolic for the same inputs (tests/test_symbolic.py); it says
 * ntasks = ns = 1 (the reference's serial analysis): tree parallelism is this library's scheduler.
 * Host-only: no device is touched. */
typedef struct stmmqr_relax { stm_long nrelax[3]; double zrelax[3]; } stmmqr_relax;
typedef struct stmmqr_analysis stmmqr_analysis;       /* owns every array the qr_symbolic view points to */
void stmmqr_relax_for_qr(stm_long n, stm_long nnz, stmmqr_relax *relax);
int stmmqr_analyze(stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const stm_long *Quser,
                   int do_rank_detection, const stmmqr_relax *relax, stmmqr_analysis **out);
const stm_qr_symbolic *stmmqr_analysis_symbolic(const stmmqr_analysis *a);   /* borrowed, valid until stmmqr_analysis_free */
/* info[0..7] = flop bound (cc->SPQR_flopcount_bound), fl and lnz of the Cholesky analysis, QR_CHUNK_FLAG (fl/lnz >= 1000,
 * SparseChol_analyze.c:727-730), bound on nnz(R), bound on nnz(H) (SPQR_istat[0..1]), maxstack, nf */
int stmmqr_analysis_info(const stmmqr_analysis *a, double *info);
void stmmqr_analysis_free(stmmqr_analysis *a);

/* ---- SURVEY.md 8 (f2 stage 2, f4): SparseQR() without the reference ---------------------------------------------------
 * stmmqr_sparseqr replaces SparseQR (STMMQR/include/SparseQR.h:25-31; src/qr/SparseQR.c:66-450): column singletons
 * (qr_1colamd :515-1128), the fill-reducing ordering (COLAMD: src/base/colamd.c + the column elimination tree's post-order,
 * SparseChol_colamd), R1 / Y (:216-329), the symbolic analysis (stmmqr_analyze) and the numeric factorization on the device.
 * ordering: the reference's QR_ORDERING_* values (SparseQR_definitions.h:6-21): 0 FIXED, 1 NATURAL, 2 COLAMD, 3 GIVEN (Quser,
 * an extension: the reference's SparseQR has no such argument), 7 DEFAULT (= COLAMD as in the stock build); AMD (5), NESDIS (6),
 * METIS (10, 11) and the best-of strategies (4, 8, 9) are third-party packages in the reference and are refused here.
 * tol <= -2 (QR_DEFAULT_TOL): 20 (m + n) eps max_j |A(:,j)|_2 as the reference's qr_tol; -2 < tol < 0: no rank detection.  relax: see stmmqr_analyze.  Bit-identical to the reference's Q1fill / P1inv / R1 / Y / qr_symbolic
 * on the committed fixtures (tests/test_sparseqr_symbolic.py).
 * stmmqr_sparseqr_symbolic is the host half alone (no device), stmmqr_sparseqr_numeric the device half. */
typedef struct stmmqr_qr stmmqr_qr;
int stmmqr_sparseqr(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                    const stm_long *Quser, const stmmqr_relax *relax, int device, stmmqr_qr **out);
int stmmqr_sparseqr_symbolic(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai,
                             const double *Ax, const stm_long *Quser, const stmmqr_relax *relax, stmmqr_qr **out);
int stmmqr_sparseqr_numeric(stmmqr_qr *qr, int device);
/* keep = 0 between stmmqr_sparseqr_symbolic and _numeric: the numeric phase keeps R only (keepH = 0); stmmqr_sparseqr_solve works,
 * stmmqr_sparseqr_qmult returns STMMQR_ERR_INVALID */
int stmmqr_sparseqr_set_keep_h(stmmqr_qr *qr, int keep);
/* least squares by the corrected seminormal equations (stmmqr_plan_solve_seminormal) on a factorized object, with or without H:
 * A (Ap, Ai, Ax) is the caller's full matrix, the one factorized (products with it run on the device); R'\ and R\ are systems 3
 * and 1 of stmmqr_sparseqr_solve.  B m x nrhs, X n x nrhs (host arrays); info (may be NULL) as for the plan */
int stmmqr_sparseqr_solve_seminormal(stmmqr_qr *qr, const stm_long *Ap, const stm_long *Ai, const double *Ax, const double *B, stm_long ldb,
                                     stm_long nrhs, double *X, stm_long ldx, int refine, double *info);
void stmmqr_sparseqr_free(stmmqr_qr *qr);
/* info[0..11] = rank, n1rows, n1cols, nf, analyze seconds (ordering + analysis: Ana_time), factorize seconds (the qr_factorize
 * interval: Fac_time), flops (the reference's count), flop bound, device ms of the factorization, ordering used,
 * QR_CHUNK_FLAG, retries */
int stmmqr_sparseqr_info(const stmmqr_qr *qr, double *info);
double stmmqr_sparseqr_tol(const stmmqr_qr *qr);                                   /* the tolerance really used: qr_tol(A) for QR_DEFAULT_TOL, -1 (EMPTY) for other negative ones (SparseQR.c:126-139) */
const stm_long *stmmqr_sparseqr_q1fill(const stmmqr_qr *qr);                      /* [n] column permutation (singletons first) */
const stm_qr_symbolic *stmmqr_sparseqr_symbolic_view(const stmmqr_qr *qr);       /* qr_symbolic of A or Y */
stmmqr_plan *stmmqr_sparseqr_plan(stmmqr_qr *qr);                                 /* the device plan holding the factors */
int stmmqr_sparseqr_y(const stmmqr_qr *qr, const stm_long **Yp, const stm_long **Yi, const double **Yx);
/* QR_qmult (SparseQR.h:403-409): X nrow x ncol (m x k for methods 0 QR_QTX / 1 QR_QX, k x m for 2 QR_XQT / 3 QR_XQ), result
 * in Y (same shape).  QR_solve (SparseQR.h:411-417): systems 0..3 as in stmmqr_plan_rsolve, singleton rows included. */
int stmmqr_sparseqr_qmult(stmmqr_qr *qr, int method, const double *X, stm_long ldx, stm_long nrow, stm_long ncol, double *Y,
                          stm_long ldy);
int stmmqr_sparseqr_solve(stmmqr_qr *qr, int system, const double *B, stm_long ldb, stm_long nrhs, double *X, stm_long ldx);
/* On the QR object of A' (from stmmqr_sparselq, or stmmqr_sparseqr on the transpose): X (qr->m x nrhs) = the minimum-2-norm solution
 * of A x = b for B (qr->n x nrhs), x = Q (R' \ (E' b)), singleton rows included (host arrays).  The multifrontal part is one
 * stmmqr_plan_solve_minnorm call: no limit on the width of a front.  Needs H. */
int stmmqr_sparseqr_min2norm(stmmqr_qr *qr, const double *B, stm_long ldb, stm_long nrhs, double *X, stm_long ldx);

/* ---- New values of the same pattern (a Newton step, a time step): stmmqr_sparseqr_refactorize ------------------------------------
 * gives a factorized object new values.  Ax has the pattern and the storage order of the matrix the object was made from: A for
 * stmmqr_sparseqr, the caller's A (not A') for an object from stmmqr_sparselq; a host array, or a device pointer with ax_on_device.
 * Kept: column order and singleton set, R1's and Y's patterns, the analysis, the plan with its arenas (nothing is analysed, planned
 * or allocated again, and also objects with keepH = 0 take new values).  Made again, so that every stmmqr_sparseqr_* call afterwards
 * acts on the new factorization: the tolerance by the rule of the object's tol argument (tol <= -2: 20 (m + n) eps max_j |A(:,j)|_2
 * of the NEW values, bit for bit what a new object computes; tol >= 0 stays; -2 < tol < 0 stays "none"), R1x, the Yx of
 * stmmqr_sparseqr_y, the factors on the device, Rdead, rank, HP1inv, and of stmmqr_sparseqr_info the factorize seconds, flops,
 * device ms and retries (the analyze seconds stay).
 * Singletons depend on values.  The first values fixed the structure; new ones keep it valid as long as the pivot of every live
 * singleton still exceeds the new tolerance (|a| > tol, the test of creation; dead singletons have no pivot).  That is checked on
 * the device before anything of the old factorization is touched.  If it fails: STMMQR_ERR_STALE, the message names the first
 * failing singleton in singleton order, its column, the value and the tolerance, and the object is unchanged -- it still answers
 * with its earlier factorization; the caller makes a new object.  With tol = -1 the test always holds, as at creation.  Columns
 * that were no singletons under the first values but would be under the new ones are NOT looked for: the result is a correct QR
 * factorization all the same, only not the structure a new object would choose.
 * STMMQR_ERR_INVALID (the message says why, the object is unchanged): null object, null Ax with a non-empty pattern, no numeric
 * phase yet, a pattern of 2^31 or more entries (the maps below are int tables).  If the factorization itself fails after the values
 * were accepted (device error, out of memory), the old factors are gone: the object holds no valid factorization, and qmult, solve,
 * min2norm, solve_seminormal and stmmqr_plan_export_r through it refuse with a message that says so until a refactorization
 * succeeds.
 * Device work besides the factorization (stmmqr_refactor.hip): the column norms of the default tolerance (a lane per column in
 * storage order -- the host rule's operations in the host rule's order; slow on a dense column of tens of thousands of entries,
 * accepted for the equal bits), the split of the values into R1x and Yx, the singleton check; then ONE device-to-host copy of
 * {norm, first stale singleton, R1x, Yx}, the only host wait before the factorization.  An object without singletons that is no LQ
 * object factorizes straight from the caller's device pointer (a host array is uploaded once).
 * Measured on an MI355X (tools/time_refactor.py), wall ms of the call against the analyze + factorize seconds of a new
 * object on the same values: bcsstk14 8.5 against 3.9 + 8.9, bayer10 (1190 singleton columns) 8.0 against 8.4 + 16.2, ex18 6.1
 * against 5.7 + 6.7, the xenon1 stand-in (no singletons) 86.9 against 270.8 + 94.0; a device pointer saves up to 0.3 ms more; the
 * value kernels take 20 -- 40 us.
 *   stmmqr_sparseqr_refactor_info  info[0..7] = tolerance of the last refactorization, device ms of the value kernels, device ms of
 *                                  the factorization, wall seconds of the call, refactorizations done, stale refusals, analyses +
 *                                  plans the object has made since its creation (stays 2), device bytes it holds beyond its plan.
 *   stmmqr_sparseqr_refactor_maps  where the values go (no device needed; works on a symbolic-only object): counts[0..3] = entries of
 *                                  the caller's matrix, nnz(Y), nnz(R1), n1rows; ysrc[t] = the caller's storage position of entry t
 *                                  of Y, r1src[q] the same for R1's row form, pivsrc[k] the position of the pivot of live singleton
 *                                  row k.  The pointers are NULL when the object has no singletons and is no LQ object (Y is then A
 *                                  itself); without singletons an LQ object has ysrc (the transposition) and NULL for the others.
 *                                  Any argument but qr may be NULL. */
int stmmqr_sparseqr_refactorize(stmmqr_qr *qr, const double *Ax, int ax_on_device);
int stmmqr_sparseqr_refactor_info(const stmmqr_qr *qr, double *info /* [8] */);
int stmmqr_sparseqr_refactor_maps(const stmmqr_qr *qr, stm_long *counts /* [4] */, const int **ysrc, const int **r1src, const int **pivsrc);

/* ---- R / H out in sparse form, LQ (STMMQR/src/qr/SparseLQ.c; prototypes SparseQR.h:282-340) ---------
 * qr_rcount / qr_rconvert / qr_trapezoidal keep the reference's names, argument lists and results (bit for bit: they move
 * data).  They read a qr_numeric on the host -- the one qr_factorize returned.  stmmqr_plan_export_r does the same for the
 * factorization a plan holds in HBM (one download): R as compressed sparse columns over the columns of the factorized matrix,
 * optionally H (one column per live reflector, unit diagonal stored, rows = the permuted row ids) and its Tau; every output
 * array is malloc'ed (stmmqr_free).  stmmqr_sparselq = SparseLQ: the QR object of A' (L = R'); device -2: its host half only (no
 * device is touched; the object answers stmmqr_sparseqr_refactor_maps and the symbolic getters and never gets a numeric phase). */
void qr_rcount(stm_qr_symbolic *QRsym, stm_qr_numeric *QRnum, stm_long n1rows, stm_long econ, stm_long n2, int getT, stm_long *Ra,
               stm_long *Rb, stm_long *H2p, stm_long *p_nh);
void qr_rconvert(stm_qr_symbolic *QRsym, stm_qr_numeric *QRnum, stm_long n1rows, stm_long econ, stm_long n2, int getT,
                 stm_long *Rap, stm_long *Rai, double *Rax, stm_long *Rbp, stm_long *Rbi, double *Rbx, stm_long *H2p, stm_long *H2i,
                 double *H2x, double *H2Tau);
stm_long qr_trapezoidal(stm_long n, stm_long *Rp, stm_long *Ri, double *Rx, stm_long bncols, stm_long *Qfill,
                        int skip_if_trapezoidal, stm_long **p_Tp, stm_long **p_Ti, double **p_Tx, stm_long **p_Qtrap,
                        stm_sparse_common *cc);
int stmmqr_plan_export_r(stmmqr_plan *plan, const stm_qr_symbolic *sym, stm_long econ, stm_long **Rp, stm_long **Ri, double **Rx,
                         stm_long *nh, stm_long **Hp, stm_long **Hi, double **Hx, double **HTau);

/* R of the held factorization as a sparse matrix, made ON THE DEVICE from the resident factors: nothing is downloaded but the entries
 * kept, and with on_device nothing at all.  The matrix is the m x ncol one stmmqr_plan_export_r defines: rows numbered front by front
 * over the live pivots, columns those of the factorized matrix in its own order (the caller applies Qfill); an entry is kept if
 * row < econ, column < ncol and value != 0.0 (exact zeros are dropped, -0.0 included); dead pivot columns keep the rows above them.
 * ncol = n: all of R; ncol < n: its leading columns -- R of A for the plan of [A B] of the least-squares object (it only filters: no
 * carried-view condition).  Both forms describe the same matrix; in compressed rows, rows >= min(econ, rows of R) are empty.
 * Two calls: idx == NULL and val == NULL counts -- ptr and info are written; with both and cap >= nnz it fills.  cap < nnz:
 * STMMQR_ERR_INVALID naming nnz and cap, ptr and info written, idx / val untouched, the plan stays usable.  A fill call does not
 * depend on an earlier count call (it counts again).  on_device: ptr, idx and val are device pointers; else host arrays, and nnz
 * entries cross the bus.  info is always a host array: info[0] = nnz, info[1] = the stored entries visited before the zero test (rows
 * < econ, columns < ncol), info[2] = the rows of R, info[3] = 0.  Complete on return (the plan's stream is synchronised).
 * Deterministic: positions come from scans and from ranks within a wave's ballot, no atomics -- the same bits run after run, and the
 * bits of stmmqr_plan_export_r.  ptr and every offset are 64-bit.
 * Reads R only: plans with and without H.  H, HTau and HPinv come out the same way through stmmqr_plan_h_sparse below.
 * Memory, made at the first call of a form and kept with the plan (a plan that never calls this allocates nothing for it): compressed
 * columns 16 bytes per entry of Rj (two int counts and a 64-bit offset per slot) and the transpose of Rj (4 bytes per entry + 4 per
 * column, shared with stmmqr_plan_rmult's trans = 1); compressed rows 8 bytes per row of the matrix.  With host arrays the device
 * images of ptr, idx and val (16 bytes per entry kept) live for the length of the call.  With the level-wise scratch
 * (STMMQR_RESIDENT_CACHE=0) the count walk and the fill walk each put the levels back into front form.
 * Refusals (STMMQR_ERR_INVALID, the message says why, the plan stays usable): null plan or nothing factorized, form not 0 or 1, ncol
 * outside [0, n], econ < 0, cap < 0, ptr or info NULL, exactly one of idx / val NULL, a plan that does not hold the whole tree. */
#define STMMQR_RSPARSE_CSC 0   /* ptr[ncol + 1], idx = row of R,    rows ascending within a column            */
#define STMMQR_RSPARSE_CSR 1   /* ptr[m + 1],    idx = column of R, front order (k = 0 .. fn-1) within a row */
int stmmqr_plan_r_sparse(stmmqr_plan *plan, int form, stm_long ncol, stm_long econ, stm_long *ptr, stm_long *idx, double *val, stm_long cap,
                         stm_long *info /* [4], always a host array */, int on_device);
/* the HIP device the plan lives on -- where a caller allocates what it hands over with on_device; -1 for a null plan */
int stmmqr_plan_device_index(const stmmqr_plan *plan);

/* H of the held factorization -- the Householder vectors as compressed sparse columns, their Tau and the row permutation HPinv --
 * made ON THE DEVICE from the resident factors (keepH = 1): nothing is downloaded but the entries kept, and with on_device nothing at
 * all.  The matrix is the m x nh one stmmqr_plan_export_r returns as nh, Hp, Hi, Hx, HTau (walk_packed with n1rows = 0): the slots
 * (front ascending, k = 0 .. fn - 1) are walked; a pivotal slot has t = Stair[k], a dead one (t == 0) t = rm, a live one rm++ (at most
 * fm), both h = rm; a non-pivotal slot h = min(h + 1, fm); the slot is a column of H iff t >= h and Tau[k] != 0.0.  A column holds the
 * unit diagonal (row id of front row h - 1, 1.0) and then, for the front rows i = h .. t - 1 in that order, the entries of front column
 * k with value != 0.0 (exact zeros are dropped, -0.0 included).  Row ids are the permuted ones stmmqr_plan_download gives (Hii after
 * qr_hpinv); the rows of a column are in front-row order, NOT ascending.  HTau[q] = Tau of the q-th column.  HPinv[i] = the position
 * of row i of the factorized matrix in that permuted order: scatter w[HPinv[i]] = x[i], apply H_0 .. H_{nh-1} in order, and w is Q'x in
 * the row order stmmqr_plan_qmult method 0 returns.  No econ: it does not apply to H (nor does the host export apply it).
 * Two calls: Hp == Hi == Hx == HTau == NULL counts -- only info is written, and HPinv if given; with all four, colcap >= nh and cap >=
 * hnz it fills: Hp gets nh + 1 entries, Hi / Hx hnz, HTau nh.  A fill call does not depend on an earlier count call (it counts again).
 * colcap < nh or cap < hnz: STMMQR_ERR_INVALID naming both numbers, info written, every array untouched, the plan stays usable.
 * HPinv ([m]) is optional in either call.  on_device: Hp, Hi, Hx, HTau and HPinv are device pointers on stmmqr_plan_device_index(plan);
 * else host arrays, whose device images live for the length of the call (16 bytes per entry kept, 16 per column, 8 per row), and only
 * the entries kept cross the bus.  info is always a host array: info[0] = nh, info[1] = hnz, info[2] = the entries visited before the
 * zero test (unit diagonals included), info[3] = m.  Complete on return (the plan's stream is synchronised).
 * Deterministic: positions come from scans and from ranks within a wave's ballot, no atomics -- the same bits run after run, and the
 * bits of stmmqr_plan_export_r.  Every offset is 64-bit; the counts of one slot are int.
 * Memory, made at the first call and kept with the plan (a plan that never calls this allocates nothing for it): 20 bytes per entry
 * of Rj (two int counts, an int column number and a 64-bit offset per slot).  With the level-wise scratch (STMMQR_RESIDENT_CACHE=0) the
 * count walk and the fill walk each put the levels back into front form.
 * Refusals (STMMQR_ERR_INVALID, the message says why, nothing is written, the plan stays usable): null plan or nothing factorized, a
 * plan that keeps no Householder vectors (keepH = 0), info NULL, some but not all of Hp / Hi / Hx / HTau NULL, colcap < 0 or cap < 0,
 * a plan that does not hold the whole tree.  Out of scope: compressed rows of H, the singleton rows of the SparseQR object. */
int stmmqr_plan_h_sparse(stmmqr_plan *plan, stm_long *Hp, stm_long *Hi, double *Hx, double *HTau, stm_long *HPinv, stm_long colcap,
                         stm_long cap, stm_long *info /* [4], always a host array */, int on_device);
int stmmqr_sparselq(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                    const stmmqr_relax *relax, int device, stmmqr_qr **out);

/* ---- The least-squares object: min |A x - b_j|_2 for nrhs right-hand sides, Q never stored -----------------------------------------
 * stmmqr_ls_create, once per pattern and nrhs (1 <= nrhs <= STMMQR_LS_MAX_NRHS, else STMMQR_ERR_INVALID naming the limit): the
 * columns of A alone are ordered as stmmqr_sparseqr orders them (same `ordering` values, same refusals; Quser with ordering 3 must be
 * a permutation of 0 .. n-1), the B columns follow unpermuted, stmmqr_analyze runs on the pattern [A | nrhs dense columns] and an R-only
 * plan is created (device -2: the host half only, no device is touched).  Column singletons are NOT removed in this mode: they come
 * first in the column order and stay in the matrix (their rows must reach B).  The analysis holds m * nrhs more indices than A's.
 * stmmqr_ls_solve, any number of times: puts [Ax | B] together on the device (Ax NULL: the values given at create; ax_on_device: Ax is a
 * device pointer; on_device: B, X and resid are device pointers), factorizes with ntol = n and calls stmmqr_plan_solve_carried.  Nothing
 * is analysed or planned again.  tol follows stmmqr_sparseqr's rule on the columns of A only (tol <= -2: 20 (m + n) eps max_j |A(:,j)|_2,
 * recomputed whenever values are given -- device values are copied back once for it; -2 < tol < 0: no rank detection).
 * B m x nrhs (ldb >= m), X n x nrhs (ldx >= n), resid [nrhs] or NULL.
 * info[0..13] = rank of A (rank1), nf, flops, flop bound, device ms of the factorization, device ms of the back substitution (transfer of
 * X included), device bytes (plan + values), retries, reschedules, analyses made, plans made, solves, tol used, nrhs. */
#define STMMQR_LS_MAX_NRHS 64
typedef struct stmmqr_ls stmmqr_ls;
int stmmqr_ls_create(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                     stm_long nrhs, const stm_long *Quser, const stmmqr_relax *relax, int device, stmmqr_ls **out);
int stmmqr_ls_solve(stmmqr_ls *ls, const double *Ax, int ax_on_device, const double *B, stm_long ldb, double *X, stm_long ldx,
                    double *resid, int on_device);
const stm_qr_symbolic *stmmqr_ls_symbolic_view(const stmmqr_ls *ls);
stmmqr_plan *stmmqr_ls_plan(stmmqr_ls *ls);
int stmmqr_ls_info(const stmmqr_ls *ls, double *info);
int stmmqr_ls_resid(const stmmqr_ls *ls, double *resid);   /* [nrhs] host array: the residual norms of the last solve */
int stmmqr_ls_covariance_diag(stmmqr_ls *ls, double *var, int on_device);   /* after a solve: stmmqr_plan_covariance_diag with ncol = n of A */
/* after a solve: stmmqr_plan_leverage / stmmqr_plan_covariance_entries with ncol = n of A (lev [m], var [n] or NULL; column indices of A).
 * They refuse as stmmqr_ls_covariance_diag does: null object, the host half only, no solve yet. */
int stmmqr_ls_leverage(stmmqr_ls *ls, double *lev, double *var, int on_device);
int stmmqr_ls_covariance_entries(stmmqr_ls *ls, stm_long npairs, const stm_long *I, const stm_long *J, double *out, int on_device);
/* after a solve: stmmqr_plan_condest with ncol = n of A -- the condition of A(:, live), which says how far the solution, the variances
 * and the leverages above can be trusted (out [8], v [n] or NULL).  Refuses as stmmqr_ls_covariance_diag does. */
int stmmqr_ls_condest(stmmqr_ls *ls, int kind, int iters, double *out, double *v, int on_device);
/* after a solve: stmmqr_plan_nullspace / stmmqr_plan_project_minnorm with ncol = n of A, in A's column order: the null vectors of A
 * as the rank test saw it, and the minimum-norm solution from the basic one that stmmqr_ls_solve returns (X n x nrhs, in place; the
 * residuals do not change).  They refuse as stmmqr_ls_covariance_diag does. */
int stmmqr_ls_nullspace(stmmqr_ls *ls, stm_long *ndead, double *N, stm_long ldn, int on_device);
int stmmqr_ls_project_minnorm(stmmqr_ls *ls, double *X, stm_long ldx, stm_long nrhs, int on_device, double *info);
void stmmqr_ls_free(stmmqr_ls *ls);
int stmmqr_ls_dims(const stmmqr_ls *ls, stm_long *dims /* [4]: m, n of A, nrhs, damped (0 / 1) */);   /* either kind of object */

/* ---- The damped mode of the least-squares object: min_x |W (A x - b_j)|^2 + |D x|^2, W = diag(w), D = diag(D_jj) >= 0 -------------------
 * (Levenberg-Marquardt and trust-region steps, ridge regression, regularization paths, iteratively reweighted fits: w and D change
 * from solve to solve, the pattern does not.)  The object is the plain object of the (m + n) x n matrix [W A; D] with the right-hand
 * sides [W B; 0]: the same bits as stmmqr_ls_create / stmmqr_ls_solve on that matrix in the same column order.
 * stmmqr_ls_create_damped, once per pattern and nrhs: the columns of A ALONE are ordered exactly as stmmqr_ls_create orders them (the
 * same orderings, refusals and Quser rule; Qfill[0 .. n-1] equals the plain object's for the same arguments), then stmmqr_analyze runs
 * on the pattern of the (m + n) x (n + nrhs) matrix [A; I | dense columns]: column j holds A's entries in their given order and then
 * the entry of row m + j; the nrhs trailing columns are dense over all m + n rows (the zero block below B is stored: n * nrhs
 * doubles).  Otherwise as stmmqr_ls_create: no singleton removal, an R-only plan, device -2 = the host half only, STMMQR_LS_MAX_NRHS.
 * With a device the object also keeps there: A's values as given here (anz doubles), A's row indices and column pointers as int
 * (anz + n + 1; a pattern of 2^31 or more entries or columns is refused), D (n doubles) and, for tol <= -2, the n + 1 64-bit column
 * pointers of [A; I].  On failure *out is NULL.
 * stmmqr_ls_solve_damped, any number of times: builds the values of [W A; D | W B; 0] on the device -- entry p of A (row i) becomes
 * w[i] * Ax[p], ONE multiplication --, factorizes with ntol = n and calls stmmqr_plan_solve_carried.  Nothing is analysed or planned
 * again and no solve leaves state for the next: the values are built anew every time from A's unweighted values.
 *   Ax           NULL: the values given at create; else anz values, a device pointer with ax_on_device
 *   on_device    B, X, resid and dmp->w, d, D_out, dnorm are device pointers (all of them, or none); dmp itself is a host struct
 *   B m x nrhs (ldb >= m), X n x nrhs (ldx >= n), resid [nrhs] or NULL: resid[j] = sqrt(|W (b_j - A x_j)|^2 + |D x_j|^2), the carried
 *   residual of the augmented problem.  With dnorm[j] = |D x_j|_2 and |W b_j| a caller has the predicted reduction of a step.
 *   D_jj = sqrt(lambda) * s_j.  s_j = d[j]; or, d NULL, 1 (scale 0) or |W A(:,j)|_2 clamped to [scale_min, scale_max] (scale 1; a zero
 *   column gets scale_min).  D_out [n], A's column order.
 *   tol <= -2 at create: 20 ((m + n) + n) eps max_j |[W A; D](:,j)|_2, the rule of stmmqr_ls_create on the augmented matrix, evaluated on
 *   the device from the built values; its 8-byte copy back is the only host wait before the factorization (none for a given tol).
 * Refusals of the solve (STMMQR_ERR_INVALID, the message names the cause, nothing was touched, the object stays usable): a plain object
 * (and stmmqr_ls_solve refuses a damped one), dmp NULL, lambda negative or not finite, scale not 0 or 1, scale 1 with scale_min not
 * in (0, scale_max], the host half only, B or X NULL or ldb < m or ldx < n.  NaN or Inf in w, d or Ax is not searched for: it ends as
 * in the plain object.  (With scale 1 D_out does not show it: a NaN column norm is clamped like any other and comes out as scale_min,
 * while the NaN stays in the built values and reaches the factorization.)  A solve that fails in the factorization leaves the object usable for the next solve.
 * The other entry points on a damped object, after a solve: stmmqr_ls_covariance_diag gives diag((A'W^2 A + D^2)^-1) [n];
 * stmmqr_ls_leverage writes m + n values (lev [m + n]): the first m are the diagonal of the ridge hat matrix W A (A'W^2 A + D^2)^-1 A'W,
 * whose sum is the effective degrees of freedom, and all m + n sum to the number of live columns; stmmqr_ls_condest gives the
 * condition of [W A; D]; stmmqr_ls_covariance_entries, _nullspace, _project_minnorm and the plan's R export work unchanged;
 * stmmqr_ls_info keeps its 14 fields (device bytes include what the damped mode holds).
 * stmmqr_ls_damped_info: info[0] = device ms of building the values in the last solve (the tolerance's norm included), info[1] = device
 * bytes the object holds beyond the plain object of [A; I]. */
typedef struct {
    const double *w;        /* [m] row weights, NULL: all 1                                   */
    const double *d;        /* [n] column scales s_j, NULL: chosen by `scale`                  */
    double lambda;          /* D_jj = sqrt(lambda) * s_j ; lambda >= 0 and finite              */
    int scale;              /* d == NULL: 0 -> s_j = 1 (Levenberg, ridge);
                                          1 -> s_j = |W A(:,j)|_2 clamped to [scale_min, scale_max] (Marquardt) */
    double scale_min, scale_max;
    double *D_out;          /* [n] or NULL: receives the D_jj used, in A's column order        */
    double *dnorm;          /* [nrhs] or NULL: |D x_j|_2                                       */
} stmmqr_ls_damping;
int stmmqr_ls_create_damped(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                            stm_long nrhs, const stm_long *Quser, const stmmqr_relax *relax, int device, stmmqr_ls **out);
int stmmqr_ls_solve_damped(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_damping *dmp, const double *B,
                           stm_long ldb, double *X, stm_long ldx, double *resid, int on_device);
int stmmqr_ls_damped_info(const stmmqr_ls *ls, double *info /* [2] */);

/* ---- The adjoint of the least-squares solve: the backward pass of x = argmin |C x - Bt| -----------------------------------------------
 * (bilevel problems, learned weights and dampings, differentiable nonlinear least squares, the sensitivity of a fit to its data.)
 * C = [W A; D] and Bt = [W B; 0] for a damped object, C = A and Bt = B for a plain one: the matrix whose values the LAST solve on the
 * object factorized.  Given that solve's X (n x nrhs) and a cotangent Xbar = dL/dX (n x nrhs), with sums over the right-hand sides k:
 *   z = (C'C)^-1 xbar = E R^-1 R^-T E' xbar over the live columns,   rt = Bt - C x,   ut = C z,
 *   g(i, j) = sum_k rt[i,k] z[j,k] - ut[i,k] x[j,k]  for every stored entry (i, j) of C, the entries of D included,
 *   Axbar[p] = w_i g(i, j) for entry p = (i, j) of A's storage (plain object, or w NULL: g),   Bbar = w o ut[0:m]  (m x nrhs),
 *   wbar_i = 2 sum_k rt[i,k] ut[i,k] / w_i, and exactly 0.0 where w_i == 0 (the true value there is 2 w_i r_i (A z)_i = 0),
 *   Dbar_j = g(m + j, j) = -2 D_jj sum_k x[j,k] z[j,k]: the gradient for the D_jj that the solve used.
 * From Dbar a caller has dbar_j = sqrt(lambda) Dbar_j and lambdabar = -sum_j s_j^2 sum_k x[j,k] z[j,k] = sum_j s_j Dbar_j / (2 sqrt(lambda));
 * the first form is finite at lambda = 0.
 * Rank-deficient factors: the adjoint is that of the basic solution with the dead set held fixed, argmin |C(:, live) y - Bt|.  z is
 * zero on dead columns (as R \ and the squeezed R' pass give it) and so is x: every gradient entry in a dead column is exactly 0.0.
 * Accuracy: R^-1 R^-T squares the condition number, as in stmmqr_plan_solve_seminormal; `refine` has that call's meaning: refine times
 * z += E R^-1 R^-T E' (xbar - C'(C z)), default 1.
 * The call reads the factors and the values of the last solve.  It factorizes, analyses and plans nothing; the R' pass takes fronts of
 * any width, so the call never returns STMMQR_ERR_TOO_LARGE for one; right-hand sides go in batches of STMMQR_RHS_BATCH.  Nothing in
 * the library checks that X and w are those of the last solve: a caller who passes others gets the adjoint of nothing.  With
 * scale = 1 in that solve the column scales depended on W A; Dbar is still the gradient for the D_jj used, and the gradients of Ax and
 * w then lack the part that goes through the scales.
 * Any output may be NULL and is then neither computed nor written.  on_device: X, Xbar, w and all outputs are device pointers (all of
 * them, or none).  ldx, ldxb >= n, ldbb >= m.  The first call on a plain object uploads A's column pointers and row indices as int
 * (anz + n + 1; counted in stmmqr_ls_info's device bytes, like every work buffer of this call).
 * info [8] or NULL (a host array): [0] live columns among the first n, [1] refinement steps made, [2] the largest
 * |xbar_k - C'C z_k| / |xbar_k| (0 where xbar_k = 0), [3] device ms of the call, [4] device ms of the two triangular passes alone,
 * [5] device bytes the call added to the object, [6..7] 0.
 * Refusals (STMMQR_ERR_INVALID, the message names the cause, nothing is written, the object stays usable): a null object, the host half
 * only, no solve yet, a failed last solve, X or Xbar NULL or ldx < n or ldxb < n, Bbar given with ldbb < m, refine < 0, w, wbar or
 * Dbar non-NULL on a plain object, a plan that does not hold the whole tree. */
int stmmqr_ls_adjoint(stmmqr_ls *ls, const double *X, stm_long ldx, const double *Xbar, stm_long ldxb, const double *w, int refine,
                      double *Axbar /* [anz] */, double *Bbar, stm_long ldbb /* m x nrhs */, double *wbar /* [m] */, double *Dbar /* [n] */,
                      int on_device, double *info /* [8] or NULL */);
/* the z = (C'C)^-1 xbar (n x nrhs, ldz >= n; zero on dead columns) of the last stmmqr_ls_adjoint call that succeeded, which the object
 * keeps: with it lambdabar = -sum_j s_j^2 sum_k x[j,k] z[j,k] needs no division by sqrt(lambda).  Refuses (STMMQR_ERR_INVALID) before such
 * a call, and Z NULL or ldz < n. */
int stmmqr_ls_adjoint_z(stmmqr_ls *ls, double *Z, stm_long ldz, int on_device);

/* ---- Robust least squares: iteratively reweighted solves with row multipliers made from the residual on the device ----------------------
 * (outliers in bundle adjustment, pose graphs, geodesy, regression.)  min_x sum_i rho(|w0_i r_i| / sigma) with r = b - A x, as the fixed
 * point of weighted solves: from x, the UNWEIGHTED residual r (A's values as given -- the damped object's unweighted copy, the values of
 * create, or the Ax of the call; never the weighted values a solve built), a_i = |w0_i r_i| (one product), the scale
 * sigma = max(mad_factor * median(a_i : w0_i != 0), sigma_min) or a given one, u_i = a_i / sigma, and the row multiplier
 * w_i = w0_i f(u_i) with f = sqrt(psi(u) / u) (the object's w multiplies the residual).  loss, f(u), rho(u), default cc:
 *   0 L2       1                              u^2 / 2                                              --
 *   1 Huber    u <= cc ? 1 : sqrt(cc / u)     u <= cc ? u^2 / 2 : cc (u - cc / 2)                  1.345
 *   2 Cauchy   1 / sqrt(1 + (u/cc)^2)         (cc^2 / 2) log(1 + (u/cc)^2)                         2.3849
 *   3 Tukey    u < cc ? 1 - (u/cc)^2 : 0      u < cc ? (cc^2 / 6)(1 - (1 - (u/cc)^2)^3) : cc^2 / 6 4.6851
 *   4 L1       1 / sqrt(max(u, cc))           u >= cc ? u : u^2 / (2 cc) + cc / 2                  none (smoothed below cc: cc > 0 required)
 * The median is exact: the two middle order statistics lo = a_(floor((c-1)/2)) and hi = a_(floor(c/2)) of the c rows with w0_i != 0 by a
 * radix select on the device, 0.5 * (lo + hi).  sigma == 0 after the floor (an exact fit): w = w0, loss = 0, flag 1; no division by zero
 * is formed.  The sum of rho runs over all m rows in a fixed order: the same bits run after run.  NaN in the data is not searched for.
 * The first call on an object builds the row form of A on the host (m + 1 + 2 anz ints) and uploads it with the work vectors; all of it
 * is counted in stmmqr_ls_info's device bytes (and reported in info[7] below).
 * stmmqr_median_abs needs no object: the median of |v_i| (mask NULL) or of |mask_i * v_i| over the entries with mask_i != 0;
 * out[0] = 0.5 * (lo + hi), out[1] = lo, out[2] = hi, out[3] = the count; count == 0: out[0..2] = 0.  on_device: v, mask and out are
 * device pointers.
 * stmmqr_ls_robust_weights: one reweighting from a given X [n] on either kind of object (nrhs of the object must be 1): r_out [m] and
 * w_out [m], either may be NULL.  Ax NULL: the values given at create; ax_on_device as in the solves; on_device: B, X, rb->w0, r_out, w_out
 * are device pointers (all of them, or none).  stat [8], a host array or NULL: sigma, lo, hi, count (lo, hi, count 0 with a given sigma),
 * the sum of rho, rows rejected (w_i == 0 although w0_i != 0), rows with f == 1, flags (1: sigma was 0).
 * stmmqr_ls_solve_robust, the loop: x0 NULL: the first solve uses w0 alone (the L2 start); else the first weights come from x0.  Every
 * further solve is preceded by a reweighting from the last x.  It stops after the first solve whose step satisfies
 * max_j |x_j - xprev_j| <= rtol * max_j |x_j| (the first solve without x0 has no step), or at max_iter solves.  sigma_iters >= 0 (with
 * rb->sigma == 0): the scale is estimated in the first max(sigma_iters, 1) reweightings and frozen afterwards; < 0: every time.
 * A damped object takes its damping in dmp (dmp->w must be NULL: prior weights go in rb->w0; d, D_out, dnorm host or device with
 * on_device) and every solve is stmmqr_ls_solve_damped with the device w; a plain object takes dmp NULL, and every solve is
 * stmmqr_ls_solve of the values w[Ai[p]] * Ax[p] and the right-hand side w o b, one multiplication each -- afterwards the object's
 * values are weighted ones, and a later stmmqr_ls_solve with Ax NULL uploads the values of create again.  With host arrays the inputs
 * go up once and the outputs come down once; between two solves only the eight statistics and the two maxima of the step reach the host.
 * X [n], w_out [m] or NULL: the multipliers of the LAST solve, resid [1] or NULL: that solve's residual norm.  hist [4 * max_iter] or
 * NULL, a host array, per solve: sigma and sum of rho of the reweighting that made its weights (0, 0 for a first solve from w0 alone),
 * the step max |x - xprev| (infinity where there is none), the solve's residual norm.  info [8] or NULL, a host array: solves made,
 * converged (0 / 1), the last step over max |x|, sigma, sum of rho and rows rejected of the last reweighting, device ms of the
 * reweightings alone, device bytes this feature holds.
 * After the call the factors are those of the last solve: stmmqr_ls_covariance_diag, _leverage, _condest and the R export work
 * unchanged, on W A (or [W A; D]) with the final weights, and on a damped object stmmqr_ls_adjoint works with w = w_out -- the adjoint
 * with the weights HELD FIXED, not the derivative through the fixed point.
 * Refusals (STMMQR_ERR_INVALID, the message names the cause, nothing is written, the object stays usable; all decided before any device
 * work): a null object, an object created with nrhs != 1, rb NULL, loss outside 0 .. 4, sigma, sigma_min, cc or mad_factor not finite,
 * sigma < 0 or sigma_min < 0, L1 with cc <= 0, max_iter < 1, rtol negative or NaN, dmp given on a plain object or missing on a damped
 * one, dmp->w non-NULL (and what stmmqr_ls_solve_damped refuses of dmp), B or X NULL, the host half only.  A solve that fails inside
 * the loop returns its code and leaves the object usable.
 * stmmqr_ls_robust_times: ms [4] = device ms of the last reweighting's residual (with |w0 o r|), selection, weights, and their sum. */
int stmmqr_median_abs(const double *v, const double *mask, stm_long len, int device, int on_device, double *out /* [4] */);
typedef struct {
    int loss;              /* 0 .. 4 above */
    double cc;             /* tuning constant; <= 0: the default of the loss (L1 has none: refused) */
    double sigma;          /* > 0: fixed scale; 0: sigma = mad_factor * median |w0_i r_i| over w0_i != 0 */
    double mad_factor;     /* <= 0: 1.4826 */
    double sigma_min;      /* >= 0: floor of the scale */
    const double *w0;      /* [m] prior row multipliers (inverse standard deviations), NULL: all 1 */
} stmmqr_ls_robust;
int stmmqr_ls_robust_weights(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_robust *rb, const double *B,
                             const double *X, double *r_out, double *w_out, int on_device, double *stat /* [8] */);
int stmmqr_ls_solve_robust(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_robust *rb, const stmmqr_ls_damping *dmp,
                           const double *B, const double *x0, int max_iter, double rtol, int sigma_iters,
                           double *X, double *w_out, double *resid, int on_device, double *hist, double *info);
int stmmqr_ls_robust_times(const stmmqr_ls *ls, double *ms /* [4] */);

void stmmqr_shutdown(void);                           /* optional end-of-use call for dlopen()ing hosts: device sync  */
/* Device buffers for hosts without HIP bindings of their own (FFI callers of stmmqr_export_front_dev /
 * stmmqr_import_front_dev, device-resident A values): allocated by the HIP runtime THIS library is bound to, on the
 * current device.  0 or a negative STMMQR_ERR_* code. */
int stmmqr_device_alloc(size_t bytes, void **ptr);
int stmmqr_device_free(void *ptr);
int stmmqr_device_count(void);                        /* number of visible HIP devices (0 = none)          */
const char *stmmqr_device_name(int device);           /* gcnArchName, e.g. "gfx950:sramecc+:xnack-"        */
const char *stmmqr_last_error(void);                  /* thread-local message of the last failure          */
const char *stmmqr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* STMMQR_HIP_H */
