// stmmqr_host.cpp -- host side of libstmmqr_hip.so: device set-up, the symbolic plan (build_plan), the C ABI of the
// factorization and the download.  The schedule of a plan is built in stmmqr_schedule.cpp and run by stmmqr_run.cpp; the
// environment knobs are the table of stmmqr_knobs.h.
//
// Reference counterparts (paths relative to /root/reference/STMMQR):
//   stmmqr_plan_create      the allocation / setup half of qr_factorize   src/qr/SparseQR_factorize.c:222-498
//   stmmqr_plan_download    the wrap-up half of qr_factorize (:554-742) incl. qr_hpinv (:991-1060)
//   qr_factorize            the drop-in seam                                include/SparseQR.h:127-135
//
// There is NO CPU fallback in this file: every numeric operation is a kernel of the stmmqr_*.hip translation units.  If no
// gfx950 device is usable the entry points fail with STMMQR_ERR_DEVICE.
#include "stmmqr_plan.h"

#include <functional>
#include <string>

thread_local std::string g_err;
stmmqr_options g_opt = {STM_NB, 64, 0, 0, 0, 1, STM_TALL_MIN, 2, 0, 4};      // (panel_algo 0: by panel height; lookahead 2: passenger launches)
size_t g_chunk[4] = {32, 5000, 4, 4};     // FCHUNK, SMALL, MINCHUNK, MINCHUNK_RATIO (SparseQR.h:16-19)

stm_common_layout g_layout = {
    /* status */ 1004, /* malloc_count */ 1032, /* memory_usage */ 1040, /* memory_inuse */ 1048,
    /* blas_ok */ 1100, /* SPQR_grain */ 1104, /* SPQR_small */ 1112, /* SPQR_shrink */ 1120,
    /* SPQR_flopcount */ 1128, /* SPQR_flopcount_bound */ 1136};

int fail(int code, const std::string &msg)
{
    g_err = msg;
    if (g_opt.verbose) fprintf(stderr, "[stmmqr_hip] error %d: %s\n", code, msg.c_str());
    return code;
}

int stm_ensure_device(int device)
{
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return fail(STMMQR_ERR_DEVICE, "no HIP device visible: the MI355X path has no CPU fallback");
    if (device >= cnt) return fail(STMMQR_ERR_DEVICE, "device index out of range");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    static bool configured = false;
    if (!configured) {
        LCHK(stm_configure_kernels());
        LCHK(stm_configure_capanel());
        configured = true;
    }
    return 0;
}

namespace {

// The side stream of the look-ahead schedule: ONE per device and process, created at the first look-ahead factorization
// and kept (a CU-masked stream owns a hardware queue; creating one per plan exhausted them).  Its CU mask leaves
// STMMQR_SIDE_RESERVE compute units (the mask bits interleave over the 8 XCDs, so 4 per XCD at 32) to the plan
// streams: the workgroups of a panel kernel need most of a CU's LDS and would otherwise wait until the side stream's
// update grid has drained.  Plans of one device that factorize at the same time share it (still ordered by events).
std::mutex g_side_mu;
hipStream_t g_side[64] = {};
bool g_side_tried[64] = {};

// (registered with atexit at the first creation, i.e. after the HIP runtime registered its own handlers: it runs before
//  them; stmmqr_shutdown() calls it too)
void destroy_side_streams()
{
    std::lock_guard<std::mutex> lock(g_side_mu);
    for (int d = 0; d < 64; d++) {
        if (g_side[d]) {
            if (hipSetDevice(d) == hipSuccess) { (void)hipStreamSynchronize(g_side[d]); (void)hipStreamDestroy(g_side[d]); }
            g_side[d] = nullptr;
        }
        g_side_tried[d] = false;
    }
}

hipStream_t side_stream_for(int device)
{
    hipStream_t *side = g_side;
    bool *tried = g_side_tried;
    static bool registered = false;
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(g_side_mu);
    if (tried[device]) return side[device];
    tried[device] = true;
    if (!registered) { registered = true; atexit(destroy_side_streams); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    const int ncu = prop.multiProcessorCount;
    int reserve = (int)knobs::num(knobs::K_SIDE_RESERVE);
    if (reserve > ncu / 2) reserve = ncu / 2;
    hipStream_t q = nullptr;
    if (reserve > 0) {
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        for (int i = reserve; i < ncu; i++) mask[(size_t)i >> 5] |= 1u << (i & 31);
        if (hipExtStreamCreateWithCUMask(&q, (uint32_t)mask.size(), mask.data()) != hipSuccess) q = nullptr;
    }
    if (!q && hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess) q = nullptr;
    side[device] = q;
    return q;
}

// ------------------------------------------------------------------------------------------------
// planner: everything that depends only on the symbolic analysis
// ------------------------------------------------------------------------------------------------
int build_plan(stmmqr_plan &P, const stmmqr_symbolic_view &v)
{
    P.m = v.m; P.n = v.n; P.anz = v.anz; P.nf = v.nf; P.maxfn = v.maxfn; P.rjsize = v.rjsize;
    P.hisize = v.hisize; P.do_rank = v.do_rank_detection ? 1 : 0;
    P.keep_h = v.r_only ? 0 : 1;
    P.maxstack = v.maxstack > 0 ? v.maxstack : 0;
    // (a plan-time knob that every later rebuild of the schedule keeps: a reschedule must not give the plan another arena)
    P.rh_est_scale = knobs::value(knobs::K_RH_EST_SCALE);
    const long m = v.m, n = v.n, nf = v.nf;
    if (m < 0 || n < 0 || nf < 0) return fail(STMMQR_ERR_INVALID, "negative dimension");
    if (v.anz >= (1L << 31) - 1 || v.rjsize >= (1L << 31) - 1 || v.hisize >= (1L << 31) - 1 || m >= (1L << 30) ||
        n >= (1L << 30))
        return fail(STMMQR_ERR_TOO_LARGE, "problem exceeds the 32-bit device index range");
    auto cp = [](std::vector<long> &dst, const stm_long *src, long cnt) {
        dst.assign(src, src + (cnt > 0 ? cnt : 0));
    };
    cp(P.Sp, v.Sp, m + 1); cp(P.Sj, v.Sj, v.anz); cp(P.PLinv, v.PLinv, m); cp(P.Sleft, v.Sleft, n + 2);
    cp(P.Child, v.Child, nf + 1); cp(P.Childp, v.Childp, nf + 2); cp(P.Super, v.Super, nf + 1);
    cp(P.Rp, v.Rp, nf + 1); cp(P.Rj, v.Rj, v.rjsize); cp(P.Post, v.Post, nf); cp(P.Hip, v.Hip, nf + 1);
    P.has_qfill = v.Qfill != nullptr;
    if (P.has_qfill) cp(P.Qfill, v.Qfill, n);

    // ---- per-front symbolic sizes -----------------------------------------------------------
    std::vector<long> parent(nf, -1);
    for (long f = 0; f < nf; f++)
        for (long q = P.Childp[f]; q < P.Childp[f + 1]; q++) parent[P.Child[q]] = f;

    // upper bound on the rows of every front: taken from the analysis when given (QRsym->Fm, worst case when
    // rank detection is on: SparseQR_analyze.c:461-471), otherwise recomputed with the same recurrence
    P.Fm.assign(nf, 0);
    if (v.Fm) {
        for (long f = 0; f < nf; f++) P.Fm[f] = v.Fm[f];
    } else {
        std::vector<long> cmub(nf, 0);
        for (long kf = 0; kf < nf; kf++) {
            const long f = P.Post[kf];
            const long fp = P.Super[f + 1] - P.Super[f], fn = P.Rp[f + 1] - P.Rp[f];
            long fm = P.Sleft[P.Super[f + 1]] - P.Sleft[P.Super[f]];
            for (long q = P.Childp[f]; q < P.Childp[f + 1]; q++) fm += cmub[P.Child[q]];
            P.Fm[f] = fm;
            const long cn = fn - fp;
            cmub[f] = P.do_rank ? std::min(fm, cn) : std::min(std::max(fm - std::min(fm, fp), 0L), cn);
        }
    }

    // the row count every front will have if no pivot column dies (exact for full-rank input): used only to plan the
    // number of panel launches (stm_tall_panel); the kernels cope with any actual row count
    std::vector<long> fmest(nf, 0), cmest(nf, 0);
    for (long kf = 0; kf < nf; kf++) {
        const long f = P.Post[kf];
        const long fp = P.Super[f + 1] - P.Super[f], fn = P.Rp[f + 1] - P.Rp[f];
        long fe = P.Sleft[P.Super[f + 1]] - P.Sleft[P.Super[f]];
        for (long q = P.Childp[f]; q < P.Childp[f + 1]; q++) fe += cmest[P.Child[q]];
        fmest[f] = std::min(fe, P.Fm[f]);
        cmest[f] = std::min(std::max(fe - std::min(fe, fp), 0L), fn - fp);
    }

    P.fs.assign(nf, FrontSym());
    long long foff = 0, coff = 0, tpan_total = 0;
    for (long kf = 0; kf < nf; kf++) {
        const long f = P.Post[kf];
        FrontSym &s = P.fs[f];
        const long fp = P.Super[f + 1] - P.Super[f], fn = P.Rp[f + 1] - P.Rp[f];
        const long fm = P.Fm[f];
        // (front-local offsets are 64-bit on the device: row + column * ld; rows and columns themselves are int32)
        if (fm * fn >= (1L << 36)) return fail(STMMQR_ERR_TOO_LARGE, "a single front exceeds 2^36 entries");
        s.fn = (int)fn; s.fp = (int)fp; s.col1 = (int)P.Super[f]; s.rp = (int)P.Rp[f]; s.hip = (int)P.Hip[f];
        s.child0 = (int)P.Childp[f]; s.child1 = (int)P.Childp[f + 1];
        s.srow0 = (int)P.Sleft[P.Super[f]]; s.srow1 = (int)P.Sleft[P.Super[f + 1]];
        s.fm_ub = (int)fm;
        s.fm_est = (int)fmest[f];
        s.ld = (int)std::max(2L, (fm + 1) & ~1L);
        s.npanels = (int)((fn + STM_NB - 1) / STM_NB);
        s.tpan = (int)tpan_total;
        tpan_total += s.npanels;
        {
            // Q-apply: fronts with this many entries or more are split over workgroups (k_qbig_*); STMMQR_QBIG_MIN
            // overrides the threshold (tests send small fronts through that path).  2 M entries until round 4; with the grouped launches
            // (k_qbig_step4) smaller fronts pay too, at 256 KB of T4 per four panels -- default workload, threshold: Q'b / solve ms,
            // GB of T4: 2 M 13.1 / 20.6, 0.31; 1 M 12.5 / 20.0, 0.39; 256 K 11.9 / 19.5, 0.61; 128 K 11.6 / 19.2, 0.81.  1 M.
            const long qbig_min = knobs::num(knobs::K_QBIG_MIN);
            // ... and, whatever its entry count, a front that one workgroup cannot hold in LDS: a tall thin one (16 363 rows at 40
            // columns) or a short wide one whose columns are all pivotal (10 921 of them) -- the split kernels have no such limit
            const bool over_lds = stm_lds_qapply(fm, fn) > STM_RES_LDS_MAX || stm_lds_rsolve(fp, fn) > STM_RES_LDS_MAX;
            s.qbig = ((fm * fn >= qbig_min || over_lds) && fn >= 1) ? 1 : 0;
            // R' x = b: the one-workgroup kernel keeps the front's u and x in LDS (6 550 columns of a square-ish front, 10 890 of a
            // short wide one); a front beyond that is split over its columns (k_rtbig_*) by the pass that knows how, rt_pass in mode RT_SPLIT.
            // STMMQR_RTBIG_MIN splits smaller ones too
            s.rtbig = (stm_lds_rtsolve(fp, fm, fn) > STM_RES_LDS_MAX || fm * fn >= knobs::num(knobs::K_RTBIG_MIN)) ? 1 : 0;
        }
        s.parent = (int)parent[f];
        s.foff = 0; s.coff = 0;                                    // (stm_assign_arenas, once the groups are known)
    }
    (void)foff; (void)coff;
    P.tpanels = tpan_total;

    // ---- relative indices (value independent): child column -> parent column, S entry -> front column ----
    std::vector<int> Rjrel(std::max(1L, v.rjsize), 0), Sjrel(std::max(1L, v.anz), 0), Sj0(std::max(1L, m), -1);
    {
        std::vector<int> Fmap(std::max(1L, n), -1);
        for (long f = 0; f < nf; f++) {
            const long p1 = P.Rp[f], fn = P.Rp[f + 1] - p1;
            for (long j = 0; j < fn; j++) Fmap[P.Rj[p1 + j]] = (int)j;
            for (long r = P.fs[f].srow0; r < P.fs[f].srow1; r++)
                for (long p = P.Sp[r]; p < P.Sp[r + 1]; p++) Sjrel[p] = Fmap[P.Sj[p]];
            for (long q = P.Childp[f]; q < P.Childp[f + 1]; q++) {
                const long c = P.Child[q];
                const long fpc = P.Super[c + 1] - P.Super[c], pc = P.Rp[c] + fpc, cn = P.Rp[c + 1] - pc;
                for (long cj = 0; cj < cn; cj++) Rjrel[pc + cj] = Fmap[P.Rj[pc + cj]];
                P.bytes_assemble_idx += 4.0 * (double)(2 * cn);
            }
        }
        for (long r = 0; r < m; r++)
            if (P.Sp[r + 1] > P.Sp[r]) Sj0[r] = (int)P.Sj[P.Sp[r]];
        P.bytes_assemble_idx += 4.0 * (double)v.anz;
    }
    // ---- size of every packed R+H block if no pivot column dies (exact for full-rank input): the symbolic staircase of the front
    // (qr_fsize: rows of S by leftmost column + the children's contribution rows, whose leftmost columns are the columns of their
    // C) run through qr_front's row bookkeeping (:1434-1609) and qr_rhpack's column lengths (:1691-1784).  Sizes the R+H arena of
    // the slab recycling (with a margin; QRsym->maxstack is the hard bound the arena falls back to) ----
    P.rh_est_total = 0;
    P.rh_est_front.assign((size_t)std::max(1L, nf), 0);
    {
        std::vector<long> stair;
        for (long kf = 0; kf < nf; kf++) {
            const long f = P.Post[kf];
            const long fp = P.fs[f].fp, fn = P.fs[f].fn, fm = fmest[f];
            stair.assign((size_t)fn + 1, 0);
            for (long j = 0; j < fp; j++) stair[(size_t)j] = P.Sleft[P.Super[f] + j + 1] - P.Sleft[P.Super[f] + j];
            for (long q = P.Childp[f]; q < P.Childp[f + 1]; q++) {
                const long c = P.Child[q];
                const long fpc = P.Super[c + 1] - P.Super[c], pc = P.Rp[c] + fpc;
                for (long i = 0; i < cmest[c]; i++) stair[(size_t)Rjrel[(size_t)(pc + i)]]++;
            }
            long run = 0;
            for (long j = 0; j < fn; j++) { run += stair[(size_t)j]; stair[(size_t)j] = run; }       // rows with leftmost column <= j
            long g = 0, rm = 0;
            long long sz = 0;
            for (long k = 0; k < fn; k++) {
                long t;
                if (g >= fm) t = (k < fp) ? 0 : fm;                       // rows ran out
                else { t = std::min(fm, std::max(g + 1, stair[(size_t)k])); g++; }
                if (!P.keep_h) { if (k < fp && t > 0 && rm < fm) rm++; sz += rm; continue; }   // (R only: rm rows per column)
                if (k < fp) { if (t > 0) rm++; sz += (t > 0) ? t : rm; }
                else { const long h = std::min(rm + (k - fp) + 1, fm); sz += rm + std::max(t - h, 0L); }
            }
            P.rh_est_total += sz;
            P.rh_est_front[(size_t)f] = sz;
        }
    }

    // ---- level schedule: one group holding every front (multi-GPU callers regroup with set_groups) ----
    P.group.assign(nf, 0);
    stm_assign_arenas(P);
    std::vector<int> tslot;
    stm_build_schedule(P, tslot);

    // ---- device memory ----------------------------------------------------------------------------
    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    // (the front and contribution-block arenas are allocated by the first factorization, stm_ensure_arenas: a plan that is
    //  regrouped for one rank of a sharded run never holds the whole tree's fronts)
    const double need = 8.0 * 1024.0 * (double)P.tpanels * 1.05 + 64.0 * (double)(v.rjsize + v.anz);
    if (need > 0.92 * (double)freeb)
        return fail(STMMQR_ERR_OUT_OF_MEMORY, "the plan's index arrays do not fit in free HBM");
    hipStream_t st = P.stream;
    auto up32 = [&](DevBuf<int> &d, const std::vector<long> &h) {
        std::vector<int> t(h.begin(), h.end());
        return d.upload(t, st);
    };
    LCHK(P.d_fs.upload(P.fs, st));
    LCHK(P.d_fnum.alloc(std::max(1L, nf)));
    HIPCHK(hipMemsetAsync(P.d_fnum.p, 0, std::max(1L, nf) * sizeof(FrontNum), st));
    LCHK(P.d_T.alloc((size_t)STM_PD_RING * P.tslots * STM_NB * STM_NB));
    LCHK(P.d_Gp.alloc((size_t)P.tslots * (P.gp_slabs + 1) * STM_NB * STM_NB));
    LCHK(P.d_Tall.alloc((size_t)std::max(1LL, P.tpanels) * STM_NB * STM_NB));
    LCHK(P.d_Wp.alloc((size_t)P.wp_doubles));
    LCHK(P.d_Ypend.alloc((size_t)std::max(1LL, P.yp_doubles)));
    LCHK(P.d_ypoff.upload(P.ypoff, st));
    LCHK(P.d_Wp2.alloc((size_t)std::max(1LL, P.wp2_doubles)));
    P.wcnt_n = (size_t)(P.wp_doubles / (STM_NB * 32) + 1);
    LCHK(P.d_wcnt.alloc(P.wcnt_n));
    LCHK(P.d_wcnt2.alloc(P.wcnt_n));
    LCHK(P.d_wflag.alloc(P.wcnt_n));
    if (!P.d_abort.p) LCHK(P.d_abort.alloc(4));
    LCHK(P.d_wflag2.alloc(P.wcnt_n));
    HIPCHK(hipMemset(P.d_wcnt.p, 0, P.wcnt_n * sizeof(int)));
    HIPCHK(hipMemset(P.d_wcnt2.p, 0, P.wcnt_n * sizeof(int)));
    LCHK(P.d_tslot.upload(tslot, st));
    LCHK(P.d_Sx.alloc((size_t)v.anz));
    LCHK(P.d_Ax.alloc((size_t)v.anz));
    LCHK(P.d_smap.alloc((size_t)v.anz));
    LCHK(up32(P.d_Sp, P.Sp));
    LCHK(P.d_Sjrel.upload(Sjrel, st));
    LCHK(P.d_Sj0.upload(Sj0, st));
    LCHK(up32(P.d_Sleft, P.Sleft));
    LCHK(up32(P.d_Child, P.Child));
    LCHK(P.d_Rjrel.upload(Rjrel, st));
    LCHK(P.d_Stair.alloc((size_t)v.rjsize));
    LCHK(P.d_Tau.alloc((size_t)v.rjsize));
    LCHK(P.d_Hii.alloc((size_t)v.hisize));
    LCHK(P.d_Cmap.alloc((size_t)v.rjsize));
    LCHK(P.d_Cursor.alloc((size_t)v.rjsize));
    LCHK(P.d_Rhoff.alloc((size_t)v.rjsize));
    LCHK(P.d_Rboff.alloc((size_t)std::max(1L, nf)));
    LCHK(P.d_total.alloc(1));
    LCHK(P.d_dbg.alloc(2048));                                // ([64] counters + the timeline of a STAMPS build: 16 + 64 b + idx)
    LCHK(P.d_amax.alloc(1));
    LCHK(P.d_sig.alloc(2));
    HIPCHK(hipMemsetAsync(P.d_dbg.p, 0, 2048 * sizeof(unsigned long long), st));
    LCHK(P.d_Rdead.alloc((size_t)std::max(1L, n)));
    LCHK(P.d_lists.upload(P.lists, st));
    LCHK(P.d_wlists.upload(P.wlists, st));
    HIPCHK(hipStreamSynchronize(st));
    LCHK(stm_upload_recycle(P));
    return 0;
}

// qr_stranspose2 as a symbolic map: smap[s] = p such that Sx[s] = Ax[p]  (SparseQR_factorize.c:755-785)
int set_pattern(stmmqr_plan &P, const stm_long *Ap, const stm_long *Ai)
{
    const long m = P.m, n = P.n;
    if (!Ap || !Ai) return fail(STMMQR_ERR_INVALID, "Ap/Ai are required");
    if (Ap[n] != P.anz) return fail(STMMQR_ERR_INVALID, "nnz(A) differs from the symbolic analysis");
    std::vector<long> W(P.Sp.begin(), P.Sp.begin() + m);
    std::vector<int> smap(std::max(1L, P.anz), 0);
    for (long col = 0; col < n; col++) {
        const long j = P.has_qfill ? P.Qfill[col] : col;
        for (long p = Ap[j]; p < Ap[j + 1]; p++) {
            const long i = Ai[p];
            if (i < 0 || i >= m) return fail(STMMQR_ERR_INVALID, "row index out of range");
            smap[W[P.PLinv[i]]++] = (int)p;
        }
    }
    if (P.anz > 0)
        HIPCHK(hipMemcpyAsync(P.d_smap.p, smap.data(), (size_t)P.anz * sizeof(int), hipMemcpyHostToDevice, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    P.h_smap.swap(smap);                                     // (the products with A rebuild A's pattern from it: stm_ensure_a_index)
    P.a_index_ready = false;
    P.pattern_set = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// the level-batched schedule (device resident inputs -> device resident factors)
// ------------------------------------------------------------------------------------------------
// State every factorization starts from (issued by stmmqr_factorize_begin, BEFORE any stmmqr_plan_import_front of the
// phased interface: an imported front's fm / rank / cm must survive until its parent assembles it).
int reset_factorization(stmmqr_plan &P)
{
    hipStream_t st = P.stream;
    LCHK(stm_ensure_arenas(P));
    // (with slab recycling every front's slab is zeroed when the front starts: k_zero_slabs in prep)
    if (!P.recycle) HIPCHK(hipMemsetAsync(P.d_F.p, 0, (size_t)P.farena * sizeof(double), st));
    HIPCHK(hipMemsetAsync(P.d_rhtop.p, 0, 2 * sizeof(long long), st));
    HIPCHK(hipMemsetAsync(P.d_Rdead.p, 0, (size_t)std::max(1L, P.n), st));
    HIPCHK(hipMemsetAsync(P.d_fnum.p, 0, (size_t)std::max(1L, P.nf) * sizeof(FrontNum), st));
    // (tickets are back at zero after every launch unless a wait ran out; the flags carry step numbers)
    HIPCHK(hipMemsetAsync(P.d_wcnt.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wcnt2.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wflag.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wflag2.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_abort.p, 0, 4 * sizeof(int), st));
    LCHK(stm_launch_sigma(P.d_Ax.p, (int)P.anz, P.d_amax.p, P.d_sig.p, st));
    LCHK(stm_launch_gather_sx(P.d_Ax.p, P.d_smap.p, P.d_Sx.p, (int)P.anz, st));
    P.stats.nlaunch += 6;
    return 0;
}

// Recovery of ONE group of the phased interface after a bounded panel wait ran out in it: everything its fronts wrote is
// put back to the state reset_factorization left (fronts of other groups and imported fronts are not touched).
int reset_group(stmmqr_plan &P, int grp)
{
    hipStream_t st = P.stream;
    const FrontNum zero = FrontNum();
    for (long f = 0; f < P.nf; f++) {
        if (P.group[f] != grp) continue;
        const FrontSym &s = P.fs[f];
        HIPCHK(hipMemsetAsync(P.d_F.p + s.foff, 0, (size_t)s.ld * (size_t)s.fn * sizeof(double), st));
        HIPCHK(hipMemcpyAsync(P.d_fnum.p + f, &zero, sizeof zero, hipMemcpyHostToDevice, st));
        if (s.fp > 0) HIPCHK(hipMemsetAsync(P.d_Rdead.p + s.col1, 0, (size_t)s.fp, st));
    }
    HIPCHK(hipMemsetAsync(P.d_wcnt.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wcnt2.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wflag.p, 0, P.wcnt_n * sizeof(int), st));
    HIPCHK(hipMemsetAsync(P.d_wflag2.p, 0, P.wcnt_n * sizeof(int), st));
    // abort[0..1] only: [3], a refused message of the subtree exchange, stays, and [2] goes back to what the groups before this one
    // left (P.abort2_before: a front of an EARLIER group that outlived its cut schedule must still be reported at finish, while a
    // front of this group that the wait left unfinished is not such a front -- the rerun raises [2] again if it is one)
    HIPCHK(hipMemsetAsync(P.d_abort.p, 0, 2 * sizeof(int), st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(P.d_abort.p + 2), P.abort2_before, 1, st));
    // slab recycling: a recycling plan holds the whole tree in this one group, and the aborted attempt has staged packed blocks behind
    // the arena's bump pointer; the rerun stages every block again, so the pointer (and the overflow word) go back to zero -- otherwise
    // the second set lands behind the first and overflows an arena that holds the estimate + 12.5 %
    if (P.recycle) HIPCHK(hipMemsetAsync(P.d_rhtop.p, 0, 2 * sizeof(long long), st));
    HIPCHK(hipStreamSynchronize(st));                       // (`zero` lives on this stack frame)
    return 0;
}

}  // namespace


// Products with A (stmmqr_plan_spmv, the seminormal solve): A's column form and a row form whose entries point at A's values,
// built at the first such call after set_pattern from the plan's S pattern and the S -> A map (S = A(P, Q), smap[S entry] =
// position in A); the factorization itself never needs them.  Rows keep A's column order.
int stm_ensure_a_index(stmmqr_plan &P)
{
    if (P.a_index_ready) return 0;
    if (!P.pattern_set) return fail(STMMQR_ERR_INVALID, "pattern of A was never given");
    const long m = P.m, n = P.n, anz = P.anz;
    std::vector<int> rowof((size_t)std::max(1L, m)), arow((size_t)std::max(1L, anz)), acol((size_t)std::max(1L, anz));
    for (long i = 0; i < m; i++) rowof[(size_t)P.PLinv[i]] = (int)i;
    for (long r = 0; r < m; r++)
        for (long q = P.Sp[r]; q < P.Sp[r + 1]; q++) {
            const int p = P.h_smap[(size_t)q];
            arow[(size_t)p] = rowof[(size_t)r];
            acol[(size_t)p] = (int)(P.has_qfill ? P.Qfill[P.Sj[q]] : P.Sj[q]);
        }
    std::vector<int> acp((size_t)n + 1, 0), arp, arj, arq;
    for (long p = 0; p < anz; p++) acp[(size_t)acol[(size_t)p] + 1]++;
    for (long j = 0; j < n; j++) acp[(size_t)j + 1] += acp[(size_t)j];
    stm_row_form(m, anz, arow.data(), acol.data(), arp, arj, arq);      // (A's order: column by column, so every row in column order)
    LCHK(P.a_idx.cp.upload(acp, P.stream)); LCHK(P.a_idx.ci.upload(arow, P.stream));
    LCHK(P.a_idx.rp.upload(arp, P.stream)); LCHK(P.a_idx.rj.upload(arj, P.stream)); LCHK(P.a_idx.rq.upload(arq, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    P.a_index_ready = true;
    return 0;
}

// The schedule rebuilt on the plan's own grouping (after a factorization that asked for another schedule: the full one, a larger
// arena, the cut one on or off).  P.group holds the group ids only; the shared fronts get their STMMQR_GROUP_SHARED bit back, or
// stmmqr_plan_set_groups would take them for fronts of this rank alone.
static int regroup_same(stmmqr_plan &P)
{
    std::vector<int> grp(P.group.begin(), P.group.end());
    for (size_t f = 0; f < grp.size(); f++) if (f < P.shared.size() && P.shared[f]) grp[f] |= STMMQR_GROUP_SHARED;
    return stmmqr_plan_set_groups(&P, grp.data());
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char *stmmqr_version(void) { return "stmmqr_hip 0.1 (gfx950)"; }
const char *stmmqr_last_error(void) { return g_err.c_str(); }
void stmmqr_get_options(stmmqr_options *o) { if (o) *o = g_opt; }
void stmmqr_set_options(const stmmqr_options *o)
{
    if (!o) return;
    g_opt = *o;
    if (g_opt.big_front_cols < 1) g_opt.big_front_cols = 1;
}
void stmmqr_set_common_layout(const stm_common_layout *l) { if (l) g_layout = *l; }
void stmmqr_get_common_layout(stm_common_layout *l) { if (l) *l = g_layout; }

/* End of use (optional): waits for the device and releases what the library holds process-wide.  A host program that
 * dlopen()s the library calls it before returning from main; the library has no static object whose destructor calls
 * into the HIP runtime, so nothing else happens at exit / dlclose. */
int stmmqr_device_alloc(size_t bytes, void **ptr)
{
    if (!ptr) return fail(STMMQR_ERR_INVALID, "null argument");
    *ptr = nullptr;
    if (hipMalloc(ptr, bytes ? bytes : 1) != hipSuccess) return fail(STMMQR_ERR_OUT_OF_MEMORY, "hipMalloc failed");
    return 0;
}
/* device-to-device copy, complete on return (after everything `hip_stream` -- may be NULL -- held before it); for callers that
 * implement a stmmqr_transport of their own on one GPU (tests).  With a stream the copy is a command OF that stream: what the
 * library records on the stream after the transport's call (the event its compute stream waits for before it unpacks a panel
 * message) then orders the copy's writes before the kernels that read them.  As a null-stream copy beside an empty stream that
 * event carried no dependency on the copy, and the unpacking kernel now and then read the PREVIOUS message of a reused ring
 * buffer (thread ranks on one GPU: a shared front wrong from one panel on, one run in two of the sharded tests). */
int stmmqr_device_copy(void *dst, const void *src, size_t bytes, void *hip_stream)
{
    if (hip_stream) {
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    } else if (bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}
int stmmqr_device_free(void *ptr)
{
    if (ptr && hipFree(ptr) != hipSuccess) return fail(STMMQR_ERR_DEVICE, "hipFree failed");
    return 0;
}

void stmmqr_plan_cache_clear(void);
void stmmqr_shutdown(void)
{
    stmmqr_plan_cache_clear();
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) == hipSuccess && cnt > 0) {
        (void)hipDeviceSynchronize();
        int dev = 0;
        (void)hipGetDevice(&dev);
        destroy_side_streams();
        (void)hipSetDevice(dev);
    }
}

int stmmqr_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}
const char *stmmqr_device_name(int device)
{
    static thread_local char name[256];
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return "";
    snprintf(name, sizeof name, "%s", prop.gcnArchName);
    return name;
}

int chunk_getSettings(size_t a, size_t b, size_t c, size_t d)
{
    g_chunk[0] = a; g_chunk[1] = b; g_chunk[2] = c; g_chunk[3] = d;
    return 0;
}

stmmqr_plan *stmmqr_plan_create(const stmmqr_symbolic_view *sym, int device, int *status)
{
    int st = 0;
    stmmqr_plan *P = nullptr;
    if (!sym) st = fail(STMMQR_ERR_INVALID, "null symbolic view");
    if (!st) st = stm_ensure_device(device);
    if (!st) {
        P = new (std::nothrow) stmmqr_plan();
        if (!P) st = fail(STMMQR_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    if (!st) {
        (void)hipGetDevice(&P->device);
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        if (hipStreamCreateWithPriority(&P->stream, hipStreamNonBlocking, prio_hi) != hipSuccess)
            st = fail(STMMQR_ERR_DEVICE, "hipStreamCreate failed");
        for (auto &e : P->ev)
            if (!st && hipEventCreate(&e) != hipSuccess) st = fail(STMMQR_ERR_DEVICE, "hipEventCreate failed");
    }
    if (!st) {
        const double t0 = now_ms();
        st = build_plan(*P, *sym);
        if (!st) P->stats.ms_host = now_ms() - t0;
    }
    if (st && P) { delete P; P = nullptr; }
    if (status) *status = st;
    return P;
}

void stmmqr_plan_release_rings(stmmqr_plan *plan);
void stmmqr_plan_destroy(stmmqr_plan *plan)
{
    if (plan) stmmqr_plan_release_rings(plan);
    delete plan;
}

int stmmqr_plan_set_pattern(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai)
{
    if (!plan) return fail(STMMQR_ERR_INVALID, "null plan");
    HIPCHK(hipSetDevice(plan->device));
    return set_pattern(*plan, Ap, Ai);
}

// ---- phased interface: begin -> factorize_group(g) ... -> finish.  stmmqr_factorize_device = all of it ----
int stmmqr_factorize_begin(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                           int ax_on_device, double tol, stm_long ntol)
{
    if (!plan || !Ax) return fail(STMMQR_ERR_INVALID, "null plan / values");
    stmmqr_plan &P = *plan;
    HIPCHK(hipSetDevice(P.device));
    if (Ap && Ai) {
        int e = set_pattern(P, Ap, Ai);
        if (e) return e;
    }
    if (!P.pattern_set) return fail(STMMQR_ERR_INVALID, "pattern of A was never given");
    if (!P.keep_h)
        for (long f = 0; f < P.nf; f++)
            if (P.group[f] != 0) return fail(STMMQR_ERR_INVALID, "a plan without H (keepH = 0) takes one group only");
    if (((P.early_end && !P.early_phased) || P.early_end_failed) && !P.whole_call) {
        // phased use (begin / group / finish by the caller): no retry loop around the factorization, so the plan schedules every
        // panel of every front (the cut schedule needs stmmqr_factorize_device's rerun when a front outlives it)
        P.early_end_failed = false;
        P.full_schedule = true;
        P.begun = false;
        int e = regroup_same(P);
        if (e) return e;
    }
    if (P.arena_overflow && P.recycle && !P.whole_call) {
        // phased use (begin / group / finish by the caller): the previous factorization of this plan did not fit the R+H arena
        // (finish returned OUT_OF_MEMORY and noted rh_grow / overflowed).  Those only take effect when the schedule is
        // rebuilt, which stmmqr_factorize_device does in its own retry loop; here the rebuild happens at the next begin, so a
        // caller that simply tries again gets the arena at its hard bound (then no recycling) instead of the same failure.
        P.arena_overflow = false;
        P.begun = false;
        int e = regroup_same(P);
        if (e) return e;
    }
    const double host_ms_plan = P.stats.ms_host;
    P.stats = stmmqr_stats();
    P.stats.ms_host = host_ms_plan;
    P.factored = false;
    P.res.new_factorization();
    P.evused = 0;
    P.begun = true;
    P.first_group = true;
    P.abort2_before = 0;                                       // (reset_factorization clears abort[])
    if (!P.do_rank) tol = -1;                                  // SparseQR_factorize.c:285-289
    P.last_tol = tol; P.last_ntol = ntol;
    hipStream_t st = P.stream;
    HIPCHK(hipEventRecord(P.ev[0], st));
    if (P.anz > 0) {
        HIPCHK(hipMemcpyAsync(P.d_Ax.p, Ax, (size_t)P.anz * sizeof(double),
                              ax_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipEventRecord(P.ev[1], st));
    return reset_factorization(P);
}

int stmmqr_factorize_group(stmmqr_plan *plan, int group, int detail)
{
    if (!plan || !plan->begun) return fail(STMMQR_ERR_INVALID, "stmmqr_factorize_begin was not called");
    stmmqr_plan &P = *plan;
    HIPCHK(hipSetDevice(P.device));
    int e = 0;
    const bool recoverable = !P.whole_call && !P.serial_panels;
    const bool graph_ok = g_opt.use_graph && !detail && group == 0 && P.first_group && !knobs::on(knobs::K_DUMPLV);
    if (graph_ok) {
        // replay the step schedule of group 0 as a hipGraph, captured once per plan and per everything that travels in the
        // kernel arguments or decides what is launched: (tol, ntol, debug mask), the schedule generation (set_groups
        // rebuilds the lists and may move the workspaces) and the run-time options
        const DevCtx c = P.ctx();
        // (everything stm_run_schedule reads at capture time and that decides WHAT is launched or travels in the kernel arguments:
        //  the knobs of the environment as the very struct it reads them into, the run-time options incl. pair_update, STMMQR_TUNE)
        const knobs::RunKnobs rk = knobs::RunKnobs::read();
        unsigned long long optkey = rk.key();
        for (long long v : {(long long)g_opt.lookahead, (long long)g_opt.split_update, (long long)g_opt.fused_update, (long long)g_opt.pair_update,
                            (long long)P.serial_panels, (long long)c.tune, (long long)P.keep_h})
            optkey = knobs::fold(optkey, (unsigned long long)v);
        if (!P.graph_exec || P.graph_tol != c.tol || P.graph_ntol != c.ntol || P.graph_dbg != c.dbg || P.graph_gen != P.sched_gen ||
            P.graph_opt != optkey) {
            if (P.graph_exec) { (void)hipGraphExecDestroy(P.graph_exec); P.graph_exec = nullptr; }
            P.graph_nlaunch = 0;
            // everything stm_run_schedule creates lazily is created BEFORE the capture: the device's side stream (device
            // properties, a CU-masked stream, an atexit handler) and the per-step events of the look-ahead
            if (g_opt.lookahead && !P.serial_panels && P.gsteps[0].size() > 1) {
                if (!P.side) P.side = side_stream_for(P.device);
                PASS(stm_ensure_la_events(P, P.gsteps[0].size(), rk));
            }
            const long nl0 = P.stats.nlaunch;
            hipGraph_t gph = nullptr;
            // the side stream is shared by the plans of a device: captures are serialised against each other (a plan that
            // factorizes without a graph while another one captures is the caller's to avoid, as for any shared stream)
            static std::mutex capture_mu;
            std::lock_guard<std::mutex> lock(capture_mu);
            HIPCHK(hipStreamBeginCapture(P.stream, hipStreamCaptureModeThreadLocal));
            e = stm_run_schedule(P, false, 0, nullptr);
            const hipError_t ce = hipStreamEndCapture(P.stream, &gph);
            if (e) { if (gph) (void)hipGraphDestroy(gph); return e; }
            HIPCHK(ce);
            HIPCHK(hipGraphInstantiate(&P.graph_exec, gph, nullptr, nullptr, 0));
            (void)hipGraphDestroy(gph);
            P.graph_tol = c.tol; P.graph_ntol = c.ntol; P.graph_dbg = c.dbg; P.graph_gen = P.sched_gen; P.graph_opt = optkey;
            P.graph_nlaunch = P.stats.nlaunch - nl0;
        } else {
            // (the statistics stm_run_schedule accumulates on the host)
            P.stats.nlaunch += P.graph_nlaunch;
            P.stats.nlevels += (long)P.glevels[0].size();
            P.stats.nsteps += (long)P.gsteps[0].size();
        }
        HIPCHK(hipGraphLaunch(P.graph_exec, P.stream));
    } else
        e = stm_run_schedule(P, detail != 0, group, nullptr);
    // Phased use (begin / group / finish called by the host: the sharded path): a bounded panel wait that ran out is found
    // HERE and the group is run again with one-workgroup panels (no inter-workgroup waits), exactly as
    // stmmqr_factorize_device does for the whole factorization -- the other groups and the imported fronts are not touched.
    if (!e && recoverable) {
        // (eight bytes: the kernels raise abort[1] beside the front's own perr -- not a copy of every FrontNum per phase -- and
        //  abort[2], which the host keeps as it stands after every group that needs no rerun)
        int flags[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(flags, P.d_abort.p + 1, 2 * sizeof(int), hipMemcpyDeviceToHost, P.stream));
        HIPCHK(hipStreamSynchronize(P.stream));
        const int failed = flags[0];
        if (!failed) P.abort2_before = flags[1];
        if (failed) {
            if (g_opt.verbose) fprintf(stderr, "[stmmqr_hip] a panel wait ran out in group %d: running it again with one-workgroup panels\n", group);
            P.stats.retries++;
            e = reset_group(P, group);
            P.serial_panels = true;
            if (!e) e = stm_run_schedule(P, detail != 0, group, nullptr);
            P.serial_panels = false;
            if (!e) {
                HIPCHK(hipMemcpyAsync(&P.abort2_before, P.d_abort.p + 2, sizeof(int), hipMemcpyDeviceToHost, P.stream));
                HIPCHK(hipStreamSynchronize(P.stream));
            }
        }
    }
    P.first_group = false;
    return e;
}

int stmmqr_factorize_finish(stmmqr_plan *plan, stmmqr_stats *stats)
{
    if (!plan || !plan->begun) return fail(STMMQR_ERR_INVALID, "stmmqr_factorize_begin was not called");
    stmmqr_plan &P = *plan;
    HIPCHK(hipSetDevice(P.device));
    hipStream_t st = P.stream;
    HIPCHK(hipEventRecord(P.ev[4], st));
    bool overflow = false;
    int e = stm_run_pack(P, overflow);
    if (e) return e;
    HIPCHK(hipEventRecord(P.ev[5], st));
    int hard[3] = {0, 0, 0};                                  // abort[1]: a bounded wait ran out; [2]: a front outlived its schedule; [3]: a refused message
    HIPCHK(hipMemcpyAsync(hard, P.d_abort.p + 1, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // per-front numeric summary (small): flops, ranks, and which panel chain gave up waiting
    P.h_fnum.resize((size_t)std::max(1L, P.nf));
    if (P.nf > 0)
        HIPCHK(hipMemcpy(P.h_fnum.data(), P.d_fnum.p, (size_t)P.nf * sizeof(FrontNum), hipMemcpyDeviceToHost));
    bool perr = hard[0] != 0;
    const bool dbg_early = knobs::on(knobs::K_DBG_EARLY);
    for (long f = 0; f < P.nf; f++) {
        if (P.group[f] < 0) continue;                  // factorized elsewhere
        const FrontNum &nm = P.h_fnum[f];
        const FrontSym &s = P.fs[f];
        perr = perr || nm.perr;
        if (dbg_early && s.nsched < s.npanels && (!nm.done || nm.g < std::min(nm.fm, s.fn)))
            fprintf(stderr, "[early] front %ld fn %d fp %d fm %d fm_est %d fm_ub %d g %d rank %d done %d nsched %d npanels %d\n", f, s.fn, s.fp, nm.fm, s.fm_est,
                    s.fm_ub, nm.g, nm.rank, nm.done, s.nsched, s.npanels);
    }
    // The causes, most specific first.  A wait that ran out leaves its front unfinished, so it also looks like a front that outlived
    // its schedule: that is the wait's failure (serial retry, the cut schedule stays).  Either leaves fronts that packed what they
    // held when they stopped, which may not fit the recycled arena: that overflow is theirs, not the arena's (rh_grow stays).
    if (hard[2]) return fail(STMMQR_ERR_DEVICE, "a contribution block received from another rank does not fit its front's symbolic bounds");
    if (perr) {
        P.panel_wait_failed = true;
        P.evused = 0;
        return fail(STMMQR_ERR_DEVICE, "a panel workgroup gave up waiting for its neighbours (device shared with another job?)");
    }
    if (hard[1]) {
        // (rank-deficient fronts: more rows reached a front than the full-rank estimate its schedule was cut to)
        P.early_end_failed = true;
        P.evused = 0;
        return fail(STMMQR_ERR_RESCHEDULE, "a front was not finished by its last scheduled panel (the schedule is rebuilt with every panel)");
    }
    if (overflow) {
        if (!P.rh_grow) P.rh_grow = 1;                            // next: the hard bound (QRsym->maxstack / all recycled slabs)
        else P.overflowed = true;                                 // that too: no recycling for this plan
        P.arena_overflow = true;
        P.evused = 0;
        return fail(STMMQR_ERR_OUT_OF_MEMORY, "the packed factors exceed the R+H arena of the slab recycling");
    }
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, P.ev[0], P.ev[1])); P.stats.ms_h2d = ms;
    HIPCHK(hipEventElapsedTime(&ms, P.ev[1], P.ev[5])); P.stats.ms_total = ms;
    HIPCHK(hipEventElapsedTime(&ms, P.ev[4], P.ev[5])); P.stats.ms_pack += ms;
    // STMMQR_DUMPSTEPS=file (detail runs, diagnosis): one line per timeline step with what ran and how long it took
    FILE *dump = (P.evused && knobs::text(knobs::K_DUMPSTEPS)) ? fopen(knobs::text(knobs::K_DUMPSTEPS), "w") : nullptr;
    std::vector<float> st_panel, st_upd;
    if (dump && !P.gsteps.empty()) { st_panel.assign(P.gsteps[0].size(), 0.f); st_upd.assign(P.gsteps[0].size(), 0.f); }
    for (size_t q = 0; q < P.evused; q++) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, P.evpairs[q].a, P.evpairs[q].b));
        if (dump && (size_t)P.evpairs[q].step < st_panel.size()) {
            if (P.evpairs[q].cat == 2) st_panel[(size_t)P.evpairs[q].step] += t;
            if (P.evpairs[q].cat == 3) st_upd[(size_t)P.evpairs[q].step] += t;
        }
        switch (P.evpairs[q].cat) {
            case 0: P.stats.ms_assemble += t; break;
            case 1: P.stats.ms_front += t; P.stats.ms_small += t; break;
            case 2: P.stats.ms_front += t; P.stats.ms_panel += t; P.stats.npanel_launch++; break;
            case 3: P.stats.ms_front += t; P.stats.ms_update += t; P.stats.nupdate_launch++; break;
            default: P.stats.ms_pack += t; break;
        }
    }
    P.evused = 0;
    if (dump) {
        for (size_t t = 0; t < st_panel.size(); t++) {
            const Step &S = P.gsteps[0][t];
            int maxrows = 0, pwg = 0;
            long tiles = 0;
            for (int i = 0; i < S.n_act; i++) {
                const FrontSym &fsym = P.fs[P.lists[S.act_off + i]];
                const int p = P.lists[S.plist_off + i];
                maxrows = std::max(maxrows, stm_panel_rows_est(fsym, p));
                pwg += stm_use_ca(fsym, p, P.plan_algo, P.ca_min) ? stm_ca_slabs(fsym) : stm_tall_launches(fsym, p, P.tall_min);
                tiles += (long)stm_upd_ncb(fsym, p) * stm_upd_nsl(fsym);
            }
            fprintf(dump, "%zu n_act %d maxrows %d nsub %d pwg %d nca_use %d maxcb %d maxsl %d split %d tiles %ld panel_us %.1f upd_us %.1f\n", t,
                    S.n_act, maxrows, S.nsub, pwg, S.nca_use, S.maxcb, S.maxsl, S.split, tiles, 1e3 * st_panel[t], 1e3 * st_upd[t]);
        }
        fclose(dump);
    }

    double flops = 0, bytes_asm = 0, bytes_pack = 0, fl_upd = 0, fl_upd_pair = 0;
    long rank = 0;
    for (long f = 0; f < P.nf; f++) {
        if (P.group[f] < 0) continue;                  // factorized elsewhere
        const FrontNum &nm = P.h_fnum[f];
        const FrontSym &s = P.fs[f];
        flops += nm.flops;
        fl_upd += nm.flops_upd;
        if ((size_t)f < P.pair_front.size() && P.pair_front[f]) fl_upd_pair += nm.flops_upd;
        rank += nm.rank;
        const double cn = s.fn - s.fp, cm = nm.cm;
        const double csize = cm * (cm + 1) / 2 + cm * (cn - cm);
        bytes_asm += 8.0 * ((double)nm.fm * s.fn) + 8.0 * csize;   // F first write + child C read (as a child)
        bytes_pack += 16.0 * (csize + (double)nm.rsize);
    }
    bytes_asm += 8.0 * (double)P.anz + P.bytes_assemble_idx;
    const int dbg = (int)knobs::num(knobs::K_DBG);
    if ((dbg & 32) && knobs::on(knobs::K_TIMELINE)) {
        // -DSTMMQR_STAMPS builds: wall-clock (100 MHz) timeline of panel 1 of the LAST front that ran one (the root), per column group
        std::vector<unsigned long long> hb(2048);
        HIPCHK(hipMemcpy(hb.data(), P.d_dbg.p, hb.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull;
        for (int b = 0; b < 16; b++) if (hb[16 + 64 * b]) t0 = std::min(t0, hb[16 + 64 * b]);
        for (int b = 0; b < 16; b++) {
            const unsigned long long *q = &hb[16 + 64 * b];
            if (!q[0]) continue;
            fprintf(stderr, "[panel timeline] group %2d:", b);
            auto us = [&](int i) { return q[i] ? 0.01 * (double)(q[i] - t0) : -1.0; };
            fprintf(stderr, " start %.2f loaded %.2f |", us(0), us(1));
            for (int h = 0; h < 6 && q[2 + 3 * h]; h++) fprintf(stderr, " wait %.2f vload %.2f applied %.2f |", us(2 + 3 * h), us(3 + 3 * h), us(4 + 3 * h));
            fprintf(stderr, " cols");
            for (int j = 0; j < 8; j++) if (q[20 + j]) fprintf(stderr, " %.2f", us(20 + j));
            fprintf(stderr, " | published %.2f final %.2f\n", us(30), us(31));
        }
    }
    if (dbg & 32768) {
        unsigned long long hb[64];
        HIPCHK(hipMemcpy(hb, P.d_dbg.p, sizeof hb, hipMemcpyDeviceToHost));
        const double n = hb[56] ? 100.0 * (double)hb[56] : 1.0;
        fprintf(stderr, "[block-0 launch, slab 0, us] descriptors+loads issued %.2f  phase 1 %.2f  partials+ticket %.2f  wait %.2f  sums %.2f  T %.2f  W2 %.2f  phase 2 %.2f  (%llu)\n",
                hb[48] / n, hb[49] / n, hb[50] / n, hb[51] / n, hb[52] / n, hb[53] / n, hb[54] / n, hb[55] / n, hb[56]);
        HIPCHK(hipMemset(P.d_dbg.p, 0, sizeof hb));
    }
    if (dbg & 48) {
        unsigned long long hb[64];
        HIPCHK(hipMemcpy(hb, P.d_dbg.p, sizeof hb, hipMemcpyDeviceToHost));
        fprintf(stderr, "[pipeline panels by actual rows] <=128 %llu  <=256 %llu  <=512 %llu  <=1024 %llu  <=2048 %llu  <=4096 %llu  more %llu;  of the <=512: %llu with a row estimate > 512\n",
                hb[32], hb[33], hb[34], hb[35], hb[36], hb[37], hb[38], hb[39]);
        fprintf(stderr, "[k_upd_w workgroups] launched %llu  with work %llu\n", hb[40], hb[41]);
        fprintf(stderr, "[panel cycles, summed over workgroups] stage-in+apply %llu  columns %llu  write-back %llu  - %llu  gram %llu\n",
                hb[0], hb[1], hb[2], hb[3], hb[4]);
        fprintf(stderr, "[last group of the panel pipeline, cycles] load %llu  waits %llu  apply-loads %llu  applies %llu  factor %llu  gram %llu\n", hb[6],
                hb[7], hb[12], hb[8] + hb[11], hb[9], hb[10]);
        fprintf(stderr, "[panel workgroups] %llu  cycles %llu  100 MHz ticks %llu  => %.3f GHz, %.2f us per workgroup\n", hb[46], hb[44], hb[45],
                hb[45] ? 0.1 * (double)hb[44] / (double)hb[45] : 0.0, hb[46] ? 0.01 * (double)hb[45] / (double)hb[46] : 0.0);
        fprintf(stderr, "[Gram-based panels] panels %llu  refresh rounds %llu  slab workgroups %llu\n", hb[13], hb[14], hb[15]);
        HIPCHK(hipMemset(P.d_dbg.p, 0, sizeof hb));
    }
    P.rank = rank;
    P.stats.flops = flops;
    P.stats.flops_update = fl_upd;
    P.stats.flops_update_pair = fl_upd_pair;
    P.stats.bytes_assemble = bytes_asm;
    P.stats.bytes_pack = bytes_pack;
    P.stats.device_bytes = P.device_bytes();
    if (knobs::on(knobs::K_MEMDUMP)) {
        auto gb = [](const auto &b) { return (double)b.n * sizeof(*b.p) * 1e-9; };
        fprintf(stderr, "[stmmqr_hip] device memory (GB): fronts %.3f  contribution blocks %.3f  R+H %.3f  update workspaces %.3f + %.3f  "
                        "kept T %.3f  pair -Y %.3f  Sx/Ax/smap %.3f  per-column arrays %.3f  total %.3f  (recycle %d, kept fronts %d, maxstack %.3f)\n",
                gb(P.d_F), gb(P.d_C), gb(P.d_RH), gb(P.d_Wp), gb(P.d_Wp2), gb(P.d_Tall), gb(P.d_Ypend), gb(P.d_Sx) + gb(P.d_Ax) + gb(P.d_smap),
                gb(P.d_Stair) + gb(P.d_Tau) + gb(P.d_Hii) + gb(P.d_Cmap) + gb(P.d_Cursor) + gb(P.d_Rhoff) + gb(P.d_Rjrel) + gb(P.d_Sjrel),
                P.stats.device_bytes * 1e-9, (int)P.recycle, (int)std::count(P.kept.begin(), P.kept.end(), (char)1), 8e-9 * (double)P.maxstack);
    }
    P.factored = true;
    P.begun = false;
    if (stats) *stats = P.stats;
    return 0;
}

int stmmqr_factorize_device(stmmqr_plan *plan, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                            int ax_on_device, double tol, stm_long ntol, stmmqr_stats *stats)
{
    if (!plan) return fail(STMMQR_ERR_INVALID, "null plan");
    const bool detail = g_opt.verbose >= 2 || (stats && stats->nlaunch == -1);
    // The multi-workgroup panel kernels wait for each other inside a launch (bounded).  Should such a wait ever run out
    // (the workgroups of a launch are not guaranteed to run together: a GPU shared with another job), the factorization is
    // not lost: it is run once more with every panel factorized by ONE workgroup (dev_panel: no inter-workgroup wait
    // anywhere), slower but independent of co-residency.
    int arena_retries = 0, reschedules = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        plan->serial_panels = (attempt == 1);
        plan->panel_wait_failed = false;
        plan->whole_call = true;
        int e = stmmqr_factorize_begin(plan, Ap, Ai, Ax, ax_on_device, tol, ntol);
        if (!e) plan->stats.retries = (attempt == 1 ? 1 : 0) + arena_retries;   // (visible in stmmqr_stats: bench.py asserts 0)
        if (!e) plan->stats.reschedules = reschedules;
        for (int g = 0; g < (int)plan->glevels.size() && !e; g++) e = stmmqr_factorize_group(plan, g, detail);
        if (!e) e = stmmqr_factorize_finish(plan, stats);
        plan->whole_call = false;
        if (e && plan->arena_overflow && plan->recycle) {
            // the packed factors did not fit the arena: sized from the full-rank estimate -> once more with the hard bound
            // (QRsym->maxstack); at the hard bound (never seen) -> once more with every front in a slab of its own and the packed
            // blocks placed at the end, as sharded plans always run
            plan->arena_overflow = false;
            if (g_opt.verbose) fprintf(stderr, "[stmmqr_hip] R+H arena overflow: factorizing again %s\n", plan->overflowed ? "without slab recycling" : "with the arena at its hard bound");
            plan->begun = false;
            int e2 = regroup_same(*plan);                             // (rh_grow / overflowed: the planner sizes the arena anew)
            if (e2) return e2;
            arena_retries++;
            attempt = -1;                                             // (both attempts again)
            Ap = nullptr; Ai = nullptr;
            continue;
        }
        if (e && plan->early_end_failed) {
            // a front had rows left at its last scheduled panel: once more with every panel scheduled (and from now on)
            plan->early_end_failed = false;
            plan->full_schedule = true;
            if (g_opt.verbose) fprintf(stderr, "[stmmqr_hip] a front outlived its schedule (rank-deficient fronts): factorizing again on the full schedule\n");
            plan->begun = false;
            int e2 = regroup_same(*plan);
            if (e2) return e2;
            reschedules++;
            attempt = -1;
            Ap = nullptr; Ai = nullptr;
            continue;
        }
        const bool retry = e && plan->panel_wait_failed && attempt == 0;
        plan->serial_panels = false;
        if (!retry) return e;
        if (g_opt.verbose) fprintf(stderr, "[stmmqr_hip] a panel wait ran out: factorizing again with one-workgroup panels\n");
        if (stats && detail) stats->nlaunch = -1;
        Ap = nullptr; Ai = nullptr;                  // (the pattern is set; begin uploads / copies the values again)
    }
    return fail(STMMQR_ERR_DEVICE, "panel kernels failed twice");
}

int stmmqr_plan_set_early_end(stmmqr_plan *plan, int mode)
{
    if (!plan) return fail(STMMQR_ERR_INVALID, "null plan");
    stmmqr_plan &P = *plan;
    if (P.begun && !P.early_end_failed) return fail(STMMQR_ERR_INVALID, "stmmqr_plan_set_early_end between factorize_begin and factorize_finish");
    P.begun = false;
    P.early_end_failed = false;
    P.early_phased = (mode != 0);
    P.full_schedule = (mode == 0);
    return regroup_same(P);
}

// ---- multi-GPU support: regroup the fronts, move contribution blocks in and out of a plan --------------
int stmmqr_plan_set_groups(stmmqr_plan *plan, const int *group)
{
    if (!plan || !group) return fail(STMMQR_ERR_INVALID, "null plan / groups");
    stmmqr_plan &P = *plan;
    if (!P.keep_h)                                           // (the plan's own rebuilds pass group 0 for every front)
        for (long f = 0; f < P.nf; f++)
            if (group[f] != 0)
                return fail(STMMQR_ERR_INVALID, "a plan without H (keepH = 0) takes one group only: no sharded R-only factorization");
    HIPCHK(hipSetDevice(P.device));
    // validate BEFORE anything of the plan changes: a refused call leaves groups and schedule as they were
    auto gid = [&](long f) { return group[f] < 0 ? -1 : (group[f] & ~STMMQR_GROUP_SHARED); };
    for (long f = 0; f < P.nf; f++)
        for (long q = P.Childp[f]; q < P.Childp[f + 1]; q++)
            if (gid(f) >= 0 && gid(P.Child[q]) > gid(f))
                return fail(STMMQR_ERR_INVALID, "a child is scheduled in a later phase than its parent");
    {
        // a shared front is alone in its group and takes the panel-by-panel path
        std::vector<int> cnt, nsh;
        for (long f = 0; f < P.nf; f++) {
            const int g = gid(f);
            if (g < 0) continue;
            if (g >= (1 << 24)) return fail(STMMQR_ERR_INVALID, "group id out of range");
            if ((size_t)g >= cnt.size()) { cnt.resize((size_t)g + 1, 0); nsh.resize((size_t)g + 1, 0); }
            cnt[(size_t)g]++;
            if (group[f] & STMMQR_GROUP_SHARED) {
                nsh[(size_t)g]++;
                if (!(P.fs[f].fn >= g_opt.big_front_cols && P.fs[f].fm_ub >= 64))
                    return fail(STMMQR_ERR_INVALID, "a shared front must be one of the large fronts (options.big_front_cols)");
            }
        }
        for (size_t g = 0; g < cnt.size(); g++)
            if (nsh[g] > 0 && cnt[g] != 1) return fail(STMMQR_ERR_INVALID, "a shared front must be alone in its group");
    }
    if (P.begun) return fail(STMMQR_ERR_INVALID, "stmmqr_plan_set_groups between factorize_begin and factorize_finish");
    HIPCHK(hipStreamSynchronize(P.stream));
    P.shared.assign((size_t)std::max(1L, P.nf), 0);
    for (long f = 0; f < P.nf; f++) {
        P.group[f] = gid(f);
        P.shared[(size_t)f] = (group[f] >= 0 && (group[f] & STMMQR_GROUP_SHARED)) ? 1 : 0;
    }
    // a captured schedule describes the old step lists and workspaces
    if (P.graph_exec) { (void)hipGraphExecDestroy(P.graph_exec); P.graph_exec = nullptr; }
    P.graph_nlaunch = 0;
    stm_assign_arenas(P);                                        // (the arenas follow at the next stmmqr_factorize_begin)
    P.factored = false;                                      // (the factors of the old grouping live at the old offsets)
    std::vector<int> tslot;
    stm_build_schedule(P, tslot);                                // (a plan that holds the whole tree again recycles its slabs: new offsets)
    LCHK(P.d_fs.upload(P.fs, P.stream));
    LCHK(stm_upload_recycle(P));
    // workspaces only grow (a regrouping of the same tree usually needs what it needed before)
    auto grow = [](auto &buf, size_t n) -> int { return buf.n >= n && buf.p ? 0 : buf.alloc(n); };
    LCHK(grow(P.d_T, (size_t)STM_PD_RING * P.tslots * STM_NB * STM_NB));
    LCHK(grow(P.d_Gp, (size_t)P.tslots * (P.gp_slabs + 1) * STM_NB * STM_NB));
    LCHK(grow(P.d_Wp, (size_t)P.wp_doubles));
    LCHK(grow(P.d_Ypend, (size_t)std::max(1LL, P.yp_doubles)));
    LCHK(P.d_ypoff.upload(P.ypoff, P.stream));
    LCHK(grow(P.d_Wp2, (size_t)std::max(1LL, P.wp2_doubles)));
    P.wcnt_n = std::max(P.wcnt_n, (size_t)(P.wp_doubles / (STM_NB * 32) + 1));
    LCHK(grow(P.d_wcnt, P.wcnt_n));
    LCHK(grow(P.d_wcnt2, P.wcnt_n));
    LCHK(grow(P.d_wflag, P.wcnt_n));
    if (!P.d_abort.p) LCHK(P.d_abort.alloc(4));
    LCHK(grow(P.d_wflag2, P.wcnt_n));
    HIPCHK(hipMemset(P.d_wcnt.p, 0, P.wcnt_n * sizeof(int)));
    HIPCHK(hipMemset(P.d_wcnt2.p, 0, P.wcnt_n * sizeof(int)));
    LCHK(P.d_tslot.upload(tslot, P.stream));
    LCHK(P.d_lists.upload(P.lists, P.stream));
    LCHK(P.d_wlists.upload(P.wlists, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    return 0;
}

// Does front f have a contribution-block slot on this plan, allocated, that holds `csize` doubles?  A front that is neither
// factorized here nor a child of a front that is has NO slot (its coff is 0: the first resident block's), and the arenas exist
// only between the first stmmqr_factorize_begin after a (re)grouping and the next regrouping.
int stm_check_c_slot(const stmmqr_plan &P, stm_long f, long long csize, const char *what)
{
    if (f < 0 || f >= P.nf) return fail(STMMQR_ERR_INVALID, std::string(what) + ": no such front");
    if (P.recycle)
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": this plan holds the whole tree and recycles its contribution blocks "
                                        "(nothing to exchange; regroup with stmmqr_plan_set_groups first)");
    if ((size_t)f >= P.has_c.size() || !P.has_c[(size_t)f])
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": the front has no contribution-block slot on this plan (it is neither "
                                        "factorized here nor a child of a front that is)");
    if (!P.d_C.p || P.d_C.n != (size_t)P.carena)
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": the arenas of the current grouping are not allocated yet "
                                        "(stmmqr_factorize_begin comes first)");
    if (csize < 0 || csize > P.c_slot[(size_t)f])
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": the block exceeds the front's slot");
    return 0;
}

int stmmqr_plan_download(stmmqr_plan *plan, double *Stack, stm_long *Rblock_off, char *Rdead, stm_long *HStair,
                         double *HTau, stm_long *Hii, stm_long *HPinv, stm_long *Hm, stm_long *Hr,
                         stm_long *scalars, stmmqr_stats *stats)
{
    if (!plan || !plan->factored) return fail(STMMQR_ERR_INVALID, "no factorization held by the plan");
    stmmqr_plan &P = *plan;
    HIPCHK(hipSetDevice(P.device));
    hipStream_t st = P.stream;
    const long nf = P.nf, m = P.m, n = P.n;
    HIPCHK(hipEventRecord(P.ev[6], st));
    if (Stack && P.rh_total > 0 && P.recycle) {
        // slab recycling: the blocks lie in the arena in the order the fronts finished (kept fronts: still in front form); the
        // reference's layout is produced window by window in a bounce buffer (k_rh_window) and copied out, two windows in flight
        const long long win = std::min<long long>(P.rh_total, 32LL << 20);            // 256 MB windows
        if (P.d_bounce.n < (size_t)(2 * win)) LCHK(P.d_bounce.alloc((size_t)(2 * win)));
        const DevCtx c = P.ctx();
        const int parts = (int)std::min<long long>(64, std::max<long long>(1, win / (64 * 1024)));
        hipEvent_t evw[2] = {nullptr, nullptr};
        for (auto &e : evw) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        int rc = 0;
        for (long long w0 = 0, i = 0; w0 < P.rh_total && !rc; w0 += win, i++) {
            const long long w1 = std::min(P.rh_total, w0 + win);
            double *out = P.d_bounce.p + (i & 1) * win;
            if (i >= 2 && hipEventSynchronize(evw[i & 1]) != hipSuccess) rc = 1;       // (the copy that last read this half is done)
            if (!rc && (P.keep_h ? stm_launch_rh_window(c, P.d_lists.p + P.own_off, P.n_own, parts, P.d_fin.p, P.d_kept.p, P.d_RH.p, w0, w1, out, st)
                                 : stm_launch_r_window(c, P.d_lists.p + P.own_off, P.n_own, parts, P.d_fin.p, P.d_kept.p, P.d_RH.p, w0, w1, out, st)))
                rc = 1;
            if (!rc && hipMemcpyAsync(Stack + w0, out, (size_t)(w1 - w0) * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) rc = 1;
            if (!rc && hipEventRecord(evw[i & 1], st) != hipSuccess) rc = 1;
        }
        if (hipStreamSynchronize(st) != hipSuccess) rc = 1;
        for (auto &e : evw) (void)hipEventDestroy(e);
        if (rc) return fail(STMMQR_ERR_DEVICE, "download of the packed factors failed");
    } else if (Stack && P.rh_total > 0)
        HIPCHK(hipMemcpyAsync(Stack, P.d_RH.p, (size_t)P.rh_total * sizeof(double), hipMemcpyDeviceToHost, st));
    std::vector<int> stair32((size_t)std::max(1L, P.rjsize)), hii32((size_t)std::max(1L, P.hisize));
    std::vector<long long> rboff((size_t)std::max(1L, nf));
    if (P.rjsize > 0)
        HIPCHK(hipMemcpyAsync(stair32.data(), P.d_Stair.p, (size_t)P.rjsize * sizeof(int), hipMemcpyDeviceToHost, st));
    if (P.hisize > 0)
        HIPCHK(hipMemcpyAsync(hii32.data(), P.d_Hii.p, (size_t)P.hisize * sizeof(int), hipMemcpyDeviceToHost, st));
    if (HTau && P.rjsize > 0)
        HIPCHK(hipMemcpyAsync(HTau, P.d_Tau.p, (size_t)P.rjsize * sizeof(double), hipMemcpyDeviceToHost, st));
    if (Rdead && n > 0) HIPCHK(hipMemcpyAsync(Rdead, P.d_Rdead.p, (size_t)n, hipMemcpyDeviceToHost, st));
    if (nf > 0)
        HIPCHK(hipMemcpyAsync(rboff.data(), P.recycle ? P.d_fin.p : P.d_Rboff.p, (size_t)nf * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(P.ev[7], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, P.ev[6], P.ev[7]));
    P.stats.ms_d2h = ms;

    const double t0 = now_ms();
    if (HStair) for (long i = 0; i < P.rjsize; i++) HStair[i] = stair32[i];
    if (Rblock_off) for (long f = 0; f < nf; f++) Rblock_off[f] = (stm_long)rboff[f];
    long maxfrank = 1, maxfm = 0, rank = 0;
    bool all_here = true;
    for (long f = 0; f < nf; f++) {
        const FrontNum &nm = P.h_fnum[f];
        const bool own = P.group[f] >= 0;
        all_here = all_here && own;
        if (Hm) Hm[f] = own ? nm.fm : 0;
        if (Hr) Hr[f] = own ? nm.rank : 0;
        if (!own) continue;
        maxfrank = std::max(maxfrank, (long)nm.rank);
        maxfm = std::max(maxfm, (long)nm.fm);
        rank += nm.rank;
    }
    if (!P.keep_h) { Hii = nullptr; HPinv = nullptr; }        // (R only: no qr_hpinv, SparseQR_factorize.c:717)
    if (!all_here) {
        // sharded run: the caller merges the shards and runs qr_hpinv on the union; Hii stays in S-row ids
        if (Hii)
            for (long f = 0; f < nf; f++)
                if (P.group[f] >= 0)
                    for (long i = 0; i < P.h_fnum[f].fm; i++) Hii[P.Hip[f] + i] = hii32[P.Hip[f] + i];
        Hii = nullptr; HPinv = nullptr;
    }
    // qr_hpinv (SparseQR_factorize.c:991-1060): global row permutation, Hii rewritten in place
    if (Hii || HPinv) {
        std::vector<long> W((size_t)std::max(1L, m), 0);
        long row1 = 0, row2 = m;
        for (long i = P.Sleft[n]; i < m; i++) W[i] = --row2;
        for (long f = 0; f < nf; f++) {
            const int *Hi = hii32.data() + P.Hip[f];
            const FrontNum &nm = P.h_fnum[f];
            const long rm = nm.rank, fm = nm.fm;
            for (long i = 0; i < rm; i++) W[Hi[i]] = row1++;
            const long cn = P.fs[f].fn - P.fs[f].fp;
            const long cm = std::min(fm - rm, cn);
            for (long i = fm - 1; i >= rm + cm; i--) W[Hi[i]] = --row2;
        }
        if (HPinv) for (long i = 0; i < m; i++) HPinv[i] = W[P.PLinv[i]];
        if (Hii) {
            for (long f = 0; f < nf; f++) {
                const int *Hi = hii32.data() + P.Hip[f];
                stm_long *Ho = Hii + P.Hip[f];
                const long fm = P.h_fnum[f].fm;
                for (long i = 0; i < fm; i++) Ho[i] = W[Hi[i]];
            }
        }
    }
    if (scalars) {
        scalars[0] = rank;
        long rank1 = rank;
        if (P.last_ntol < n) {
            std::vector<char> rd((size_t)std::max(1L, n));
            if (Rdead) memcpy(rd.data(), Rdead, (size_t)n);
            else HIPCHK(hipMemcpy(rd.data(), P.d_Rdead.p, (size_t)n, hipMemcpyDeviceToHost));
            rank1 = 0;
            for (long j = 0; j < P.last_ntol; j++) rank1 += !rd[j];
        }
        scalars[1] = rank1; scalars[2] = maxfrank; scalars[3] = maxfm;
    }
    P.stats.ms_host += now_ms() - t0;
    if (stats) *stats = P.stats;
    return 0;
}

int stmmqr_factorize_arrays(const stmmqr_symbolic_view *sym, const stm_long *Ap, const stm_long *Ai,
                            const double *Ax, double tol, stm_long ntol, double *Stack, stm_long stack_cap,
                            stm_long *Rblock_off, char *Rdead, stm_long *HStair, double *HTau, stm_long *Hii,
                            stm_long *HPinv, stm_long *Hm, stm_long *Hr, stm_long *scalars, stmmqr_stats *stats)
{
    int st = 0;
    stmmqr_plan *P = stmmqr_plan_create(sym, -1, &st);
    if (!P) return st;
    st = stmmqr_factorize_device(P, Ap, Ai, Ax, 0, tol, ntol, stats);
    if (!st && Stack && P->rh_total > stack_cap) st = fail(STMMQR_ERR_INVALID, "Stack buffer too small");
    if (!st) st = stmmqr_plan_download(P, Stack, Rblock_off, Rdead, HStair, HTau, Hii, HPinv, Hm, Hr, scalars, stats);
    stmmqr_plan_destroy(P);
    return st;
}

}  // extern "C"
