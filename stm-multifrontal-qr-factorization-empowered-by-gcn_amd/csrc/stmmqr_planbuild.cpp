// stmmqr_planbuild.cpp -- everything of a plan that depends only on the symbolic analysis and the pattern of A: build_plan (sizes,
// relative indices, the estimate of the packed factors, the first schedule and the plan's device memory), the S -> A map of a
// pattern, plan create / destroy, the regrouping of the fronts (stmmqr_plan_set_groups) and the index of A for the products with A.
//
// Reference counterparts (paths relative to /root/reference/STMMQR):
//   stmmqr_plan_create      the allocation / setup half of qr_factorize   src/qr/SparseQR_factorize.c:222-498
#include "stmmqr_plan.h"

namespace {

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

}  // namespace

// qr_stranspose2 as a symbolic map: smap[s] = p such that Sx[s] = Ax[p]  (SparseQR_factorize.c:755-785)
int stm_set_pattern(stmmqr_plan &P, const stm_long *Ap, const stm_long *Ai)
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

extern "C" {

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
    return stm_set_pattern(*plan, Ap, Ai);
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

}  // extern "C"
