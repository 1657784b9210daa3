// stmmqr_rfactor.cpp -- SURVEY.md 8 (f1): QR_qmult / QR_solve on the factors resident in HBM (host side; kernels: stmmqr_resident.hip).
#include "stmmqr_plan.h"
#include <climits>
#include <memory>

// ---------------------------------------------------------------------------------------------
// QR_qmult (SparseQR.c:1790-2020, methods QR_QTX / QR_QX) and QR_solve (RETX_EQUALS_B, :2024-2216)
// on the factors that are still in HBM -- no download of the packed R+H.
// ---------------------------------------------------------------------------------------------
namespace {
// a callee's own refusal goes up as it is (LCHK is for HIP error codes and would re-label it)

// Slab recycling: the resident-factor kernels read fronts in front form.  A front whose slab was recycled is put back into
// that form, level by level, in a scratch that holds the widest tree level (res_ctx: the FrontSym array whose offsets point into
// the scratch; level_to_front_form: zeros + the inverse of k_rh_copy for the level's fronts).  Kept fronts are read where they are
// (their offset is taken relative to the scratch's base: one flat device address space).
// The FrontSym array those kernels read (host copy): fs, or with recycling fs_scr with the kept fronts rebased
std::vector<FrontSym> resident_front_syms(const stmmqr_plan &P)
{
    if (!P.recycle) return P.fs;
    std::vector<FrontSym> t = P.fs_scr;
    for (long f = 0; f < P.nf; f++)
        if (P.kept[(size_t)f]) t[(size_t)f].foff = (long long)((P.d_F.p + P.fs[f].foff) - P.d_scr.p);
    return t;
}
// ... and who may cut that array back to a view that ends at column ncol of a plan of [A B] (the carried solve, the covariance): the
// columns of A were rank-tested, those of B were not and sit where they were given
int check_carried_view(const stmmqr_plan &P, long ncol)
{
    if (P.last_ntol != ncol)
        return fail(STMMQR_ERR_INVALID, "carried solve: the factorization was made with ntol = " + std::to_string(P.last_ntol) + ", not n = " +
                                            std::to_string(ncol) + " (the columns of B must not be rank-tested, those of A must)");
    if (P.has_qfill)
        for (long j = ncol; j < P.n; j++)
            if (P.Qfill[(size_t)j] != j)
                return fail(STMMQR_ERR_INVALID, "carried solve: column " + std::to_string(j) + " of [A B] is permuted (Qfill must be the identity on the B columns)");
    return 0;
}
int ensure_scratch(stmmqr_plan &P)
{
    if (!P.recycle || (P.d_scr.p && P.d_fs_scr.p)) return 0;
    // Two layouts.  Where HBM has room (all recycled slabs within a quarter of what is free; STMMQR_RESIDENT_CACHE=0 / 1 forces) the
    // scratch holds EVERY front in front form, rebuilt once per factorization at the first Q-apply / solve and kept for the
    // following ones: the memory comes back only while the factors are being used, never during the factorization.  Otherwise it
    // holds the widest tree level and every level is rebuilt whenever a kernel walks it.
    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    long long all = 0;
    for (long f = 0; f < P.nf; f++) if (!P.kept[(size_t)f]) all += (long long)P.fs[f].ld * P.fs[f].fn;
    const long cache = knobs::num(knobs::K_RESIDENT_CACHE);
    P.scr_all = cache >= 0 ? cache != 0 : (8.0 * (double)all <= 0.25 * (double)freeb);
    if (P.scr_all) {
        long long o = 0;
        for (long f = 0; f < P.nf; f++)
            if (!P.kept[(size_t)f]) { P.fs_scr[(size_t)f].foff = o; o += (long long)P.fs[f].ld * P.fs[f].fn; }
    }
    P.scr_valid = false;
    P.t4_valid = false;
    LCHK(P.d_scr.alloc((size_t)std::max(1LL, P.scr_all ? all : P.scr_doubles)));
    LCHK(P.d_fs_scr.upload(resident_front_syms(P), P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    return 0;
}
DevCtx res_ctx(stmmqr_plan &P)
{
    DevCtx c = P.ctx();
    if (P.recycle) { c.fs = P.d_fs_scr.p; c.Farena = P.d_scr.p; }
    return c;
}
// staged blocks back in front form: R+H by k_rh_unpack, R only (keepH = 0) by k_rh_unpack's zero fill + k_r_unpack
int unpack_fronts(stmmqr_plan &P, const DevCtx &c, const int *flist, int nfr)
{
    if (P.keep_h) return stm_launch_rh_unpack(c, P.d_fs_scr.p, flist, nfr, 64, P.d_kept.p, P.d_RH.p, P.d_scr.p, P.stream);
    return stm_launch_r_unpack(c, flist, nfr, 64, P.d_kept.p, P.d_RH.p, P.d_fs_scr.p, P.d_scr.p, P.stream);
}
int level_to_front_form(stmmqr_plan &P, size_t l)
{
    if (!P.recycle) return 0;
    const auto &LV = P.glevels[0];
    const DevCtx c = P.ctx();
    if (P.scr_all) {
        if (P.scr_valid) return 0;
        // every front at once, kept until the next factorization (marked valid only once the launch was accepted)
        const int e = unpack_fronts(P, c, P.d_lists.p + P.own_off, P.n_own);
        P.scr_valid = (e == 0);
        return e;
    }
    if (LV[l].n_all <= 0) return 0;
    return unpack_fronts(P, c, P.d_lists.p + LV[l].all_off, LV[l].n_all);
}

// Of THIS factorization: the host half of qr_hpinv for the device, Wmap[S-row id] = position in the permuted row order (same rule as
// in stmmqr_plan_download), the rows of R above every front, and the host copy of the fronts' numeric results
int map_rows_of_factorization(stmmqr_plan &P)
{
    hipStream_t st = P.stream;
    const long nf = P.nf, m = P.m, n = P.n;
    std::vector<int> hii32((size_t)std::max(1L, P.hisize));
    if (P.hisize > 0)
        HIPCHK(hipMemcpyAsync(hii32.data(), P.d_Hii.p, (size_t)P.hisize * sizeof(int), hipMemcpyDeviceToHost, st));
    if (P.h_fnum.size() != (size_t)nf) P.h_fnum.resize((size_t)nf);
    if (nf > 0)
        HIPCHK(hipMemcpyAsync(P.h_fnum.data(), P.d_fnum.p, (size_t)nf * sizeof(FrontNum), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int> W((size_t)std::max(1L, m), 0);
    long row1 = 0, row2 = m;
    for (long i = P.Sleft[n]; i < m; i++) W[i] = (int)--row2;
    for (long f = 0; f < nf; f++) {
        const int *Hi = hii32.data() + P.Hip[f];
        const FrontNum &nm = P.h_fnum[f];
        const long rm = nm.rank, fm = nm.fm;
        for (long i = 0; i < rm; i++) W[Hi[i]] = (int)row1++;
        const long cn = P.fs[f].fn - P.fs[f].fp;
        const long cm = std::min(fm - rm, cn);
        for (long i = fm - 1; i >= rm + cm; i--) W[Hi[i]] = (int)--row2;
    }
    LCHK(P.d_Wmap.upload(W, st));
    std::vector<int> rb((size_t)std::max(1L, nf), 0);
    long run = 0;
    for (long f = 0; f < nf; f++) { rb[f] = (int)run; run += P.h_fnum[f].rank; }
    LCHK(P.d_rowbase.upload(rb, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// Once per plan: the static integer maps, the work vectors for one right-hand side, the dynamic LDS of every tree level's launches
// (stm_lds_*, stmmqr_device.h), the descriptors of the split fronts and the bookkeeping of their grouped Q-apply (T4)
int build_resident_tables(stmmqr_plan &P)
{
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    std::vector<int> t((size_t)std::max(1L, P.rjsize));
    for (long i = 0; i < P.rjsize; i++) t[i] = (int)P.Rj[i];
    LCHK(P.d_Rj.upload(t, st));
    HIPCHK(hipStreamSynchronize(st));
    t.assign((size_t)std::max(1L, m), 0);
    for (long i = 0; i < m; i++) t[i] = (int)P.PLinv[i];
    LCHK(P.d_PLinv.upload(t, st));
    HIPCHK(hipStreamSynchronize(st));
    if (P.has_qfill) {
        t.assign((size_t)std::max(1L, n), 0);
        for (long j = 0; j < n; j++) t[j] = (int)P.Qfill[j];
        LCHK(P.d_Qfill.upload(t, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    LCHK(P.d_W.alloc((size_t)std::max(1L, m)));
    LCHK(P.d_Xs.alloc((size_t)std::max(1L, n)));
    LCHK(P.d_Io.alloc((size_t)std::max(1L, std::max(m, n))));
    LCHK(P.d_err.alloc(1));
    const auto &LV = P.glevels[0];
    P.level_lds_qa.assign(LV.size(), 0);
    P.level_lds_qa_all.assign(LV.size(), 0);
    P.level_lds_rs.assign(LV.size(), 0);
    P.level_lds_rt.assign(LV.size(), 0);
    P.level_qbig.assign(LV.size(), stmmqr_plan::QbLevel());
    P.level_rtbig.assign(LV.size(), stmmqr_plan::RtLevel());
    P.h_rtb.clear(); P.rtlc_ints = 1;
    P.t4items.clear(); P.t4fronts.clear(); P.t4dqo.clear(); P.qbt4off.clear();
    P.t4_doubles = 0; P.dq4_ints = 0; P.t4_ok = false; P.t4_tried = false; P.t4_valid = false;
    std::vector<QbDesc> qb;
    long xf = 1, dq = 1, wq = 1;
    for (size_t l = 0; l < LV.size(); l++) {
        long xo = 0, dqo = 0, wo = 0, lco = 0;
        P.level_qbig[l].off = (int)qb.size();
        P.level_rtbig[l].off = (int)P.h_rtb.size();
        P.level_qbig[l].t4i_off = (int)P.t4items.size();
        for (int q = 0; q < LV[l].n_all; q++) {
            const int f = P.lists[LV[l].all_off + q];
            const FrontSym &s = P.fs[f];
            const int need = (int)std::min(stm_lds_qapply(s.fm_ub, s.fn), (long)INT_MAX);
            P.level_lds_rt[l] = std::max(P.level_lds_rt[l], (int)std::min(stm_lds_rtsolve(s.fp, s.fm_ub, s.fn), (long)INT_MAX));
            P.level_lds_qa_all[l] = std::max(P.level_lds_qa_all[l], need);
            if (s.rtbig) {
                auto &T = P.level_rtbig[l];
                RtDesc d;
                d.f = f; d.lcoff = (int)lco;
                P.h_rtb.push_back(d);
                lco += s.fp;
                const int rmax = std::min(s.fp, s.fm_ub);
                T.n++; T.max_steps = std::max(T.max_steps, (rmax + 31) / 32);
                T.max_nslab = std::max(T.max_nslab, std::max(1, (rmax + s.fn - s.fp + STM_RTB_COLS - 1) / STM_RTB_COLS));
            } else {
                P.level_rtbig[l].lds_small = std::max(P.level_rtbig[l].lds_small, (int)stm_lds_rtsolve(s.fp, s.fm_ub, s.fn));
            }
            if (s.qbig) {
                QbDesc d;
                d.f = f; d.xoff = (int)xo; d.dqoff = (int)dqo; d.wqoff = (int)wo; d.nslab = (s.fm_ub + STM_QB_ROWS - 1) / STM_QB_ROWS; d.np_live = s.npanels;
                qb.push_back(d);
                const int ngr = (s.npanels + 3) / 4;
                P.qbt4off.push_back(P.t4_doubles);
                P.t4fronts.push_back(f);
                P.t4dqo.push_back(P.dq4_ints);
                for (int g = 0; g < ngr; g++) {
                    Qt4ItemHost it;
                    it.f = f; it.g = g; it.off = P.t4_doubles + (long long)g * stm_qt4_doubles(); it.dqo = P.dq4_ints;
                    P.t4items.push_back(it);
                }
                P.t4_doubles += (long long)ngr * stm_qt4_doubles();
                P.dq4_ints += s.fn;
                xo += s.fm_ub; dqo += s.fn; wo += 2L * d.nslab * STM_NB;
                auto &Q = P.level_qbig[l];
                Q.n++; Q.max_np = std::max(Q.max_np, s.npanels); Q.max_nslab = std::max(Q.max_nslab, d.nslab);
                Q.max_fm = std::max(Q.max_fm, s.fm_ub);
                Q.max_rsteps = std::max(Q.max_rsteps, (std::min(s.fp, s.fm_ub) + 31) / 32);
            } else {
                P.level_lds_qa[l] = std::max(P.level_lds_qa[l], need);
                P.level_lds_rs[l] = std::max(P.level_lds_rs[l], (int)std::min(stm_lds_rsolve(s.fp, s.fn), (long)INT_MAX));
            }
        }
        P.level_qbig[l].t4i_n = (int)P.t4items.size() - P.level_qbig[l].t4i_off;
        xf = std::max(xf, xo); dq = std::max(dq, dqo); wq = std::max(wq, wo);
        P.rtlc_ints = std::max(P.rtlc_ints, (long long)lco);
    }
    LCHK(P.d_Xf.alloc((size_t)xf));
    LCHK(P.d_Dq.alloc((size_t)dq));
    LCHK(P.d_Wq.alloc((size_t)wq));
    P.wq4_doubles = 4 * wq;
    P.xf_doubles = xf; P.wq_doubles = wq; P.rhs_cap = 1;
    P.d_U.release(); P.d_Xr.release(); P.d_rtLc.release(); P.d_rtRm.release();
    if (!P.h_rtb.empty()) LCHK(P.d_rtb.upload(P.h_rtb, st));
    if (qb.empty()) qb.push_back(QbDesc());
    LCHK(P.d_qb.alloc(qb.size()));
    LCHK(P.d_Rm.alloc(qb.size()));
    HIPCHK(hipMemcpy(P.d_qb.p, qb.data(), qb.size() * sizeof(QbDesc), hipMemcpyHostToDevice));
    P.h_qb = qb;
    return 0;
}

// Of THIS factorization: the panels of a split front that can hold a live reflector and the blocks of live pivot columns.  A
// front of fm rows has fm live reflectors at most; they sit in its first fm + (dead pivot columns) columns, and a front has at
// most fp - rank dead pivot columns.  The panels behind that column were launches that did nothing: on the default workload
// 330 launches per Q'b, 177 of them for panels without a reflector (same finding as the factorization's own schedule,
// stmmqr_schedule.cpp "how many panels").  STMMQR_LIVE_PANELS=0: every panel.
int count_live_panels(stmmqr_plan &P)
{
    const bool live = knobs::on(knobs::K_LIVE_PANELS);
    bool changed = false;
    for (size_t l = 0; l < P.level_qbig.size(); l++) {
        auto &Q = P.level_qbig[l];
        Q.live_np = 0; Q.live_rsteps = 0;
        for (int q = 0; q < Q.n; q++) {
            QbDesc &d = P.h_qb[(size_t)(Q.off + q)];
            const FrontSym &s = P.fs[d.f];
            const FrontNum &nm = P.h_fnum[d.f];
            int npl = s.npanels;
            if (live) {
                const long lastcol = std::min((long)s.fn, (long)nm.fm + std::max(0L, (long)s.fp - (long)nm.rank));
                npl = (nm.fm <= 0) ? 0 : (int)std::min((long)s.npanels, (lastcol - 1) / STM_NB + 1);
            }
            if (d.np_live != npl) { d.np_live = npl; changed = true; }
            Q.live_np = std::max(Q.live_np, npl);
            Q.live_rsteps = std::max(Q.live_rsteps, live ? (int)((nm.rank + 31) / 32) : Q.max_rsteps);
        }
    }
    for (size_t l = 0; l < P.level_rtbig.size(); l++) {
        auto &T = P.level_rtbig[l];
        T.live_steps = live ? 0 : T.max_steps;
        for (int q = 0; q < T.n && live; q++) T.live_steps = std::max(T.live_steps, (int)((P.h_fnum[P.h_rtb[(size_t)(T.off + q)].f].rank + 31) / 32));
    }
    if (changed && !P.h_qb.empty()) HIPCHK(hipMemcpy(P.d_qb.p, P.h_qb.data(), P.h_qb.size() * sizeof(QbDesc), hipMemcpyHostToDevice));
    return 0;
}

// what every resident-factor operation needs of the plan and of the factorization it holds, built at the first one after a factorization
int ensure_rowmap(stmmqr_plan &P)
{
    LCHK(ensure_scratch(P));
    if (P.rowmap_ready) return 0;
    for (long f = 0; f < P.nf; f++)
        if (P.group[f] < 0) return fail(STMMQR_ERR_INVALID, "Q-apply / solve need every front on this device");
    PASS(map_rows_of_factorization(P));
    if (!P.d_Rj.p) PASS(build_resident_tables(P));
    PASS(count_live_panels(P));
    // (the planner sends such fronts to the split kernels, so neither can happen; no launch may ask for more LDS than configured)
    for (int b : P.level_lds_qa)
        if (b > STM_RES_LDS_MAX) return fail(STMMQR_ERR_TOO_LARGE, "a front has more rows than the Q-apply kernel holds in LDS");
    for (int b : P.level_lds_rs)
        if (b > STM_RES_LDS_MAX) return fail(STMMQR_ERR_TOO_LARGE, "a front has more columns than the back-substitution kernel holds in LDS");
    P.rowmap_ready = true;
    return 0;
}

// How every entry point starts and ends: the refusal that comes before it looks at its other arguments; once they are accepted, the
// plan's device and the maps of the factorization held; and, where it cleared the kernels' error word d_err on its way (the Q-apply
// alone does not), the check of that word, which synchronizes the stream.
int check_factored(const stmmqr_plan *plan) { return (plan && plan->factored) ? 0 : fail(STMMQR_ERR_INVALID, "no factorization held by the plan"); }
int begin_resident_op(stmmqr_plan &P) { HIPCHK(hipSetDevice(P.device)); LCHK(ensure_rowmap(P)); return 0; }
int end_resident_op(stmmqr_plan &P)
{
    int e = 0;
    HIPCHK(hipMemcpyAsync(&e, P.d_err.p, sizeof(int), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    if (e) return fail(STMMQR_ERR_INVALID, "internal: live pivot count of a front differs from its rank");
    return 0;
}

// the per-vector buffers of the resident-factor operations for a batch of nb right-hand sides (grown on demand, never shrunk)
int ensure_rhs_batch(stmmqr_plan &P, int nb)
{
    if (nb <= P.rhs_cap) return 0;
    const size_t k = (size_t)nb;
    LCHK(P.d_W.alloc(k * (size_t)std::max(1L, P.m)));
    LCHK(P.d_Xs.alloc(k * (size_t)std::max(1L, P.n)));
    LCHK(P.d_Xf.alloc(k * (size_t)P.xf_doubles));
    LCHK(P.d_Wq.alloc(k * (size_t)P.wq_doubles));
    if (P.d_Wq4.p) LCHK(P.d_Wq4.alloc(k * (size_t)std::max(1LL, P.wq4_doubles)));
    if (P.d_U.p) { LCHK(P.d_U.alloc(k * (size_t)std::max(1L, P.rjsize))); LCHK(P.d_Xr.alloc(k * (size_t)std::max(1L, P.m))); }
    P.rhs_cap = nb;
    return 0;
}
RhsBatch rhs_strides(const stmmqr_plan &P)
{
    RhsBatch B;
    B.w = P.m; B.x = P.n; B.xf = P.xf_doubles; B.wq = P.wq_doubles; B.wq4 = std::max(1LL, P.wq4_doubles); B.u = std::max(1L, P.rjsize);
    return B;
}
// the largest batch the operations take in one pass (STMMQR_RHS_BATCH; 1: one vector after the other, as until round 4)
int rhs_batch_max() { return (int)knobs::once<knobs::K_RHS_BATCH>(); }
// op(j0, nb) for the right-hand sides j0 .. j0 + nb - 1, batch after batch: every launch of a pass over the tree carries a whole batch
// (RhsBatch), and the per-vector buffers hold it before op runs
template <class Op> int for_each_batch(stmmqr_plan &P, stm_long nrhs, Op op)
{
    for (stm_long j0 = 0; j0 < nrhs; j0 += rhs_batch_max()) {
        const int nb = (int)std::min<stm_long>(rhs_batch_max(), nrhs - j0);
        LCHK(ensure_rhs_batch(P, nb));
        PASS(op(j0, nb));
    }
    return 0;
}

// W (device, S-row order; nb vectors at stride m) <- Q' W or Q W
int run_qapply(stmmqr_plan &P, int method, int nb = 1)
{
    const RhsBatch B = rhs_strides(P);
    DevCtx c = res_ctx(P);
    const int *L0 = P.d_lists.p;
    const auto &LV = P.glevels[0];
    // blocked form with the kept T factors; STMMQR_DBG bit 13 selects the reflector-by-reflector kernel (same result up
    // to rounding: used by the tests to cross-check the two)
    const bool blocked = c.Tall && !(c.dbg & 8192);
    // grouped split Q-apply: its buffers at the first use (STMMQR_QT4=0: the per-panel launches)
    const bool want_t4 = knobs::on(knobs::K_QT4);                                          // (read at every call: tests compare both)
    if (blocked && want_t4 && !P.t4_tried && !P.t4items.empty()) {
        P.t4_tried = true;
        size_t freeb = 0, totalb = 0;
        if (hipMemGetInfo(&freeb, &totalb) == hipSuccess &&
            8.0 * ((double)P.t4_doubles + (double)P.wq4_doubles) + 4.0 * (double)P.dq4_ints < 0.25 * (double)freeb) {
            LCHK(P.d_T4.alloc((size_t)P.t4_doubles));
            LCHK(P.d_Wq4.alloc((size_t)P.rhs_cap * (size_t)std::max(1LL, P.wq4_doubles)));
            LCHK(P.d_Dq4.alloc((size_t)std::max(1LL, P.dq4_ints)));
            LCHK(P.d_t4items.upload(P.t4items, P.stream));
            LCHK(P.d_t4fronts.upload(P.t4fronts, P.stream));
            LCHK(P.d_t4dqo.upload(P.t4dqo, P.stream));
            LCHK(P.d_qbt4off.upload(P.qbt4off, P.stream));
            P.t4_ok = true;
            P.t4_valid = false;
        }
    }
    const bool use_t4 = blocked && want_t4 && P.t4_ok;
    if (use_t4 && knobs::on(knobs::K_MEMDUMP) && !P.t4_valid)
        fprintf(stderr, "[stmmqr_hip] grouped Q-apply: T4 of %zu groups of %zu split fronts, %.3f GB (+ %.3f GB of slab partials)\n", P.t4items.size(),
                P.t4fronts.size(), 8e-9 * (double)P.t4_doubles, 8e-9 * (double)P.wq4_doubles);
    auto launch = [&](size_t l, int m) -> int {
        LCHK(level_to_front_form(P, l));
        if (blocked) {
            LCHK(stm_launch_qapply_t(c, L0 + LV[l].all_off, LV[l].n_all, m, P.d_W.p, P.level_lds_qa[l], P.stream, nb, B));
            // the large fronts of the level (independent of the others): rows split over workgroups, a launch per group of four panels
            // (k_qbig_step4, T4 built at the first use after a factorization) or per panel
            const auto &Q = P.level_qbig[l];
            if (Q.n > 0 && use_t4) {
                if (!P.t4_valid) { P.t4_level_valid.assign(LV.size(), 0); P.t4_valid = true; }
                if (!P.t4_level_valid[l]) {                          // (the level's fronts are in front form now: level_to_front_form)
                    LCHK(stm_launch_qt4_build(c, P.d_t4fronts.p + Q.off, P.d_t4dqo.p + Q.off, Q.n, P.d_t4items.p + Q.t4i_off, Q.t4i_n, P.d_Dq4.p,
                                              P.d_T4.p, P.stream));
                    P.t4_level_valid[l] = 1;
                }
                LCHK(stm_launch_qapply_big4(c, P.d_qb.p + Q.off, P.d_qbt4off.p + Q.off, Q.n, Q.live_np, Q.max_nslab, Q.max_fm, m, P.d_W.p, P.d_Xf.p,
                                            P.d_Dq.p, P.d_Wq4.p, P.d_T4.p, P.stream, nb, B));
                return 0;
            }
            LCHK(stm_launch_qapply_big(c, P.d_qb.p + Q.off, Q.n, Q.live_np, Q.max_nslab, Q.max_fm, m, P.d_W.p, P.d_Xf.p, P.d_Dq.p,
                                       P.d_Wq.p, P.stream, nb, B));
            return 0;
        }
        if (P.level_lds_qa_all[l] > STM_RES_LDS_MAX) return fail(STMMQR_ERR_TOO_LARGE, "a front has more rows than the unblocked Q-apply kernel holds in LDS");
        for (int j = 0; j < nb; j++)                                  // (the reflector-by-reflector cross-check kernel: one vector per launch)
            LCHK(stm_launch_qapply(c, L0 + LV[l].all_off, LV[l].n_all, m, P.d_W.p + (size_t)j * (size_t)P.m, P.level_lds_qa_all[l], P.d_err.p, P.stream));
        return 0;
    };
    if (method == 0) {
        for (size_t l = 0; l < LV.size(); l++) LCHK(launch(l, 0));
    } else {
        for (size_t l = LV.size(); l-- > 0;) LCHK(launch(l, 1));
    }
    return 0;
}

// rows x cols doubles from one column-major array (leading dimension lds) to another (ldd), host or device by `kind`: one transfer
int copy_cols(double *dst, long ldd, const double *src, long lds, long rows, long cols, hipMemcpyKind kind, hipStream_t st)
{
    if (rows > 0 && cols > 0)
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(double), src, (size_t)lds * sizeof(double), (size_t)rows * sizeof(double), (size_t)cols,
                                kind, st));
    return 0;
}
int grow(DevBuf<double> &d, size_t n) { return (d.p && d.n >= n) ? 0 : d.alloc(std::max<size_t>(n, 1)); }
// ... from the host into a device buffer that holds the columns one after the other and is grown if needed
int upload_cols(DevBuf<double> &d, const double *H, long ld, long rows, long cols, hipStream_t st)
{
    LCHK(grow(d, (size_t)(rows * cols)));
    return copy_cols(d.p, rows, H, ld, rows, cols, hipMemcpyHostToDevice, st);
}
// ... and back out of such a buffer (to the host, or with `kind` to a caller's device array); waits for it
int download_cols(stmmqr_plan &P, const DevBuf<double> &d, double *H, long ld, long rows, long cols, hipMemcpyKind kind = hipMemcpyDeviceToHost)
{
    PASS(copy_cols(H, ld, d.p, rows, rows, cols, kind, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    return 0;
}

// nb vectors (stride m in `in` / `out`, device, the reference's row order) through Q' (method 0) or Q (method 1) in ONE pass over the tree
int qapply_vectors(stmmqr_plan &P, int method, const double *in, double *out, int nb)
{
    const int m = (int)P.m, scatter = method == 0;
    // Q': W[PLinv[i]] = x[i], then out[Wmap[r]] = W[r];  Q: W[r] = x[Wmap[r]], then out[i] = W[PLinv[i]]
    LCHK(stm_launch_perm(in, scatter ? P.d_PLinv.p : P.d_Wmap.p, P.d_W.p, m, scatter, P.stream, nb, m, m));
    LCHK(run_qapply(P, method, nb));
    LCHK(stm_launch_perm(P.d_W.p, scatter ? P.d_Wmap.p : P.d_PLinv.p, out, m, scatter, P.stream, nb, m, m));
    return 0;
}

// The backward pass, R x = y, from the root to the leaves: y in the device work vectors W (internal row order; nb of them at stride
// m) -> d_Xs (R's column order, stride n).  The kernels read the factorization through c; before_level(l), a launch of the caller's
// or nothing (it returns the launcher's code), comes once the level is in front form, before its solves.
template <class Hook> int r_pass(stmmqr_plan &P, const DevCtx &c, int nb, Hook before_level)
{
    const RhsBatch B = rhs_strides(P);
    const int *L0 = P.d_lists.p;
    const auto &LV = P.glevels[0];
    for (size_t l = LV.size(); l-- > 0;) {
        LCHK(level_to_front_form(P, l));
        LCHK(before_level(l));
        LCHK(stm_launch_rsolve(c, L0 + LV[l].all_off, LV[l].n_all, P.d_Rj.p, P.d_W.p, P.d_Xs.p, P.level_lds_rs[l], P.d_err.p, P.stream, nb, B));
        const auto &Q = P.level_qbig[l];         // the large fronts of the level: rows split over workgroups
        LCHK(stm_launch_rsolve_big(c, P.d_qb.p + Q.off, Q.n, Q.live_rsteps, Q.max_nslab, P.d_Rj.p, P.d_W.p, P.d_Xs.p, P.d_Xf.p,
                                   P.d_Dq.p, P.d_Rm.p + Q.off, P.d_err.p, P.stream, nb, B));
    }
    return 0;
}
int rsolve_vector(stmmqr_plan &P, int nb = 1) { return r_pass(P, res_ctx(P), nb, [](size_t) { return 0; }); }
// nb vectors Y (device, stride m, R's row order) -> X (device, stride n) = R \ Y or, through Qfill, E (R \ Y): stmmqr_plan_rsolve 0, 1
int r_vectors(stmmqr_plan &P, const double *Y, double *X, int nb, bool through_qfill)
{
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    LCHK(stm_launch_perm(Y, P.d_Wmap.p, P.d_W.p, (int)m, 0, st, nb, m, m));                                  // W[r] = y[Wmap[r]]
    LCHK(rsolve_vector(P, nb));
    LCHK(stm_launch_perm(P.d_Xs.p, (through_qfill && P.has_qfill) ? P.d_Qfill.p : nullptr, X, (int)n, 1, st, nb, n, n));   // X[Qfill[j]] = x[j]
    return 0;
}

// The forward pass, R' x = b, from the leaves to the root: b in R's column order in d_Xs (nb vectors at stride n) -> d_Xr (R's row
// order, stride m; rows beyond the rank stay zero).  ensure_rt comes before the first batch: it refuses a tree that k_rtsolve cannot
// take and makes the pass's own buffers (U, Xr) at the plan's current batch size, from where ensure_rhs_batch grows them.
int ensure_rt_buffers(stmmqr_plan &P)
{
    if (!P.d_U.p) {
        LCHK(P.d_U.alloc((size_t)P.rhs_cap * (size_t)std::max(1L, P.rjsize)));
        LCHK(P.d_Xr.alloc((size_t)P.rhs_cap * (size_t)std::max(1L, P.m)));
    }
    return 0;
}
int ensure_rt(stmmqr_plan &P)
{
    for (int need : P.level_lds_rt)
        if (need > STM_RES_LDS_MAX) return fail(STMMQR_ERR_TOO_LARGE, "a front is too wide for the one-workgroup R' solve");
    return ensure_rt_buffers(P);
}
int rt_pass(stmmqr_plan &P, int nb)
{
    const RhsBatch B = rhs_strides(P);
    DevCtx c = res_ctx(P);
    const int *L0 = P.d_lists.p;
    const auto &LV = P.glevels[0];
    HIPCHK(hipMemsetAsync(P.d_Xr.p, 0, (size_t)nb * (size_t)std::max(1L, P.m) * sizeof(double), P.stream));
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        LCHK(stm_launch_rtsolve(c, L0 + LV[l].all_off, LV[l].n_all, P.d_Xs.p, P.d_U.p, P.d_Xr.p, P.d_rowbase.p, P.level_lds_rt[l], P.stream, nb, B));
    }
    return 0;
}
// The same pass for a tree with fronts of any width: the fronts with FrontSym::rtbig go through k_rtbig_* (init + a launch per
// block of 32 live pivot columns, all split fronts of a level together), the others through k_rtsolve as above; the fronts of a level
// are independent.  A split front leaves its pass vector where k_rtsolve leaves it, so either kind feeds either kind.  Sets d_err
// on an inconsistent front (end_resident_op).  ensure_rt_any comes before the first batch; it refuses nothing.
int ensure_rt_any(stmmqr_plan &P)
{
    LCHK(ensure_rt_buffers(P));
    if (!P.d_rtLc.p && !P.h_rtb.empty()) {
        LCHK(P.d_rtLc.alloc((size_t)P.rtlc_ints));
        LCHK(P.d_rtRm.alloc(P.h_rtb.size()));
    }
    return 0;
}
int rt_pass_any(stmmqr_plan &P, int nb)
{
    const RhsBatch B = rhs_strides(P);
    DevCtx c = res_ctx(P);
    const int *L0 = P.d_lists.p;
    const auto &LV = P.glevels[0];
    HIPCHK(hipMemsetAsync(P.d_Xr.p, 0, (size_t)nb * (size_t)std::max(1L, P.m) * sizeof(double), P.stream));
    for (size_t l = 0; l < LV.size(); l++) {
        const auto &T = P.level_rtbig[l];
        if (T.lds_small > STM_RES_LDS_MAX) return fail(STMMQR_ERR_INVALID, "internal: a front that k_rtsolve cannot hold was not split");
        LCHK(level_to_front_form(P, l));
        if (T.n < LV[l].n_all)
            LCHK(stm_launch_rtsolve(c, L0 + LV[l].all_off, LV[l].n_all, P.d_Xs.p, P.d_U.p, P.d_Xr.p, P.d_rowbase.p, T.lds_small, P.stream, nb, B, 1));
        LCHK(stm_launch_rtsolve_big(c, P.d_rtb.p + T.off, T.n, T.live_steps, T.max_nslab, P.d_Xs.p, P.d_U.p, P.d_Xr.p, P.d_rowbase.p, P.d_rtLc.p,
                                    P.d_rtRm.p + T.off, P.d_err.p, P.stream, nb, B));
    }
    return 0;
}
// nb vectors Z (device, stride n) -> Y (device, stride m) = R' \ Z or, through Qfill, R' \ (E' Z): stmmqr_plan_rsolve 2, 3
int rt_vectors(stmmqr_plan &P, const double *Z, double *Y, int nb, bool through_qfill)
{
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    // b in R's column order: E'Z gathers through Qfill
    LCHK(stm_launch_perm(Z, (through_qfill && P.has_qfill) ? P.d_Qfill.p : nullptr, P.d_Xs.p, (int)n, 0, st, nb, n, n));
    LCHK(rt_pass(P, nb));
    HIPCHK(hipMemcpyAsync(Y, P.d_Xr.p, (size_t)nb * (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, st));
    return 0;
}
}  // namespace

// QR_qmult (STMMQR/include/SparseQR.h:403-409, SparseQR.c:1815-2116) on the resident factors, in place:
//   method 0 QR_QTX: X (m x k, ldx >= m) <- Q' X      method 1 QR_QX: X <- Q X
//   method 2 QR_XQT: X (k x m, ldx >= k) <- X Q'      method 3 QR_XQ: X <- X Q
// Row (methods 0, 1) / column (2, 3) order as in the reference: Q'X and X Q come out in the permuted order of the
// factorization (HPinv), Q X and X Q' take it.  All vectors cross PCIe in ONE transfer each way.
int stmmqr_plan_qmult(stmmqr_plan *plan, int method, double *X, stm_long ldx, stm_long k)
{
    PASS(check_factored(plan));
    if (!X || k < 0 || method < 0 || method > 3 || ldx < ((method <= 1) ? plan->m : k))
        return fail(STMMQR_ERR_INVALID, "bad qmult arguments");
    if (!plan->keep_h) return fail(STMMQR_ERR_INVALID, "the plan keeps no Householder vectors (keepH = 0): no Q-apply");
    stmmqr_plan &P = *plan;
    PASS(begin_resident_op(P));
    const long m = P.m;
    if (k == 0 || m == 0) return 0;
    // X Q' = (Q X')' and X Q = (Q' X')': the rows of X are the vectors (SparseQR.c:2040-2075: the same permutation pattern)
    const bool rows = method >= 2;
    const int vm = rows ? (method == 2) : method;
    std::vector<double> T(rows ? (size_t)m * (size_t)k : 0);
    for (stm_long r = 0; r < k && rows; r++)
        for (long i = 0; i < m; i++) T[(size_t)r * m + i] = X[r + (size_t)i * ldx];
    double *H = rows ? T.data() : X;
    const long ldh = rows ? m : ldx;
    LCHK(upload_cols(P.d_Xall, H, ldh, m, k, P.stream));
    PASS(for_each_batch(P, k, [&](stm_long j, int nb) { return qapply_vectors(P, vm, P.d_Xall.p + j * m, P.d_Xall.p + j * m, nb); }));
    PASS(download_cols(P, P.d_Xall, H, ldh, m, k));
    for (stm_long r = 0; r < k && rows; r++)
        for (long i = 0; i < m; i++) X[r + (size_t)i * ldx] = T[(size_t)r * m + i];
    return 0;
}

// QR_solve (STMMQR/include/SparseQR.h:411-417, SparseQR.c:2118-2216) on the resident factors:
//   system 0 QR_RX_EQUALS_B   : X (n x nrhs) = R \ B            B (m x nrhs) in R's row order (what QR_QTX returns)
//   system 1 QR_RETX_EQUALS_B : X = E (R \ B)
//   system 2 QR_RTX_EQUALS_B  : X (m x nrhs) = R' \ B           B (n x nrhs), rows of X beyond the rank are zero
//   system 3 QR_RTX_EQUALS_ETB: X = R' \ (E' B)
// Dead pivot columns: x = 0 (systems 0, 1: the basic solution of qr_rsolve) / no equation (2, 3: the squeezed R).
int stmmqr_plan_rsolve(stmmqr_plan *plan, int system, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs)
{
    PASS(check_factored(plan));
    if (system < 0 || system > 3 || !B || !X || nrhs < 0) return fail(STMMQR_ERR_INVALID, "bad solve arguments");
    stmmqr_plan &P = *plan;
    const long m = P.m, n = P.n, brows = (system <= 1) ? m : n, xrows = (system <= 1) ? n : m;
    if (ldb < brows || ldx < xrows) return fail(STMMQR_ERR_INVALID, "bad leading dimension");
    PASS(begin_resident_op(P));
    if (nrhs == 0) return 0;
    HIPCHK(hipMemsetAsync(P.d_err.p, 0, sizeof(int), P.stream));
    LCHK(upload_cols(P.d_Xall, B, ldb, brows, nrhs, P.stream));
    LCHK(grow(P.d_Yall, (size_t)(xrows * nrhs)));
    if (system >= 2) PASS(ensure_rt(P));
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) {
        return system <= 1 ? r_vectors(P, P.d_Xall.p + j * m, P.d_Yall.p + j * n, nb, system == 1)
                           : rt_vectors(P, P.d_Xall.p + j * n, P.d_Yall.p + j * m, nb, system == 3);
    }));
    LCHK(download_cols(P, P.d_Yall, X, ldx, xrows, nrhs));
    return end_resident_op(P);
}

// X (n x nrhs, ldx >= n) = E * R^{-1} * (Q' B)(1:n)  for B (m x nrhs, ldb >= m): QR_qmult(QR_QTX) followed by
// QR_solve(QR_RETX_EQUALS_B), the driver's least-squares solve (qrtest.c:11-53), without the trip to the host in between;
// dead columns get x = 0 (basic solution).
int stmmqr_plan_solve(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs)
{
    PASS(check_factored(plan));
    if (!B || !X || ldb < plan->m || ldx < plan->n || nrhs < 0) return fail(STMMQR_ERR_INVALID, "bad solve arguments");
    if (!plan->keep_h)
        return fail(STMMQR_ERR_INVALID, "the plan keeps no Householder vectors (keepH = 0): no Q'B; stmmqr_plan_solve_seminormal solves with R only");
    stmmqr_plan &P = *plan;
    PASS(begin_resident_op(P));
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    if (nrhs == 0) return 0;
    HIPCHK(hipMemsetAsync(P.d_err.p, 0, sizeof(int), P.stream));
    LCHK(upload_cols(P.d_Xall, B, ldb, m, nrhs, st));
    LCHK(grow(P.d_Yall, (size_t)(n * nrhs)));
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) -> int {
        LCHK(stm_launch_perm(P.d_Xall.p + j * m, P.d_PLinv.p, P.d_W.p, (int)m, 1, st, nb, m, m));
        LCHK(run_qapply(P, 0, nb));
        LCHK(rsolve_vector(P, nb));
        LCHK(stm_launch_perm(P.d_Xs.p, P.has_qfill ? P.d_Qfill.p : nullptr, P.d_Yall.p + j * n, (int)n, 1, st, nb, n, n));   // X[Qfill[j]] = x[j]
        return 0;
    }));
    LCHK(download_cols(P, P.d_Yall, X, ldx, n, nrhs));
    return end_resident_op(P);
}

// The minimum-2-norm solution of an underdetermined system from the factorization of its transpose: X = Q (R' \ (E' B)), all on the
// device -- the R' pass that takes fronts of any width, then the Q pass fed from its result; see include/stmmqr_hip.h
int stmmqr_plan_solve_minnorm(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs, int permuted,
                              int on_device)
{
    PASS(check_factored(plan));
    if (!B || !X || nrhs < 0) return fail(STMMQR_ERR_INVALID, "bad minimum-norm solve arguments");
    if (ldb < plan->n || ldx < plan->m) return fail(STMMQR_ERR_INVALID, "bad leading dimension");
    if (!plan->keep_h)
        return fail(STMMQR_ERR_INVALID, "the plan keeps no Householder vectors (keepH = 0): no Q-apply, so no minimum-norm solve");
    stmmqr_plan &P = *plan;
    PASS(begin_resident_op(P));
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    if (nrhs == 0 || m == 0) return 0;
    HIPCHK(hipMemsetAsync(P.d_err.p, 0, sizeof(int), st));
    LCHK(grow(P.d_Xall, (size_t)(std::max(1L, n) * nrhs)));
    LCHK(grow(P.d_Yall, (size_t)(m * nrhs)));
    PASS(copy_cols(P.d_Xall.p, n, B, ldb, n, nrhs, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    PASS(ensure_rt_any(P));
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) -> int {
        // b in R's column order (E'B gathers through Qfill), y = R' \ b in R's row order, x = Q y in the caller's row order
        LCHK(stm_launch_perm(P.d_Xall.p + j * n, (!permuted && P.has_qfill) ? P.d_Qfill.p : nullptr, P.d_Xs.p, (int)n, 0, st, nb, n, n));
        PASS(rt_pass_any(P, nb));
        return qapply_vectors(P, 1, P.d_Xr.p, P.d_Yall.p + j * m, nb);
    }));
    LCHK(download_cols(P, P.d_Yall, X, ldx, m, nrhs, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return end_resident_op(P);
}

// ---- products with R and R', and the condition estimate built on them (factors with or without H) ----
namespace {
// Once per plan, at the first product: per tree level the most row slabs (R x) and column slabs (R' y) of a front -- all R x needs
int ensure_rmult(stmmqr_plan &P)
{
    const auto &LV = P.glevels[0];
    if (P.level_rm_rslab.size() == LV.size()) return 0;
    P.level_rm_rslab.assign(LV.size(), 0);
    P.level_rm_cslab.assign(LV.size(), 0);
    for (size_t l = 0; l < LV.size(); l++)
        for (int q = 0; q < LV[l].n_all; q++) {
            const FrontSym &s = P.fs[P.lists[LV[l].all_off + q]];
            P.level_rm_rslab[l] = std::max(P.level_rm_rslab[l], (std::min(s.fp, s.fm_ub) + STM_RM_ROWS - 1) / STM_RM_ROWS);
            P.level_rm_cslab[l] = std::max(P.level_rm_cslab[l], (s.fn + STM_RM_COLS - 1) / STM_RM_COLS);
        }
    return 0;
}
// ... and what R' y needs besides, at the first transposed product: the pass-vector array U of the R' solve and the transpose of Rj
// (column j of R -> the slots Rp[f] + k with Rj = j, in slot order)
int ensure_rtmult(stmmqr_plan &P)
{
    PASS(ensure_rmult(P));
    LCHK(ensure_rt_buffers(P));
    if (P.d_rmcp.p) return 0;
    const long n = P.n;
    std::vector<int> cp((size_t)n + 1, 0), slot((size_t)std::max(1L, P.rjsize), 0);
    for (long p = 0; p < P.rjsize; p++) cp[(size_t)P.Rj[(size_t)p] + 1]++;
    for (long j = 0; j < n; j++) cp[(size_t)j + 1] += cp[(size_t)j];
    std::vector<int> fill(cp.begin(), cp.end() - 1);
    for (long p = 0; p < P.rjsize; p++) slot[(size_t)fill[(size_t)P.Rj[(size_t)p]]++] = (int)p;
    LCHK(P.d_rmslot.upload(slot, P.stream));
    LCHK(P.d_rmcp.upload(cp, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));                    // (cp / slot are local)
    return 0;
}
// nb vectors X (device, R's column order, stride n) -> Y (device, R's row order, stride m) = R X; rows beyond the rank are zero
int rmult_pass(stmmqr_plan &P, const double *X, double *Y, int nb)
{
    const RhsBatch B = rhs_strides(P);
    const DevCtx c = res_ctx(P);
    const auto &LV = P.glevels[0];
    HIPCHK(hipMemsetAsync(Y, 0, (size_t)nb * (size_t)std::max(1L, P.m) * sizeof(double), P.stream));
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        LCHK(stm_launch_rmult(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, P.level_rm_rslab[l], P.d_Rj.p, P.d_rowbase.p, X, Y, P.stream, nb, B));
    }
    return 0;
}
// nb vectors Y (device, R's row order, stride m; rows beyond the rank are not read) -> Z (device, R's column order, stride n) = R' Y,
// or with absval the column 1-norms of R (one vector, Y not read)
int rtmult_pass(stmmqr_plan &P, const double *Y, double *Z, int nb, int absval = 0)
{
    const RhsBatch B = rhs_strides(P);
    const DevCtx c = res_ctx(P);
    const auto &LV = P.glevels[0];
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        LCHK(stm_launch_rtmult_dots(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, P.level_rm_cslab[l], P.d_rowbase.p, Y, P.d_U.p, absval, P.stream, nb, B));
    }
    return stm_launch_rtmult_gather(P.d_rmcp.p, P.d_rmslot.p, P.d_U.p, Z, (int)P.n, P.stream, nb, B.u, P.n);
}
// does the plan hold the whole tree in one group (what the selected inversion asks as well)
bool holds_whole_tree(const stmmqr_plan &P)
{
    bool whole = P.glevels.size() == 1;
    for (long f = 0; f < P.nf && whole; f++) whole = P.group[(size_t)f] == 0 && !((size_t)f < P.shared.size() && P.shared[(size_t)f]);
    return whole;
}
}  // namespace

// Y = R X (trans 0) or R' X (trans 1) with the whole rank x n factor on the device; see include/stmmqr_hip.h
int stmmqr_plan_rmult(stmmqr_plan *plan, int trans, const double *X, stm_long ldx, double *Y, stm_long ldy, stm_long nrhs, int permuted,
                      int on_device)
{
    PASS(check_factored(plan));
    if ((trans != 0 && trans != 1) || !X || !Y || nrhs < 0) return fail(STMMQR_ERR_INVALID, "bad rmult arguments");
    stmmqr_plan &P = *plan;
    const long m = P.m, n = P.n, xrows = trans ? m : n, yrows = trans ? n : m;
    if (ldx < xrows || ldy < yrows) return fail(STMMQR_ERR_INVALID, "bad leading dimension");
    PASS(begin_resident_op(P));
    if (nrhs == 0 || yrows == 0) return 0;
    hipStream_t st = P.stream;
    HIPCHK(hipMemsetAsync(P.d_err.p, 0, sizeof(int), st));
    PASS(trans ? ensure_rtmult(P) : ensure_rmult(P));
    LCHK(grow(P.d_Xall, (size_t)(std::max(1L, xrows) * nrhs)));
    LCHK(grow(P.d_Yall, (size_t)(yrows * nrhs)));
    PASS(copy_cols(P.d_Xall.p, xrows, X, ldx, xrows, nrhs, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    const int *qf = (!permuted && P.has_qfill) ? P.d_Qfill.p : nullptr;
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) -> int {
        if (!trans) {
            LCHK(stm_launch_perm(P.d_Xall.p + j * n, qf, P.d_Xs.p, (int)n, 0, st, nb, n, n));                 // x[k] = X[Qfill[k]]
            return rmult_pass(P, P.d_Xs.p, P.d_Yall.p + j * m, nb);
        }
        PASS(rtmult_pass(P, P.d_Xall.p + j * m, P.d_Xs.p, nb));
        return stm_launch_perm(P.d_Xs.p, qf, P.d_Yall.p + j * n, (int)n, 1, st, nb, n, n);                   // Y[Qfill[k]] = z[k]
    }));
    LCHK(download_cols(P, P.d_Yall, Y, ldy, yrows, nrhs, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return end_resident_op(P);
}

// The condition of R over its live pivot columns, estimated on the device; see include/stmmqr_hip.h.  Vectors: the r-vector of the
// live pivot columns lives either in an n-vector in R's column order (entry i at pc[i], zero elsewhere: what R x reads, what R \ and
// R' y write) or in the first r entries of an m-vector in R's row order (what R \ and R' y read, what R x and R' \ write).  With
// ncol < n the trailing columns stay zero in every input and are never read from an output: R [x; 0] = R11 x, R \ [y; 0] = R11 \ y,
// and the leading rows of R' \ [z; *] are R11' \ z.
int stmmqr_plan_condest(stmmqr_plan *plan, stm_long ncol, int kind, int iters, double *out, double *v, int on_device)
{
    PASS(check_factored(plan));
    if (!out) return fail(STMMQR_ERR_INVALID, "condest: out is NULL");
    stmmqr_plan &P = *plan;
    const long m = P.m, n = P.n;
    if (ncol < 0 || ncol > n)
        return fail(STMMQR_ERR_INVALID, "condest: ncol = " + std::to_string(ncol) + " is not between 0 and the " + std::to_string(n) + " columns of the plan");
    if (kind != 1 && kind != 2) return fail(STMMQR_ERR_INVALID, "condest: kind = " + std::to_string(kind) + " is neither 1 (one-norm) nor 2 (two-norm)");
    if (ncol < n) PASS(check_carried_view(P, ncol));
    if (!holds_whole_tree(P))
        return fail(STMMQR_ERR_INVALID, "condest: the plan does not hold the whole tree in one group (groups were set, or fronts are imported or shared)");
    PASS(begin_resident_op(P));
    hipStream_t st = P.stream;
    if (iters <= 0) iters = 8;
    // the live pivot columns among the first ncol, in R's column order = in the order of the rows of R
    std::vector<char> rd((size_t)std::max(1L, (long)ncol), 0);
    if (ncol > 0) HIPCHK(hipMemcpyAsync(rd.data(), P.d_Rdead.p, (size_t)ncol, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int> pc;
    for (long j = 0; j < ncol; j++)
        if (!rd[(size_t)j]) pc.push_back((int)j);
    const int r = (int)pc.size();
    double res[8] = {1.0, 0.0, 0.0, 0.0, (double)r, (double)kind, 0.0, 0.0};
    auto give = [&](double *dst, const double *src, size_t cnt) -> int {      // a host array to the caller's, host or device
        if (on_device) { HIPCHK(hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyHostToDevice, st)); HIPCHK(hipStreamSynchronize(st)); }
        else memcpy(dst, src, cnt * sizeof(double));
        return 0;
    };
    if (r == 0) {
        if (v && ncol > 0) { const std::vector<double> z((size_t)ncol, 0.0); PASS(give(v, z.data(), z.size())); }
        return give(out, res, 8);
    }
    HIPCHK(hipMemsetAsync(P.d_err.p, 0, sizeof(int), st));
    PASS(ensure_rtmult(P));
    PASS(ensure_rt_any(P));
    const size_t nn = (size_t)std::max(1L, n), mm = (size_t)std::max(1L, m);
    LCHK(grow(P.d_ceA, nn)); LCHK(grow(P.d_ceB, nn)); LCHK(grow(P.d_ceV, nn)); LCHK(grow(P.d_ceY, mm)); LCHK(grow(P.d_ceS, 8));
    if (P.d_cepc.n < (size_t)r) LCHK(P.d_cepc.alloc((size_t)r));
    HIPCHK(hipMemcpyAsync(P.d_cepc.p, pc.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, st));
    double *dA = P.d_ceA.p, *dB = P.d_ceB.p, *dV = P.d_ceV.p, *dY = P.d_ceY.p, *dS = P.d_ceS.p;
    const int *dpc = P.d_cepc.p;
    double sc[4] = {0, 0, 0, 0};
    auto scalars = [&]() -> int {                                              // the few scalars the host steers by
        HIPCHK(hipMemcpyAsync(sc, dS, sizeof(sc), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    // the r-vector h (host) into the zeroed m-vector dY / the zeroed n-vector dst
    auto put_rows = [&](const std::vector<double> &h) -> int {
        HIPCHK(hipMemsetAsync(dY, 0, mm * sizeof(double), st));
        HIPCHK(hipMemcpyAsync(dY, h.data(), (size_t)r * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));                                      // (h is pageable)
        return 0;
    };
    // dY (R's row order, zero beyond r) -> d_Xs = R \ dY
    auto solve_r = [&]() -> int {
        LCHK(stm_launch_perm(dY, P.d_Wmap.p, P.d_W.p, (int)m, 0, st, 1, m, m));
        return rsolve_vector(P, 1);
    };
    std::vector<double> safe((size_t)r, 1.0);                                  // x_i = (-1)^i (1 + i / (r - 1))
    for (int i = 0; i < r && r > 1; i++) safe[(size_t)i] = ((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)(r - 1));
    double vnorm = 1.0;                                                        // v = dV / vnorm
    if (kind == 1) {
        // |R_live|_1: exact, the largest column sum of |R| over the live columns
        PASS(rtmult_pass(P, dY, dB, 1, 1));
        LCHK(stm_launch_ce_reduce(2, dB, dpc, nullptr, r, dS, st));
        PASS(scalars());
        res[1] = sc[0];
        // Hager's iteration in Higham's form on R_live^-1
        double est = 0.0;
        int rounds = 0, jprev = -1;
        PASS(put_rows(std::vector<double>((size_t)r, 1.0 / (double)r)));
        for (int round = 1; round <= 5; round++) {
            rounds = round;
            PASS(solve_r());                                                   // y = R \ x
            LCHK(stm_launch_ce_reduce(0, P.d_Xs.p, dpc, nullptr, r, dS, st));
            PASS(scalars());
            if (round > 1 && !(sc[0] > est)) break;                            // the estimate does not grow
            est = vnorm = sc[0];
            HIPCHK(hipMemcpyAsync(dV, P.d_Xs.p, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (round == 5) break;
            LCHK(stm_launch_ce_map(0, P.d_Xs.p, dpc, nullptr, r, 0.0, st));    // xi = sign(y)
            PASS(rt_pass_any(P, 1));                                           // z = R' \ xi: the first r rows of d_Xr
            LCHK(stm_launch_ce_reduce(3, P.d_Xr.p, nullptr, dY, r, dS, st));
            PASS(scalars());
            const int j = (int)sc[2];
            if (sc[1] <= sc[3] || j == jprev) break;                           // |z|_inf <= z'x, or the arg-max repeats
            jprev = j;
            const double one = 1.0;
            HIPCHK(hipMemsetAsync(dY, 0, (size_t)r * sizeof(double), st));
            HIPCHK(hipMemcpyAsync(dY + j, &one, sizeof(double), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        PASS(put_rows(safe));                                                  // the safeguard vector
        PASS(solve_r());
        LCHK(stm_launch_ce_reduce(0, P.d_Xs.p, dpc, nullptr, r, dS, st));
        PASS(scalars());
        const double est2 = 2.0 * sc[0] / (3.0 * (double)r);
        if (est2 > est) {
            est = est2; vnorm = sc[0];
            HIPCHK(hipMemcpyAsync(dV, P.d_Xs.p, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        res[2] = est; res[3] = (double)rounds;
    } else {
        double s2 = 0.0;
        for (double t : safe) s2 += t * t;
        s2 = std::sqrt(s2);
        std::vector<double> start(safe);
        for (double &t : start) t /= s2;
        // |R_live|_2: power iteration on R'R, x <- R'(R x) / |R'(R x)|, estimate sqrt |R'(R x)|
        PASS(put_rows(start));
        HIPCHK(hipMemsetAsync(dA, 0, nn * sizeof(double), st));
        LCHK(stm_launch_ce_map(2, dY, dpc, dA, r, 0.0, st));
        double lam = 0.0;
        for (int it = 0; it < iters; it++) {
            PASS(rmult_pass(P, dA, dY, 1));
            PASS(rtmult_pass(P, dY, dB, 1));
            LCHK(stm_launch_ce_reduce(1, dB, dpc, nullptr, r, dS, st));
            PASS(scalars());
            lam = std::sqrt(sc[0]);
            if (!(lam > 0.0)) break;
            LCHK(stm_launch_ce_map(1, dB, dpc, dA, r, lam, st));
        }
        res[1] = std::sqrt(lam);
        // |R_live^-1|_2: the same on (R'R)^-1, x <- R \ (R' \ x) / |.|; the estimate is 1 / |R_live v|_2 of the last iterate v
        PASS(put_rows(start));
        HIPCHK(hipMemsetAsync(dV, 0, nn * sizeof(double), st));
        LCHK(stm_launch_ce_map(2, dY, dpc, dV, r, 0.0, st));
        int made = 0;                                                          // solve pairs whose result became the iterate
        for (int it = 0; it < iters; it++) {
            HIPCHK(hipMemcpyAsync(P.d_Xs.p, dV, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
            PASS(rt_pass_any(P, 1));                                           // t = R' \ x: the first r rows of d_Xr
            HIPCHK(hipMemcpyAsync(dY, P.d_Xr.p, (size_t)r * sizeof(double), hipMemcpyDeviceToDevice, st));   // (dY is zero beyond r)
            PASS(solve_r());                                                   // w = R \ t
            LCHK(stm_launch_ce_reduce(1, P.d_Xs.p, dpc, nullptr, r, dS, st));
            PASS(scalars());
            const double mu = std::sqrt(sc[0]);
            if (!(mu > 0.0) || !std::isfinite(mu)) break;
            LCHK(stm_launch_ce_map(1, P.d_Xs.p, dpc, dV, r, mu, st));
            made++;
        }
        PASS(rmult_pass(P, dV, dY, 1));
        LCHK(stm_launch_ce_reduce(1, dY, nullptr, nullptr, r, dS, st));
        PASS(scalars());
        res[2] = 1.0 / std::sqrt(sc[0]);
        res[3] = (double)made;
    }
    res[0] = res[1] * res[2];
    if (v) {
        // in the caller's column order, zeros on dead columns (R \ leaves them zero), unit norm of the kind
        double *dv = on_device ? v : dB;
        HIPCHK(hipMemsetAsync(dv, 0, (size_t)ncol * sizeof(double), st));
        LCHK(stm_launch_ce_vector(dV, P.has_qfill ? P.d_Qfill.p : nullptr, dv, (int)ncol, vnorm, st));
        if (!on_device) HIPCHK(hipMemcpyAsync(v, dv, (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    PASS(end_resident_op(P));
    return give(out, res, 8);
}

// ---- products with A and the corrected seminormal equations (factors with or without H) ----
namespace {
// Y = A X (trans 0: X n x nrhs, Y m x nrhs), A' X (trans 1: X m, Y n), or with B (trans 0 only) Y = B - A X for the m x n matrix with
// index A and values Ax; device arrays
int spmv(const AIndexDev &A, const double *Ax, long m, long n, int trans, const double *X, long long ldx, const double *B, long long ldb,
         double *Y, long long ldy, long long nrhs, hipStream_t st)
{
    if (trans) return stm_launch_spmv((int)n, A.cp.p, A.ci.p, nullptr, Ax, X, ldx, B, ldb, Y, ldy, nrhs, st);
    return stm_launch_spmv((int)m, A.rp.p, A.rj.p, A.rq.p, Ax, X, ldx, B, ldb, Y, ldy, nrhs, st);
}
// ... for the plan's A with the values of the last factorization
int spmv_dev(stmmqr_plan &P, int trans, const double *X, long long ldx, const double *B, long long ldb, double *Y, long long ldy, long long nrhs)
{
    return spmv(P.a_idx, P.d_Ax.p, P.m, P.n, trans, X, ldx, B, ldb, Y, ldy, nrhs, P.stream);
}
}  // namespace

// Y = A X (trans 0) or A' X (trans 1) with the values of the last factorization; see include/stmmqr_hip.h
int stmmqr_plan_spmv(stmmqr_plan *plan, int trans, const double *X, stm_long ldx, double *Y, stm_long ldy, stm_long nrhs, int on_device)
{
    PASS(check_factored(plan));
    stmmqr_plan &P = *plan;
    const long xr = trans ? P.m : P.n, yr = trans ? P.n : P.m;
    if (!X || !Y || nrhs < 0 || (trans != 0 && trans != 1) || ldx < xr || ldy < yr) return fail(STMMQR_ERR_INVALID, "bad spmv arguments");
    if (!P.pattern_set) return fail(STMMQR_ERR_INVALID, "pattern of A was never given");
    HIPCHK(hipSetDevice(P.device));
    if (nrhs == 0 || yr == 0) return 0;
    LCHK(stm_ensure_a_index(P));
    if (on_device) {
        LCHK(spmv_dev(P, trans, X, ldx, nullptr, 0, Y, ldy, nrhs));
        HIPCHK(hipStreamSynchronize(P.stream));
        return 0;
    }
    LCHK(grow(P.d_csY, (size_t)yr * (size_t)nrhs));
    LCHK(upload_cols(P.d_csX, X, ldx, xr, nrhs, P.stream));
    LCHK(spmv_dev(P, trans, P.d_csX.p, xr, nullptr, 0, P.d_csY.p, yr, nrhs));
    return download_cols(P, P.d_csY, Y, ldy, yr, nrhs);
}

// Least squares through the corrected seminormal equations with R only; see include/stmmqr_hip.h
int stmmqr_plan_solve_seminormal(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs, int refine,
                                 int on_device, double *info)
{
    PASS(check_factored(plan));
    stmmqr_plan &P = *plan;
    const long m = P.m, n = P.n;
    if (!B || !X || nrhs < 0 || refine < 0 || ldb < m || ldx < n) return fail(STMMQR_ERR_INVALID, "bad seminormal solve arguments");
    if (!P.pattern_set) return fail(STMMQR_ERR_INVALID, "pattern of A was never given");
    PASS(begin_resident_op(P));
    PASS(ensure_rt(P));                              // (the R' \ step: refused before any launch of the solve)
    LCHK(stm_ensure_a_index(P));
    if (info) *info = 0;
    if (nrhs == 0) return 0;
    hipStream_t st = P.stream;
    const size_t mm = (size_t)std::max(1L, m), nn = (size_t)std::max(1L, n), nbm = (size_t)std::min<stm_long>(rhs_batch_max(), nrhs);
    LCHK(grow(P.d_csB, mm * (size_t)nrhs)); LCHK(grow(P.d_csX, nn * (size_t)nrhs));
    LCHK(grow(P.d_csR, mm * nbm)); LCHK(grow(P.d_csY, mm * nbm));
    LCHK(grow(P.d_csZ, nn * nbm)); LCHK(grow(P.d_csD, nn * nbm));
    LCHK(grow(P.d_csN, 3 * (size_t)nrhs + 1));
    HIPCHK(hipMemsetAsync(P.d_err.p, 0, sizeof(int), P.stream));
    PASS(copy_cols(P.d_csB.p, m, B, ldb, m, nrhs, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) -> int {
        const double *b = P.d_csB.p + j * m;
        double *x = P.d_csX.p + j * n;
        LCHK(spmv_dev(P, 1, b, m, nullptr, 0, P.d_csZ.p, n, nb));                        // z = A'b
        LCHK(rt_vectors(P, P.d_csZ.p, P.d_csY.p, nb, true));                              // y = R' \ (E'z)
        LCHK(r_vectors(P, P.d_csY.p, x, nb, true));                                       // x = E (R \ y)
        for (int it = 0; it < refine; it++) {
            LCHK(spmv_dev(P, 0, x, n, b, m, P.d_csR.p, m, nb));                          // r = b - A x
            LCHK(spmv_dev(P, 1, P.d_csR.p, m, nullptr, 0, P.d_csZ.p, n, nb));             // A'r
            LCHK(rt_vectors(P, P.d_csZ.p, P.d_csY.p, nb, true));
            LCHK(r_vectors(P, P.d_csY.p, P.d_csD.p, nb, true));
            LCHK(stm_launch_add_cols((int)n, nb, P.d_csD.p, n, x, n, st));                // x += E R^-1 R^-T E' A'r
        }
        if (info) {
            LCHK(spmv_dev(P, 0, x, n, b, m, P.d_csR.p, m, nb));
            LCHK(spmv_dev(P, 1, P.d_csR.p, m, nullptr, 0, P.d_csZ.p, n, nb));
            LCHK(stm_launch_colnorm2(n, P.d_csZ.p, n, nb, P.d_csN.p + j, st));           // |A'r|^2, |x|^2, |b|^2
            LCHK(stm_launch_colnorm2(n, x, n, nb, P.d_csN.p + nrhs + j, st));
            LCHK(stm_launch_colnorm2(m, b, m, nb, P.d_csN.p + 2 * nrhs + j, st));
        }
        return 0;
    }));
    if (info) {
        LCHK(stm_launch_colnorm2(P.anz, P.d_Ax.p, std::max(1L, P.anz), 1, P.d_csN.p + 3 * nrhs, st));   // |A|_F^2
        std::vector<double> nr((size_t)(3 * nrhs + 1));
        HIPCHK(hipMemcpyAsync(nr.data(), P.d_csN.p, nr.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *info = stm_seminormal_info(std::sqrt(nr[(size_t)(3 * nrhs)]), nr.data(), nr.data() + nrhs, nr.data() + 2 * nrhs, nrhs);
    }
    LCHK(download_cols(P, P.d_csX, X, ldx, n, nrhs, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return end_resident_op(P);
}

// Least squares with the right-hand sides carried through the factorization; see include/stmmqr_hip.h.  The plan holds the R of
// [A B] (n = P.n - nrhs columns of A, ntol = n).  The back substitution is r_pass on a view of the factorization that ends at
// column n (stmmqr_carried.hip): fronts that hold B columns as pivots have fp cut back to their A pivots
// and their live A pivots as rank, y = 0 and x(n + j) = -1 for right-hand side j -- so y - R12 x is C(:, j) minus the A part, and
// no diagonal entry of the B block is ever a divisor.
int stmmqr_plan_solve_carried(stmmqr_plan *plan, stm_long nrhs, double *X, stm_long ldx, double *resid, int on_device)
{
    PASS(check_factored(plan));
    stmmqr_plan &P = *plan;
    if (nrhs < 1 || nrhs > P.n) return fail(STMMQR_ERR_INVALID, "carried solve: nrhs must be between 1 and the number of columns of the factorized [A B]");
    const long m = P.m, na = P.n, n = P.n - nrhs;
    if (!X || ldx < n) return fail(STMMQR_ERR_INVALID, "bad carried solve arguments");
    PASS(check_carried_view(P, n));
    PASS(begin_resident_op(P));
    hipStream_t st = P.stream;
    const auto &LV = P.glevels[0];
    // ---- the view: FrontSym of the array the resident-factor kernels read (res_ctx) with fp cut back, the B fronts level by level ----
    std::vector<FrontSym> vs = resident_front_syms(P);
    std::vector<int> blist, boff(LV.size() + 1, 0);
    for (size_t l = 0; l < LV.size(); l++) {
        for (int q = 0; q < LV[l].n_all; q++) {
            const int f = P.lists[LV[l].all_off + q];
            const FrontSym &s = P.fs[f];
            if ((long)s.col1 + s.fp > n) { blist.push_back(f); vs[(size_t)f].fp = (int)std::max(0L, n - (long)s.col1); }
        }
        boff[l + 1] = (int)blist.size();
    }
    if (blist.empty()) blist.push_back(0);
    if (P.d_fs_car.n != vs.size()) LCHK(P.d_fs_car.alloc(vs.size()));
    if (P.d_carlist.n < blist.size()) LCHK(P.d_carlist.alloc(blist.size()));
    if (!vs.empty()) HIPCHK(hipMemcpyAsync(P.d_fs_car.p, vs.data(), vs.size() * sizeof(FrontSym), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(P.d_carlist.p, blist.data(), blist.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                            // (vs / blist are pageable and local)
    if (P.d_fnum_car.n != (size_t)std::max(1L, P.nf)) LCHK(P.d_fnum_car.alloc((size_t)std::max(1L, P.nf)));
    if (P.nf > 0) HIPCHK(hipMemcpyAsync(P.d_fnum_car.p, P.d_fnum.p, (size_t)P.nf * sizeof(FrontNum), hipMemcpyDeviceToDevice, st));
    LCHK(grow(P.d_carN, (size_t)nrhs));
    HIPCHK(hipMemsetAsync(P.d_carN.p, 0, (size_t)nrhs * sizeof(double), st));
    HIPCHK(hipMemsetAsync(P.d_err.p, 0, sizeof(int), P.stream));
    LCHK(grow(P.d_Yall, (size_t)(std::max(1L, n) * nrhs)));
    const DevCtx ct = res_ctx(P);
    DevCtx cv = ct;
    cv.fs = P.d_fs_car.p; cv.fnum = P.d_fnum_car.p;
    PASS(for_each_batch(P, nrhs, [&](stm_long j0, int nb) -> int {
        HIPCHK(hipMemsetAsync(P.d_W.p, 0, (size_t)nb * (size_t)std::max(1L, m) * sizeof(double), st));
        HIPCHK(hipMemsetAsync(P.d_Xs.p, 0, (size_t)nb * (size_t)na * sizeof(double), st));
        LCHK(stm_launch_carried_seed(P.d_Xs.p, na, (int)n, (int)j0, nb, st));
        // (the first pass sets the view's ranks of the level's B fronts before its kernels read them, and takes the residual norms
        //  while the level is in front form)
        PASS(r_pass(P, cv, nb, [&](size_t l) {
            return j0 == 0 ? stm_launch_carried_view(ct, P.d_carlist.p + boff[l], boff[l + 1] - boff[l], (int)n, P.d_fnum_car.p, P.d_carN.p, st) : 0;
        }));
        LCHK(stm_launch_perm(P.d_Xs.p, P.has_qfill ? P.d_Qfill.p : nullptr, P.d_Yall.p + j0 * n, (int)n, 1, st, nb, na, n));   // X[Qfill[j]] = x[j], j < n
        return 0;
    }));
    if (on_device) {
        PASS(copy_cols(X, ldx, P.d_Yall.p, n, n, nrhs, hipMemcpyDeviceToDevice, st));
        if (resid) HIPCHK(hipMemcpyAsync(resid, P.d_carN.p, (size_t)nrhs * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    } else {
        if (resid) HIPCHK(hipMemcpyAsync(resid, P.d_carN.p, (size_t)nrhs * sizeof(double), hipMemcpyDeviceToHost, st));
        LCHK(download_cols(P, P.d_Yall, X, ldx, n, nrhs));
    }
    return end_resident_op(P);
}

// The selected inverse of R'R on the device, for the length of one call; see include/stmmqr_hip.h and stmmqr_selinv.hip.  The frontal
// tree is walked from the root to the leaves, a level at a time: every front's block of Z is built from its parent's, and every block
// stays where it is (SiDesc::zoff is cumulative), so after the level loop the whole selected inverse is resident.  Device memory of
// the call alone (released with the SelInv): the arena of the blocks, sum over fronts of (min(fp, fm_ub) + cn)^2 doubles; the widest
// level's [G | S], sum over its fronts of min(fp, fm_ub) (min(fp, fm_ub) + cn) doubles; two int tables of the size of Rj.
// ncol < n: the view of stmmqr_plan_solve_carried (fp cut back to the A pivots, their live ones as rank) with fn cut back to the
// columns of A as well -- the B columns are the last entries of every front's list.
namespace {
struct SelInv {
    DevBuf<double> Z, Wk, Var;
    DevBuf<int> Lc, Pos, Rm;
    DevBuf<SiDesc> Sd;
    std::vector<SiDesc> sd;              // (host copy: the upload reads it until the entry point's final synchronization)
    double *dv = nullptr;                // the variances on the device: the caller's buffer or Var
    DevCtx c;                            // the fronts the kernels read (res_ctx)
    bool ran = false;                    // false: ncol = 0, nothing was allocated or launched
};
// The checks of stmmqr_plan_covariance_diag, then `host_checks` (the entry point's own, on the host: nothing is allocated or launched
// before it passed), then the view, the buffers, stm_launch_si_prep and the level loop.  Returns with the launches in flight on the
// plan's stream (the SelInv must outlive their synchronization); var (device pointer when on_device, else ignored here: the entry point downloads si.dv) may be NULL.
template <class HostChecks>
int selected_inverse(stmmqr_plan *plan, stm_long ncol, double *var, int on_device, HostChecks host_checks, SelInv &si)
{
    PASS(check_factored(plan));
    stmmqr_plan &P = *plan;
    const long n = P.n;
    if (ncol < 0 || ncol > n)
        return fail(STMMQR_ERR_INVALID, "covariance: ncol = " + std::to_string(ncol) + " is not between 0 and the " + std::to_string(n) + " columns of the plan");
    if (ncol < n) PASS(check_carried_view(P, ncol));
    if (!holds_whole_tree(P))
        return fail(STMMQR_ERR_INVALID, "covariance: the plan does not hold the whole tree in one group (groups were set, or fronts are imported or shared)");
    PASS(host_checks(P));
    PASS(begin_resident_op(P));
    if (ncol == 0) return 0;
    hipStream_t st = P.stream;
    const auto &LV = P.glevels[0];
    const long nf = P.nf;
    // ---- the view and where every front's block lies ----
    std::vector<SiDesc> &sd = si.sd;
    sd.assign((size_t)std::max(1L, nf), SiDesc());
    std::vector<int> lev_r(LV.size(), 0), lev_cn(LV.size(), 0);
    long long zall = 0, wmax = 1;
    for (size_t l = 0; l < LV.size(); l++) {
        long long w = 0;
        for (int q = 0; q < LV[l].n_all; q++) {
            const int f = P.lists[LV[l].all_off + q];
            const FrontSym &s = P.fs[f];
            SiDesc &d = sd[(size_t)f];
            d.fp = (int)std::min<long>(s.fp, std::max(0L, (long)ncol - (long)s.col1));
            d.check = d.fp == s.fp;
            d.cn = 0;
            if (d.check)
                while (s.fp + d.cn < s.fn && P.Rj[(size_t)(s.rp + s.fp + d.cn)] < ncol) d.cn++;
            d.rmax = std::min(d.fp, std::max(s.fm_ub, 0));
            const long long dim = (long long)d.rmax + d.cn;
            d.zoff = zall; zall += dim * dim;
            d.woff = w; w += (long long)std::max(d.rmax, 1) * dim;
            lev_r[l] = std::max(lev_r[l], d.rmax); lev_cn[l] = std::max(lev_cn[l], d.cn);
        }
        wmax = std::max(wmax, w);
    }
    // ---- the call's own device memory ----
    const bool own_var = !on_device || !var;
    const size_t rjs = (size_t)std::max(1L, P.rjsize);
    if (si.Z.alloc((size_t)std::max(1LL, zall)) || si.Wk.alloc((size_t)wmax) || si.Lc.alloc(rjs) || si.Pos.alloc(rjs) ||
        si.Rm.alloc((size_t)std::max(1L, nf)) || si.Sd.alloc(sd.size()) || (own_var && si.Var.alloc((size_t)ncol))) {
        (void)hipGetLastError();
        return fail(STMMQR_ERR_OUT_OF_MEMORY, "covariance: no device memory for the blocks of the selected inverse (" +
                                                  std::to_string(8e-9 * ((double)zall + (double)wmax)) + " GB)");
    }
    double *dv = si.dv = own_var ? si.Var.p : var;
    HIPCHK(hipMemcpyAsync(si.Sd.p, sd.data(), sd.size() * sizeof(SiDesc), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dv, 0, (size_t)ncol * sizeof(double), st));                       // (dead columns: 0)
    HIPCHK(hipMemsetAsync(P.d_err.p, 0, sizeof(int), P.stream));
    const DevCtx c = si.c = res_ctx(P);
    LCHK(stm_launch_si_prep(c, (int)nf, si.Sd.p, si.Lc.p, si.Pos.p, si.Rm.p, P.d_err.p, st));
    for (size_t l = LV.size(); l-- > 0;) {
        LCHK(level_to_front_form(P, l));
        LCHK(stm_launch_si_level(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, lev_r[l], lev_cn[l], si.Sd.p, si.Rm.p, si.Lc.p, si.Pos.p, P.d_Rj.p,
                                 P.has_qfill ? P.d_Qfill.p : nullptr, si.Wk.p, si.Z.p, dv, st));
    }
    si.ran = true;
    return 0;
}
// what the leverage and entry kernels read of a finished SelInv, beside their own tables
SiView si_view(const stmmqr_plan &P, const SelInv &si, const int *colfront) { return SiView{si.Sd.p, si.Pos.p, P.d_Rj.p, colfront, si.Z.p}; }
// colfront[k] = the front where column k (R's order) is pivotal, k < ncol
std::vector<int> column_fronts(const stmmqr_plan &P, long ncol)
{
    std::vector<int> cf((size_t)std::max(1L, ncol), 0);
    for (long f = 0; f < P.nf; f++)
        for (long k = P.Super[(size_t)f]; k < std::min<long>(P.Super[(size_t)f + 1], ncol); k++) cf[(size_t)k] = (int)f;
    return cf;
}
int no_memory_for_tables(const char *what)
{
    (void)hipGetLastError();
    return fail(STMMQR_ERR_OUT_OF_MEMORY, std::string(what) + ": no device memory for the call's index tables");
}
// the end of a call that read the blocks: d_err = 1 from k_si_prep, 2 from a lookup of k_si_leverage
int end_selinv_op(stmmqr_plan &P)
{
    int e = 0;
    HIPCHK(hipMemcpyAsync(&e, P.d_err.p, sizeof(int), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    if (e == 2) return fail(STMMQR_ERR_INVALID, "internal: two columns of one row of A are not in one block of the selected inverse");
    if (e) return fail(STMMQR_ERR_INVALID, "internal: live pivot count of a front differs from its rank");
    return 0;
}
}  // namespace

// diag(((A E)_live' (A E)_live)^-1): the diagonals of the blocks (k_si_diag, inside the level loop)
int stmmqr_plan_covariance_diag(stmmqr_plan *plan, stm_long ncol, double *var, int on_device)
{
    PASS(check_factored(plan));
    if (!var) return fail(STMMQR_ERR_INVALID, "covariance: var is NULL");
    SelInv si;
    PASS(selected_inverse(plan, ncol, var, on_device, [](stmmqr_plan &) { return 0; }, si));
    if (!si.ran) return 0;
    stmmqr_plan &P = *plan;
    if (!on_device) HIPCHK(hipMemcpyAsync(var, si.dv, (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, P.stream));
    return end_resident_op(P);                               // (synchronizes: the buffers are done with)
}

// Leverages: lev[i] = a_i' Z a_i from the resident blocks (k_si_leverage); see include/stmmqr_hip.h.  The call's own tables beside the
// selected inverse's: column -> front (ncol ints), S's row pointers and global column indices as ints (m + 1 and anz), lev on the
// device for a host caller.  Rows are read from S = A(P,Q) with the values of the last factorization (d_Sx: written by the gather of
// reset_factorization, read by the assembly, never overwritten).
int stmmqr_plan_leverage(stmmqr_plan *plan, stm_long ncol, double *lev, double *var, int on_device)
{
    PASS(check_factored(plan));
    if (!lev) return fail(STMMQR_ERR_INVALID, "leverage: lev is NULL");
    SelInv si;
    PASS(selected_inverse(plan, ncol, var, on_device, [](stmmqr_plan &P) {
        return P.pattern_set ? 0 : fail(STMMQR_ERR_INVALID, "pattern of A was never given");
    }, si));
    stmmqr_plan &P = *plan;
    hipStream_t st = P.stream;
    const long m = P.m;
    if (m == 0) return si.ran ? end_resident_op(P) : 0;
    if (!si.ran) {                                           // (ncol = 0: no column takes part)
        if (on_device) { HIPCHK(hipMemsetAsync(lev, 0, (size_t)m * sizeof(double), st)); HIPCHK(hipStreamSynchronize(st)); }
        else std::fill(lev, lev + m, 0.0);
        return 0;
    }
    std::vector<int> sp((size_t)m + 1), sj((size_t)std::max(1L, P.anz), 0);
    for (long i = 0; i <= m; i++) sp[(size_t)i] = (int)P.Sp[(size_t)i];
    for (long p = 0; p < P.anz; p++) sj[(size_t)p] = (int)P.Sj[(size_t)p];
    const std::vector<int> cf = column_fronts(P, ncol);
    DevBuf<int> dSp, dSj, dCf;
    DevBuf<double> dLev;
    if (dSp.alloc(sp.size()) || dSj.alloc(sj.size()) || dCf.alloc(cf.size()) || (!on_device && dLev.alloc((size_t)m)))
        return no_memory_for_tables("leverage");
    HIPCHK(hipMemcpyAsync(dSp.p, sp.data(), sp.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dSj.p, sj.data(), sj.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dCf.p, cf.data(), cf.size() * sizeof(int), hipMemcpyHostToDevice, st));
    double *dl = on_device ? lev : dLev.p;
    LCHK(stm_launch_si_leverage(si.c, si_view(P, si, dCf.p), (int)m, (int)ncol, P.d_PLinv.p, dSp.p, dSj.p, P.d_Sx.p, dl, P.d_err.p, st));
    if (!on_device) {
        HIPCHK(hipMemcpyAsync(lev, dl, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
        if (var) HIPCHK(hipMemcpyAsync(var, si.dv, (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    return end_selinv_op(P);                                 // (synchronizes: sp / sj / cf and the buffers are done with)
}

// Entries Z(I[p], J[p]) of the selected inverse (k_si_entries); see include/stmmqr_hip.h.  Every pair is resolved on the host to
// (front of the earlier column in R's order, its local column, the local column of the later one) before anything is allocated.
int stmmqr_plan_covariance_entries(stmmqr_plan *plan, stm_long ncol, stm_long npairs, const stm_long *I, const stm_long *J, double *out,
                                   int on_device)
{
    PASS(check_factored(plan));
    if (npairs < 0 || (npairs > 0 && (!out || !I || !J))) return fail(STMMQR_ERR_INVALID, "covariance entries: npairs is negative, or out, I or J is NULL");
    if (npairs >= (1L << 29)) return fail(STMMQR_ERR_TOO_LARGE, "covariance entries: more than 2^29 pairs in one call");
    std::vector<int> trip((size_t)(3 * npairs));
    SelInv si;
    PASS(selected_inverse(plan, ncol, nullptr, 0, [&](stmmqr_plan &P) {
        std::vector<long> qinv((size_t)std::max(1L, (long)ncol));          // caller's column -> R's order (Qfill maps [0, ncol) onto itself)
        for (long k = 0; k < ncol; k++) qinv[(size_t)(P.has_qfill ? P.Qfill[(size_t)k] : k)] = k;
        const std::vector<int> cf = column_fronts(P, ncol);
        for (long p = 0; p < npairs; p++) {
            if (I[p] < 0 || I[p] >= ncol || J[p] < 0 || J[p] >= ncol)
                return fail(STMMQR_ERR_INVALID, "covariance entries: pair " + std::to_string(p) + " = (" + std::to_string(I[p]) + ", " + std::to_string(J[p]) +
                                                    ") names a column outside 0 .. ncol - 1 = " + std::to_string(ncol - 1));
            const long k1 = std::min(qinv[(size_t)I[p]], qinv[(size_t)J[p]]), k2 = std::max(qinv[(size_t)I[p]], qinv[(size_t)J[p]]);
            const int f = cf[(size_t)k1];
            const FrontSym &s = P.fs[(size_t)f];
            long l2 = k2 - s.col1;
            if (l2 >= s.fp) {
                const long *rj = P.Rj.data() + s.rp, *hit = std::lower_bound(rj + s.fp, rj + s.fn, k2);
                if (hit == rj + s.fn || *hit != k2)
                    return fail(STMMQR_ERR_INVALID, "covariance entries: pair " + std::to_string(p) + " = columns (" + std::to_string(I[p]) + ", " +
                                                        std::to_string(J[p]) + ") is outside the pattern of the selected inverse (the later column in R's order is no column of the front whose pivots hold the earlier one)");
                l2 = hit - rj;
            }
            trip[(size_t)(3 * p)] = f; trip[(size_t)(3 * p + 1)] = (int)(k1 - s.col1); trip[(size_t)(3 * p + 2)] = (int)l2;
        }
        return 0;
    }, si));
    if (npairs == 0 || !si.ran) return si.ran ? end_resident_op(*plan) : 0;
    stmmqr_plan &P = *plan;
    hipStream_t st = P.stream;
    DevBuf<int> dTrip;
    DevBuf<double> dOut;
    if (dTrip.alloc(trip.size()) || (!on_device && dOut.alloc((size_t)npairs))) return no_memory_for_tables("covariance entries");
    HIPCHK(hipMemcpyAsync(dTrip.p, trip.data(), trip.size() * sizeof(int), hipMemcpyHostToDevice, st));
    double *dout = on_device ? out : dOut.p;
    LCHK(stm_launch_si_entries(si.c, si_view(P, si, nullptr), (int)npairs, dTrip.p, dout, st));
    if (!on_device) HIPCHK(hipMemcpyAsync(out, dout, (size_t)npairs * sizeof(double), hipMemcpyDeviceToHost, st));
    return end_selinv_op(P);
}

int stmmqr_plan_keep_h(const stmmqr_plan *plan) { return plan ? plan->keep_h : -1; }

// ---- a caller's matrix on the device (the sparseqr-level seminormal solve: products with the FULL A, singletons included) ----
struct stm_aop {
    int device = 0;
    hipStream_t st = nullptr;
    long m = 0, n = 0;
    AIndexDev A;
    DevBuf<double> ax, X, B, Y;
    ~stm_aop() { if (st) (void)hipStreamDestroy(st); }
};
int stm_aop_create(int device, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax, stm_aop **out)
{
    if (!out || !Ap || (Ap[n] > 0 && (!Ai || !Ax)) || m < 0 || n < 0) return fail(STMMQR_ERR_INVALID, "bad matrix");
    *out = nullptr;
    const long anz = Ap[n];
    if (m >= (1L << 30) || n >= (1L << 30) || anz >= (1L << 31) - 1) return fail(STMMQR_ERR_TOO_LARGE, "matrix exceeds the 32-bit device index range");
    int e = stm_ensure_device(device);
    if (e) return e;
    std::unique_ptr<stm_aop> op(new (std::nothrow) stm_aop());
    if (!op) return fail(STMMQR_ERR_OUT_OF_MEMORY, "host allocation failed");
    (void)hipGetDevice(&op->device);
    HIPCHK(hipStreamCreateWithFlags(&op->st, hipStreamNonBlocking));
    op->m = m; op->n = n;
    std::vector<int> acp((size_t)n + 1), aci((size_t)std::max(1L, anz)), acol((size_t)std::max(1L, anz)), arp, arj, arq;
    for (long j = 0; j <= n; j++) acp[(size_t)j] = (int)Ap[j];
    for (long p = 0; p < anz; p++) {
        if (Ai[p] < 0 || Ai[p] >= m) return fail(STMMQR_ERR_INVALID, "row index out of range");
        aci[(size_t)p] = (int)Ai[p];
    }
    for (long j = 0; j < n; j++)
        for (long p = Ap[j]; p < Ap[j + 1]; p++) acol[(size_t)p] = (int)j;
    stm_row_form(m, anz, aci.data(), acol.data(), arp, arj, arq);
    std::vector<double> ax(Ax, Ax + anz);
    if (ax.empty()) ax.push_back(0.0);
    LCHK(op->A.cp.upload(acp, op->st)); LCHK(op->A.ci.upload(aci, op->st)); LCHK(op->A.rp.upload(arp, op->st));
    LCHK(op->A.rj.upload(arj, op->st)); LCHK(op->A.rq.upload(arq, op->st)); LCHK(op->ax.upload(ax, op->st));
    HIPCHK(hipStreamSynchronize(op->st));
    *out = op.release();
    return 0;
}
void stm_aop_destroy(stm_aop *op) { delete op; }
int stm_aop_apply(stm_aop *op, int trans, const double *X, stm_long ldx, const double *B, stm_long ldb, double *Y, stm_long ldy,
                  stm_long nrhs)
{
    if (!op) return fail(STMMQR_ERR_INVALID, "null operator");
    const long xr = trans ? op->m : op->n, yr = trans ? op->n : op->m;
    if (nrhs <= 0 || yr == 0) return 0;
    HIPCHK(hipSetDevice(op->device));
    LCHK(upload_cols(op->X, X, ldx, xr, nrhs, op->st));
    if (B) LCHK(upload_cols(op->B, B, ldb, yr, nrhs, op->st));
    LCHK(grow(op->Y, (size_t)(yr * nrhs)));
    LCHK(spmv(op->A, op->ax.p, op->m, op->n, trans, op->X.p, xr, (B && !trans) ? op->B.p : nullptr, trans ? 0 : yr, op->Y.p, yr, nrhs, op->st));
    PASS(copy_cols(Y, ldy, op->Y.p, yr, yr, nrhs, hipMemcpyDeviceToHost, op->st));
    HIPCHK(hipStreamSynchronize(op->st));
    return 0;
}

// The minimum-2-norm solution of A x = b on the QR object of A'; see include/stmmqr_hip.h.  The singleton stages are host code of the
// object (stmmqr_sparseqr.cpp), the multifrontal part is stmmqr_plan_solve_minnorm
int stmmqr_sparseqr_min2norm(stmmqr_qr *qr, const double *B, stm_long ldb, stm_long nrhs, double *X, stm_long ldx)
{
    return stm_sparseqr_min2norm(qr, B, ldb, nrhs, X, ldx, stmmqr_plan_solve_minnorm);
}

// Least squares by the corrected seminormal equations on a SparseQR object (with or without H): x = E R^-1 R^-T E' A'b, then
// `refine` times r = b - A x, x += E R^-1 R^-T E' A'r.  A' and A are the caller's full matrix (singleton rows and columns
// included) on the device (stm_aop); R'\ and R\ are systems 3 and 1 of stmmqr_sparseqr_solve (singleton rows + the plan).
// info: stm_seminormal_info of host sums.
int stmmqr_sparseqr_solve_seminormal(stmmqr_qr *qr, const stm_long *Ap, const stm_long *Ai, const double *Ax, const double *B, stm_long ldb,
                                     stm_long nrhs, double *X, stm_long ldx, int refine, double *info)
{
    stm_long m = 0, n = 0;
    if (!qr || stm_sparseqr_dims(qr, &m, &n) || !Ap || !B || !X || nrhs < 0 || refine < 0)
        return stm_fail(STMMQR_ERR_INVALID, "stmmqr_sparseqr_solve_seminormal: bad arguments");
    if (ldb < m || ldx < n) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_sparseqr_solve_seminormal: bad leading dimension");
    if (Ap[n] < 0) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_sparseqr_solve_seminormal: bad matrix");
    if (info) *info = 0;
    if (nrhs == 0) return 0;
    stm_aop *op = nullptr;
    int e = stm_aop_create(-1, m, n, Ap, Ai, Ax, &op);
    if (e) return e;
    try {
        const size_t M = (size_t)std::max<stm_long>(m, 1), N = (size_t)std::max<stm_long>(n, 1), K = (size_t)nrhs;
        std::vector<double> z(N * K), y(M * K), r(M * K), d(N * K);
        // x = E R^-1 R^-T E' z for z (n x nrhs): out (n x nrhs, leading dimension ld)
        auto rr = [&](double *out, stm_long ld) -> int {
            int e2 = stmmqr_sparseqr_solve(qr, 3, z.data(), (stm_long)N, nrhs, y.data(), (stm_long)M);
            if (!e2) e2 = stmmqr_sparseqr_solve(qr, 1, y.data(), (stm_long)M, nrhs, out, ld);
            return e2;
        };
        e = stm_aop_apply(op, 1, B, ldb, nullptr, 0, z.data(), (stm_long)N, nrhs);                 // z = A'b
        if (!e) e = rr(X, ldx);
        for (int it = 0; it < refine && !e; it++) {
            e = stm_aop_apply(op, 0, X, ldx, B, ldb, r.data(), (stm_long)M, nrhs);                 // r = b - A x
            if (!e) e = stm_aop_apply(op, 1, r.data(), (stm_long)M, nullptr, 0, z.data(), (stm_long)N, nrhs);
            if (!e) e = rr(d.data(), (stm_long)N);
            if (!e)
                for (stm_long j = 0; j < nrhs; j++)
                    for (stm_long k = 0; k < n; k++) X[k + j * ldx] += d[(size_t)k + (size_t)j * N];
        }
        if (!e && info) {
            e = stm_aop_apply(op, 0, X, ldx, B, ldb, r.data(), (stm_long)M, nrhs);
            if (!e) e = stm_aop_apply(op, 1, r.data(), (stm_long)M, nullptr, 0, z.data(), (stm_long)N, nrhs);
            if (!e) {
                double af = 0;
                for (stm_long p = 0; p < Ap[n]; p++) af += Ax[p] * Ax[p];
                std::vector<double> zz(K, 0.0), xx(K, 0.0), bb(K, 0.0);
                for (stm_long j = 0; j < nrhs; j++) {
                    for (stm_long k = 0; k < n; k++) { zz[j] += z[(size_t)k + (size_t)j * N] * z[(size_t)k + (size_t)j * N]; xx[j] += X[k + j * ldx] * X[k + j * ldx]; }
                    for (stm_long i = 0; i < m; i++) bb[j] += B[i + j * ldb] * B[i + j * ldb];
                }
                *info = stm_seminormal_info(std::sqrt(af), zz.data(), xx.data(), bb.data(), nrhs);
            }
        }
    } catch (const std::bad_alloc &) {
        e = stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_sparseqr_solve_seminormal: out of memory");
    }
    stm_aop_destroy(op);
    return e;
}
