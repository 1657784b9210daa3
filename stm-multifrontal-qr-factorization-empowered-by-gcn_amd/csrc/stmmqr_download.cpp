// stmmqr_download.cpp -- the factors out of the plan in the reference's layout.
//
// Reference counterparts (paths relative to /root/reference/STMMQR):
//   stmmqr_plan_download    the wrap-up half of qr_factorize (src/qr/SparseQR_factorize.c:554-742) incl. qr_hpinv (:991-1060)
#include "stmmqr_plan.h"

extern "C" {

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
    if (Stack && P.rh_total > 0 && P.sch.recycle) {
        // slab recycling: the blocks lie in the arena in the order the fronts finished (kept fronts: still in front form); the
        // reference's layout is produced window by window in a bounce buffer (k_rh_window) and copied out, two windows in flight
        const long long win = std::min<long long>(P.rh_total, knobs::num(knobs::K_DOWNLOAD_WIN));     // 256 MB windows (STMMQR_DOWNLOAD_WIN)
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
            if (!rc && (P.keep_h ? stm_launch_rh_window(c, P.d_lists.p + P.sch.own_off, P.sch.n_own, parts, P.d_fin.p, P.d_kept.p, P.d_RH.p, w0, w1, out, st)
                                 : stm_launch_r_window(c, P.d_lists.p + P.sch.own_off, P.sch.n_own, parts, P.d_fin.p, P.d_kept.p, P.d_RH.p, w0, w1, out, st)))
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
        HIPCHK(hipMemcpyAsync(rboff.data(), P.sch.recycle ? P.d_fin.p : P.d_Rboff.p, (size_t)nf * sizeof(long long), hipMemcpyDeviceToHost, st));
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
            const long cn = P.sch.fs[f].fn - P.sch.fs[f].fp;
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

}  // extern "C"
