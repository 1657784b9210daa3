// stmmqr_rfactor.cpp -- SURVEY.md 8 (f1): QR_qmult / QR_solve on the factors resident in HBM (host side; kernels: stmmqr_resident.hip).
// The front form, the row map, the passes over the tree and the solves; state and shared surface: stmmqr_resident.h.
#include "stmmqr_plan.h"

// ---------------------------------------------------------------------------------------------
// QR_qmult (SparseQR.c:1790-2020, methods QR_QTX / QR_QX) and QR_solve (RETX_EQUALS_B, :2024-2216)
// on the factors that are still in HBM -- no download of the packed R+H.
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(restab::T4Item) == sizeof(Qt4ItemHost) && offsetof(restab::T4Item, off) == offsetof(Qt4ItemHost, off) &&
              offsetof(restab::T4Item, dqo) == offsetof(Qt4ItemHost, dqo) && offsetof(restab::T4Item, g) == offsetof(Qt4ItemHost, g),
              "restab::T4Item is uploaded as Qt4ItemHost");

// Slab recycling: the resident-factor kernels read fronts in front form.  A front whose slab was recycled is put back into
// that form, level by level, in a scratch that holds the widest tree level (res_ctx: the FrontSym array whose offsets point into
// the scratch; level_to_front_form: zeros + the inverse of k_rh_copy for the level's fronts).  Kept fronts are read where they are
// (their offset is taken relative to the scratch's base: one flat device address space).
// The FrontSym array those kernels read (host copy): fs, or with recycling fs_scr with the kept fronts rebased
std::vector<FrontSym> resident_front_syms(const stmmqr_plan &P)
{
    if (!P.sch.recycle) return P.sch.fs;
    std::vector<FrontSym> t = P.res.sched.fs_scr;
    for (long f = 0; f < P.nf; f++)
        if (P.sch.kept[(size_t)f]) t[(size_t)f].foff = (long long)((P.d_F.p + P.sch.fs[f].foff) - P.res.sched.d_scr.p);
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
// does the plan hold the whole tree in one group (what the condition estimate and the selected inversion ask)
bool holds_whole_tree(const stmmqr_plan &P)
{
    bool whole = P.sch.glevels.size() == 1;
    for (long f = 0; f < P.nf && whole; f++) whole = P.group[(size_t)f] == 0 && !((size_t)f < P.shared.size() && P.shared[(size_t)f]);
    return whole;
}
DevCtx res_ctx(stmmqr_plan &P)
{
    DevCtx c = P.ctx();
    if (P.sch.recycle) { c.fs = P.res.sched.d_fs_scr.p; c.Farena = P.res.sched.d_scr.p; }
    return c;
}
int level_to_front_form(stmmqr_plan &P, size_t l)
{
    if (!P.sch.recycle) return 0;
    const auto &S = P.res.sched;
    const auto &LV = P.sch.glevels[0];
    const DevCtx c = P.ctx();
    // staged blocks back in front form: R+H by k_rh_unpack, R only (keepH = 0) by k_rh_unpack's zero fill + k_r_unpack
    auto unpack = [&](const int *flist, int nfr) -> int {
        if (P.keep_h) return stm_launch_rh_unpack(c, S.d_fs_scr.p, flist, nfr, 64, P.d_kept.p, P.d_RH.p, S.d_scr.p, P.stream);
        return stm_launch_r_unpack(c, flist, nfr, 64, P.d_kept.p, P.d_RH.p, S.d_fs_scr.p, S.d_scr.p, P.stream);
    };
    if (S.scr_all) {
        if (P.res.fact.scr_valid) return 0;
        // every front at once, kept until the next factorization (marked valid only once the launch was accepted)
        const int e = unpack(P.d_lists.p + P.sch.own_off, P.sch.n_own);
        P.res.fact.scr_valid = (e == 0);
        return e;
    }
    if (LV[l].n_all <= 0) return 0;
    return unpack(P.d_lists.p + LV[l].all_off, LV[l].n_all);
}

// rows x cols doubles from one column-major array (leading dimension lds) to another (ldd), host or device by `kind`: one transfer
int copy_cols(double *dst, long ldd, const double *src, long lds, long rows, long cols, hipMemcpyKind kind, hipStream_t st)
{
    if (rows > 0 && cols > 0)
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(double), src, (size_t)lds * sizeof(double), (size_t)rows * sizeof(double), (size_t)cols,
                                kind, st));
    return 0;
}
int to_host(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return 0;
}
int grow(DevBuf<double> &d, size_t n) { return (d.p && d.n >= n) ? 0 : d.alloc(std::max<size_t>(n, 1)); }
int stage_in(DevBuf<double> &d, const double *src, long ld, long rows, long cols, int on_device, hipStream_t st)
{
    LCHK(grow(d, (size_t)(std::max(1L, rows) * cols)));
    return copy_cols(d.p, rows, src, ld, rows, cols, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
}
int stage_out(const DevBuf<double> &d, double *dst, long ld, long rows, long cols, int on_device, hipStream_t st)
{
    PASS(copy_cols(dst, ld, d.p, rows, rows, cols, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
int upload_narrowed(DevBuf<int> &d, const long *v, size_t count, std::vector<int> &t, hipStream_t st)
{
    t.assign(std::max<size_t>(1, count), 0);
    for (size_t i = 0; i < count; i++) t[i] = (int)v[i];
    return d.upload(t, st);
}

namespace {
int ensure_scratch(stmmqr_plan &P)
{
    auto &S = P.res.sched;
    if (!P.sch.recycle || (S.d_scr.p && S.d_fs_scr.p)) return 0;
    // Two layouts.  Where HBM has room (all recycled slabs within a quarter of what is free; STMMQR_RESIDENT_CACHE=0 / 1 forces) the
    // scratch holds EVERY front in front form, rebuilt once per factorization at the first Q-apply / solve and kept for the
    // following ones: the memory comes back only while the factors are being used, never during the factorization.  Otherwise it
    // holds the widest tree level and every level is rebuilt whenever a kernel walks it.
    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    long long all = 0;
    for (long f = 0; f < P.nf; f++) if (!P.sch.kept[(size_t)f]) all += (long long)P.sch.fs[f].ld * P.sch.fs[f].fn;
    const long cache = knobs::num(knobs::K_RESIDENT_CACHE);
    S.scr_all = cache >= 0 ? cache != 0 : (8.0 * (double)all <= 0.25 * (double)freeb);
    S.fs_scr = P.sch.fs_scr;                                     // (the schedule's layout: one tree level at a time)
    if (S.scr_all) {
        long long o = 0;
        for (long f = 0; f < P.nf; f++)
            if (!P.sch.kept[(size_t)f]) { S.fs_scr[(size_t)f].foff = o; o += (long long)P.sch.fs[f].ld * P.sch.fs[f].fn; }
    }
    P.res.new_factorization();                                   // (nothing in the new scratch is in front form)
    LCHK(S.d_scr.alloc((size_t)std::max(1LL, S.scr_all ? all : P.sch.scr_doubles)));
    LCHK(S.d_fs_scr.upload(resident_front_syms(P), P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    return 0;
}

// Of THIS factorization: the row map (restab::row_map) on the device and the host copy of the fronts' numeric results
int map_rows_of_factorization(stmmqr_plan &P)
{
    hipStream_t st = P.stream;
    const long nf = P.nf;
    std::vector<int> hii32((size_t)std::max(1L, P.hisize));
    if (P.hisize > 0)
        HIPCHK(hipMemcpyAsync(hii32.data(), P.d_Hii.p, (size_t)P.hisize * sizeof(int), hipMemcpyDeviceToHost, st));
    if (P.h_fnum.size() != (size_t)nf) P.h_fnum.resize((size_t)nf);
    if (nf > 0)
        HIPCHK(hipMemcpyAsync(P.h_fnum.data(), P.d_fnum.p, (size_t)nf * sizeof(FrontNum), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int> W, rb;
    restab::row_map(P.Sleft, P.Hip, hii32, P.sch.fs, P.h_fnum, P.m, P.n, W, rb);
    LCHK(P.res.fact.d_Wmap.upload(W, st));
    LCHK(P.res.fact.d_rowbase.upload(rb, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// Once per schedule: the static integer maps, the work vectors for one right-hand side, the level tables (restab::level_tables) and
// the descriptors of the split fronts
int build_resident_tables(stmmqr_plan &P)
{
    hipStream_t st = P.stream;
    auto &S = P.res.sched;
    auto &K = P.res.call;
    const long m = P.m, n = P.n;
    std::vector<int> t;                                          // (one host copy for the three: a synchronize before it is reused)
    LCHK(upload_narrowed(S.d_Rj, P.Rj.data(), (size_t)P.rjsize, t, st));
    HIPCHK(hipStreamSynchronize(st));
    LCHK(upload_narrowed(S.d_PLinv, P.PLinv.data(), (size_t)m, t, st));
    HIPCHK(hipStreamSynchronize(st));
    if (P.has_qfill) {
        LCHK(upload_narrowed(S.d_Qfill, P.Qfill.data(), (size_t)n, t, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    LCHK(K.d_W.alloc((size_t)std::max(1L, m)));
    LCHK(K.d_Xs.alloc((size_t)std::max(1L, n)));
    LCHK(K.d_Io.alloc((size_t)std::max(1L, std::max(m, n))));
    LCHK(K.d_err.alloc(1));
    S.T = restab::level_tables(P.sch.fs, P.sch.glevels[0], P.sch.lists, stm_qt4_doubles());
    S.t4_ok = false; S.t4_tried = false; P.res.fact.t4_valid = false;
    LCHK(K.d_Xf.alloc((size_t)S.T.xf_doubles));
    LCHK(S.d_Dq.alloc((size_t)S.T.dq_ints));
    LCHK(K.d_Wq.alloc((size_t)S.T.wq_doubles));
    K.rhs_cap = 1;
    K.d_U.release(); K.d_Xr.release(); S.d_rtLc.release(); S.d_rtRm.release();
    if (!S.T.rtb.empty()) LCHK(S.d_rtb.upload(S.T.rtb, st));
    LCHK(S.d_qb.alloc(S.T.qb.size()));
    LCHK(S.d_Rm.alloc(S.T.qb.size()));
    HIPCHK(hipMemcpy(S.d_qb.p, S.T.qb.data(), S.T.qb.size() * sizeof(QbDesc), hipMemcpyHostToDevice));
    S.gen = P.sched_gen;
    return 0;
}

// what every resident-factor operation needs of the plan and of the factorization it holds, built at the first one after a factorization
int ensure_rowmap(stmmqr_plan &P)
{
    LCHK(ensure_scratch(P));
    auto &S = P.res.sched;
    if (P.res.fact.rowmap_ready && S.gen == P.sched_gen) return 0;
    for (long f = 0; f < P.nf; f++)
        if (P.group[f] < 0) return fail(STMMQR_ERR_INVALID, "Q-apply / solve need every front on this device");
    PASS(map_rows_of_factorization(P));
    if (S.gen != P.sched_gen) PASS(build_resident_tables(P));
    if (restab::live_counts(S.T, P.sch.fs, P.h_fnum, knobs::on(knobs::K_LIVE_PANELS), P.res.fact.live))
        HIPCHK(hipMemcpy(S.d_qb.p, S.T.qb.data(), S.T.qb.size() * sizeof(QbDesc), hipMemcpyHostToDevice));
    // (the planner sends such fronts to the split kernels, so neither can happen; no launch may ask for more LDS than configured)
    for (int b : S.T.lds_qa)
        if (b > STM_RES_LDS_MAX) return fail(STMMQR_ERR_TOO_LARGE, "a front has more rows than the Q-apply kernel holds in LDS");
    for (int b : S.T.lds_rs)
        if (b > STM_RES_LDS_MAX) return fail(STMMQR_ERR_TOO_LARGE, "a front has more columns than the back-substitution kernel holds in LDS");
    P.res.fact.rowmap_ready = true;
    return 0;
}

// the per-vector buffers of the resident-factor operations for a batch of nb right-hand sides (grown on demand, never shrunk)
int ensure_rhs_batch(stmmqr_plan &P, int nb)
{
    auto &K = P.res.call;
    const auto &T = P.res.sched.T;
    if (nb <= K.rhs_cap) return 0;
    const size_t k = (size_t)nb;
    LCHK(K.d_W.alloc(k * (size_t)std::max(1L, P.m)));
    LCHK(K.d_Xs.alloc(k * (size_t)std::max(1L, P.n)));
    LCHK(K.d_Xf.alloc(k * (size_t)T.xf_doubles));
    LCHK(K.d_Wq.alloc(k * (size_t)T.wq_doubles));
    if (K.d_Wq4.p) LCHK(K.d_Wq4.alloc(k * (size_t)std::max(1LL, T.wq4_doubles)));
    if (K.d_U.p) { LCHK(K.d_U.alloc(k * (size_t)std::max(1L, P.rjsize))); LCHK(K.d_Xr.alloc(k * (size_t)std::max(1L, P.m))); }
    K.rhs_cap = nb;
    return 0;
}
RhsBatch rhs_strides(const stmmqr_plan &P)
{
    const auto &T = P.res.sched.T;
    RhsBatch B;
    B.w = P.m; B.x = P.n; B.xf = T.xf_doubles; B.wq = T.wq_doubles; B.wq4 = std::max(1LL, T.wq4_doubles); B.u = std::max(1L, P.rjsize);
    return B;
}
}  // namespace

int check_factored(const stmmqr_plan *plan) { return (plan && plan->factored) ? 0 : fail(STMMQR_ERR_INVALID, "no factorization held by the plan"); }
int begin_resident_op(stmmqr_plan &P) { HIPCHK(hipSetDevice(P.device)); return ensure_rowmap(P); }   // (its refusals go up as they are)
// (where the entry point cleared d_err on its way -- the Q-apply alone does not; synchronizes the stream)
int end_resident_op(stmmqr_plan &P)
{
    int e = 0;
    HIPCHK(hipMemcpyAsync(&e, P.res.call.d_err.p, sizeof(int), hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    if ((e & 3) == 3)
        return fail(STMMQR_ERR_INVALID, "nullspace: pivot " + std::to_string((e >> 2) - 1) + " of the Cholesky factorization of N'N is not positive and finite (R has non-finite entries)");
    if (e == 2) return fail(STMMQR_ERR_INVALID, "internal: two columns of one row of A are not in one block of the selected inverse");
    if (e) return fail(STMMQR_ERR_INVALID, "internal: live pivot count of a front differs from its rank");
    return 0;
}
// the largest batch the operations take in one pass (STMMQR_RHS_BATCH; 1: one vector after the other, as until round 4)
int rhs_batch_max() { return (int)knobs::once<knobs::K_RHS_BATCH>(); }
// op(j0, nb) for the right-hand sides j0 .. j0 + nb - 1, batch after batch: every launch of a pass over the tree carries a whole batch
// (RhsBatch), and the per-vector buffers hold it before op runs
int for_each_batch(stmmqr_plan &P, stm_long nrhs, const std::function<int(stm_long, int)> &op)
{
    for (stm_long j0 = 0; j0 < nrhs; j0 += rhs_batch_max()) {
        const int nb = (int)std::min<stm_long>(rhs_batch_max(), nrhs - j0);
        LCHK(ensure_rhs_batch(P, nb));
        PASS(op(j0, nb));
    }
    return 0;
}

namespace {
// the grouped split Q-apply's buffers, at the first Q-apply that wants them: only where HBM has room (else the per-panel launches stay)
int ensure_t4(stmmqr_plan &P)
{
    auto &S = P.res.sched;
    const auto &T = S.T;
    S.t4_tried = true;
    size_t freeb = 0, totalb = 0;
    if (hipMemGetInfo(&freeb, &totalb) != hipSuccess ||
        !(8.0 * ((double)T.t4_doubles + (double)T.wq4_doubles) + 4.0 * (double)T.dq4_ints < 0.25 * (double)freeb))
        return 0;
    LCHK(S.d_T4.alloc((size_t)T.t4_doubles));
    LCHK(P.res.call.d_Wq4.alloc((size_t)P.res.call.rhs_cap * (size_t)std::max(1LL, T.wq4_doubles)));
    LCHK(S.d_Dq4.alloc((size_t)std::max(1LL, T.dq4_ints)));
    LCHK(S.d_t4items.alloc(T.t4items.size()));                  // (restab::T4Item has Qt4ItemHost's layout: asserted above)
    HIPCHK(hipMemcpyAsync(S.d_t4items.p, T.t4items.data(), T.t4items.size() * sizeof(Qt4ItemHost), hipMemcpyHostToDevice, P.stream));
    LCHK(S.d_t4fronts.upload(T.t4fronts, P.stream));
    LCHK(S.d_t4dqo.upload(T.t4dqo, P.stream));
    LCHK(S.d_qbt4off.upload(T.qbt4off, P.stream));
    S.t4_ok = true;
    P.res.fact.t4_valid = false;
    return 0;
}

// W (device, S-row order; nb vectors at stride m) <- Q' W or Q W
int run_qapply(stmmqr_plan &P, int method, int nb = 1)
{
    auto &S = P.res.sched;
    auto &F = P.res.fact;
    auto &K = P.res.call;
    const auto &T = S.T;
    const RhsBatch B = rhs_strides(P);
    DevCtx c = res_ctx(P);
    const int *L0 = P.d_lists.p;
    const auto &LV = P.sch.glevels[0];
    // blocked form with the kept T factors; STMMQR_DBG bit 13 selects the reflector-by-reflector kernel (same result up
    // to rounding: used by the tests to cross-check the two)
    const bool blocked = c.Tall && !(c.dbg & 8192);
    // grouped split Q-apply: its buffers at the first use (STMMQR_QT4=0: the per-panel launches)
    const bool want_t4 = knobs::on(knobs::K_QT4);                                          // (read at every call: tests compare both)
    if (blocked && want_t4 && !S.t4_tried && !T.t4items.empty()) PASS(ensure_t4(P));
    const bool use_t4 = blocked && want_t4 && S.t4_ok;
    if (use_t4 && knobs::on(knobs::K_MEMDUMP) && !F.t4_valid)
        fprintf(stderr, "[stmmqr_hip] grouped Q-apply: T4 of %zu groups of %zu split fronts, %.3f GB (+ %.3f GB of slab partials)\n", T.t4items.size(),
                T.t4fronts.size(), 8e-9 * (double)T.t4_doubles, 8e-9 * (double)T.wq4_doubles);
    auto launch = [&](size_t l, int m) -> int {
        LCHK(level_to_front_form(P, l));
        if (blocked) {
            LCHK(stm_launch_qapply_t(c, L0 + LV[l].all_off, LV[l].n_all, m, K.d_W.p, T.lds_qa[l], P.stream, nb, B));
            // the large fronts of the level (independent of the others): rows split over workgroups, a launch per group of four panels
            // (k_qbig_step4, T4 built at the first use after a factorization) or per panel
            const auto &Q = T.qbig[l];
            if (Q.n > 0 && use_t4) {
                if (!F.t4_valid) { F.t4_level_valid.assign(LV.size(), 0); F.t4_valid = true; }
                if (!F.t4_level_valid[l]) {                          // (the level's fronts are in front form now: level_to_front_form)
                    LCHK(stm_launch_qt4_build(c, S.d_t4fronts.p + Q.off, S.d_t4dqo.p + Q.off, Q.n, S.d_t4items.p + Q.t4i_off, Q.t4i_n, S.d_Dq4.p,
                                              S.d_T4.p, P.stream));
                    F.t4_level_valid[l] = 1;
                }
                LCHK(stm_launch_qapply_big4(c, S.d_qb.p + Q.off, S.d_qbt4off.p + Q.off, Q.n, F.live.np[l], Q.max_nslab, Q.max_fm, m, K.d_W.p, K.d_Xf.p,
                                            S.d_Dq.p, K.d_Wq4.p, S.d_T4.p, P.stream, nb, B));
                return 0;
            }
            LCHK(stm_launch_qapply_big(c, S.d_qb.p + Q.off, Q.n, F.live.np[l], Q.max_nslab, Q.max_fm, m, K.d_W.p, K.d_Xf.p, S.d_Dq.p,
                                       K.d_Wq.p, P.stream, nb, B));
            return 0;
        }
        if (T.lds_qa_all[l] > STM_RES_LDS_MAX) return fail(STMMQR_ERR_TOO_LARGE, "a front has more rows than the unblocked Q-apply kernel holds in LDS");
        for (int j = 0; j < nb; j++)                                  // (the reflector-by-reflector cross-check kernel: one vector per launch)
            LCHK(stm_launch_qapply(c, L0 + LV[l].all_off, LV[l].n_all, m, K.d_W.p + (size_t)j * (size_t)P.m, T.lds_qa_all[l], K.d_err.p, P.stream));
        return 0;
    };
    if (method == 0) {
        for (size_t l = 0; l < LV.size(); l++) LCHK(launch(l, 0));
    } else {
        for (size_t l = LV.size(); l-- > 0;) LCHK(launch(l, 1));
    }
    return 0;
}

// nb vectors (stride m in `in` / `out`, device, the reference's row order) through Q' (method 0) or Q (method 1) in ONE pass over the tree
int qapply_vectors(stmmqr_plan &P, int method, const double *in, double *out, int nb)
{
    const int m = (int)P.m, scatter = method == 0;
    const int *plinv = P.res.sched.d_PLinv.p, *wmap = P.res.fact.d_Wmap.p;
    double *W = P.res.call.d_W.p;
    // Q': W[PLinv[i]] = x[i], then out[Wmap[r]] = W[r];  Q: W[r] = x[Wmap[r]], then out[i] = W[PLinv[i]]
    LCHK(stm_launch_perm(in, scatter ? plinv : wmap, W, m, scatter, P.stream, nb, m, m));
    LCHK(run_qapply(P, method, nb));
    LCHK(stm_launch_perm(W, scatter ? wmap : plinv, out, m, scatter, P.stream, nb, m, m));
    return 0;
}

// The backward pass, R x = y, from the root to the leaves: y in the device work vectors W (internal row order; nb of them at stride
// m) -> d_Xs (R's column order, stride n).  The kernels read the factorization through c; before_level(l), a launch of the caller's
// or nothing (it returns the launcher's code), comes once the level is in front form, before its solves.
template <class Hook> int r_pass(stmmqr_plan &P, const DevCtx &c, int nb, Hook before_level)
{
    const auto &S = P.res.sched;
    const auto &K = P.res.call;
    const RhsBatch B = rhs_strides(P);
    const int *L0 = P.d_lists.p;
    const auto &LV = P.sch.glevels[0];
    for (size_t l = LV.size(); l-- > 0;) {
        LCHK(level_to_front_form(P, l));
        LCHK(before_level(l));
        LCHK(stm_launch_rsolve(c, L0 + LV[l].all_off, LV[l].n_all, S.d_Rj.p, K.d_W.p, K.d_Xs.p, S.T.lds_rs[l], K.d_err.p, P.stream, nb, B));
        const auto &Q = S.T.qbig[l];             // the large fronts of the level: rows split over workgroups
        LCHK(stm_launch_rsolve_big(c, S.d_qb.p + Q.off, Q.n, P.res.fact.live.rsteps[l], Q.max_nslab, S.d_Rj.p, K.d_W.p, K.d_Xs.p, K.d_Xf.p,
                                   S.d_Dq.p, S.d_Rm.p + Q.off, K.d_err.p, P.stream, nb, B));
    }
    return 0;
}
// the pass vectors of the R' pass and of R' y (U, Xr) at the plan's current batch size, from where ensure_rhs_batch grows them
int ensure_rt_buffers(stmmqr_plan &P)
{
    auto &K = P.res.call;
    if (!K.d_U.p) {
        LCHK(K.d_U.alloc((size_t)K.rhs_cap * (size_t)std::max(1L, P.rjsize)));
        LCHK(K.d_Xr.alloc((size_t)K.rhs_cap * (size_t)std::max(1L, P.m)));
    }
    return 0;
}
}  // namespace

int rsolve_vector(stmmqr_plan &P, int nb) { return r_pass(P, res_ctx(P), nb, [](size_t) { return 0; }); }
// nb vectors Y (device, stride m, R's row order) -> X (device, stride n) = R \ Y or, through Qfill, E (R \ Y): stmmqr_plan_rsolve 0, 1
int r_vectors(stmmqr_plan &P, const double *Y, double *X, int nb, bool through_qfill)
{
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    LCHK(stm_launch_perm(Y, P.res.fact.d_Wmap.p, P.res.call.d_W.p, (int)m, 0, st, nb, m, m));                 // W[r] = y[Wmap[r]]
    LCHK(rsolve_vector(P, nb));
    LCHK(stm_launch_perm(P.res.call.d_Xs.p, (through_qfill && P.has_qfill) ? P.res.sched.d_Qfill.p : nullptr, X, (int)n, 1, st, nb, n, n));   // X[Qfill[j]] = x[j]
    return 0;
}

// The forward pass, R' x = b, from the leaves to the root: b in R's column order in d_Xs (nb vectors at stride n) -> d_Xr (R's row
// order, stride m; rows beyond the rank stay zero).  Two modes that round differently, so neither replaces the other:
//   RT_ONE_WORKGROUP  k_rtsolve, one workgroup per front, on every front; ensure_rt refuses a tree with a front it cannot hold
//   RT_SPLIT          the fronts with FrontSym::rtbig go through k_rtbig_* (init + a launch per block of 32 live pivot columns, all
//                     split fronts of a level together), the others through k_rtsolve; the fronts of a level are independent, and
//                     a split front leaves its pass vector where k_rtsolve leaves it, so either kind feeds either kind.  Sets d_err
//                     on an inconsistent front (end_resident_op); ensure_rt refuses nothing.
// ensure_rt comes before the first batch and makes the pass's own buffers.
int ensure_rt(stmmqr_plan &P, RtMode mode)
{
    auto &S = P.res.sched;
    if (mode == RT_ONE_WORKGROUP)
        for (int need : S.T.lds_rt)
            if (need > STM_RES_LDS_MAX) return fail(STMMQR_ERR_TOO_LARGE, "a front is too wide for the one-workgroup R' solve");
    LCHK(ensure_rt_buffers(P));
    if (mode == RT_SPLIT && !S.d_rtLc.p && !S.T.rtb.empty()) {
        LCHK(S.d_rtLc.alloc((size_t)S.T.rtlc_ints));
        LCHK(S.d_rtRm.alloc(S.T.rtb.size()));
    }
    return 0;
}
int rt_pass(stmmqr_plan &P, int nb, RtMode mode)
{
    const auto &S = P.res.sched;
    const auto &K = P.res.call;
    const RhsBatch B = rhs_strides(P);
    DevCtx c = res_ctx(P);
    const int *L0 = P.d_lists.p, *rowbase = P.res.fact.d_rowbase.p;
    const auto &LV = P.sch.glevels[0];
    HIPCHK(hipMemsetAsync(K.d_Xr.p, 0, (size_t)nb * (size_t)std::max(1L, P.m) * sizeof(double), P.stream));
    for (size_t l = 0; l < LV.size(); l++) {
        const auto &R = S.T.rtbig[l];
        if (mode == RT_SPLIT && R.lds_small > STM_RES_LDS_MAX) return fail(STMMQR_ERR_INVALID, "internal: a front that k_rtsolve cannot hold was not split");
        LCHK(level_to_front_form(P, l));
        if (mode == RT_ONE_WORKGROUP) {
            LCHK(stm_launch_rtsolve(c, L0 + LV[l].all_off, LV[l].n_all, K.d_Xs.p, K.d_U.p, K.d_Xr.p, rowbase, S.T.lds_rt[l], P.stream, nb, B));
            continue;
        }
        if (R.n < LV[l].n_all)
            LCHK(stm_launch_rtsolve(c, L0 + LV[l].all_off, LV[l].n_all, K.d_Xs.p, K.d_U.p, K.d_Xr.p, rowbase, R.lds_small, P.stream, nb, B, 1));
        LCHK(stm_launch_rtsolve_big(c, S.d_rtb.p + R.off, R.n, P.res.fact.live.rtsteps[l], R.max_nslab, K.d_Xs.p, K.d_U.p, K.d_Xr.p, rowbase, S.d_rtLc.p,
                                    S.d_rtRm.p + R.off, K.d_err.p, P.stream, nb, B));
    }
    return 0;
}
// nb vectors Z (device, stride n) -> Y (device, stride m) = R' \ Z or, through Qfill, R' \ (E' Z): stmmqr_plan_rsolve 2, 3
int rt_vectors(stmmqr_plan &P, const double *Z, double *Y, int nb, bool through_qfill)
{
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    // b in R's column order: E'Z gathers through Qfill
    LCHK(stm_launch_perm(Z, (through_qfill && P.has_qfill) ? P.res.sched.d_Qfill.p : nullptr, P.res.call.d_Xs.p, (int)n, 0, st, nb, n, n));
    LCHK(rt_pass(P, nb, RT_ONE_WORKGROUP));
    HIPCHK(hipMemcpyAsync(Y, P.res.call.d_Xr.p, (size_t)nb * (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, st));
    return 0;
}

// ---- products with R and R' (factors with or without H) ----
// Once per schedule, at the first product: per tree level the most row slabs (R x) and column slabs (R' y) of a front -- all R x needs
int ensure_rmult(stmmqr_plan &P)
{
    auto &S = P.res.sched;
    const auto &LV = P.sch.glevels[0];
    if (S.rm_gen == P.sched_gen) return 0;
    S.rm_rslab.assign(LV.size(), 0);
    S.rm_cslab.assign(LV.size(), 0);
    for (size_t l = 0; l < LV.size(); l++)
        for (int q = 0; q < LV[l].n_all; q++) {
            const FrontSym &s = P.sch.fs[P.sch.lists[LV[l].all_off + q]];
            S.rm_rslab[l] = std::max(S.rm_rslab[l], (std::min(s.fp, s.fm_ub) + STM_RM_ROWS - 1) / STM_RM_ROWS);
            S.rm_cslab[l] = std::max(S.rm_cslab[l], (s.fn + STM_RM_COLS - 1) / STM_RM_COLS);
        }
    S.rm_gen = P.sched_gen;
    return 0;
}
// ... and what R' y needs besides, at the first transposed product: the pass-vector array U of the R' solve and the transpose of Rj
int ensure_rtmult(stmmqr_plan &P)
{
    auto &S = P.res.sched;
    PASS(ensure_rmult(P));
    LCHK(ensure_rt_buffers(P));
    if (S.rmt_gen == P.sched_gen) return 0;
    PASS(ensure_rj_transpose(P));
    S.rmt_gen = P.sched_gen;
    return 0;
}
// the transpose of Rj on the device, for whoever walks a column of R through its fronts (R' y, the sparse R)
int ensure_rj_transpose(stmmqr_plan &P)
{
    auto &S = P.res.sched;
    if (S.rjt_gen == P.sched_gen) return 0;
    std::vector<int> cp, slot;
    restab::rj_transpose(P.Rj, P.n, cp, slot);
    LCHK(S.d_rmslot.upload(slot, P.stream));
    LCHK(S.d_rmcp.upload(cp, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));                    // (cp / slot are local)
    S.rjt_gen = P.sched_gen;
    return 0;
}
// nb vectors X (device, R's column order, stride n) -> Y (device, R's row order, stride m) = R X; rows beyond the rank are zero
int rmult_pass(stmmqr_plan &P, const double *X, double *Y, int nb, int twofold)
{
    const auto &S = P.res.sched;
    const RhsBatch B = rhs_strides(P);
    const DevCtx c = res_ctx(P);
    const auto &LV = P.sch.glevels[0];
    HIPCHK(hipMemsetAsync(Y, 0, (size_t)nb * (size_t)std::max(1L, P.m) * sizeof(double), P.stream));
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        if (twofold) LCHK(stm_launch_rmult_dd(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, S.rm_rslab[l], S.d_Rj.p, P.res.fact.d_rowbase.p, X, Y, P.stream, nb, B));
        else LCHK(stm_launch_rmult(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, S.rm_rslab[l], S.d_Rj.p, P.res.fact.d_rowbase.p, X, Y, P.stream, nb, B));
    }
    return 0;
}
// nb vectors Y (device, R's row order, stride m; rows beyond the rank are not read) -> Z (device, R's column order, stride n) = R' Y,
// or with absval the column 1-norms of R (one vector, Y not read)
int rtmult_pass(stmmqr_plan &P, const double *Y, double *Z, int nb, int absval)
{
    const auto &S = P.res.sched;
    double *U = P.res.call.d_U.p;
    const RhsBatch B = rhs_strides(P);
    const DevCtx c = res_ctx(P);
    const auto &LV = P.sch.glevels[0];
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        LCHK(stm_launch_rtmult_dots(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, S.rm_cslab[l], P.res.fact.d_rowbase.p, Y, U, absval, P.stream, nb, B));
    }
    return stm_launch_rtmult_gather(S.d_rmcp.p, S.d_rmslot.p, U, Z, (int)P.n, P.stream, nb, B.u, P.n);
}

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
    DevBuf<double> &dX = P.res.call.d_Xall;
    PASS(stage_in(dX, H, ldh, m, k, 0, P.stream));
    PASS(for_each_batch(P, k, [&](stm_long j, int nb) { return qapply_vectors(P, vm, dX.p + j * m, dX.p + j * m, nb); }));
    PASS(stage_out(dX, H, ldh, m, k, 0, P.stream));
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
    auto &K = P.res.call;
    const long m = P.m, n = P.n, brows = (system <= 1) ? m : n, xrows = (system <= 1) ? n : m;
    if (ldb < brows || ldx < xrows) return fail(STMMQR_ERR_INVALID, "bad leading dimension");
    PASS(begin_resident_op(P));
    if (nrhs == 0) return 0;
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), P.stream));
    PASS(stage_in(K.d_Xall, B, ldb, brows, nrhs, 0, P.stream));
    LCHK(grow(K.d_Yall, (size_t)(xrows * nrhs)));
    if (system >= 2) PASS(ensure_rt(P, RT_ONE_WORKGROUP));
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) {
        return system <= 1 ? r_vectors(P, K.d_Xall.p + j * m, K.d_Yall.p + j * n, nb, system == 1)
                           : rt_vectors(P, K.d_Xall.p + j * n, K.d_Yall.p + j * m, nb, system == 3);
    }));
    PASS(stage_out(K.d_Yall, X, ldx, xrows, nrhs, 0, P.stream));
    return end_resident_op(P);
}

// X (n x nrhs, ldx >= n) = E * R^{-1} * (Q' B)(1:n)  for B (m x nrhs, ldb >= m): QR_qmult(QR_QTX) followed by
// QR_solve(QR_RETX_EQUALS_B), the driver's least-squares solve (qrtest.c:11-53), without the trip to the host in between;
// dead columns get x = 0 (basic solution).
int stmmqr_plan_solve(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs)
{
    return plan_solve(plan, B, ldb, X, ldx, nrhs, 0);
}
int plan_solve(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs, int on_device)
{
    PASS(check_factored(plan));
    if (!B || !X || ldb < plan->m || ldx < plan->n || nrhs < 0) return fail(STMMQR_ERR_INVALID, "bad solve arguments");
    if (!plan->keep_h)
        return fail(STMMQR_ERR_INVALID, "the plan keeps no Householder vectors (keepH = 0): no Q'B; stmmqr_plan_solve_seminormal solves with R only");
    stmmqr_plan &P = *plan;
    auto &K = P.res.call;
    PASS(begin_resident_op(P));
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    if (nrhs == 0) return 0;
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), P.stream));
    PASS(stage_in(K.d_Xall, B, ldb, m, nrhs, on_device, st));
    LCHK(grow(K.d_Yall, (size_t)(n * nrhs)));
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) -> int {
        LCHK(stm_launch_perm(K.d_Xall.p + j * m, P.res.sched.d_PLinv.p, K.d_W.p, (int)m, 1, st, nb, m, m));
        LCHK(run_qapply(P, 0, nb));
        LCHK(rsolve_vector(P, nb));
        LCHK(stm_launch_perm(K.d_Xs.p, P.has_qfill ? P.res.sched.d_Qfill.p : nullptr, K.d_Yall.p + j * n, (int)n, 1, st, nb, n, n));   // X[Qfill[j]] = x[j]
        return 0;
    }));
    PASS(stage_out(K.d_Yall, X, ldx, n, nrhs, on_device, st));
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
    auto &K = P.res.call;
    PASS(begin_resident_op(P));
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    if (nrhs == 0 || m == 0) return 0;
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), st));
    PASS(stage_in(K.d_Xall, B, ldb, n, nrhs, on_device, st));
    LCHK(grow(K.d_Yall, (size_t)(m * nrhs)));
    PASS(ensure_rt(P, RT_SPLIT));
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) -> int {
        // b in R's column order (E'B gathers through Qfill), y = R' \ b in R's row order, x = Q y in the caller's row order
        LCHK(stm_launch_perm(K.d_Xall.p + j * n, (!permuted && P.has_qfill) ? P.res.sched.d_Qfill.p : nullptr, K.d_Xs.p, (int)n, 0, st, nb, n, n));
        PASS(rt_pass(P, nb, RT_SPLIT));
        return qapply_vectors(P, 1, K.d_Xr.p, K.d_Yall.p + j * m, nb);
    }));
    PASS(stage_out(K.d_Yall, X, ldx, m, nrhs, on_device, st));
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
    auto &K = P.res.call;
    // ---- the view: FrontSym of the array the resident-factor kernels read (res_ctx) with fp cut back, the B fronts level by level ----
    std::vector<FrontSym> vs = resident_front_syms(P);
    std::vector<int> blist, boff;
    restab::carried_view(P.sch.fs, P.sch.glevels[0], P.sch.lists, n, vs, blist, boff);
    if (K.d_fs_car.n != vs.size()) LCHK(K.d_fs_car.alloc(vs.size()));
    if (K.d_carlist.n < blist.size()) LCHK(K.d_carlist.alloc(blist.size()));
    if (!vs.empty()) HIPCHK(hipMemcpyAsync(K.d_fs_car.p, vs.data(), vs.size() * sizeof(FrontSym), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(K.d_carlist.p, blist.data(), blist.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                            // (vs / blist are pageable and local)
    if (K.d_fnum_car.n != (size_t)std::max(1L, P.nf)) LCHK(K.d_fnum_car.alloc((size_t)std::max(1L, P.nf)));
    if (P.nf > 0) HIPCHK(hipMemcpyAsync(K.d_fnum_car.p, P.d_fnum.p, (size_t)P.nf * sizeof(FrontNum), hipMemcpyDeviceToDevice, st));
    LCHK(grow(K.d_carN, (size_t)nrhs));
    HIPCHK(hipMemsetAsync(K.d_carN.p, 0, (size_t)nrhs * sizeof(double), st));
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), P.stream));
    LCHK(grow(K.d_Yall, (size_t)(std::max(1L, n) * nrhs)));
    const DevCtx ct = res_ctx(P);
    DevCtx cv = ct;
    cv.fs = K.d_fs_car.p; cv.fnum = K.d_fnum_car.p;
    PASS(for_each_batch(P, nrhs, [&](stm_long j0, int nb) -> int {
        HIPCHK(hipMemsetAsync(K.d_W.p, 0, (size_t)nb * (size_t)std::max(1L, m) * sizeof(double), st));
        HIPCHK(hipMemsetAsync(K.d_Xs.p, 0, (size_t)nb * (size_t)na * sizeof(double), st));
        LCHK(stm_launch_carried_seed(K.d_Xs.p, na, (int)n, (int)j0, nb, st));
        // (the first pass sets the view's ranks of the level's B fronts before its kernels read them, and takes the residual norms
        //  while the level is in front form)
        PASS(r_pass(P, cv, nb, [&](size_t l) {
            return j0 == 0 ? stm_launch_carried_view(ct, K.d_carlist.p + boff[l], boff[l + 1] - boff[l], (int)n, K.d_fnum_car.p, K.d_carN.p, st) : 0;
        }));
        LCHK(stm_launch_perm(K.d_Xs.p, P.has_qfill ? P.res.sched.d_Qfill.p : nullptr, K.d_Yall.p + j0 * n, (int)n, 1, st, nb, na, n));   // X[Qfill[j]] = x[j], j < n
        return 0;
    }));
    if (resid) HIPCHK(hipMemcpyAsync(resid, K.d_carN.p, (size_t)nrhs * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    PASS(stage_out(K.d_Yall, X, ldx, n, nrhs, on_device, st));
    return end_resident_op(P);
}

int stmmqr_plan_keep_h(const stmmqr_plan *plan) { return plan ? plan->keep_h : -1; }
