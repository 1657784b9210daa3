// stmmqr_planbuild.cpp -- the plan around the pure planner (stmmqr_sched.h): build_plan (the symbolic arrays, relative indices and the
// plan's device memory), the S -> A map of a pattern, plan create / destroy, the regrouping of the fronts (stmmqr_plan_set_groups),
// the index of A for the products with A -- and stm_install_schedule, the one place where a schedule goes into a plan and onto the device.
//
// Reference counterparts (paths relative to /root/reference/STMMQR):
//   stmmqr_plan_create      the allocation / setup half of qr_factorize   src/qr/SparseQR_factorize.c:222-498
#include "stmmqr_plan.h"

namespace {

// The schedule of the plan's grouping (P.group / P.shared) over the fronts `fs`: the plan's symbolic data, the options, knobs and
// recovery state as they are NOW, handed to the pure builder.
sched::Schedule plan_schedule(const stmmqr_plan &P, const std::vector<FrontSym> &fs)
{
    const sched::Inputs in{P.nf, P.Post, P.Child, P.Childp, fs, P.do_rank, P.keep_h, P.maxstack, P.rh_est_total, P.rh_est_front, P.rh_est_scale,
                           P.group, P.shared, {g_opt.big_front_cols, g_opt.pair_update, g_opt.tall_min_rows, g_opt.panel_algo},
                           knobs::BuildKnobs::read(), knobs::once<knobs::K_PART_GRAIN>(), knobs::once<knobs::K_PART_CAP>(),
                           P.rec.overflowed, P.rec.rh_grow, P.rec.full_schedule, P.rec.early_phased};
    return sched::build(in);
}

// The ONE place where a schedule goes into the plan and onto the device (a fresh plan, a regrouping, a rebuild of the recovery): a
// captured graph describes the old step lists and workspaces and goes; the fronts, the recycling's device side, the lists; the
// workspaces and tickets only grow (a regrouping of the same tree usually needs what it needed before; on a fresh plan that is
// "allocate").  The front arenas follow at the next stmmqr_factorize_begin (stm_ensure_arenas).
int stm_install_schedule(stmmqr_plan &P, sched::Schedule &&S)
{
    hipStream_t st = P.stream;
    P.graph.clear();
    P.sch = std::move(S);
    P.sched_gen++;
    const sched::Schedule &Z = P.sch;
    LCHK(P.d_fs.upload(Z.fs, st));
    // slab recycling: bump words, Post-order offsets, kept flags; the R+H arena and the resident scratch of the old schedule go
    if (!P.d_rhtop.p) LCHK(P.d_rhtop.alloc(2));
    if (!P.d_fin.p || P.d_fin.n < (size_t)std::max(1L, P.nf)) LCHK(P.d_fin.alloc((size_t)std::max(1L, P.nf)));
    HIPCHK(hipMemsetAsync(P.d_rhtop.p, 0, 2 * sizeof(long long), st));
    if (Z.recycle) {
        LCHK(P.d_kept.upload(Z.kept, st));
        HIPCHK(hipStreamSynchronize(st));
        P.res.sched.d_scr.release();                             // (allocated by the first resident-factor operation: ensure_scratch)
        P.d_RH.release();                                        // (the arena follows with the front arenas: stm_ensure_arenas)
    }
    auto grow = [](auto &buf, size_t n) -> int { return buf.n >= n && buf.p ? 0 : buf.alloc(n); };
    LCHK(grow(P.d_T, (size_t)STM_PD_RING * Z.tslots * STM_NB * STM_NB));
    LCHK(grow(P.d_Gp, (size_t)Z.tslots * (Z.gp_slabs + 1) * STM_NB * STM_NB));
    LCHK(grow(P.d_Wp, (size_t)Z.wp_doubles));
    LCHK(grow(P.d_Ypend, (size_t)std::max(1LL, Z.yp_doubles)));
    LCHK(P.d_ypoff.upload(Z.ypoff, st));
    LCHK(grow(P.d_Wp2, (size_t)std::max(1LL, Z.wp2_doubles)));
    P.wcnt_n = std::max(P.wcnt_n, (size_t)(Z.wp_doubles / (STM_NB * 32) + 1));
    LCHK(grow(P.d_wcnt, P.wcnt_n));
    LCHK(grow(P.d_wcnt2, P.wcnt_n));
    LCHK(grow(P.d_wflag, P.wcnt_n));
    if (!P.d_abort.p) LCHK(P.d_abort.alloc(4));
    LCHK(grow(P.d_wflag2, P.wcnt_n));
    HIPCHK(hipMemset(P.d_wcnt.p, 0, P.wcnt_n * sizeof(int)));
    HIPCHK(hipMemset(P.d_wcnt2.p, 0, P.wcnt_n * sizeof(int)));
    LCHK(P.d_tslot.upload(Z.tslot, st));
    LCHK(P.d_lists.upload(Z.lists, st));
    LCHK(P.d_wlists.upload(Z.wlists, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
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

    // ---- per-front symbolic sizes (pure: stmmqr_schedule.cpp) ----
    const sched::Symbolic sv{nf, P.Sleft, P.Super, P.Rp, P.Hip, P.Child, P.Childp, P.Post, v.Fm, P.do_rank, P.keep_h,
                             knobs::num(knobs::K_QBIG_MIN), knobs::num(knobs::K_RTBIG_MIN)};
    sched::Fronts F;
    std::string why;
    if (sched::front_syms(sv, F, why)) return fail(STMMQR_ERR_TOO_LARGE, why);
    P.tpanels = F.tpanels;

    // ---- relative indices (value independent): child column -> parent column, S entry -> front column ----
    std::vector<int> Rjrel(std::max(1L, v.rjsize), 0), Sjrel(std::max(1L, v.anz), 0), Sj0(std::max(1L, m), -1);
    {
        std::vector<int> Fmap(std::max(1L, n), -1);
        for (long f = 0; f < nf; f++) {
            const long p1 = P.Rp[f], fn = P.Rp[f + 1] - p1;
            for (long j = 0; j < fn; j++) Fmap[P.Rj[p1 + j]] = (int)j;
            for (long r = F.fs[f].srow0; r < F.fs[f].srow1; r++)
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
    sched::rh_estimate(sv, Rjrel, F);                            // (sizes the R+H arena of the slab recycling)
    P.Fm.swap(F.Fm);
    P.rh_est_total = F.rh_est_total;
    P.rh_est_front.swap(F.rh_est_front);

    // ---- level schedule: one group holding every front (multi-GPU callers regroup with set_groups) ----
    P.group.assign(nf, 0);
    sched::Schedule S = plan_schedule(P, F.fs);

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
    LCHK(stm_install_schedule(P, std::move(S)));
    LCHK(P.d_fnum.alloc(std::max(1L, nf)));
    HIPCHK(hipMemsetAsync(P.d_fnum.p, 0, std::max(1L, nf) * sizeof(FrontNum), st));
    LCHK(P.d_Tall.alloc((size_t)std::max(1LL, P.tpanels) * STM_NB * STM_NB));
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
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

// the arenas themselves: (re)allocated when their size changed (first factorization of a plan, or after a regrouping)
int stm_ensure_arenas(stmmqr_plan &P)
{
    const sched::Schedule &Z = P.sch;
    if (P.d_F.p && P.d_F.n == (size_t)Z.farena && P.d_C.p && P.d_C.n == (size_t)Z.carena &&
        (!Z.recycle || (P.d_RH.p && P.d_RH.n == (size_t)Z.rh_cap)))
        return 0;
    HIPCHK(hipStreamSynchronize(P.stream));
    if (P.d_F.n != (size_t)Z.farena) P.d_F.release();
    if (P.d_C.n != (size_t)Z.carena) P.d_C.release();
    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    const double need = 8.0 * ((P.d_F.p ? 0.0 : (double)Z.farena) + (P.d_C.p ? 0.0 : (double)Z.carena) +
                               ((Z.recycle && P.d_RH.n != (size_t)Z.rh_cap) ? (double)Z.rh_cap : 0.0)) * 1.02;
    if (need > 0.95 * (double)freeb) return fail(STMMQR_ERR_OUT_OF_MEMORY, "front arena does not fit in free HBM");
    if (!P.d_F.p) LCHK(P.d_F.alloc((size_t)Z.farena));
    if (!P.d_C.p) LCHK(P.d_C.alloc((size_t)Z.carena));
    if (Z.recycle && P.d_RH.n != (size_t)Z.rh_cap) LCHK(P.d_RH.alloc((size_t)Z.rh_cap));
    return 0;
}

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
                if (!sched::is_big(P.sch.fs[f], g_opt.big_front_cols))
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
    P.factored = false;                                      // (the factors of the old grouping live at the old offsets)
    // (a plan that holds the whole tree again recycles its slabs: new offsets; the arenas follow at the next stmmqr_factorize_begin)
    return stm_install_schedule(P, plan_schedule(P, P.sch.fs));
}

// Does front f have a contribution-block slot on this plan, allocated, that holds `csize` doubles?  A front that is neither
// factorized here nor a child of a front that is has NO slot (its coff is 0: the first resident block's), and the arenas exist
// only between the first stmmqr_factorize_begin after a (re)grouping and the next regrouping.
int stm_check_c_slot(const stmmqr_plan &P, stm_long f, long long csize, const char *what)
{
    if (f < 0 || f >= P.nf) return fail(STMMQR_ERR_INVALID, std::string(what) + ": no such front");
    if (P.sch.recycle)
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": this plan holds the whole tree and recycles its contribution blocks "
                                        "(nothing to exchange; regroup with stmmqr_plan_set_groups first)");
    if ((size_t)f >= P.sch.has_c.size() || !P.sch.has_c[(size_t)f])
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": the front has no contribution-block slot on this plan (it is neither "
                                        "factorized here nor a child of a front that is)");
    if (!P.d_C.p || P.d_C.n != (size_t)P.sch.carena)
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": the arenas of the current grouping are not allocated yet "
                                        "(stmmqr_factorize_begin comes first)");
    if (csize < 0 || csize > P.sch.c_slot[(size_t)f])
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": the block exceeds the front's slot");
    return 0;
}

}  // extern "C"
