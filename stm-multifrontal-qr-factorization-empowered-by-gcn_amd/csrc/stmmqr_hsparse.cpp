// stmmqr_hsparse.cpp -- H of the resident factors out as compressed sparse columns, with HTau and HPinv, written on the device (factors
// with H; host side, kernels: stmmqr_hsparse.hip; the level walk is that of stmmqr_rsparse.cpp).  The host export
// (stmmqr_plan_export_r, stmmqr_export.cpp) downloads the packed stack and converts it on one thread; this counts, scans and compacts
// where the factors are and moves the kept entries only -- or nothing, when the caller's arrays are on the device.
#include "stmmqr_plan.h"

static_assert(sizeof(stm_long) == sizeof(long long), "the kernels write Hp / Hi / HPinv as 64-bit integers");

namespace {
// the buffers, at the first call (kept with the schedule: their sizes are the plan's)
int ensure_hsparse(stmmqr_plan &P)
{
    auto &S = P.res.sched;
    PASS(ensure_rmult(P));                                     // (the column slabs per level)
    const size_t slots = (size_t)std::max(1L, P.rjsize);
    if (!S.d_hsInfo.p) LCHK(S.d_hsInfo.alloc(4));
    if (!S.d_hsSlot.p) LCHK(S.d_hsSlot.alloc(3 * slots));
    if (!S.d_hsOff.p) LCHK(S.d_hsOff.alloc(slots));
    return 0;
}
}  // namespace

int stmmqr_plan_h_sparse(stmmqr_plan *plan, stm_long *Hp, stm_long *Hi, double *Hx, double *HTau, stm_long *HPinv, stm_long colcap,
                         stm_long cap, stm_long *info, int on_device)
{
    PASS(check_factored(plan));
    stmmqr_plan &P = *plan;
    const long m = P.m;
    if (!info) return fail(STMMQR_ERR_INVALID, "h_sparse: info is NULL");
    if (!P.keep_h) return fail(STMMQR_ERR_INVALID, "h_sparse: the plan keeps no Householder vectors (keepH = 0): no H to export");
    const int given = (Hp != nullptr) + (Hi != nullptr) + (Hx != nullptr) + (HTau != nullptr);
    if (given != 0 && given != 4)
        return fail(STMMQR_ERR_INVALID, "h_sparse: Hp, Hi, Hx and HTau must all be given (fill) or all be NULL (count)");
    if (colcap < 0) return fail(STMMQR_ERR_INVALID, "h_sparse: colcap = " + std::to_string(colcap) + " is negative");
    if (cap < 0) return fail(STMMQR_ERR_INVALID, "h_sparse: cap = " + std::to_string(cap) + " is negative");
    if (!holds_whole_tree(P))
        return fail(STMMQR_ERR_INVALID, "h_sparse: the plan does not hold the whole tree in one group (groups were set, or fronts are imported or shared)");
    PASS(begin_resident_op(P));
    auto &S = P.res.sched;
    hipStream_t st = P.stream;
    HIPCHK(hipMemsetAsync(P.res.call.d_err.p, 0, sizeof(int), st));
    PASS(ensure_hsparse(P));
    const bool fill = given == 4;
    const size_t slots = (size_t)std::max(1L, P.rjsize);
    const DevCtx c = res_ctx(P);
    const auto &LV = P.sch.glevels[0];
    int *cnt = S.d_hsSlot.p, *vis = cnt + slots, *col = vis + slots;

    // ---- count: one walk over the tree, the scan over the slots ----
    HIPCHK(hipMemsetAsync(cnt, 0, 3 * slots * sizeof(int), st));
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        LCHK(stm_launch_hs_count(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, S.rm_cslab[l], cnt, vis, col, st));
    }
    LCHK(stm_launch_hs_scan(cnt, vis, col, S.d_hsOff.p, P.rjsize, m, S.d_hsInfo.p, st));
    long long hinfo[4] = {0, 0, 0, 0};
    PASS(to_host(hinfo, S.d_hsInfo.p, sizeof hinfo, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 4; i++) info[i] = (stm_long)hinfo[i];
    const long long nh = hinfo[0], hnz = hinfo[1];
    if (fill && (colcap < nh || cap < hnz)) {
        PASS(end_resident_op(P));
        return fail(STMMQR_ERR_INVALID, "h_sparse: H has nh = " + std::to_string(nh) + " columns and hnz = " + std::to_string(hnz) +
                                            " entries, the arrays hold colcap = " + std::to_string(colcap) + " and cap = " + std::to_string(cap));
    }
    // the caller's arrays, or with host arrays their device images for the length of the call
    DevBuf<long long> t_p, t_i, t_pinv;
    DevBuf<double> t_x, t_tau;
    if (HPinv && m > 0) {
        long long *dpinv = (long long *)HPinv;
        if (!on_device) { LCHK(t_pinv.alloc((size_t)m)); dpinv = t_pinv.p; }
        LCHK(stm_launch_hs_pinv(S.d_PLinv.p, P.res.fact.d_Wmap.p, (int)m, dpinv, st));
        if (!on_device) PASS(to_host(HPinv, dpinv, (size_t)m * sizeof(long long), st));
    }
    if (!fill) return end_resident_op(P);

    // ---- fill: the columns' starts and Tau, then the same walk, every entry at its place ----
    long long *dp = (long long *)Hp, *di = (long long *)Hi;
    double *dx = Hx, *dtau = HTau;
    if (!on_device) {
        LCHK(t_p.alloc((size_t)nh + 1)); LCHK(t_tau.alloc((size_t)std::max(1LL, nh)));
        LCHK(t_i.alloc((size_t)std::max(1LL, hnz))); LCHK(t_x.alloc((size_t)std::max(1LL, hnz)));
        dp = t_p.p; dtau = t_tau.p; di = t_i.p; dx = t_x.p;
    }
    LCHK(stm_launch_hs_cols(c.Tau, cnt, col, S.d_hsOff.p, (int)P.rjsize, S.d_hsInfo.p, dp, dtau, st));
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        LCHK(stm_launch_hs_fill(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, S.rm_cslab[l], P.res.fact.d_Wmap.p, S.d_hsOff.p, di, dx, st));
    }
    if (!on_device) {
        PASS(to_host(Hp, dp, ((size_t)nh + 1) * sizeof(long long), st));
        PASS(to_host(HTau, dtau, (size_t)nh * sizeof(double), st));
        PASS(to_host(Hi, di, (size_t)hnz * sizeof(long long), st));
        PASS(to_host(Hx, dx, (size_t)hnz * sizeof(double), st));
    }
    return end_resident_op(P);                                 // (waits for the stream: the call is complete on return)
}
