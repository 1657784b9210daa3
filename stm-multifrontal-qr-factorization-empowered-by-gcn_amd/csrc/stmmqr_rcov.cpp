// stmmqr_rcov.cpp -- the selected inverse of R'R on the resident factors and what is read from it: variances, leverages, covariance
// entries (host side; kernels: stmmqr_selinv.hip, stmmqr_leverage.hip; the layout and the pair resolution: stmmqr_restables.cpp).
#include "stmmqr_plan.h"

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
    restab::SelInvLayout lay;            // (lay.sd is the host copy: the upload reads it until the entry point's final synchronization)
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
    const auto &LV = P.sch.glevels[0];
    const long nf = P.nf;
    // ---- the view and where every front's block lies ----
    const restab::SelInvLayout &Y = si.lay = restab::selinv_layout(P.sch.fs, LV, P.sch.lists, P.Rj, ncol);
    // ---- the call's own device memory ----
    const bool own_var = !on_device || !var;
    const size_t rjs = (size_t)std::max(1L, P.rjsize);
    if (si.Z.alloc((size_t)std::max(1LL, Y.zall)) || si.Wk.alloc((size_t)Y.wmax) || si.Lc.alloc(rjs) || si.Pos.alloc(rjs) ||
        si.Rm.alloc((size_t)std::max(1L, nf)) || si.Sd.alloc(Y.sd.size()) || (own_var && si.Var.alloc((size_t)ncol))) {
        (void)hipGetLastError();
        return fail(STMMQR_ERR_OUT_OF_MEMORY, "covariance: no device memory for the blocks of the selected inverse (" +
                                                  std::to_string(8e-9 * ((double)Y.zall + (double)Y.wmax)) + " GB)");
    }
    double *dv = si.dv = own_var ? si.Var.p : var;
    HIPCHK(hipMemcpyAsync(si.Sd.p, Y.sd.data(), Y.sd.size() * sizeof(SiDesc), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dv, 0, (size_t)ncol * sizeof(double), st));                       // (dead columns: 0)
    HIPCHK(hipMemsetAsync(P.res.call.d_err.p, 0, sizeof(int), P.stream));
    const DevCtx c = si.c = res_ctx(P);
    LCHK(stm_launch_si_prep(c, (int)nf, si.Sd.p, si.Lc.p, si.Pos.p, si.Rm.p, P.res.call.d_err.p, st));
    for (size_t l = LV.size(); l-- > 0;) {
        LCHK(level_to_front_form(P, l));
        LCHK(stm_launch_si_level(c, P.d_lists.p + LV[l].all_off, LV[l].n_all, Y.lev_r[l], Y.lev_cn[l], si.Sd.p, si.Rm.p, si.Lc.p, si.Pos.p, P.res.sched.d_Rj.p,
                                 P.has_qfill ? P.res.sched.d_Qfill.p : nullptr, si.Wk.p, si.Z.p, dv, st));
    }
    si.ran = true;
    return 0;
}
// what the leverage and entry kernels read of a finished SelInv, beside their own tables
SiView si_view(const stmmqr_plan &P, const SelInv &si, const int *colfront) { return SiView{si.Sd.p, si.Pos.p, P.res.sched.d_Rj.p, colfront, si.Z.p}; }
int no_memory_for_tables(const char *what)
{
    (void)hipGetLastError();
    return fail(STMMQR_ERR_OUT_OF_MEMORY, std::string(what) + ": no device memory for the call's index tables");
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
    const std::vector<int> cf = restab::column_fronts(P.Super, P.nf, ncol);
    std::vector<int> sp, sj;
    DevBuf<int> dSp, dSj, dCf;
    DevBuf<double> dLev;
    if (upload_narrowed(dSp, P.Sp.data(), (size_t)m + 1, sp, st) || upload_narrowed(dSj, P.Sj.data(), (size_t)P.anz, sj, st) || dCf.alloc(cf.size()) ||
        (!on_device && dLev.alloc((size_t)m))) {
        (void)hipStreamSynchronize(st);                      // (sp / sj may be on their way)
        return no_memory_for_tables("leverage");
    }
    HIPCHK(hipMemcpyAsync(dCf.p, cf.data(), cf.size() * sizeof(int), hipMemcpyHostToDevice, st));
    double *dl = on_device ? lev : dLev.p;
    LCHK(stm_launch_si_leverage(si.c, si_view(P, si, dCf.p), (int)m, (int)ncol, P.res.sched.d_PLinv.p, dSp.p, dSj.p, P.d_Sx.p, dl, P.res.call.d_err.p, st));
    if (!on_device) {
        HIPCHK(hipMemcpyAsync(lev, dl, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
        if (var) HIPCHK(hipMemcpyAsync(var, si.dv, (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    return end_resident_op(P);                               // (synchronizes: sp / sj / cf and the buffers are done with)
}

// Entries Z(I[p], J[p]) of the selected inverse (k_si_entries); see include/stmmqr_hip.h.  Every pair is resolved on the host to
// (front of the earlier column in R's order, its local column, the local column of the later one) before anything is allocated.
int stmmqr_plan_covariance_entries(stmmqr_plan *plan, stm_long ncol, stm_long npairs, const stm_long *I, const stm_long *J, double *out,
                                   int on_device)
{
    PASS(check_factored(plan));
    if (npairs < 0 || (npairs > 0 && (!out || !I || !J))) return fail(STMMQR_ERR_INVALID, "covariance entries: npairs is negative, or out, I or J is NULL");
    if (npairs >= (1L << 29)) return fail(STMMQR_ERR_TOO_LARGE, "covariance entries: more than 2^29 pairs in one call");
    std::vector<int> trip;
    SelInv si;
    PASS(selected_inverse(plan, ncol, nullptr, 0, [&](stmmqr_plan &P) {
        std::string msg;
        return restab::resolve_pairs(P.sch.fs, P.Super, P.Rj, P.has_qfill ? P.Qfill.data() : nullptr, ncol, npairs, I, J, trip, msg)
                   ? fail(STMMQR_ERR_INVALID, msg) : 0;
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
    return end_resident_op(P);
}
