// stmmqr_rsparse.cpp -- R of the resident factors out as compressed sparse columns or rows, written on the device (factors with or
// without H; host side, kernels: stmmqr_rsparse.hip; the level walk is that of the products with R, stmmqr_rfactor.cpp).  The host
// export (stmmqr_plan_export_r, stmmqr_export.cpp) downloads the packed stack and converts it on one thread; this counts, scans and
// compacts where the factors are and moves the kept entries only -- or nothing, when the caller's arrays are on the device.
#include "stmmqr_plan.h"

static_assert(sizeof(stm_long) == sizeof(long long), "the kernels write ptr / idx as 64-bit integers");

namespace {
// the buffers of a form, at its first call (kept with the schedule: their sizes are the plan's)
int ensure_rsparse(stmmqr_plan &P, int form)
{
    auto &S = P.res.sched;
    PASS(ensure_rmult(P));
    const size_t slots = (size_t)std::max(1L, P.rjsize), rows = (size_t)std::max(1L, P.m), items = (size_t)std::max(P.m, P.n);
    if (!S.d_rsInfo.p) LCHK(S.d_rsInfo.alloc(4));
    if (!S.d_rsPart.p) LCHK(S.d_rsPart.alloc(items / 256 + 1));
    if (form == STMMQR_RSPARSE_CSC) {
        PASS(ensure_rj_transpose(P));
        if (!S.d_rsSlot.p) LCHK(S.d_rsSlot.alloc(2 * slots));
        if (!S.d_rsOff.p) LCHK(S.d_rsOff.alloc(slots));
    } else if (!S.d_rsRow.p) LCHK(S.d_rsRow.alloc(2 * rows));
    return 0;
}
}  // namespace

int stmmqr_plan_device_index(const stmmqr_plan *plan) { return plan ? plan->device : -1; }

int stmmqr_plan_r_sparse(stmmqr_plan *plan, int form, stm_long ncol, stm_long econ, stm_long *ptr, stm_long *idx, double *val, stm_long cap,
                         stm_long *info, int on_device)
{
    PASS(check_factored(plan));
    stmmqr_plan &P = *plan;
    const long m = P.m, n = P.n;
    if (form != STMMQR_RSPARSE_CSC && form != STMMQR_RSPARSE_CSR)
        return fail(STMMQR_ERR_INVALID, "r_sparse: form = " + std::to_string(form) + " is neither 0 (compressed columns) nor 1 (compressed rows)");
    if (ncol < 0 || ncol > n)
        return fail(STMMQR_ERR_INVALID, "r_sparse: ncol = " + std::to_string(ncol) + " is not between 0 and the " + std::to_string(n) + " columns of the plan");
    if (econ < 0) return fail(STMMQR_ERR_INVALID, "r_sparse: econ = " + std::to_string(econ) + " is negative");
    if (cap < 0) return fail(STMMQR_ERR_INVALID, "r_sparse: cap = " + std::to_string(cap) + " is negative");
    if (!ptr) return fail(STMMQR_ERR_INVALID, "r_sparse: ptr is NULL");
    if (!info) return fail(STMMQR_ERR_INVALID, "r_sparse: info is NULL");
    if ((idx == nullptr) != (val == nullptr)) return fail(STMMQR_ERR_INVALID, "r_sparse: idx and val must both be given (fill) or both be NULL (count)");
    if (!holds_whole_tree(P))
        return fail(STMMQR_ERR_INVALID, "r_sparse: the plan does not hold the whole tree in one group (groups were set, or fronts are imported or shared)");
    PASS(begin_resident_op(P));
    auto &S = P.res.sched;
    hipStream_t st = P.stream;
    HIPCHK(hipMemsetAsync(P.res.call.d_err.p, 0, sizeof(int), st));
    PASS(ensure_rsparse(P, form));
    const bool csc = form == STMMQR_RSPARSE_CSC, fill = idx != nullptr;
    const long nitems = csc ? (long)ncol : m;
    const int nc = (int)ncol, ec = (int)std::min<stm_long>(econ, m);
    long long rtot = 0;
    for (long f = 0; f < P.nf; f++) rtot += P.h_fnum[(size_t)f].rank;
    const DevCtx c = res_ctx(P);
    const auto &LV = P.sch.glevels[0];
    const int *dRj = S.d_Rj.p, *rowbase = P.res.fact.d_rowbase.p;
    int *cnt = csc ? S.d_rsSlot.p : S.d_rsRow.p;
    int *vis = cnt + (csc ? std::max(1L, P.rjsize) : std::max(1L, m));
    // the caller's arrays, or with host arrays their device images for the length of the call
    DevBuf<long long> t_ptr, t_idx;
    DevBuf<double> t_val;
    long long *dptr = (long long *)ptr;
    if (!on_device) { LCHK(t_ptr.alloc((size_t)nitems + 1)); dptr = t_ptr.p; }

    // ---- count: one walk over the tree, the sums per item, the scan ----
    HIPCHK(hipMemsetAsync(cnt, 0, 2 * (size_t)(csc ? std::max(1L, P.rjsize) : std::max(1L, m)) * sizeof(int), st));
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        const int *flist = P.d_lists.p + LV[l].all_off;
        if (csc) LCHK(stm_launch_rs_count_cols(c, flist, LV[l].n_all, S.rm_cslab[l], dRj, rowbase, nc, ec, cnt, vis, st));
        else LCHK(stm_launch_rs_rows(c, flist, LV[l].n_all, S.rm_rslab[l], dRj, rowbase, nc, ec, cnt, vis, nullptr, nullptr, nullptr, 0, st));
    }
    LCHK(stm_launch_rs_item_sums(csc ? S.d_rmcp.p : nullptr, csc ? S.d_rmslot.p : nullptr, cnt, vis, (int)nitems, dptr, S.d_rsPart.p, st));
    LCHK(stm_launch_rs_scan(dptr, nitems, S.d_rsPart.p, (int)((nitems + 255) / 256), rtot, S.d_rsInfo.p, st));
    long long hinfo[4] = {0, 0, 0, 0};
    PASS(to_host(hinfo, S.d_rsInfo.p, sizeof hinfo, st));
    if (!on_device) PASS(to_host(ptr, dptr, ((size_t)nitems + 1) * sizeof(long long), st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 4; i++) info[i] = (stm_long)hinfo[i];
    const long long nnz = hinfo[0];
    if (!fill) return end_resident_op(P);
    if (cap < nnz) {
        PASS(end_resident_op(P));
        return fail(STMMQR_ERR_INVALID, "r_sparse: R has nnz = " + std::to_string(nnz) + " entries, the arrays hold cap = " + std::to_string(cap));
    }

    // ---- fill: the same walk, every entry at its place ----
    long long *didx = (long long *)idx;
    double *dval = val;
    if (!on_device) {
        LCHK(t_idx.alloc((size_t)std::max(1LL, nnz))); LCHK(t_val.alloc((size_t)std::max(1LL, nnz)));
        didx = t_idx.p; dval = t_val.p;
    }
    if (csc) LCHK(stm_launch_rs_slot_offsets(S.d_rmcp.p, S.d_rmslot.p, cnt, dptr, S.d_rsOff.p, nc, st));
    for (size_t l = 0; l < LV.size(); l++) {
        LCHK(level_to_front_form(P, l));
        const int *flist = P.d_lists.p + LV[l].all_off;
        if (csc) LCHK(stm_launch_rs_fill_cols(c, flist, LV[l].n_all, S.rm_cslab[l], dRj, rowbase, nc, ec, S.d_rsOff.p, didx, dval, st));
        else LCHK(stm_launch_rs_rows(c, flist, LV[l].n_all, S.rm_rslab[l], dRj, rowbase, nc, ec, cnt, vis, dptr, didx, dval, 1, st));
    }
    if (!on_device) {
        PASS(to_host(idx, didx, (size_t)nnz * sizeof(long long), st));
        PASS(to_host(val, dval, (size_t)nnz * sizeof(double), st));
    }
    return end_resident_op(P);                                 // (waits for the stream: the call is complete on return)
}
