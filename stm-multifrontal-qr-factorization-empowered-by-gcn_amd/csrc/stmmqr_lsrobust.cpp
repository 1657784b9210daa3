// stmmqr_lsrobust.cpp -- robust least squares on either kind of least-squares object: iteratively reweighted solves with row
// multipliers made from the UNWEIGHTED residual on the device (the kernels of stmmqr_lsrobust.hip).
//   stmmqr_median_abs          the selection alone, no object
//   stmmqr_ls_robust_weights   one reweighting from a given X: r = b - A x, a = |w0 o r|, sigma, w, the statistics
//   stmmqr_ls_solve_robust     the loop: reweighting, then the object's own solve with the device w -- stmmqr_ls_solve_damped on a damped
//                              object; on a plain one stmmqr_ls_solve of the weighted values w[Ai[p]] * Ax[p] and w o b, built into work
//                              buffers by one multiplication each
// Between two solves nothing crosses the bus but the eight statistics of a reweighting and the two maxima of the step.  What the
// feature keeps on the device (stmmqr_ls::Robust) is made at the first call: the row form of A (m + 1 + 2 anz ints), built on the
// host from the pattern the object keeps, and the work vectors.
#include <cfloat>
#include <new>

#include "stmmqr_lsobj.h"

namespace {

// what a call works with: the loss, its constant, the scale rule
struct Rule { int loss; double cc, sigma, mad, smin; };

const double DEFAULT_CC[5] = {1.0, 1.345, 2.3849, 4.6851, 0.0};     // (L2 has no constant: any positive one; L1 has no default)

// the refusals the two entry points share, decided before the device is looked at (the host half last: every other one can be
// decided on it)
int robust_args(const std::string &F, const stmmqr_ls *ls, const stmmqr_ls_robust *rb, Rule &R)
{
    if (!ls) return fail(STMMQR_ERR_INVALID, F + "null object");
    if (ls->nrhs != 1)
        return fail(STMMQR_ERR_INVALID, F + "the object was created with nrhs = " + std::to_string(ls->nrhs) + " (a robust fit takes nrhs = 1)");
    if (!rb) return fail(STMMQR_ERR_INVALID, F + "null rule (rb)");
    if (rb->loss < 0 || rb->loss > 4) return fail(STMMQR_ERR_INVALID, F + "loss must be 0 .. 4");
    if (!std::isfinite(rb->sigma) || !std::isfinite(rb->sigma_min) || !std::isfinite(rb->cc) || !std::isfinite(rb->mad_factor))
        return fail(STMMQR_ERR_INVALID, F + "sigma, sigma_min, cc and mad_factor must be finite");
    if (rb->sigma < 0) return fail(STMMQR_ERR_INVALID, F + "sigma is negative");
    if (rb->sigma_min < 0) return fail(STMMQR_ERR_INVALID, F + "sigma_min is negative");
    if (rb->loss == 4 && rb->cc <= 0) return fail(STMMQR_ERR_INVALID, F + "the smoothed L1 loss has no default cc: cc > 0 required");
    R.loss = rb->loss;
    R.cc = rb->cc > 0 ? rb->cc : DEFAULT_CC[rb->loss];
    R.sigma = rb->sigma;
    R.mad = rb->mad_factor > 0 ? rb->mad_factor : 1.4826;
    R.smin = rb->sigma_min;
    return 0;
}

int device_half(const std::string &F, const stmmqr_ls *ls)
{
    if (!ls->plan) return fail(STMMQR_ERR_INVALID, F + "the object holds the host half only (device = -2 at create)");
    const stm_long m = ls->damped ? ls->am : ls->m, anz = ls->damped ? ls->aanz : ls->anz;
    if (m >= INT_MAX || anz >= INT_MAX || ls->n >= INT_MAX)
        return fail(STMMQR_ERR_INVALID, F + "2^31 or more rows, columns or entries (the row form of A is int)");
    return 0;
}

template <class T> int want(DevBuf<T> &b, size_t count)
{
    return (b.p && b.n >= count) ? 0 : b.alloc(std::max<size_t>(count, 1));
}

// the row form of A and the work vectors, once
int ensure(stmmqr_ls &L)
{
    auto &R = L.rob;
    const stm_long m = L.damped ? L.am : L.m, n = L.n, anz = L.damped ? L.aanz : L.anz;
    if (!R.rp.p) {
        // entry p of A (column j) sits at p + j of the damped object's pattern [A; I], whose column pointers are Ap[j] + j
        const stm_long sh = L.damped ? 1 : 0;
        std::vector<int> row((size_t)std::max<stm_long>(anz, 1), 0), col(row.size(), 0), rp, rj, rq;
        for (stm_long j = 0; j < n; j++)
            for (stm_long p = L.Ap[(size_t)j] - sh * j; p < L.Ap[(size_t)j + 1] - sh * (j + 1); p++) {
                row[(size_t)p] = (int)L.Bi[(size_t)(p + sh * j)]; col[(size_t)p] = (int)j;
            }
        stm_row_form((long)m, (long)anz, row.data(), col.data(), rp, rj, rq);
        hipStream_t st = L.plan->stream;
        LCHK(R.rp.upload(rp, st)); LCHK(R.rj.upload(rj, st)); LCHK(R.rq.upload(rq, st));
        HIPCHK(hipStreamSynchronize(st));                  // (the host vectors end here)
    }
    const size_t mm = (size_t)m, nn = (size_t)n;
    LCHK(want(R.b, mm)); LCHK(want(R.r, mm)); LCHK(want(R.a, mm)); LCHK(want(R.w, mm));
    LCHK(want(R.x, nn)); LCHK(want(R.xprev, nn));
    LCHK(want(R.part, (size_t)stm_lsr_part_doubles(m))); LCHK(want(R.stat, 12)); LCHK(want(R.step, 2)); LCHK(want(R.res, 1));
    LCHK(want(R.sel, (size_t)stm_lsr_sel_words()));
    for (auto &e : R.ev) if (!e) HIPCHK(hipEventCreate(&e));
    return 0;
}

// A's unweighted values on the device: a device pointer of the caller's as it is; host values (the caller's, or those of create)
// into the damped object's d_ax -- as stmmqr_ls_solve_damped does --, into the feature's own copy on a plain object, whose d_val
// holds weighted values
int unweighted_values(stmmqr_ls &L, const double *Ax, int ax_on_device, const double **out)
{
    hipStream_t st = L.plan->stream;
    if (Ax && ax_on_device) { *out = Ax; return 0; }
    if (L.damped) {
        if (Ax || !L.ax_current) {
            if (L.aanz > 0)
                HIPCHK(hipMemcpyAsync(L.d_ax.p, Ax ? Ax : L.Ax.data(), (size_t)L.aanz * sizeof(double), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
            L.ax_current = (Ax == nullptr);
        }
        *out = L.d_ax.p;
        return 0;
    }
    auto &R = L.rob;
    if (Ax || !R.ax_create) {
        LCHK(want(R.ax, (size_t)L.anz));
        if (L.anz > 0) HIPCHK(hipMemcpyAsync(R.ax.p, Ax ? Ax : L.Ax.data(), (size_t)L.anz * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        R.ax_create = (Ax == nullptr);
    }
    *out = R.ax.p;
    return 0;
}

// a vector of the caller's on the device: the pointer itself, or a copy into buf
int staged(DevBuf<double> &buf, const double *src, size_t count, int on_device, hipStream_t st, const double **out)
{
    if (on_device) { *out = src; return 0; }
    LCHK(want(buf, count));
    if (count > 0) HIPCHK(hipMemcpyAsync(buf.p, src, count * sizeof(double), hipMemcpyHostToDevice, st));
    *out = buf.p;
    return 0;
}

// one reweighting on the stream: r, a, (sigma), w into the feature's vectors; stat [8] comes back (the one host wait).  sigma > 0:
// that scale; 0: from the median.
int reweight(stmmqr_ls &L, const Rule &Q, double sigma, const double *dAx, const double *dB, const double *dX, const double *dw0,
             double *stat)
{
    auto &R = L.rob;
    hipStream_t st = L.plan->stream;
    const stm_long m = L.damped ? L.am : L.m;
    const double *med = sigma > 0 ? nullptr : R.stat.p + 8;
    HIPCHK(hipEventRecord(R.ev[0], st));
    LCHK(stm_launch_lsr_resid(m, R.rp.p, R.rj.p, R.rq.p, dAx, dX, dB, R.r.p, st));
    LCHK(stm_launch_lsr_abs(m, dw0, R.r.p, R.a.p, st));
    HIPCHK(hipEventRecord(R.ev[1], st));
    if (med) LCHK(stm_launch_lsr_select(m, R.a.p, dw0, R.sel.p, R.stat.p + 8, st));
    HIPCHK(hipEventRecord(R.ev[2], st));
    LCHK(stm_launch_lsr_weights(m, R.a.p, dw0, med, sigma, Q.mad, Q.smin, Q.loss, Q.cc, R.w.p, R.part.p, R.stat.p, st));
    HIPCHK(hipEventRecord(R.ev[3], st));
    HIPCHK(hipMemcpyAsync(stat, R.stat.p, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++) HIPCHK(hipEventElapsedTime(&ms[k], R.ev[k], R.ev[k + 1]));
    R.ms[0] = ms[0]; R.ms[1] = ms[1]; R.ms[2] = ms[2]; R.ms[3] = (double)ms[0] + ms[1] + ms[2];
    return 0;
}

int weights_impl(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_robust *rb, const double *B, const double *X,
                 double *r_out, double *w_out, int on_device, double *stat)
{
    const std::string F = "stmmqr_ls_robust_weights: ";
    Rule Q;
    PASS(robust_args(F, ls, rb, Q));
    if (!B || !X) return fail(STMMQR_ERR_INVALID, F + "B or X is NULL");
    PASS(device_half(F, ls));
    stmmqr_ls &L = *ls;
    auto &R = L.rob;
    HIPCHK(hipSetDevice(L.plan->device));
    hipStream_t st = L.plan->stream;
    const stm_long m = L.damped ? L.am : L.m, n = L.n;
    PASS(ensure(L));
    const double *dAx = nullptr, *dB = nullptr, *dX = nullptr, *dw0 = nullptr;
    PASS(unweighted_values(L, Ax, ax_on_device, &dAx));
    PASS(staged(R.b, B, (size_t)m, on_device, st, &dB));
    PASS(staged(R.x, X, (size_t)n, on_device, st, &dX));
    if (rb->w0) PASS(staged(R.w0, rb->w0, (size_t)m, on_device, st, &dw0));
    double s8[8];
    PASS(reweight(L, Q, Q.sigma, dAx, dB, dX, dw0, s8));
    const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (r_out && m > 0) HIPCHK(hipMemcpyAsync(r_out, R.r.p, (size_t)m * sizeof(double), back, st));
    if (w_out && m > 0) HIPCHK(hipMemcpyAsync(w_out, R.w.p, (size_t)m * sizeof(double), back, st));
    HIPCHK(hipStreamSynchronize(st));
    if (stat) memcpy(stat, s8, sizeof s8);
    return 0;
}

int solve_impl(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_robust *rb, const stmmqr_ls_damping *dmp, const double *B,
               const double *x0, int max_iter, double rtol, int sigma_iters, double *X, double *w_out, double *resid, int on_device,
               double *hist, double *info)
{
    const std::string F = "stmmqr_ls_solve_robust: ";
    Rule Q;
    PASS(robust_args(F, ls, rb, Q));
    if (max_iter < 1) return fail(STMMQR_ERR_INVALID, F + "max_iter must be at least 1");
    if (!(rtol >= 0)) return fail(STMMQR_ERR_INVALID, F + "rtol is negative or not a number");
    if (dmp && !ls->damped) return fail(STMMQR_ERR_INVALID, F + "damping (dmp) given on a plain object (stmmqr_ls_create)");
    if (!dmp && ls->damped) return fail(STMMQR_ERR_INVALID, F + "a damped object (stmmqr_ls_create_damped) needs its damping (dmp)");
    if (dmp && dmp->w) return fail(STMMQR_ERR_INVALID, F + "dmp->w must be NULL: prior weights go in rb->w0");
    if (dmp) {                                             // (what stmmqr_ls_solve_damped would refuse inside the loop)
        if (!(dmp->lambda >= 0) || !std::isfinite(dmp->lambda)) return fail(STMMQR_ERR_INVALID, F + "lambda must be finite and not negative");
        if (dmp->scale != 0 && dmp->scale != 1) return fail(STMMQR_ERR_INVALID, F + "scale must be 0 or 1");
        if (dmp->scale == 1 && !(dmp->scale_min > 0 && dmp->scale_min <= dmp->scale_max))
            return fail(STMMQR_ERR_INVALID, F + "scale = 1 needs 0 < scale_min <= scale_max");
    }
    if (!B || !X) return fail(STMMQR_ERR_INVALID, F + "B or X is NULL");
    PASS(device_half(F, ls));
    stmmqr_ls &L = *ls;
    auto &R = L.rob;
    HIPCHK(hipSetDevice(L.plan->device));
    hipStream_t st = L.plan->stream;
    const stm_long m = L.damped ? L.am : L.m, n = L.n, anz = L.damped ? L.aanz : L.anz;
    const size_t mb = (size_t)m * sizeof(double), nb = (size_t)n * sizeof(double);
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    PASS(ensure(L));
    // ---- the inputs, once ----
    const double *dAx = nullptr, *dB = nullptr, *dw0 = nullptr;
    PASS(unweighted_values(L, Ax, ax_on_device, &dAx));
    PASS(staged(R.b, B, (size_t)m, on_device, st, &dB));
    if (rb->w0) PASS(staged(R.w0, rb->w0, (size_t)m, on_device, st, &dw0));
    stmmqr_ls_damping d2 = {};
    if (dmp) {
        d2 = *dmp;
        d2.w = R.w.p;
        if (!on_device) {
            if (dmp->d) PASS(staged(R.dd, dmp->d, (size_t)n, 0, st, &d2.d));
            if (dmp->D_out) { LCHK(want(R.dout, (size_t)n)); d2.D_out = R.dout.p; }
            if (dmp->dnorm) { LCHK(want(R.dn, 1)); d2.dnorm = R.dn.p; }
        }
    } else {
        PASS(ls_ensure_int_pattern(L));
        LCHK(want(R.wax, (size_t)anz)); LCHK(want(R.wb, (size_t)m));
    }
    // ---- the first weights: from x0, or w0 alone ----
    double s8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ms = 0;
    int nrew = 0;
    auto reweigh = [&]() -> int {                           // (the scale: given; or estimated in the first sigma_iters reweightings)
        double sigma = Q.sigma;
        if (sigma == 0 && sigma_iters >= 0 && nrew >= std::max(sigma_iters, 1)) sigma = s8[0];
        PASS(reweight(L, Q, sigma, dAx, dB, R.x.p, dw0, s8));
        ms += R.ms[3];
        nrew++;
        return 0;
    };
    bool have_prev = false;
    if (x0) {
        if (n > 0) HIPCHK(hipMemcpyAsync(R.x.p, x0, nb, in, st));
        PASS(reweigh());
        have_prev = true;
    } else if (dw0) {
        if (m > 0) HIPCHK(hipMemcpyAsync(R.w.p, dw0, mb, hipMemcpyDeviceToDevice, st));
    } else
        LCHK(stm_launch_lsr_fill(m, 1.0, R.w.p, st));
    // ---- the loop ----
    int solves = 0, converged = 0;
    double ratio = INFINITY;
    for (int it = 0; it < max_iter; it++) {
        if (it > 0) PASS(reweigh());
        if (have_prev && n > 0) HIPCHK(hipMemcpyAsync(R.xprev.p, R.x.p, nb, hipMemcpyDeviceToDevice, st));
        if (dmp)
            PASS(stmmqr_ls_solve_damped(ls, dAx, 1, &d2, dB, std::max<stm_long>(m, 1), R.x.p, std::max<stm_long>(n, 1), R.res.p, 1));
        else {
            LCHK(stm_launch_lsr_scale(anz, L.d_ai.p, R.w.p, dAx, R.wax.p, st));
            LCHK(stm_launch_lsr_scale(m, nullptr, R.w.p, dB, R.wb.p, st));
            PASS(stmmqr_ls_solve(ls, R.wax.p, 1, R.wb.p, std::max<stm_long>(m, 1), R.x.p, std::max<stm_long>(n, 1), R.res.p, 1));
        }
        solves++;
        double step = INFINITY, sx[2] = {0, 0};
        if (have_prev) {
            LCHK(stm_launch_lsr_step(n, R.x.p, R.xprev.p, R.step.p, st));
            HIPCHK(hipMemcpyAsync(sx, R.step.p, sizeof sx, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            step = sx[0];
            ratio = sx[1] > 0 ? step / sx[1] : (step == 0 ? 0.0 : INFINITY);
            converged = step <= rtol * sx[1];
        }
        have_prev = true;
        if (hist) { double *h = hist + 4 * (size_t)it; h[0] = s8[0]; h[1] = s8[4]; h[2] = step; h[3] = L.resid[0]; }
        if (converged) break;
    }
    // ---- the outputs, once ----
    if (n > 0) HIPCHK(hipMemcpyAsync(X, R.x.p, nb, back, st));
    if (w_out && m > 0) HIPCHK(hipMemcpyAsync(w_out, R.w.p, mb, back, st));
    if (resid) HIPCHK(hipMemcpyAsync(resid, R.res.p, sizeof(double), back, st));
    if (dmp && !on_device) {
        if (dmp->D_out && n > 0) HIPCHK(hipMemcpyAsync(dmp->D_out, R.dout.p, nb, back, st));
        if (dmp->dnorm) HIPCHK(hipMemcpyAsync(dmp->dnorm, R.dn.p, sizeof(double), back, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (info) {
        info[0] = solves; info[1] = converged; info[2] = ratio; info[3] = s8[0]; info[4] = s8[4]; info[5] = s8[5]; info[6] = ms;
        info[7] = R.bytes();
    }
    return 0;
}

int median_impl(const double *v, const double *mask, stm_long len, int device, int on_device, double *out)
{
    const std::string F = "stmmqr_median_abs: ";
    if (!out) return fail(STMMQR_ERR_INVALID, F + "null output");
    if (len < 0 || (len > 0 && !v)) return fail(STMMQR_ERR_INVALID, F + "bad arguments");
    PASS(stm_ensure_device(device));
    hipStream_t st = nullptr;                               // (the device's own stream: the call ends with its synchronisation)
    DevBuf<double> dv, dm, da, dout;
    DevBuf<unsigned long long> sel;
    const size_t n = (size_t)len;
    const double *pv = v, *pm = mask;
    if (!on_device) {
        LCHK(dv.alloc(n));
        if (n > 0) HIPCHK(hipMemcpyAsync(dv.p, v, n * sizeof(double), hipMemcpyHostToDevice, st));
        pv = dv.p;
        if (mask) {
            LCHK(dm.alloc(n));
            if (n > 0) HIPCHK(hipMemcpyAsync(dm.p, mask, n * sizeof(double), hipMemcpyHostToDevice, st));
            pm = dm.p;
        }
        LCHK(dout.alloc(4));
    }
    LCHK(da.alloc(n));
    LCHK(sel.alloc((size_t)stm_lsr_sel_words()));
    LCHK(stm_launch_lsr_abs(len, pm, pv, da.p, st));
    LCHK(stm_launch_lsr_select(len, da.p, pm, sel.p, on_device ? out : dout.p, st));
    if (!on_device) HIPCHK(hipMemcpyAsync(out, dout.p, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" {

int stmmqr_median_abs(const double *v, const double *mask, stm_long len, int device, int on_device, double *out)
{
    try {
        return median_impl(v, mask, len, device, on_device, out);
    } catch (const std::bad_alloc &) {
        return stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_median_abs: out of memory");
    }
}

int stmmqr_ls_robust_weights(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_robust *rb, const double *B,
                             const double *X, double *r_out, double *w_out, int on_device, double *stat)
{
    try {
        return weights_impl(ls, Ax, ax_on_device, rb, B, X, r_out, w_out, on_device, stat);
    } catch (const std::bad_alloc &) {
        return stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_ls_robust_weights: out of memory");
    }
}

int stmmqr_ls_solve_robust(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_robust *rb, const stmmqr_ls_damping *dmp,
                           const double *B, const double *x0, int max_iter, double rtol, int sigma_iters, double *X, double *w_out,
                           double *resid, int on_device, double *hist, double *info)
{
    try {
        return solve_impl(ls, Ax, ax_on_device, rb, dmp, B, x0, max_iter, rtol, sigma_iters, X, w_out, resid, on_device, hist, info);
    } catch (const std::bad_alloc &) {
        return stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_ls_solve_robust: out of memory");
    }
}

int stmmqr_ls_robust_times(const stmmqr_ls *ls, double *ms)
{
    if (!ls || !ms) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_robust_times: null argument");
    memcpy(ms, ls->rob.ms, 4 * sizeof(double));
    return 0;
}

}  // extern "C"
