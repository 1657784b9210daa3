// stmmqr_refactor.hip -- stmmqr_sparseqr_refactorize: a factorized SparseQR object takes new values of the same pattern, from a host
// array or a device pointer.  Column order, singleton set, R1's and Y's patterns, the analysis and the plan with its arenas stay;
// the tolerance, R1x, Yx, the factors, Rdead, rank and HP1inv are made again.  Everything that touches HIP for the object is here
// (stmmqr_sparseqr.cpp is host code and is also built without the device half): what the object keeps on the device hangs on its
// `ext` pointer and is released through `ext_release`.
//
// Three small kernels on the plan's stream turn the caller's values into what the plan factorizes:
//   k_rf_colnorm  the largest column 2-norm for QR_DEFAULT_TOL, bit for bit stm_qr_default_tol's: a lane walks a column in storage
//                 order with dnrm2's scale / ssq recurrence, the same operations in the same order with contraction off (the host
//                 build has no FMA, the device would fuse 1 + ssq * r * r); the maximum over the columns is exact in any order.
//                 A lane per column is slow on a dense column of tens of thousands of entries: accepted, the same bits as the host
//                 rule are worth more here than the microseconds.
//   k_rf_split    Yx[t] = Ax[ysrc[t]], R1x[q] = Ax[r1src[q]] into the object's staging buffer
//   k_rf_check    the smallest live singleton row k with !(|Ax[pivsrc[k]]| > tol), the tolerance formed from the norm in device
//                 memory: the largest n1rows - k by an atomic maximum, deterministic whatever the execution order
// One device-to-host copy then brings {norm, stale k, R1x, Yx} back; it is the only host wait between the arrival of the values
// and stmmqr_factorize_device on the staged Yx.  An object without singletons that is no LQ object has nothing to split: it runs
// k_rf_colnorm alone (and only for the default tolerance) and factorizes straight from the caller's device pointer or from the one
// staged upload of a host array.  Host arrays take the same path as device pointers after that upload.
#include "stmmqr_plan.h"
#include "stmmqr_sparseqr.h"

#include <sys/time.h>

#include <memory>

#define RF_NT 256

namespace {

// head of the staging buffer: what the kernels report
struct RfHead {
    unsigned long long mx_bits;   // the largest column norm as the bits of a non-negative double (ordered like the values)
    int stale;                    // n1rows - (first stale live singleton row), 0: none
    int pad;
};
static_assert(sizeof(RfHead) == 2 * sizeof(double), "two doubles in front of R1x");

__global__ __launch_bounds__(RF_NT) void k_rf_colnorm(long long ncol, const long long *__restrict__ ap, const int *__restrict__ tsrc,
                                                      const double *__restrict__ Ax, RfHead *head)
{
#pragma clang fp contract(off)
    const long long j = (long long)blockIdx.x * RF_NT + threadIdx.x;
    double v = 0.0;
    if (j < ncol) {
        double scale = 0, ssq = 1;
        for (long long p = ap[j]; p < ap[j + 1]; p++) {
            const double a = fabs(Ax[tsrc ? (long long)tsrc[p] : p]);
            if (a == 0) continue;
            if (scale < a) { ssq = 1 + ssq * (scale / a) * (scale / a); scale = a; }
            else ssq += (a / scale) * (a / scale);
        }
        v = scale * sqrt(ssq);
    }
    if (!(v > 0)) v = 0.0;                              // (a NaN norm never wins the host's std::max either)
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0 && v > 0) atomicMax(&head->mx_bits, (unsigned long long)__double_as_longlong(v));
}

__global__ __launch_bounds__(RF_NT) void k_rf_split(long long ny, long long nr1, const int *__restrict__ ysrc, const int *__restrict__ r1src,
                                                    const double *__restrict__ Ax, double *__restrict__ R1x, double *__restrict__ Yx)
{
    const long long t = (long long)blockIdx.x * RF_NT + threadIdx.x;
    if (t < ny) Yx[t] = Ax[ysrc[t]];
    else if (t - ny < nr1) R1x[t - ny] = Ax[r1src[t - ny]];
}

__global__ __launch_bounds__(RF_NT) void k_rf_check(long long n1rows, const int *__restrict__ pivsrc, const double *__restrict__ Ax,
                                                    RfHead *head, long long m, long long n, int default_tol, double fixed_tol)
{
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * RF_NT + threadIdx.x;
    if (k >= n1rows) return;
    const double tol = default_tol ? fmin(20.0 * ((double)m + (double)n) * DBL_EPSILON * __longlong_as_double((long long)head->mx_bits), DBL_MAX)
                                   : fixed_tol;
    if (!(fabs(Ax[pivsrc[k]]) > tol)) atomicMax(&head->stale, (int)(n1rows - k));
}

double wall()
{
    struct timeval tv;
    gettimeofday(&tv, nullptr);
    return tv.tv_sec + tv.tv_usec / 1e6;
}

// what an object keeps on the device beyond its plan, made at the first refactorization
struct RfExt {
    DevBuf<int> ysrc, r1src, pivsrc, tsrc;
    DevBuf<long long> ap;
    DevBuf<double> stage;                               // RfHead, R1x [nr1], Yx [ny]; without maps the head alone
    DevBuf<double> axin;                                // a host array's values, uploaded once per call
    std::vector<double> hstage;                         // where the one copy back lands
    hipEvent_t ev[2] = {nullptr, nullptr};
    double bytes() const
    {
        return 4.0 * (double)(ysrc.n + r1src.n + pivsrc.n + tsrc.n) + 8.0 * (double)(ap.n + stage.n + axin.n);
    }
    ~RfExt()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

void rf_release(void *p) { delete (RfExt *)p; }

int rf_make_ext(stmmqr_qr *qr, hipStream_t st, long long ny, long long nr1, RfExt **out)
{
    RfExt *X = new RfExt();
    std::unique_ptr<RfExt> hold(X);
    HIPCHK(hipEventCreate(&X->ev[0]));
    HIPCHK(hipEventCreate(&X->ev[1]));
    // (the host tables carry a placeholder where a count is zero: only the counted part travels; the copies are declared before
    //  the guard, so that they outlive every transfer also when a step fails)
    std::vector<int> hy, hr;
    std::vector<long long> hap;
    struct Settle { hipStream_t st; ~Settle() { (void)hipStreamSynchronize(st); } } settle = {st};
    if (qr->have_maps) {
        hy.assign(qr->ysrc.begin(), qr->ysrc.begin() + ny);
        hr.assign(qr->r1src.begin(), qr->r1src.begin() + nr1);
        HIPCHK((hipError_t)X->ysrc.upload(hy, st));
        HIPCHK((hipError_t)X->r1src.upload(hr, st));
        if (qr->n1rows > 0) HIPCHK((hipError_t)X->pivsrc.upload(qr->pivsrc, st));
    }
    if (qr->tol_arg <= -2) {
        hap.assign(qr->Ap0.begin(), qr->Ap0.end());
        HIPCHK((hipError_t)X->ap.upload(hap, st));
        if (qr->is_lq) HIPCHK((hipError_t)X->tsrc.upload(qr->tsrc, st));
    }
    const size_t ns = 2 + (qr->have_maps ? (size_t)(nr1 + ny) : 0);
    HIPCHK((hipError_t)X->stage.alloc(ns));
    X->hstage.assign(ns, 0.0);
    HIPCHK(hipStreamSynchronize(st));
    *out = hold.release();
    return 0;
}

int refactorize(stmmqr_qr *qr, const double *Ax, int ax_on_device)
{
    typedef stm_long Long;
    if (!qr) return fail(STMMQR_ERR_INVALID, "stmmqr_sparseqr_refactorize: null object");
    if (!qr->plan) return fail(STMMQR_ERR_INVALID, "stmmqr_sparseqr_refactorize: the object has no numeric phase yet (stmmqr_sparseqr_numeric first)");
    if (qr->maps_too_large)
        return fail(STMMQR_ERR_INVALID, "stmmqr_sparseqr_refactorize: a pattern of 2^31 or more entries (the value maps are int tables): make a new object");
    const Long nz = qr->nz, n1rows = qr->n1rows, n2 = qr->n - qr->n1cols;
    if (nz > 0 && !Ax) return fail(STMMQR_ERR_INVALID, "stmmqr_sparseqr_refactorize: null values");
    const double t0 = wall();
    stmmqr_plan &P = *qr->plan;
    const bool sing = qr->n1cols > 0, maps = qr->have_maps, deftol = qr->tol_arg <= -2;
    const long long ny = sing ? qr->Yp[(size_t)n2] : nz, nr1 = sing ? qr->R1p[(size_t)n1rows] : 0;
    if ((long long)P.anz != ny) return fail(STMMQR_ERR_INVALID, "stmmqr_sparseqr_refactorize: internal (the plan's matrix is not the object's)");
    HIPCHK(hipSetDevice(P.device));
    hipStream_t st = P.stream;
    RfExt *X = (RfExt *)qr->ext;
    if (!X) {
        PASS(rf_make_ext(qr, st, ny, nr1, &X));
        qr->ext = X; qr->ext_release = rf_release;
    }
    // ---- the values on the device ----
    const double *dAx = Ax;
    if (!ax_on_device && nz > 0) {
        if (X->axin.n < (size_t)nz) HIPCHK((hipError_t)X->axin.alloc((size_t)nz));
        HIPCHK(hipMemcpyAsync(X->axin.p, Ax, (size_t)nz * sizeof(double), hipMemcpyHostToDevice, st));
        dAx = X->axin.p;
    }
    RfHead *head = (RfHead *)X->stage.p;
    double *dR1x = X->stage.p + 2, *dYx = dR1x + nr1;
    const double fixed_tol = qr->tol_arg < 0 ? -1.0 : qr->tol_arg;                // (-2 < tol < 0: none, as at creation)
    HIPCHK(hipEventRecord(X->ev[0], st));
    HIPCHK(hipMemsetAsync(head, 0, sizeof(RfHead), st));
    const long long ncol = (long long)qr->Ap0.size() - 1;
    if (deftol && ncol > 0) {
        HIPCHK((hipError_t)stm_launch_rf_colnorm(ncol, X->ap.p, qr->is_lq ? X->tsrc.p : (const int *)nullptr, dAx, &head->mx_bits, st));
    }
    if (maps && ny + nr1 > 0) {
        hipLaunchKernelGGL(k_rf_split, dim3((unsigned)((ny + nr1 + RF_NT - 1) / RF_NT)), dim3(RF_NT), 0, st, ny, nr1, X->ysrc.p, X->r1src.p, dAx,
                           dR1x, dYx);
        HIPCHK(hipGetLastError());
    }
    if (maps && n1rows > 0) {
        hipLaunchKernelGGL(k_rf_check, dim3((unsigned)((n1rows + RF_NT - 1) / RF_NT)), dim3(RF_NT), 0, st, (long long)n1rows, X->pivsrc.p, dAx, head,
                           (long long)qr->m, (long long)qr->n, deftol ? 1 : 0, fixed_tol);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(X->ev[1], st));
    // ---- the one copy back, the one wait ----
    const size_t nback = maps ? X->hstage.size() : 2;
    if (maps || deftol) HIPCHK(hipMemcpyAsync(X->hstage.data(), X->stage.p, nback * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    RfHead hh;
    memcpy(&hh, X->hstage.data(), sizeof hh);
    double mx;
    memcpy(&mx, &hh.mx_bits, sizeof mx);
    const double tol = deftol ? stm_qr_tol_of_maxnorm(qr->m, qr->n, mx) : fixed_tol;
    float ms_values = 0;
    (void)hipEventElapsedTime(&ms_values, X->ev[0], X->ev[1]);
    qr->rf_info[7] = X->bytes();
    if (maps && n1rows > 0 && hh.stale > 0) {
        // the singleton structure of the first values does not hold for these: nothing of the object was touched
        const Long k = n1rows - hh.stale, p0 = qr->R1p[(size_t)k], kcol = qr->R1j[(size_t)p0];
        char msg[400];
        snprintf(msg, sizeof msg, "stmmqr_sparseqr_refactorize: the singletons of the first values do not hold for these: singleton %ld (live row %ld), "
                 "column %ld of %s, has the pivot %.17g, which does not exceed the tolerance %.17g; make a new object",
                 (long)kcol, (long)k, (long)qr->Q1fill[(size_t)kcol], qr->is_lq ? "A' (row of A)" : "A", X->hstage[2 + (size_t)p0], tol);
        qr->rf_info[5] += 1;
        return fail(STMMQR_ERR_STALE, msg);
    }
    // ---- accepted: from here on the old factorization is given up ----
    qr->valid = 0;
    qr->tol = tol;
    if (sing) {
        std::copy(X->hstage.begin() + 2, X->hstage.begin() + 2 + nr1, qr->R1x.begin());
        std::copy(X->hstage.begin() + 2 + nr1, X->hstage.begin() + 2 + nr1 + ny, qr->Yx.begin());
    }
    qr->stats = stmmqr_stats();
    // (the staged Yx stays untouched until the call returns: its retry paths copy the values again)
    PASS(stmmqr_factorize_device(qr->plan, nullptr, nullptr, maps ? dYx : (nz > 0 ? dAx : X->stage.p), 1, tol, sing ? n2 : qr->n, &qr->stats));
    PASS(stm_sparseqr_after_factorization(qr));
    qr->valid = 1;
    const double secs = wall() - t0;
    qr->fac_seconds = secs;
    qr->rf_info[0] = tol; qr->rf_info[1] = ms_values; qr->rf_info[2] = qr->stats.ms_total; qr->rf_info[3] = secs;
    qr->rf_info[4] += 1;
    return 0;
}

}  // namespace

// k_rf_colnorm for the library's other files (the damped least-squares object): mx_bits is the first member of the head
int stm_launch_rf_colnorm(long long ncol, const long long *ap, const int *tsrc, const double *Ax, unsigned long long *mx_bits, hipStream_t st)
{
    static_assert(offsetof(RfHead, mx_bits) == 0, "the norm's bits lead the head");
    if (ncol <= 0) return 0;
    hipLaunchKernelGGL(k_rf_colnorm, dim3((unsigned)((ncol + RF_NT - 1) / RF_NT)), dim3(RF_NT), 0, st, ncol, ap, tsrc, Ax, (RfHead *)mx_bits);
    return (int)hipGetLastError();
}

extern "C" int stmmqr_sparseqr_refactorize(stmmqr_qr *qr, const double *Ax, int ax_on_device)
{
    try {
        return refactorize(qr, Ax, ax_on_device);
    } catch (const std::bad_alloc &) {
        return fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_sparseqr_refactorize: out of memory");
    }
}
