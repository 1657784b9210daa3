// stmmqr_seminormal.cpp -- products with A on the device and the corrected seminormal equations on factors with or without H, on a
// plan and on a SparseQR object; the minimum-norm forwarder of the object (host side; kernels: stmmqr_qless.hip; R' \ and R \:
// stmmqr_rfactor.cpp).
#include "stmmqr_plan.h"
#include <memory>

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
    auto &K = P.res.call;
    LCHK(grow(K.d_csY, (size_t)yr * (size_t)nrhs));
    PASS(stage_in(K.d_csX, X, ldx, xr, nrhs, 0, P.stream));
    LCHK(spmv_dev(P, trans, K.d_csX.p, xr, nullptr, 0, K.d_csY.p, yr, nrhs));
    return stage_out(K.d_csY, Y, ldy, yr, nrhs, 0, P.stream);
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
    PASS(ensure_rt(P, RT_ONE_WORKGROUP));                            // (the R' \ step: refused before any launch of the solve)
    LCHK(stm_ensure_a_index(P));
    if (info) *info = 0;
    if (nrhs == 0) return 0;
    hipStream_t st = P.stream;
    auto &K = P.res.call;
    const size_t mm = (size_t)std::max(1L, m), nn = (size_t)std::max(1L, n), nbm = (size_t)std::min<stm_long>(rhs_batch_max(), nrhs);
    LCHK(grow(K.d_csX, nn * (size_t)nrhs));
    LCHK(grow(K.d_csR, mm * nbm)); LCHK(grow(K.d_csY, mm * nbm));
    LCHK(grow(K.d_csZ, nn * nbm)); LCHK(grow(K.d_csD, nn * nbm));
    LCHK(grow(K.d_csN, 3 * (size_t)nrhs + 1));
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), P.stream));
    PASS(stage_in(K.d_csB, B, ldb, m, nrhs, on_device, st));
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) -> int {
        const double *b = K.d_csB.p + j * m;
        double *x = K.d_csX.p + j * n;
        LCHK(spmv_dev(P, 1, b, m, nullptr, 0, K.d_csZ.p, n, nb));                        // z = A'b
        LCHK(rt_vectors(P, K.d_csZ.p, K.d_csY.p, nb, true));                              // y = R' \ (E'z)
        LCHK(r_vectors(P, K.d_csY.p, x, nb, true));                                       // x = E (R \ y)
        for (int it = 0; it < refine; it++) {
            LCHK(spmv_dev(P, 0, x, n, b, m, K.d_csR.p, m, nb));                          // r = b - A x
            LCHK(spmv_dev(P, 1, K.d_csR.p, m, nullptr, 0, K.d_csZ.p, n, nb));             // A'r
            LCHK(rt_vectors(P, K.d_csZ.p, K.d_csY.p, nb, true));
            LCHK(r_vectors(P, K.d_csY.p, K.d_csD.p, nb, true));
            LCHK(stm_launch_add_cols((int)n, nb, K.d_csD.p, n, x, n, st));                // x += E R^-1 R^-T E' A'r
        }
        if (info) {
            LCHK(spmv_dev(P, 0, x, n, b, m, K.d_csR.p, m, nb));
            LCHK(spmv_dev(P, 1, K.d_csR.p, m, nullptr, 0, K.d_csZ.p, n, nb));
            LCHK(stm_launch_colnorm2(n, K.d_csZ.p, n, nb, K.d_csN.p + j, st));           // |A'r|^2, |x|^2, |b|^2
            LCHK(stm_launch_colnorm2(n, x, n, nb, K.d_csN.p + nrhs + j, st));
            LCHK(stm_launch_colnorm2(m, b, m, nb, K.d_csN.p + 2 * nrhs + j, st));
        }
        return 0;
    }));
    if (info) {
        LCHK(stm_launch_colnorm2(P.anz, P.d_Ax.p, std::max(1L, P.anz), 1, K.d_csN.p + 3 * nrhs, st));   // |A|_F^2
        std::vector<double> nr((size_t)(3 * nrhs + 1));
        HIPCHK(hipMemcpyAsync(nr.data(), K.d_csN.p, nr.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *info = stm_seminormal_info(std::sqrt(nr[(size_t)(3 * nrhs)]), nr.data(), nr.data() + nrhs, nr.data() + 2 * nrhs, nrhs);
    }
    PASS(stage_out(K.d_csX, X, ldx, n, nrhs, on_device, st));
    return end_resident_op(P);
}

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
    PASS(stage_in(op->X, X, ldx, xr, nrhs, 0, op->st));
    if (B) PASS(stage_in(op->B, B, ldb, yr, nrhs, 0, op->st));
    LCHK(grow(op->Y, (size_t)(yr * nrhs)));
    LCHK(spmv(op->A, op->ax.p, op->m, op->n, trans, op->X.p, xr, (B && !trans) ? op->B.p : nullptr, trans ? 0 : yr, op->Y.p, yr, nrhs, op->st));
    return stage_out(op->Y, Y, ldy, yr, nrhs, 0, op->st);
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
