// stmmqr_rcond.cpp -- products with R and R' on the resident factors and the condition estimate built on them (factors with or without
// H; host side, kernels: stmmqr_rmult.hip; the passes: stmmqr_rfactor.cpp).
#include "stmmqr_plan.h"

// Y = R X (trans 0) or R' X (trans 1) with the whole rank x n factor on the device; see include/stmmqr_hip.h
int stmmqr_plan_rmult(stmmqr_plan *plan, int trans, const double *X, stm_long ldx, double *Y, stm_long ldy, stm_long nrhs, int permuted,
                      int on_device)
{
    PASS(check_factored(plan));
    if ((trans != 0 && trans != 1) || !X || !Y || nrhs < 0) return fail(STMMQR_ERR_INVALID, "bad rmult arguments");
    stmmqr_plan &P = *plan;
    auto &K = P.res.call;
    const long m = P.m, n = P.n, xrows = trans ? m : n, yrows = trans ? n : m;
    if (ldx < xrows || ldy < yrows) return fail(STMMQR_ERR_INVALID, "bad leading dimension");
    PASS(begin_resident_op(P));
    if (nrhs == 0 || yrows == 0) return 0;
    hipStream_t st = P.stream;
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), st));
    PASS(trans ? ensure_rtmult(P) : ensure_rmult(P));
    PASS(stage_in(K.d_Xall, X, ldx, xrows, nrhs, on_device, st));
    LCHK(grow(K.d_Yall, (size_t)(yrows * nrhs)));
    const int *qf = (!permuted && P.has_qfill) ? P.res.sched.d_Qfill.p : nullptr;
    PASS(for_each_batch(P, nrhs, [&](stm_long j, int nb) -> int {
        if (!trans) {
            LCHK(stm_launch_perm(K.d_Xall.p + j * n, qf, K.d_Xs.p, (int)n, 0, st, nb, n, n));                 // x[k] = X[Qfill[k]]
            return rmult_pass(P, K.d_Xs.p, K.d_Yall.p + j * m, nb);
        }
        PASS(rtmult_pass(P, K.d_Xall.p + j * m, K.d_Xs.p, nb));
        return stm_launch_perm(K.d_Xs.p, qf, K.d_Yall.p + j * n, (int)n, 1, st, nb, n, n);                   // Y[Qfill[k]] = z[k]
    }));
    PASS(stage_out(K.d_Yall, Y, ldy, yrows, nrhs, on_device, st));
    return end_resident_op(P);
}

// The condition of R over its live pivot columns, estimated on the device; see include/stmmqr_hip.h.  Vectors: the r-vector of the
// live pivot columns lives either in an n-vector in R's column order (entry i at pc[i], zero elsewhere: what R x reads, what R \ and
// R' y write) or in the first r entries of an m-vector in R's row order (what R \ and R' y read, what R x and R' \ write).  With
// ncol < n the trailing columns stay zero in every input and are never read from an output: R [x; 0] = R11 x, R \ [y; 0] = R11 \ y,
// and the leading rows of R' \ [z; *] are R11' \ z.
namespace {
struct Condest {                         // what the two estimates share: the plan's vectors and the few scalars the host steers by
    stmmqr_plan &P;
    hipStream_t st;
    int r;                               // live pivot columns
    size_t nn, mm;                       // max(1, n), max(1, m)
    double *dA, *dB, *dV, *dY, *dS, *dXs, *dXr;
    const int *dpc;
    std::vector<double> safe;            // x_i = (-1)^i (1 + i / (r - 1))
    double sc[4];
    double vnorm;                        // v = dV / vnorm
};
int read_scalars(Condest &C)
{
    HIPCHK(hipMemcpyAsync(C.sc, C.dS, sizeof(C.sc), hipMemcpyDeviceToHost, C.st));
    HIPCHK(hipStreamSynchronize(C.st));
    return 0;
}
// the r-vector h (host) into the zeroed m-vector dY
int put_rows(Condest &C, const std::vector<double> &h)
{
    HIPCHK(hipMemsetAsync(C.dY, 0, C.mm * sizeof(double), C.st));
    HIPCHK(hipMemcpyAsync(C.dY, h.data(), (size_t)C.r * sizeof(double), hipMemcpyHostToDevice, C.st));
    HIPCHK(hipStreamSynchronize(C.st));                                      // (h is pageable)
    return 0;
}
// dY (R's row order, zero beyond r) -> d_Xs = R \ dY
int solve_r(Condest &C)
{
    const long m = C.P.m;
    LCHK(stm_launch_perm(C.dY, C.P.res.fact.d_Wmap.p, C.P.res.call.d_W.p, (int)m, 0, C.st, 1, m, m));
    return rsolve_vector(C.P, 1);
}

// res[1] = |R_live|_1, exact: the largest column sum of |R| over the live columns; res[2] = Hager's estimate of |R_live^-1|_1 in
// Higham's form, res[3] = its rounds
int condest_one_norm(Condest &C, double *res)
{
    stmmqr_plan &P = C.P;
    hipStream_t st = C.st;
    const int r = C.r;
    PASS(rtmult_pass(P, C.dY, C.dB, 1, 1));
    LCHK(stm_launch_ce_reduce(2, C.dB, C.dpc, nullptr, r, C.dS, st));
    PASS(read_scalars(C));
    res[1] = C.sc[0];
    double est = 0.0;
    int rounds = 0, jprev = -1;
    PASS(put_rows(C, std::vector<double>((size_t)r, 1.0 / (double)r)));
    for (int round = 1; round <= 5; round++) {
        rounds = round;
        PASS(solve_r(C));                                                  // y = R \ x
        LCHK(stm_launch_ce_reduce(0, C.dXs, C.dpc, nullptr, r, C.dS, st));
        PASS(read_scalars(C));
        if (round > 1 && !(C.sc[0] > est)) break;                          // the estimate does not grow
        est = C.vnorm = C.sc[0];
        HIPCHK(hipMemcpyAsync(C.dV, C.dXs, C.nn * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (round == 5) break;
        LCHK(stm_launch_ce_map(0, C.dXs, C.dpc, nullptr, r, 0.0, st));     // xi = sign(y)
        PASS(rt_pass(P, 1, RT_SPLIT));                                     // z = R' \ xi: the first r rows of d_Xr
        LCHK(stm_launch_ce_reduce(3, C.dXr, nullptr, C.dY, r, C.dS, st));
        PASS(read_scalars(C));
        const int j = (int)C.sc[2];
        if (C.sc[1] <= C.sc[3] || j == jprev) break;                       // |z|_inf <= z'x, or the arg-max repeats
        jprev = j;
        const double one = 1.0;
        HIPCHK(hipMemsetAsync(C.dY, 0, (size_t)r * sizeof(double), st));
        HIPCHK(hipMemcpyAsync(C.dY + j, &one, sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    PASS(put_rows(C, C.safe));                                             // the safeguard vector
    PASS(solve_r(C));
    LCHK(stm_launch_ce_reduce(0, C.dXs, C.dpc, nullptr, r, C.dS, st));
    PASS(read_scalars(C));
    const double est2 = 2.0 * C.sc[0] / (3.0 * (double)r);
    if (est2 > est) {
        est = est2; C.vnorm = C.sc[0];
        HIPCHK(hipMemcpyAsync(C.dV, C.dXs, C.nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    res[2] = est; res[3] = (double)rounds;
    return 0;
}

// res[1] = |R_live|_2 by the power iteration on R'R, res[2] = |R_live^-1|_2 by the same on its inverse, res[3] = the solve pairs of
// the latter whose result became the iterate
int condest_two_norm(Condest &C, int iters, double *res)
{
    stmmqr_plan &P = C.P;
    hipStream_t st = C.st;
    const int r = C.r;
    double s2 = 0.0;
    for (double t : C.safe) s2 += t * t;
    s2 = std::sqrt(s2);
    std::vector<double> start(C.safe);
    for (double &t : start) t /= s2;
    // |R_live|_2: x <- R'(R x) / |R'(R x)|, estimate sqrt |R'(R x)|
    PASS(put_rows(C, start));
    HIPCHK(hipMemsetAsync(C.dA, 0, C.nn * sizeof(double), st));
    LCHK(stm_launch_ce_map(2, C.dY, C.dpc, C.dA, r, 0.0, st));
    double lam = 0.0;
    for (int it = 0; it < iters; it++) {
        PASS(rmult_pass(P, C.dA, C.dY, 1));
        PASS(rtmult_pass(P, C.dY, C.dB, 1));
        LCHK(stm_launch_ce_reduce(1, C.dB, C.dpc, nullptr, r, C.dS, st));
        PASS(read_scalars(C));
        lam = std::sqrt(C.sc[0]);
        if (!(lam > 0.0)) break;
        LCHK(stm_launch_ce_map(1, C.dB, C.dpc, C.dA, r, lam, st));
    }
    res[1] = std::sqrt(lam);
    // |R_live^-1|_2: x <- R \ (R' \ x) / |.|; the estimate is 1 / |R_live v|_2 of the last iterate v
    PASS(put_rows(C, start));
    HIPCHK(hipMemsetAsync(C.dV, 0, C.nn * sizeof(double), st));
    LCHK(stm_launch_ce_map(2, C.dY, C.dpc, C.dV, r, 0.0, st));
    int made = 0;
    for (int it = 0; it < iters; it++) {
        HIPCHK(hipMemcpyAsync(C.dXs, C.dV, C.nn * sizeof(double), hipMemcpyDeviceToDevice, st));
        PASS(rt_pass(P, 1, RT_SPLIT));                                     // t = R' \ x: the first r rows of d_Xr
        HIPCHK(hipMemcpyAsync(C.dY, C.dXr, (size_t)r * sizeof(double), hipMemcpyDeviceToDevice, st));   // (dY is zero beyond r)
        PASS(solve_r(C));                                                  // w = R \ t
        LCHK(stm_launch_ce_reduce(1, C.dXs, C.dpc, nullptr, r, C.dS, st));
        PASS(read_scalars(C));
        const double mu = std::sqrt(C.sc[0]);
        if (!(mu > 0.0) || !std::isfinite(mu)) break;
        LCHK(stm_launch_ce_map(1, C.dXs, C.dpc, C.dV, r, mu, st));
        made++;
    }
    PASS(rmult_pass(P, C.dV, C.dY, 1));
    LCHK(stm_launch_ce_reduce(1, C.dY, nullptr, nullptr, r, C.dS, st));
    PASS(read_scalars(C));
    res[2] = 1.0 / std::sqrt(C.sc[0]);
    res[3] = (double)made;
    return 0;
}
// a host array to the caller's, host or device
int give(double *dst, const double *src, size_t cnt, int on_device, hipStream_t st)
{
    if (on_device) { HIPCHK(hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyHostToDevice, st)); HIPCHK(hipStreamSynchronize(st)); }
    else memcpy(dst, src, cnt * sizeof(double));
    return 0;
}
}  // namespace

int stmmqr_plan_condest(stmmqr_plan *plan, stm_long ncol, int kind, int iters, double *out, double *v, int on_device)
{
    PASS(check_factored(plan));
    if (!out) return fail(STMMQR_ERR_INVALID, "condest: out is NULL");
    stmmqr_plan &P = *plan;
    auto &K = P.res.call;
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
    if (r == 0) {
        if (v && ncol > 0) { const std::vector<double> z((size_t)ncol, 0.0); PASS(give(v, z.data(), z.size(), on_device, st)); }
        return give(out, res, 8, on_device, st);
    }
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), st));
    PASS(ensure_rtmult(P));
    PASS(ensure_rt(P, RT_SPLIT));
    const size_t nn = (size_t)std::max(1L, n), mm = (size_t)std::max(1L, m);
    LCHK(grow(K.d_ceA, nn)); LCHK(grow(K.d_ceB, nn)); LCHK(grow(K.d_ceV, nn)); LCHK(grow(K.d_ceY, mm)); LCHK(grow(K.d_ceS, 8));
    if (K.d_cepc.n < (size_t)r) LCHK(K.d_cepc.alloc((size_t)r));
    HIPCHK(hipMemcpyAsync(K.d_cepc.p, pc.data(), (size_t)r * sizeof(int), hipMemcpyHostToDevice, st));
    Condest C{P, st, r, nn, mm, K.d_ceA.p, K.d_ceB.p, K.d_ceV.p, K.d_ceY.p, K.d_ceS.p, K.d_Xs.p, K.d_Xr.p, K.d_cepc.p,
              std::vector<double>((size_t)r, 1.0), {0, 0, 0, 0}, 1.0};
    for (int i = 0; i < r && r > 1; i++) C.safe[(size_t)i] = ((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)(r - 1));
    PASS(kind == 1 ? condest_one_norm(C, res) : condest_two_norm(C, iters, res));
    res[0] = res[1] * res[2];
    if (v) {
        // in the caller's column order, zeros on dead columns (R \ leaves them zero), unit norm of the kind
        double *dv = on_device ? v : C.dB;
        HIPCHK(hipMemsetAsync(dv, 0, (size_t)ncol * sizeof(double), st));
        LCHK(stm_launch_ce_vector(C.dV, P.has_qfill ? P.res.sched.d_Qfill.p : nullptr, dv, (int)ncol, C.vnorm, st));
        if (!on_device) HIPCHK(hipMemcpyAsync(v, dv, (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    PASS(end_resident_op(P));
    return give(out, res, 8, on_device, st);
}
