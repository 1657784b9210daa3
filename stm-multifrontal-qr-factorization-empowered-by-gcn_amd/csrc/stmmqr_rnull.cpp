// stmmqr_rnull.cpp -- the null-space basis N of R over the first ncol columns, G = N'N = L L', and the projector (I - N G^-1 N')^2 that
// turns the basic least-squares solution into the minimum-norm one (factors with or without H; host side, kernels:
// stmmqr_nullspace.hip; the passes: stmmqr_rfactor.cpp).  See include/stmmqr_hip.h and DESIGN.md 6l.
// Column k of N is e_jd[k] - R \ (R e_jd[k]): R e_j is column j of R (a unit vector through rmult_pass is exact: products with 1, sums
// with 0), and R \ . over the live columns leaves W(:, k) = R11^-1 R12(:, k) on them and zero on every dead one.  With ncol < n the
// trailing columns stay zero in every input and no output reads them (the zero-padding argument at the head of stmmqr_rcond.cpp).
#include "stmmqr_plan.h"

namespace {
// (the pure index work -- pc / jd, the slab partition, the panels -- is restab::null_* of stmmqr_restables.cpp)
using restab::null_lower_tiles;
using restab::null_panels;
using restab::null_slabs;
using restab::null_split;
using restab::NullSlabs;

typedef ResidentState::Factorization::NullSpace NullSpace;
// the four marks between the three parts of a build (no timing unless all four exist)
struct BuildMarks {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ok = true;
    BuildMarks() { for (auto &e : ev) ok = ok && hipEventCreate(&e) == hipSuccess; }
    ~BuildMarks() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    void mark(int i, hipStream_t st) { if (ok) ok = hipEventRecord(ev[i], st) == hipSuccess; }
    void read(double *ms) const
    {
        for (int i = 0; i < 3; i++) {
            float t = 0.0f;
            ms[i] = (ok && hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess) ? (double)t : 0.0;
        }
    }
};

// the refusals every entry point shares, in the order of stmmqr_plan_condest
int null_checks(const stmmqr_plan &P, stm_long ncol, const char *what)
{
    if (ncol < 0 || ncol > P.n)
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": ncol = " + std::to_string(ncol) + " is not between 0 and the " + std::to_string(P.n) +
                                            " columns of the plan");
    if (ncol < P.n) PASS(check_carried_view(P, ncol));
    if (!holds_whole_tree(P))
        return fail(STMMQR_ERR_INVALID, std::string(what) + ": the plan does not hold the whole tree in one group (groups were set, or fronts are imported or shared)");
    return 0;
}
int read_rdead(stmmqr_plan &P, long ncol, std::vector<char> &rd)
{
    HIPCHK(hipSetDevice(P.device));
    rd.assign((size_t)ncol, 0);
    if (ncol > 0) HIPCHK(hipMemcpyAsync(rd.data(), P.d_Rdead.p, (size_t)ncol, hipMemcpyDeviceToHost, P.stream));
    HIPCHK(hipStreamSynchronize(P.stream));
    return 0;
}
// d of the first ncol columns: from the basis held, or counted
int count_dead(stmmqr_plan &P, long ncol, long &d)
{
    const NullSpace &Z = P.res.fact.null;
    if (Z.ready && Z.ncol == ncol) { d = Z.d; return 0; }
    std::vector<char> rd;
    PASS(read_rdead(P, ncol, rd));
    d = 0;
    for (char c : rd) d += (c != 0);
    return 0;
}
int no_room(NullSpace &Z, const char *what)
{
    Z.release();
    (void)hipGetLastError();
    return fail(STMMQR_ERR_OUT_OF_MEMORY, std::string("nullspace: no device memory for ") + what);
}

// N, G = N'N and L of the factorization held, for the first ncol columns (d > 0; inside a resident op, d_err cleared)
int build_nullspace(stmmqr_plan &P, long ncol)
{
    auto &K = P.res.call;
    NullSpace &Z = P.res.fact.null;
    hipStream_t st = P.stream;
    const long m = P.m, n = P.n;
    Z.release();
    std::vector<char> rd;
    PASS(read_rdead(P, ncol, rd));
    std::vector<int> pc, jd;
    null_split(rd, pc, jd);
    const int d = (int)jd.size(), np = null_panels(d);
    const NullSlabs sl = null_slabs(ncol, knobs::num(knobs::K_NULL_SLAB));
    DevBuf<double> d_part;                                                   // the Gram matrix's partial tiles: this call's only
    if (Z.d_N.alloc((size_t)ncol * (size_t)d)) return no_room(Z, "N");
    if (Z.d_L.alloc((size_t)d * (size_t)d) || Z.d_Ld.alloc((size_t)np * STM_NULL_NB * STM_NULL_NB)) return no_room(Z, "the Gram matrix N'N");
    if (Z.d_jd.alloc((size_t)d)) return no_room(Z, "the list of dead columns");
    if (d_part.alloc((size_t)null_lower_tiles(d) * (size_t)sl.count * STM_NULL_NB * STM_NULL_NB)) return no_room(Z, "the partial sums of N'N");
    HIPCHK(hipMemcpyAsync(Z.d_jd.p, jd.data(), (size_t)d * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                                        // (jd is pageable and local)
    // ---- N, a batch of dead columns per pass over the tree ----
    PASS(ensure_rmult(P));
    BuildMarks marks;
    marks.mark(0, st);
    const size_t nbmax = (size_t)std::min<long>(rhs_batch_max(), d);
    LCHK(grow(K.d_Xall, nbmax * (size_t)std::max(1L, n)));
    LCHK(grow(K.d_Yall, nbmax * (size_t)std::max(1L, m)));
    PASS(for_each_batch(P, d, [&](stm_long k0, int nb) -> int {
        HIPCHK(hipMemsetAsync(K.d_Xall.p, 0, (size_t)nb * (size_t)n * sizeof(double), st));
        LCHK(stm_launch_null_unit(Z.d_jd.p, (int)k0, nb, K.d_Xall.p, n, st));
        PASS(rmult_pass(P, K.d_Xall.p, K.d_Yall.p, nb));                     // column jd[k] of R, in R's row order
        LCHK(stm_launch_perm(K.d_Yall.p, P.res.fact.d_Wmap.p, K.d_W.p, (int)m, 0, st, nb, m, m));
        PASS(rsolve_vector(P, nb));                                          // d_Xs = R \ it: W(:, k) on the live columns
        LCHK(stm_launch_null_scatter(K.d_Xs.p, n, P.d_Rdead.p, Z.d_jd.p, (int)k0, nb, (int)ncol, Z.d_N.p, st));
        return 0;
    }));
    // ---- one step of refinement: r = R N(:, k) with the row sums in two doubles (in exact arithmetic 0; as computed, the error of W
    // through cond(R11) eps), W += R11 \ r.  It takes the error of N from eps cond(R11) to eps (1 + eps cond(R11)^2) ----
    PASS(for_each_batch(P, d, [&](stm_long k0, int nb) -> int {
        HIPCHK(hipMemsetAsync(K.d_Xall.p, 0, (size_t)nb * (size_t)n * sizeof(double), st));
        PASS(copy_cols(K.d_Xall.p, n, Z.d_N.p + k0 * ncol, ncol, ncol, nb, hipMemcpyDeviceToDevice, st));
        PASS(rmult_pass(P, K.d_Xall.p, K.d_Yall.p, nb, 1));
        LCHK(stm_launch_perm(K.d_Yall.p, P.res.fact.d_Wmap.p, K.d_W.p, (int)m, 0, st, nb, m, m));
        PASS(rsolve_vector(P, nb));
        LCHK(stm_launch_null_refine(K.d_Xs.p, n, P.d_Rdead.p, (int)k0, nb, (int)ncol, Z.d_N.p, st));
        return 0;
    }));
    marks.mark(1, st);
    // ---- G = N'N; |N|_F^2 is its trace ----
    LCHK(stm_launch_null_gram(Z.d_N.p, (int)ncol, d, sl.height, sl.count, d_part.p, Z.d_L.p, st));
    std::vector<double> diag((size_t)d);
    HIPCHK(hipMemcpy2DAsync(diag.data(), sizeof(double), Z.d_L.p, ((size_t)d + 1) * sizeof(double), sizeof(double), (size_t)d, hipMemcpyDeviceToHost, st));
    marks.mark(2, st);
    // ---- G = L L' ----
    for (int p = 0; p < np; p++) {
        LCHK(stm_launch_null_chol_panel(Z.d_L.p, Z.d_Ld.p, d, p, K.d_err.p, st));
        LCHK(stm_launch_null_chol_update(Z.d_L.p, d, p, st));
    }
    marks.mark(3, st);
    std::vector<double> ld((size_t)np * STM_NULL_NB * STM_NULL_NB);
    HIPCHK(hipMemcpyAsync(ld.data(), Z.d_Ld.p, ld.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    PASS(end_resident_op(P));                                                // (a pivot that is not positive and finite; synchronizes)
    marks.read(Z.ms);
    double tr = 0.0, lmin = HUGE_VAL;
    for (double g : diag) tr += g;
    for (int k = 0; k < d; k++)
        lmin = std::min(lmin, ld[(size_t)(k / STM_NULL_NB) * STM_NULL_NB * STM_NULL_NB + (size_t)(k % STM_NULL_NB) * (STM_NULL_NB + 1)]);
    Z.ncol = ncol; Z.d = d; Z.r = (int)pc.size(); Z.nfro = std::sqrt(tr); Z.lmin = lmin;
    Z.ready = true;
    return 0;
}
// *built: this call made N and L (0: it found them)
int ensure_nullspace(stmmqr_plan &P, long ncol, int *built)
{
    NullSpace &Z = P.res.fact.null;
    *built = 0;
    if (Z.ready && Z.ncol == ncol) return 0;
    const int e = build_nullspace(P, ncol);
    if (e) { Z.release(); return e; }
    *built = 1;
    return 0;
}

// X (ncol x nrhs at K.d_Xall, the caller's column order or, permuted, R's) <- (I - N G^-1 N')^2 X; *worst = the largest
// |N'x_out| / (|N|_F |x_in|) of the vectors
int project_vectors(stmmqr_plan &P, long ncol, stm_long nrhs, int permuted, double *worst)
{
    auto &K = P.res.call;
    const NullSpace &Z = P.res.fact.null;
    hipStream_t st = P.stream;
    const int d = Z.d, bmax = rhs_batch_max();
    const NullSlabs sl = null_slabs(ncol, knobs::num(knobs::K_NULL_SLAB));
    const size_t nbmax = (size_t)std::min<stm_long>(bmax, nrhs);
    const int *qf = (!permuted && P.has_qfill) ? P.res.sched.d_Qfill.p : nullptr;
    LCHK(grow(K.d_nlX, nbmax * (size_t)ncol));
    LCHK(grow(K.d_nlT, nbmax * (size_t)d));
    LCHK(grow(K.d_nlP, nbmax * (size_t)sl.count * (size_t)d));
    LCHK(grow(K.d_nlS, 2 * nbmax));
    std::vector<double> sc(2 * nbmax);
    *worst = 0.0;
    for (stm_long j0 = 0; j0 < nrhs; j0 += bmax) {
        const int nb = (int)std::min<stm_long>(bmax, nrhs - j0);
        double *Xc = K.d_Xall.p + j0 * ncol, *Xw = K.d_nlX.p;
        LCHK(stm_launch_perm(Xc, qf, Xw, (int)ncol, 0, st, nb, ncol, ncol));                 // x[k] = X[Qfill[k]]
        LCHK(stm_launch_null_norm2(Xw, ncol, (int)ncol, nb, K.d_nlS.p, st));
        for (int pass = 0; pass < 2; pass++) {                                              // twice is enough
            LCHK(stm_launch_null_nt(Z.d_N.p, (int)ncol, d, sl.height, sl.count, Xw, ncol, nb, K.d_nlP.p, K.d_nlT.p, st));
            LCHK(stm_launch_null_llt(Z.d_L.p, Z.d_Ld.p, d, K.d_nlT.p, nb, st));
            LCHK(stm_launch_null_sub(Z.d_N.p, (int)ncol, d, K.d_nlT.p, nb, Xw, ncol, st));
        }
        LCHK(stm_launch_null_nt(Z.d_N.p, (int)ncol, d, sl.height, sl.count, Xw, ncol, nb, K.d_nlP.p, K.d_nlT.p, st));
        LCHK(stm_launch_null_norm2(K.d_nlT.p, d, d, nb, K.d_nlS.p + nb, st));
        LCHK(stm_launch_perm(Xw, qf, Xc, (int)ncol, 1, st, nb, ncol, ncol));                 // X[Qfill[k]] = x[k]
        HIPCHK(hipMemcpyAsync(sc.data(), K.d_nlS.p, 2 * (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int v = 0; v < nb; v++)
            if (sc[(size_t)v] > 0.0) *worst = std::max(*worst, std::sqrt(sc[(size_t)(nb + v)]) / (Z.nfro * std::sqrt(sc[(size_t)v])));
    }
    return 0;
}
void write_info(double *info, double d, double worst, double nfro, double lmin, int built)
{
    if (!info) return;
    const double v[8] = {d, worst, nfro, lmin, (double)built, 0.0, 0.0, 0.0};
    memcpy(info, v, sizeof v);
}
int project_impl(stmmqr_plan *plan, stm_long ncol, double *X, stm_long ldx, stm_long nrhs, int permuted, int on_device, double *info,
                 const char *what)
{
    PASS(check_factored(plan));
    stmmqr_plan &P = *plan;
    if (!X || nrhs < 0) return fail(STMMQR_ERR_INVALID, std::string(what) + ": bad arguments (X is NULL or nrhs < 0)");
    PASS(null_checks(P, ncol, what));
    if (ldx < ncol) return fail(STMMQR_ERR_INVALID, std::string(what) + ": bad leading dimension");
    if (nrhs == 0) return 0;
    long d = 0;
    PASS(count_dead(P, ncol, d));
    if (d == 0) { write_info(info, 0.0, 0.0, 0.0, 0.0, 0); return 0; }      // full rank: X stays as it is, nothing is launched
    PASS(begin_resident_op(P));
    auto &K = P.res.call;
    hipStream_t st = P.stream;
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), st));
    int built = 0;
    PASS(ensure_nullspace(P, ncol, &built));
    PASS(stage_in(K.d_Xall, X, ldx, ncol, nrhs, on_device, st));
    double worst = 0.0;
    PASS(project_vectors(P, ncol, nrhs, permuted, &worst));
    PASS(stage_out(K.d_Xall, X, ldx, ncol, nrhs, on_device, st));
    PASS(end_resident_op(P));
    const auto &Z = P.res.fact.null;
    write_info(info, (double)Z.d, worst, Z.nfro, Z.lmin, built);
    return 0;
}
}  // namespace

// the null-space basis of R over the first ncol columns; see include/stmmqr_hip.h
int stmmqr_plan_nullspace(stmmqr_plan *plan, stm_long ncol, stm_long *ndead, double *N, stm_long ldn, int permuted, int on_device)
{
    PASS(check_factored(plan));
    stmmqr_plan &P = *plan;
    if (!ndead) return fail(STMMQR_ERR_INVALID, "nullspace: ndead is NULL");
    PASS(null_checks(P, ncol, "nullspace"));
    if (N && ldn < ncol) return fail(STMMQR_ERR_INVALID, "nullspace: bad leading dimension");
    long d = 0;
    PASS(count_dead(P, ncol, d));
    if (!N || d == 0) { *ndead = d; return 0; }
    PASS(begin_resident_op(P));
    auto &K = P.res.call;
    hipStream_t st = P.stream;
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), st));
    int built = 0;
    PASS(ensure_nullspace(P, ncol, &built));
    const auto &Z = P.res.fact.null;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (permuted || !P.has_qfill) {
        PASS(copy_cols(N, ldn, Z.d_N.p, ncol, ncol, d, kind, st));
    } else {
        // rows through Qfill: out[Qfill[j]] = N[j], the columns in launches of at most 32768
        double *dst = N;
        long ldd = ldn;
        if (!on_device) { LCHK(grow(K.d_Yall, (size_t)ncol * (size_t)d)); dst = K.d_Yall.p; ldd = ncol; }
        for (long k0 = 0; k0 < d; k0 += 32768) {
            const int nb = (int)std::min(32768L, d - k0);
            LCHK(stm_launch_perm(Z.d_N.p + k0 * ncol, P.res.sched.d_Qfill.p, dst + k0 * ldd, (int)ncol, 1, st, nb, ncol, ldd));
        }
        if (!on_device) PASS(copy_cols(N, ldn, dst, ncol, ncol, d, kind, st));
    }
    PASS(end_resident_op(P));
    *ndead = d;
    return 0;
}

// device ms of the last build of the basis held: N, the Gram matrix, the Cholesky factorization (tools/time_lsminnorm.py)
int stmmqr_plan_nullspace_times(const stmmqr_plan *plan, double *ms)
{
    if (!plan || !ms) return fail(STMMQR_ERR_INVALID, "nullspace_times: null argument");
    const auto &Z = plan->res.fact.null;
    if (!Z.ready || Z.d == 0) return fail(STMMQR_ERR_INVALID, "nullspace_times: the plan holds no null-space basis");
    memcpy(ms, Z.ms, sizeof Z.ms);
    return 0;
}

int stmmqr_plan_project_minnorm(stmmqr_plan *plan, stm_long ncol, double *X, stm_long ldx, stm_long nrhs, int permuted, int on_device,
                                double *info)
{
    return project_impl(plan, ncol, X, ldx, nrhs, permuted, on_device, info, "project_minnorm");
}

// stmmqr_plan_solve, then the projector on its result
int stmmqr_plan_solve_lsminnorm(stmmqr_plan *plan, const double *B, stm_long ldb, double *X, stm_long ldx, stm_long nrhs, int on_device,
                                double *info)
{
    PASS(check_factored(plan));
    if (!B || !X || ldb < plan->m || ldx < plan->n || nrhs < 0) return fail(STMMQR_ERR_INVALID, "bad solve arguments");
    if (!plan->keep_h)
        return fail(STMMQR_ERR_INVALID, "the plan keeps no Householder vectors (keepH = 0): no Q'B; stmmqr_plan_solve_seminormal solves with R only");
    PASS(null_checks(*plan, plan->n, "solve_lsminnorm"));
    if (nrhs == 0) return 0;
    PASS(plan_solve(plan, B, ldb, X, ldx, nrhs, on_device));
    return project_impl(plan, plan->n, X, ldx, nrhs, 0, on_device, info, "solve_lsminnorm");
}
