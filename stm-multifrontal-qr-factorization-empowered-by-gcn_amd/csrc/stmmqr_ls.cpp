// stmmqr_ls.cpp -- the least-squares object: min |A x - B| with the right-hand sides carried through the factorization.
// create (once per pattern and nrhs): the column order stmmqr_sparseqr gives A, the B columns appended unpermuted, stmmqr_analyze of
// the pattern [A | nrhs dense columns], an R-only plan.  solve (any number of times, new values and new B: a Gauss-Newton loop):
// the values [Ax | B] put together on the device, the factorization with ntol = n, stmmqr_plan_solve_carried.  Q is never stored.
#include <cfloat>
#include <memory>
#include <new>

#include "stmmqr_plan.h"

struct stmmqr_ls {
    stm_long m = 0, n = 0, nrhs = 0, anz = 0;
    double tol_arg = -2, tol = 0;                       // as given to create / as used by the last factorization
    std::vector<stm_long> Ap, Bp, Bi, Q;                // A's column pointers; pattern and column order of [A B]
    std::vector<double> Ax;                             // A's values as at create
    stmmqr_analysis *sym = nullptr;
    stmmqr_plan *plan = nullptr;
    int device = -1;
    DevBuf<double> d_val;                               // [Ax | B] on the device
    DevBuf<double> d_resid;                             // residual norms of a solve with device pointers
    std::vector<double> resid;                          // ... of the last solve, on the host (stmmqr_ls_resid)
    bool ax_current = false;                            // d_val holds the values given at create (and tol belongs to them)
    bool pattern_given = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    stmmqr_stats stats = {};
    double sym_info[8] = {}, solve_ms = 0;
    stm_long rank1 = 0, nanalyses = 0, nplans = 0, nsolves = 0;
    ~stmmqr_ls()
    {
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        if (plan) stmmqr_plan_destroy(plan);
        if (sym) stmmqr_analysis_free(sym);
    }
};

extern "C" {

static int ls_create_impl(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                          stm_long nrhs, const stm_long *Quser, const stmmqr_relax *relax, int device, stmmqr_ls **out)
{
    if (!out) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_create: null output");
    *out = nullptr;
    if (m < 0 || n < 0 || !Ap || (Ap[n] > 0 && (!Ai || !Ax))) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_create: bad matrix");
    if (nrhs < 1) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_create: nrhs must be at least 1");
    if (nrhs > STMMQR_LS_MAX_NRHS)
        return fail(STMMQR_ERR_INVALID, "stmmqr_ls_create: nrhs = " + std::to_string(nrhs) + " exceeds the limit of " +
                                            std::to_string(STMMQR_LS_MAX_NRHS) + " right-hand sides per object");
    if (Quser && ordering == 3) {
        std::vector<char> seen((size_t)std::max<stm_long>(n, 1), 0);
        for (stm_long k = 0; k < n; k++) {
            if (Quser[k] < 0 || Quser[k] >= n || seen[(size_t)Quser[k]])
                return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_create: Quser is not a permutation of the columns of A");
            seen[(size_t)Quser[k]] = 1;
        }
    }
    std::unique_ptr<stmmqr_ls> L(new stmmqr_ls());
    L->m = m; L->n = n; L->nrhs = nrhs; L->anz = Ap[n]; L->tol_arg = tol; L->device = device;
    L->Ap.assign(Ap, Ap + n + 1);
    L->Ax.assign(Ax, Ax + L->anz);
    // the tolerance: stmmqr_sparseqr's rule on the columns of A alone (the singleton search below sees the same one)
    double t = tol;
    if (t <= -2) t = stm_qr_default_tol(m, n, Ap, Ax);
    if (t < 0) t = -1;
    L->tol = t;
    // ---- column order of A (orderings and refusals of stmmqr_sparseqr), B columns behind it, unpermuted ----
    L->Q.assign((size_t)(n + nrhs), 0);
    int e = stm_sparseqr_order(ordering, tol, m, n, Ap, Ai, Ax, Quser, L->Q.data());
    if (e) return e;
    for (stm_long j = 0; j < nrhs; j++) L->Q[(size_t)(n + j)] = n + j;
    // ---- pattern of [A | nrhs dense columns] ----
    L->Bp.assign((size_t)(n + nrhs + 1), 0);
    L->Bi.resize((size_t)std::max<stm_long>(L->anz + m * nrhs, 1));
    for (stm_long j = 0; j <= n; j++) L->Bp[(size_t)j] = Ap[j];
    for (stm_long p = 0; p < L->anz; p++) L->Bi[(size_t)p] = Ai[p];
    for (stm_long j = 0; j < nrhs; j++) {
        L->Bp[(size_t)(n + j + 1)] = L->anz + (j + 1) * m;
        for (stm_long i = 0; i < m; i++) L->Bi[(size_t)(L->anz + j * m + i)] = i;
    }
    e = stmmqr_analyze(m, n + nrhs, L->Bp.data(), L->Bi.data(), L->Q.data(), t >= 0, relax, &L->sym);
    if (e) return e;
    L->nanalyses++;
    (void)stmmqr_analysis_info(L->sym, L->sym_info);
    if (device != -2) {
        const stm_qr_symbolic *S = stmmqr_analysis_symbolic(L->sym);
        stmmqr_symbolic_view V;
        memset(&V, 0, sizeof V);
        V.m = S->m; V.n = S->n; V.anz = S->anz; V.nf = S->nf; V.maxfn = S->maxfn; V.rjsize = S->rjsize; V.hisize = S->hisize;
        V.do_rank_detection = S->do_rank_detection;
        V.Sp = S->Sp; V.Sj = S->Sj; V.Qfill = S->Qfill; V.PLinv = S->PLinv; V.Sleft = S->Sleft; V.Child = S->Child; V.Childp = S->Childp;
        V.Super = S->Super; V.Rp = S->Rp; V.Rj = S->Rj; V.Post = S->Post; V.Hip = S->Hip; V.Fm = S->Fm; V.maxstack = S->maxstack;
        V.r_only = 1;
        int st = 0;
        L->plan = stmmqr_plan_create(&V, device, &st);
        if (!L->plan) return st ? st : STMMQR_ERR_DEVICE;
        L->nplans++;
        HIPCHK(hipSetDevice(L->plan->device));
        HIPCHK(hipEventCreate(&L->ev[0]));
        HIPCHK(hipEventCreate(&L->ev[1]));
        LCHK(L->d_val.alloc((size_t)std::max<stm_long>(L->anz + m * nrhs, 1)));
    }
    *out = L.release();
    return 0;
}

int stmmqr_ls_create(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                     stm_long nrhs, const stm_long *Quser, const stmmqr_relax *relax, int device, stmmqr_ls **out)
{
    try {
        return ls_create_impl(ordering, tol, m, n, Ap, Ai, Ax, nrhs, Quser, relax, device, out);
    } catch (const std::bad_alloc &) {
        return stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_ls_create: out of memory");
    }
}

int stmmqr_ls_solve(stmmqr_ls *ls, const double *Ax, int ax_on_device, const double *B, stm_long ldb, double *X, stm_long ldx,
                    double *resid, int on_device)
{
    if (!ls) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve: null object");
    if (!ls->plan) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve: the object holds the host half only (device = -2 at create)");
    stmmqr_ls &L = *ls;
    const stm_long m = L.m, n = L.n, k = L.nrhs, anz = L.anz;
    if (!B || !X || ldb < m || ldx < n) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve: bad arguments");
    stmmqr_plan &P = *L.plan;
    HIPCHK(hipSetDevice(P.device));
    hipStream_t st = P.stream;
    // ---- values [Ax | B] on the device; the tolerance follows the values of A ----
    try {
        if (Ax || !L.ax_current) {
            const double *src = Ax ? Ax : L.Ax.data();
            const bool dev = Ax && ax_on_device;
            if (anz > 0) HIPCHK(hipMemcpyAsync(L.d_val.p, src, (size_t)anz * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
            if (L.tol_arg <= -2) {
                std::vector<double> h;
                if (dev) {                                  // (the rule reads every value: one copy back of A's values)
                    h.resize((size_t)std::max<stm_long>(anz, 1));
                    if (anz > 0) HIPCHK(hipMemcpyAsync(h.data(), Ax, (size_t)anz * sizeof(double), hipMemcpyDeviceToHost, st));
                    HIPCHK(hipStreamSynchronize(st));
                    src = h.data();
                }
                L.tol = stm_qr_default_tol(m, n, L.Ap.data(), src);
            }
            HIPCHK(hipStreamSynchronize(st));
            L.ax_current = (Ax == nullptr);
        }
    } catch (const std::bad_alloc &) {
        return stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_ls_solve: out of memory");
    }
    if (m > 0)
        HIPCHK(hipMemcpy2DAsync(L.d_val.p + anz, (size_t)m * sizeof(double), B, (size_t)ldb * sizeof(double), (size_t)m * sizeof(double), (size_t)k,
                                on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    // ---- factorize [A B], the B columns never rank-tested; solve with R alone ----
    const bool first = !L.pattern_given;
    int e = stmmqr_factorize_device(L.plan, first ? L.Bp.data() : nullptr, first ? L.Bi.data() : nullptr, L.d_val.p, 1, L.tol, n, &L.stats);
    if (e) return e;
    L.pattern_given = true;
    HIPCHK(hipEventRecord(L.ev[0], st));
    L.resid.assign((size_t)k, 0.0);
    if (on_device && !L.d_resid.p) LCHK(L.d_resid.alloc((size_t)k));
    e = stmmqr_plan_solve_carried(L.plan, k, X, ldx, on_device ? L.d_resid.p : L.resid.data(), on_device);
    if (e) return e;
    if (on_device) {
        HIPCHK(hipMemcpyAsync(L.resid.data(), L.d_resid.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
        if (resid) HIPCHK(hipMemcpyAsync(resid, L.d_resid.p, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, st));
    } else if (resid) memcpy(resid, L.resid.data(), (size_t)k * sizeof(double));
    HIPCHK(hipEventRecord(L.ev[1], st));
    // rank of A: the live columns among the first n (SparseQR's rank1)
    std::vector<char> rd((size_t)std::max<stm_long>(n, 1), 0);
    if (n > 0) HIPCHK(hipMemcpyAsync(rd.data(), P.d_Rdead.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, L.ev[0], L.ev[1]));
    L.solve_ms = ms;
    L.rank1 = 0;
    for (stm_long j = 0; j < n; j++) L.rank1 += !rd[(size_t)j];
    L.nsolves++;
    return 0;
}

const stm_qr_symbolic *stmmqr_ls_symbolic_view(const stmmqr_ls *ls) { return (ls && ls->sym) ? stmmqr_analysis_symbolic(ls->sym) : nullptr; }
stmmqr_plan *stmmqr_ls_plan(stmmqr_ls *ls) { return ls ? ls->plan : nullptr; }

int stmmqr_ls_info(const stmmqr_ls *ls, double *info)
{
    if (!ls || !info) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_info: null argument");
    const stm_qr_symbolic *S = stmmqr_analysis_symbolic(ls->sym);
    info[0] = (double)ls->rank1; info[1] = (double)S->nf; info[2] = ls->stats.flops; info[3] = ls->sym_info[0];
    info[4] = ls->stats.ms_total; info[5] = ls->solve_ms; info[6] = ls->stats.device_bytes + (double)ls->d_val.n * sizeof(double);
    info[7] = (double)ls->stats.retries; info[8] = (double)ls->stats.reschedules;
    info[9] = (double)ls->nanalyses; info[10] = (double)ls->nplans; info[11] = (double)ls->nsolves;
    info[12] = ls->tol; info[13] = (double)ls->nrhs;
    return 0;
}

int stmmqr_ls_resid(const stmmqr_ls *ls, double *resid)
{
    if (!ls || !resid || ls->resid.size() != (size_t)ls->nrhs) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_resid: no solve yet");
    memcpy(resid, ls->resid.data(), ls->resid.size() * sizeof(double));
    return 0;
}

// the unscaled variances of the last solve's x: diag((A_live' A_live)^-1) from the R of [A B] the object holds (the A part of the view)
int stmmqr_ls_covariance_diag(stmmqr_ls *ls, double *var, int on_device)
{
    if (!ls) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_covariance_diag: null object");
    if (!ls->plan) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_covariance_diag: the object holds the host half only (device = -2 at create)");
    if (ls->nsolves < 1) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_covariance_diag: no solve yet");
    return stmmqr_plan_covariance_diag(ls->plan, ls->n, var, on_device);
}

// the refusals the diagnostics of a fit share (what = the entry point's name)
static int ls_fit_ready(const stmmqr_ls *ls, const char *what)
{
    if (!ls) return stm_fail(STMMQR_ERR_INVALID, (std::string(what) + ": null object").c_str());
    if (!ls->plan) return stm_fail(STMMQR_ERR_INVALID, (std::string(what) + ": the object holds the host half only (device = -2 at create)").c_str());
    if (ls->nsolves < 1) return stm_fail(STMMQR_ERR_INVALID, (std::string(what) + ": no solve yet").c_str());
    return 0;
}
// leverages of the rows of A (and, var non-NULL, the variances from the same selected inversion) / entries of (A_live' A_live)^-1
int stmmqr_ls_leverage(stmmqr_ls *ls, double *lev, double *var, int on_device)
{
    if (int e = ls_fit_ready(ls, "stmmqr_ls_leverage")) return e;
    return stmmqr_plan_leverage(ls->plan, ls->n, lev, var, on_device);
}
int stmmqr_ls_covariance_entries(stmmqr_ls *ls, stm_long npairs, const stm_long *I, const stm_long *J, double *out, int on_device)
{
    if (int e = ls_fit_ready(ls, "stmmqr_ls_covariance_entries")) return e;
    return stmmqr_plan_covariance_entries(ls->plan, ls->n, npairs, I, J, out, on_device);
}

// the condition of A(:, live) from the R of [A B] the object holds
int stmmqr_ls_condest(stmmqr_ls *ls, int kind, int iters, double *out, double *v, int on_device)
{
    if (int e = ls_fit_ready(ls, "stmmqr_ls_condest")) return e;
    return stmmqr_plan_condest(ls->plan, ls->n, kind, iters, out, v, on_device);
}

// the null vectors of A(:, Q) from the R of [A B] the object holds, and the projector that makes the last solve's x the minimum-norm one
int stmmqr_ls_nullspace(stmmqr_ls *ls, stm_long *ndead, double *N, stm_long ldn, int on_device)
{
    if (int e = ls_fit_ready(ls, "stmmqr_ls_nullspace")) return e;
    return stmmqr_plan_nullspace(ls->plan, ls->n, ndead, N, ldn, 0, on_device);
}
int stmmqr_ls_project_minnorm(stmmqr_ls *ls, double *X, stm_long ldx, stm_long nrhs, int on_device, double *info)
{
    if (int e = ls_fit_ready(ls, "stmmqr_ls_project_minnorm")) return e;
    return stmmqr_plan_project_minnorm(ls->plan, ls->n, X, ldx, nrhs, 0, on_device, info);
}

void stmmqr_ls_free(stmmqr_ls *ls) { delete ls; }

}  // extern "C"
