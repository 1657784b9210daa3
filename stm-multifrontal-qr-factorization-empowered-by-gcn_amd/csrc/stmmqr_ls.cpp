// stmmqr_ls.cpp -- the least-squares object: min |A x - B| with the right-hand sides carried through the factorization.
// create (once per pattern and nrhs): the column order stmmqr_sparseqr gives A, the B columns appended unpermuted, stmmqr_analyze of
// the pattern [A | nrhs dense columns], an R-only plan.  solve (any number of times, new values and new B: a Gauss-Newton loop):
// the values [Ax | B] put together on the device, the factorization with ntol = n, stmmqr_plan_solve_carried.  Q is never stored.
// The damped mode (stmmqr_ls_create_damped / stmmqr_ls_solve_damped): min |W (A x - b)|^2 + |D x|^2 as the plain object of the
// (m + n) x n matrix [W A; D] with the right-hand sides [W B; 0].  A's columns are ordered as the plain object orders them, the
// analysis is made once of the pattern [A; I | dense columns], and every solve builds the values on the device from
// (Ax, w, d, lambda, B) with the kernels of stmmqr_lsbuild.hip: no host round trip, nothing analysed or planned again.
// The adjoint (stmmqr_ls_adjoint): the backward pass of the last solve on either kind of object -- gradients on A's pattern, of B, w
// and D -- from the resident factors: two triangular passes per normal solve, products with the plan's own matrix, the kernels of
// stmmqr_lsadjoint.hip.
#include <cfloat>
#include <climits>
#include <memory>
#include <new>

#include "stmmqr_plan.h"
#include "stmmqr_sparseqr.h"          // (stm_qr_tol_of_maxnorm)
#include "stmmqr_lsobj.h"             // (struct stmmqr_ls)

extern "C" {

// the refusals both kinds of object share at create (what = the entry point's name); *out = NULL
static int ls_create_args(const std::string &what, int ordering, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai,
                          const double *Ax, stm_long nrhs, const stm_long *Quser, stmmqr_ls **out)
{
    if (!out) return fail(STMMQR_ERR_INVALID, what + ": null output");
    *out = nullptr;
    if (m < 0 || n < 0 || !Ap || (Ap[n] > 0 && (!Ai || !Ax))) return fail(STMMQR_ERR_INVALID, what + ": bad matrix");
    if (nrhs < 1) return fail(STMMQR_ERR_INVALID, what + ": nrhs must be at least 1");
    if (nrhs > STMMQR_LS_MAX_NRHS)
        return fail(STMMQR_ERR_INVALID, what + ": nrhs = " + std::to_string(nrhs) + " exceeds the limit of " +
                                            std::to_string(STMMQR_LS_MAX_NRHS) + " right-hand sides per object");
    if (Quser && ordering == 3) {
        std::vector<char> seen((size_t)std::max<stm_long>(n, 1), 0);
        for (stm_long k = 0; k < n; k++) {
            if (Quser[k] < 0 || Quser[k] >= n || seen[(size_t)Quser[k]])
                return fail(STMMQR_ERR_INVALID, what + ": Quser is not a permutation of the columns of A");
            seen[(size_t)Quser[k]] = 1;
        }
    }
    return 0;
}

static int ls_create_impl(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                          stm_long nrhs, const stm_long *Quser, const stmmqr_relax *relax, int device, stmmqr_ls **out)
{
    PASS(ls_create_args("stmmqr_ls_create", ordering, m, n, Ap, Ai, Ax, nrhs, Quser, out));
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

// The damped object: A's columns ordered as ls_create_impl orders them, then the plain object of the pattern [A; I] with that order
// GIVEN; what the device path reads of A besides the plan goes up once.
static int ls_create_damped_impl(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                                 stm_long nrhs, const stm_long *Quser, const stmmqr_relax *relax, int device, stmmqr_ls **out)
{
    PASS(ls_create_args("stmmqr_ls_create_damped", ordering, m, n, Ap, Ai, Ax, nrhs, Quser, out));
    const stm_long anz = Ap[n];
    if (device != -2 && (n >= INT_MAX || anz >= INT_MAX))
        return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_create_damped: 2^31 or more columns or entries (the device tables of A are int)");
    std::vector<stm_long> Q((size_t)std::max<stm_long>(n, 1), 0);
    PASS(stm_sparseqr_order(ordering, tol, m, n, Ap, Ai, Ax, Quser, Q.data()));
    // ---- [A; I]: column j = A's entries in their given order, then row m + j (the value 1 stands in until a solve builds D) ----
    std::vector<stm_long> Cp((size_t)n + 1, 0), Ci((size_t)std::max<stm_long>(anz + n, 1), 0);
    std::vector<double> Cx((size_t)std::max<stm_long>(anz + n, 1), 1.0);
    for (stm_long j = 0; j < n; j++) {
        Cp[(size_t)j] = Ap[j] + j;
        for (stm_long p = Ap[j]; p < Ap[j + 1]; p++) {
            if (Ai[p] < 0 || Ai[p] >= m) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_create_damped: row index out of range");
            Ci[(size_t)(p + j)] = Ai[p]; Cx[(size_t)(p + j)] = Ax[p];
        }
        Ci[(size_t)(Ap[j + 1] + j)] = m + j;
    }
    Cp[(size_t)n] = anz + n;
    stmmqr_ls *made = nullptr;
    PASS(ls_create_impl(3, tol, m + n, n, Cp.data(), Ci.data(), Cx.data(), nrhs, n > 0 ? Q.data() : nullptr, relax, device, &made));
    std::unique_ptr<stmmqr_ls> L(made);
    L->damped = true; L->am = m; L->aanz = anz;
    L->Ax.assign(Ax, Ax + anz);
    if (L->plan) {
        HIPCHK(hipSetDevice(L->plan->device));
        HIPCHK(hipEventCreate(&L->ev_build[0]));
        HIPCHK(hipEventCreate(&L->ev_build[1]));
        std::vector<int> ap((size_t)n + 1), ai((size_t)std::max<stm_long>(anz, 1), 0);
        for (stm_long j = 0; j <= n; j++) ap[(size_t)j] = (int)Ap[j];
        for (stm_long p = 0; p < anz; p++) ai[(size_t)p] = (int)Ai[p];
        LCHK(L->d_ap.alloc(ap.size()));
        LCHK(L->d_ai.alloc((size_t)anz));
        LCHK(L->d_ax.alloc((size_t)anz));
        LCHK(L->d_D.alloc((size_t)n));
        HIPCHK(hipMemcpy(L->d_ap.p, ap.data(), ap.size() * sizeof(int), hipMemcpyHostToDevice));
        if (anz > 0) {
            HIPCHK(hipMemcpy(L->d_ai.p, ai.data(), (size_t)anz * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L->d_ax.p, Ax, (size_t)anz * sizeof(double), hipMemcpyHostToDevice));
        }
        L->ax_current = true;
        if (tol <= -2) {
            std::vector<long long> ap2(Cp.begin(), Cp.end());
            LCHK(L->d_ap2.alloc(ap2.size()));
            LCHK(L->d_head.alloc(2));
            HIPCHK(hipMemcpy(L->d_ap2.p, ap2.data(), ap2.size() * sizeof(long long), hipMemcpyHostToDevice));
        }
    }
    *out = L.release();
    return 0;
}

int stmmqr_ls_create_damped(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                            stm_long nrhs, const stm_long *Quser, const stmmqr_relax *relax, int device, stmmqr_ls **out)
{
    try {
        return ls_create_damped_impl(ordering, tol, m, n, Ap, Ai, Ax, nrhs, Quser, relax, device, out);
    } catch (const std::bad_alloc &) {
        if (out) *out = nullptr;
        return stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_ls_create_damped: out of memory");
    }
}

int stmmqr_ls_solve(stmmqr_ls *ls, const double *Ax, int ax_on_device, const double *B, stm_long ldb, double *X, stm_long ldx,
                    double *resid, int on_device)
{
    if (!ls) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve: null object");
    if (ls->damped) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve: a damped object (stmmqr_ls_create_damped): use stmmqr_ls_solve_damped");
    if (!ls->plan) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve: the object holds the host half only (device = -2 at create)");
    stmmqr_ls &L = *ls;
    const stm_long m = L.m, n = L.n, k = L.nrhs, anz = L.anz;
    if (!B || !X || ldb < m || ldx < n) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve: bad arguments");
    stmmqr_plan &P = *L.plan;
    HIPCHK(hipSetDevice(P.device));
    hipStream_t st = P.stream;
    L.last_solve_ok = false;                               // (until this solve has come to its end: stmmqr_ls_adjoint)
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
    L.last_solve_ok = true;
    return 0;
}

// One damped solve: the values of [W A; D | W B; 0] built on the plan's stream, the factorization with ntol = n, the carried solve,
// |D x_j|.  The only host wait before the factorization is the copy of the largest column norm (default tolerance).
static int ls_solve_damped_impl(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_damping *dmp, const double *B,
                                stm_long ldb, double *X, stm_long ldx, double *resid, int on_device)
{
    if (!ls) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve_damped: null object");
    if (!ls->damped) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve_damped: a plain object (stmmqr_ls_create): use stmmqr_ls_solve");
    if (!dmp) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve_damped: null damping (dmp)");
    if (!(dmp->lambda >= 0) || !std::isfinite(dmp->lambda))
        return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve_damped: lambda must be finite and not negative");
    if (dmp->scale != 0 && dmp->scale != 1) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve_damped: scale must be 0 or 1");
    if (dmp->scale == 1 && !(dmp->scale_min > 0 && dmp->scale_min <= dmp->scale_max))
        return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve_damped: scale = 1 needs 0 < scale_min <= scale_max");
    if (!ls->plan)
        return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve_damped: the object holds the host half only (device = -2 at create)");
    stmmqr_ls &L = *ls;
    const stm_long am = L.am, mn = L.m, n = L.n, k = L.nrhs, aanz = L.aanz, anz = L.anz;
    if (!B || !X || ldb < am || ldx < n) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_solve_damped: bad arguments");
    stmmqr_plan &P = *L.plan;
    HIPCHK(hipSetDevice(P.device));
    hipStream_t st = P.stream;
    L.last_solve_ok = false;                               // (until this solve has come to its end: stmmqr_ls_adjoint)
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const double sl = std::sqrt(dmp->lambda);
    // ---- the inputs on the device ----
    const double *dAx = L.d_ax.p;
    if (Ax && ax_on_device) dAx = Ax;
    else if (Ax) {
        L.ax_current = false;
        if (aanz > 0) HIPCHK(hipMemcpyAsync(L.d_ax.p, Ax, (size_t)aanz * sizeof(double), hipMemcpyHostToDevice, st));
    } else if (!L.ax_current) {
        if (aanz > 0) HIPCHK(hipMemcpyAsync(L.d_ax.p, L.Ax.data(), (size_t)aanz * sizeof(double), hipMemcpyHostToDevice, st));
        L.ax_current = true;
    }
    const double *dw = dmp->w;
    if (dmp->w && !on_device) {
        if (!L.d_w.p) LCHK(L.d_w.alloc((size_t)am));
        if (am > 0) HIPCHK(hipMemcpyAsync(L.d_w.p, dmp->w, (size_t)am * sizeof(double), hipMemcpyHostToDevice, st));
        dw = L.d_w.p;
    }
    const double *dd = dmp->d;
    if (dmp->d && !on_device) {                             // (the scales go into D, which k_lsb_diag then rewrites in place)
        if (n > 0) HIPCHK(hipMemcpyAsync(L.d_D.p, dmp->d, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        dd = L.d_D.p;
    }
    double *dBv = L.d_val.p + anz;
    if (am > 0)
        HIPCHK(hipMemcpy2DAsync(dBv, (size_t)mn * sizeof(double), B, (size_t)ldb * sizeof(double), (size_t)am * sizeof(double), (size_t)k, in, st));
    // ---- the values of [W A; D | W B; 0] ----
    HIPCHK(hipEventRecord(L.ev_build[0], st));
    HIPCHK((hipError_t)stm_launch_lsb_values((long long)aanz, (int)n, L.d_ap.p, L.d_ai.p, dAx, dw, L.d_val.p, st));
    if (dd || dmp->scale == 0) HIPCHK((hipError_t)stm_launch_lsb_diag((int)n, L.d_ap.p, dd, sl, L.d_D.p, L.d_val.p, st));
    else HIPCHK((hipError_t)stm_launch_lsb_marquardt((int)n, L.d_ap.p, sl, dmp->scale_min, dmp->scale_max, L.d_D.p, L.d_val.p, st));
    HIPCHK((hipError_t)stm_launch_lsb_rhs((long long)am, (long long)n, (int)k, dw, dBv, st));
    if (L.tol_arg <= -2) {                                  // the project's rule on [W A; D], from the built values
        HIPCHK(hipMemsetAsync(L.d_head.p, 0, 2 * sizeof(double), st));
        HIPCHK((hipError_t)stm_launch_rf_colnorm((long long)n, L.d_ap2.p, nullptr, L.d_val.p, (unsigned long long *)L.d_head.p, st));
    }
    HIPCHK(hipEventRecord(L.ev_build[1], st));
    if (L.tol_arg <= -2) {
        double mx = 0;
        HIPCHK(hipMemcpyAsync(&mx, L.d_head.p, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        L.tol = stm_qr_tol_of_maxnorm(mn, n, mx);
    }
    // ---- factorize, the B columns never rank-tested; solve with R alone ----
    const bool first = !L.pattern_given;
    PASS(stmmqr_factorize_device(L.plan, first ? L.Bp.data() : nullptr, first ? L.Bi.data() : nullptr, L.d_val.p, 1, L.tol, n, &L.stats));
    L.pattern_given = true;
    HIPCHK(hipEventRecord(L.ev[0], st));
    double *dX = X;
    stm_long ldd = ldx;
    if (!on_device) {
        ldd = std::max<stm_long>(n, 1);
        if (!L.d_x.p) LCHK(L.d_x.alloc((size_t)(ldd * k)));
        dX = L.d_x.p;
    }
    if (!L.d_resid.p) LCHK(L.d_resid.alloc((size_t)k));
    if (!L.d_dn.p) LCHK(L.d_dn.alloc((size_t)k));
    L.resid.assign((size_t)k, 0.0);
    PASS(stmmqr_plan_solve_carried(L.plan, k, dX, ldd, L.d_resid.p, 1));
    HIPCHK((hipError_t)stm_launch_lsb_dnorm((int)n, (int)k, L.d_D.p, dX, (long long)ldd, L.d_dn.p, st));
    HIPCHK(hipMemcpyAsync(L.resid.data(), L.d_resid.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    if (resid) HIPCHK(hipMemcpyAsync(resid, L.d_resid.p, (size_t)k * sizeof(double), back, st));
    if (dmp->dnorm) HIPCHK(hipMemcpyAsync(dmp->dnorm, L.d_dn.p, (size_t)k * sizeof(double), back, st));
    if (dmp->D_out && n > 0) HIPCHK(hipMemcpyAsync(dmp->D_out, L.d_D.p, (size_t)n * sizeof(double), back, st));
    if (!on_device && n > 0)
        HIPCHK(hipMemcpy2DAsync(X, (size_t)ldx * sizeof(double), dX, (size_t)ldd * sizeof(double), (size_t)n * sizeof(double), (size_t)k,
                                hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(L.ev[1], st));
    std::vector<char> rd((size_t)std::max<stm_long>(n, 1), 0);
    if (n > 0) HIPCHK(hipMemcpyAsync(rd.data(), P.d_Rdead.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, L.ev[0], L.ev[1]));
    L.solve_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, L.ev_build[0], L.ev_build[1]));
    L.build_ms = ms;
    L.rank1 = 0;
    for (stm_long j = 0; j < n; j++) L.rank1 += !rd[(size_t)j];
    L.nsolves++;
    L.last_solve_ok = true;
    return 0;
}

int stmmqr_ls_solve_damped(stmmqr_ls *ls, const double *Ax, int ax_on_device, const stmmqr_ls_damping *dmp, const double *B, stm_long ldb,
                           double *X, stm_long ldx, double *resid, int on_device)
{
    try {
        return ls_solve_damped_impl(ls, Ax, ax_on_device, dmp, B, ldb, X, ldx, resid, on_device);
    } catch (const std::bad_alloc &) {
        return stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_ls_solve_damped: out of memory");
    }
}

// The adjoint of the last solve; see include/stmmqr_hip.h.  z = E R11^-1 R11^-T E' xbar on the view of the R of [C | Bt] that ends at
// column n (vectors zero beyond n, as the condition estimate has them: the leading rows of R' \ [v; 0] are R11' \ v and
// R \ [y; 0] = R11 \ y), refined with products with the plan's own matrix: rt_k = [C | Bt] [-x_k; e_k], ut_k = [C | Bt] [z_k; 0], and
// C'(C z) is the head of [C | Bt]' (C z).  Then the kernels of stmmqr_lsadjoint.hip.
static int ls_adjoint_impl(stmmqr_ls *ls, const double *X, stm_long ldx, const double *Xbar, stm_long ldxb, const double *w, int refine,
                           double *Axbar, double *Bbar, stm_long ldbb, double *wbar, double *Dbar, int on_device, double *info)
{
    const std::string F = "stmmqr_ls_adjoint: ";
    if (!ls) return fail(STMMQR_ERR_INVALID, F + "null object");
    if (!ls->plan) return fail(STMMQR_ERR_INVALID, F + "the object holds the host half only (device = -2 at create)");
    if (ls->nsolves < 1) return fail(STMMQR_ERR_INVALID, F + "no solve yet");
    if (!ls->last_solve_ok) return fail(STMMQR_ERR_INVALID, F + "the last solve failed (the factors belong to no solution)");
    stmmqr_ls &L = *ls;
    const stm_long am = L.damped ? L.am : L.m, mc = L.m, n = L.n, k = L.nrhs, na = n + k, aanz = L.damped ? L.aanz : L.anz;
    if (!X || !Xbar) return fail(STMMQR_ERR_INVALID, F + "X or Xbar is NULL");
    if (ldx < n || ldxb < n) return fail(STMMQR_ERR_INVALID, F + "a leading dimension of X or Xbar is smaller than n = " + std::to_string(n));
    if (Bbar && ldbb < am) return fail(STMMQR_ERR_INVALID, F + "ldbb = " + std::to_string(ldbb) + " is smaller than m = " + std::to_string(am));
    if (refine < 0) return fail(STMMQR_ERR_INVALID, F + "refine is negative");
    if (!L.damped && (w || wbar || Dbar))
        return fail(STMMQR_ERR_INVALID, F + "w, wbar and Dbar must be NULL on a plain object (stmmqr_ls_create)");
    if (!L.damped && aanz >= INT_MAX) return fail(STMMQR_ERR_INVALID, F + "2^31 or more entries (the device table of A's rows is int)");
    stmmqr_plan &P = *L.plan;
    PASS(check_factored(&P));
    PASS(check_carried_view(P, n));
    if (!holds_whole_tree(P))
        return fail(STMMQR_ERR_INVALID, F + "the plan does not hold the whole tree in one group (groups were set, or fronts are imported or shared)");
    auto &A = L.adj;
    auto &K = P.res.call;
    const double bytes0 = L.damped_bytes() + A.bytes();
    A.have_z = false;
    PASS(begin_resident_op(P));
    hipStream_t st = P.stream;
    for (auto &e : A.ev) if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(A.ev[0], st));
    HIPCHK(hipMemsetAsync(K.d_err.p, 0, sizeof(int), st));
    PASS(ensure_rt(P, RT_SPLIT));
    PASS(ls_ensure_int_pattern(L));                         // the plain object's int pattern of A, once
    const double *dw = w;
    if (w && !on_device) {
        if (!L.d_w.p) LCHK(L.d_w.alloc((size_t)std::max<stm_long>(am, 1)));
        if (am > 0) HIPCHK(hipMemcpyAsync(L.d_w.p, w, (size_t)am * sizeof(double), hipMemcpyHostToDevice, st));
        dw = L.d_w.p;
    }
    // the live columns among the first n, in R's column order = the leading rows of R
    std::vector<char> rd((size_t)std::max<stm_long>(n, 1), 0);
    if (n > 0) HIPCHK(hipMemcpyAsync(rd.data(), P.d_Rdead.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    stm_long r = 0;
    for (stm_long j = 0; j < n; j++) r += !rd[(size_t)j];
    const size_t nn = (size_t)std::max<stm_long>(n, 1), mm = (size_t)std::max<stm_long>(mc, 1), kk = (size_t)k;
    const size_t nbm = (size_t)std::min<stm_long>(rhs_batch_max(), k);
    PASS(stage_in(A.x, X, ldx, n, k, on_device, st));
    PASS(stage_in(A.xb, Xbar, ldxb, n, k, on_device, st));
    LCHK(grow(A.x, nn * kk)); LCHK(grow(A.xb, nn * kk)); LCHK(grow(A.z, nn * kk));
    LCHK(grow(A.v, (size_t)na * kk)); LCHK(grow(A.t, (size_t)na * nbm));
    LCHK(grow(A.rt, mm * kk)); LCHK(grow(A.ut, mm * kk));
    LCHK(grow(A.y, mm * nbm)); LCHK(grow(A.cz, mm * nbm)); LCHK(grow(A.res, nn * nbm)); LCHK(grow(A.dz, nn * nbm)); LCHK(grow(A.nrm, 2 * kk));
    const int *qf = P.has_qfill ? P.res.sched.d_Qfill.p : nullptr;
    double pass_ms = 0;
    // out (n x nb) = E R11^-1 R11^-T E' rhs (n x nb), both with leading dimension n
    auto normal_solve = [&](const double *rhs, double *out, int nb) -> int {
        if (r == 0 || n == 0) { HIPCHK(hipMemsetAsync(out, 0, nn * (size_t)nb * sizeof(double), st)); return 0; }
        HIPCHK(hipMemsetAsync(K.d_Xs.p, 0, (size_t)nb * (size_t)na * sizeof(double), st));
        LCHK(stm_launch_perm(rhs, qf, K.d_Xs.p, (int)n, 0, st, nb, n, na));                      // b[j] = rhs[Qfill[j]], j < n; 0 beyond
        HIPCHK(hipEventRecord(A.ev[2], st));
        PASS(rt_pass(P, nb, RT_SPLIT));                                                         // R' \ b: the first r rows of d_Xr
        HIPCHK(hipMemsetAsync(A.y.p, 0, mm * (size_t)nb * sizeof(double), st));
        PASS(copy_cols(A.y.p, mc, K.d_Xr.p, mc, r, nb, hipMemcpyDeviceToDevice, st));
        LCHK(stm_launch_perm(A.y.p, P.res.fact.d_Wmap.p, K.d_W.p, (int)mc, 0, st, nb, mc, mc));
        PASS(rsolve_vector(P, nb));                                                             // R \ [y; 0] -> d_Xs
        HIPCHK(hipEventRecord(A.ev[3], st));
        LCHK(stm_launch_perm(K.d_Xs.p, qf, out, (int)n, 1, st, nb, na, n));                     // out[Qfill[j]] = x[j], j < n
        HIPCHK(hipEventSynchronize(A.ev[3]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, A.ev[2], A.ev[3]));
        pass_ms += ms;
        return 0;
    };
    // A.res (n x nb) = xb - C'(C z); nrm non-NULL: |res|^2 and |xb|^2 per column
    auto residual = [&](const double *xb, const double *z, int nb, double *nrm) -> int {
        LCHK(stm_launch_lsa_pad((int)n, (int)na, nb, z, n, 1.0, -1, A.v.p, st));
        PASS(stmmqr_plan_spmv(&P, 0, A.v.p, std::max<stm_long>(na, 1), A.cz.p, (stm_long)mm, nb, 1));
        PASS(stmmqr_plan_spmv(&P, 1, A.cz.p, (stm_long)mm, A.t.p, std::max<stm_long>(na, 1), nb, 1));
        LCHK(stm_launch_lsa_resid((int)n, nb, xb, n, A.t.p, na, A.res.p, n, nrm, st));
        return 0;
    };
    int steps = 0;
    PASS(for_each_batch(P, k, [&](stm_long j0, int nb) -> int {
        const double *xb = A.xb.p + j0 * n;
        double *z = A.z.p + j0 * n;
        PASS(normal_solve(xb, z, nb));
        for (int it = 0; it < refine; it++) {
            PASS(residual(xb, z, nb, nullptr));
            PASS(normal_solve(A.res.p, A.dz.p, nb));
            LCHK(stm_launch_add_cols((int)n, nb, A.dz.p, n, z, n, st));
            if (j0 == 0) steps++;
        }
        if (info) PASS(residual(xb, z, nb, A.nrm.p + 2 * j0));
        return 0;
    }));
    // rt = Bt - C x and ut = C z, all right-hand sides at once
    LCHK(stm_launch_lsa_pad((int)n, (int)na, (int)k, A.z.p, n, 1.0, -1, A.v.p, st));
    PASS(stmmqr_plan_spmv(&P, 0, A.v.p, std::max<stm_long>(na, 1), A.ut.p, (stm_long)mm, k, 1));
    LCHK(stm_launch_lsa_pad((int)n, (int)na, (int)k, A.x.p, n, -1.0, 0, A.v.p, st));
    PASS(stmmqr_plan_spmv(&P, 0, A.v.p, std::max<stm_long>(na, 1), A.rt.p, (stm_long)mm, k, 1));
    // ---- the gradients ----
    const hipMemcpyKind back = hipMemcpyDeviceToHost;
    if (Bbar && am > 0) {
        if (!on_device) LCHK(grow(A.o_bb, (size_t)am * kk));
        LCHK(stm_launch_lsa_bbar(am, (int)k, A.ut.p, (long long)mm, dw, on_device ? Bbar : A.o_bb.p, on_device ? ldbb : am, st));
        if (!on_device) PASS(copy_cols(Bbar, ldbb, A.o_bb.p, am, am, k, back, st));
    }
    if (wbar && am > 0) {
        if (!on_device) LCHK(grow(A.o_wb, (size_t)am));
        LCHK(stm_launch_lsa_wbar(am, (int)k, A.rt.p, A.ut.p, (long long)mm, dw, on_device ? wbar : A.o_wb.p, st));
        if (!on_device) HIPCHK(hipMemcpyAsync(wbar, A.o_wb.p, (size_t)am * sizeof(double), back, st));
    }
    double *gA = (Axbar && aanz > 0) ? Axbar : nullptr, *gD = (Dbar && n > 0) ? Dbar : nullptr;
    if (gA || gD) {
        const double *x = A.x.p, *z = A.z.p, *rt = A.rt.p, *ut = A.ut.p;
        long long si = 1, sk_r = (long long)mm, sk_c = (long long)n;
        if (k > 1) {                                        // the four vectors k-fastest
            LCHK(grow(A.xT, nn * kk)); LCHK(grow(A.zT, nn * kk)); LCHK(grow(A.rtT, mm * kk)); LCHK(grow(A.utT, mm * kk));
            LCHK(stm_launch_lsa_kfast(n, (int)k, x, n, A.xT.p, st));
            LCHK(stm_launch_lsa_kfast(n, (int)k, z, n, A.zT.p, st));
            LCHK(stm_launch_lsa_kfast(mc, (int)k, rt, (long long)mm, A.rtT.p, st));
            LCHK(stm_launch_lsa_kfast(mc, (int)k, ut, (long long)mm, A.utT.p, st));
            x = A.xT.p; z = A.zT.p; rt = A.rtT.p; ut = A.utT.p;
            si = k; sk_r = sk_c = 1;
        }
        if (gA && !on_device) { LCHK(grow(A.o_ax, (size_t)aanz)); gA = A.o_ax.p; }
        if (gD && !on_device) { LCHK(grow(A.o_db, nn)); gD = A.o_db.p; }
        LCHK(stm_launch_lsa_entries(aanz, (int)n, am, (int)k, L.d_ap.p, L.d_ai.p, rt, ut, si, sk_r, x, z, si, sk_c, dw, gA, gD, st));
        if (gA && !on_device) HIPCHK(hipMemcpyAsync(Axbar, gA, (size_t)aanz * sizeof(double), back, st));
        if (gD && !on_device) HIPCHK(hipMemcpyAsync(Dbar, gD, (size_t)n * sizeof(double), back, st));
    }
    std::vector<double> nr(2 * kk, 0.0);
    if (info) HIPCHK(hipMemcpyAsync(nr.data(), A.nrm.p, nr.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(A.ev[1], st));
    PASS(end_resident_op(P));
    A.have_z = true;
    if (info) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, A.ev[0], A.ev[1]));
        double worst = 0;
        for (size_t j = 0; j < kk; j++)
            if (nr[2 * j + 1] > 0) worst = std::max(worst, std::sqrt(nr[2 * j] / nr[2 * j + 1]));
        info[0] = (double)r; info[1] = (double)steps; info[2] = worst; info[3] = ms; info[4] = pass_ms;
        info[5] = L.damped_bytes() + A.bytes() - bytes0; info[6] = info[7] = 0;
    }
    return 0;
}

int stmmqr_ls_adjoint(stmmqr_ls *ls, const double *X, stm_long ldx, const double *Xbar, stm_long ldxb, const double *w, int refine,
                      double *Axbar, double *Bbar, stm_long ldbb, double *wbar, double *Dbar, int on_device, double *info)
{
    try {
        return ls_adjoint_impl(ls, X, ldx, Xbar, ldxb, w, refine, Axbar, Bbar, ldbb, wbar, Dbar, on_device, info);
    } catch (const std::bad_alloc &) {
        return stm_fail(STMMQR_ERR_OUT_OF_MEMORY, "stmmqr_ls_adjoint: out of memory");
    }
}

// the z = (C'C)^-1 xbar of the last stmmqr_ls_adjoint call, which the object keeps (what lambdabar is made of)
int stmmqr_ls_adjoint_z(stmmqr_ls *ls, double *Z, stm_long ldz, int on_device)
{
    if (!ls || !ls->plan || !ls->adj.have_z) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_adjoint_z: no adjoint call yet on this object");
    if (!Z || ldz < ls->n) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_adjoint_z: Z is NULL or ldz < n");
    HIPCHK(hipSetDevice(ls->plan->device));
    return stage_out(ls->adj.z, Z, ldz, ls->n, ls->nrhs, on_device, ls->plan->stream);
}

int stmmqr_ls_dims(const stmmqr_ls *ls, stm_long *dims)
{
    if (!ls || !dims) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_dims: null argument");
    dims[0] = ls->damped ? ls->am : ls->m; dims[1] = ls->n; dims[2] = ls->nrhs; dims[3] = ls->damped ? 1 : 0;
    return 0;
}

int stmmqr_ls_damped_info(const stmmqr_ls *ls, double *info)
{
    if (!ls || !info) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_damped_info: null argument");
    if (!ls->damped) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_damped_info: a plain object (stmmqr_ls_create)");
    info[0] = ls->build_ms; info[1] = ls->damped_bytes();
    return 0;
}

const stm_qr_symbolic *stmmqr_ls_symbolic_view(const stmmqr_ls *ls) { return (ls && ls->sym) ? stmmqr_analysis_symbolic(ls->sym) : nullptr; }
stmmqr_plan *stmmqr_ls_plan(stmmqr_ls *ls) { return ls ? ls->plan : nullptr; }

int stmmqr_ls_info(const stmmqr_ls *ls, double *info)
{
    if (!ls || !info) return stm_fail(STMMQR_ERR_INVALID, "stmmqr_ls_info: null argument");
    const stm_qr_symbolic *S = stmmqr_analysis_symbolic(ls->sym);
    info[0] = (double)ls->rank1; info[1] = (double)S->nf; info[2] = ls->stats.flops; info[3] = ls->sym_info[0];
    info[4] = ls->stats.ms_total; info[5] = ls->solve_ms; info[6] = ls->stats.device_bytes + (double)ls->d_val.n * sizeof(double) + ls->damped_bytes() + ls->adj.bytes() + ls->rob.bytes();
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
