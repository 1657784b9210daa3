// stmmqr_lsobj.h -- the least-squares object as the host units that work on it see it (stmmqr_ls.cpp: create, solve, adjoint,
// diagnostics; stmmqr_lsrobust.cpp: the robust fits).  Local to the library.
#pragma once
#include <climits>

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
    // ---- the damped mode: m, anz, Ap, Bp, Bi above are those of [A; I] (m = rows of A + n, anz = entries of A + n), Ax holds A's own
    // values as at create, and ax_current says that d_ax (not d_val, which every solve builds anew) holds them
    bool damped = false;
    stm_long am = 0, aanz = 0;                          // rows and entries of A
    DevBuf<int> d_ap, d_ai;                             // A's column pointers and row indices, uploaded once at create
    DevBuf<long long> d_ap2;                            // the column pointers of [A; I] for k_rf_colnorm (default tolerance only)
    DevBuf<double> d_ax;                                // A's unweighted values: those of create, or a host array given to a solve
    DevBuf<double> d_D;                                 // [n] the D_jj of the last solve, A's column order
    DevBuf<double> d_head;                              // two doubles: where k_rf_colnorm leaves the largest column norm
    DevBuf<double> d_w, d_x, d_dn;                      // for host arrays (made when first needed): w, X; |D x_j| of the last solve
    hipEvent_t ev_build[2] = {nullptr, nullptr};
    double build_ms = 0;
    double damped_bytes() const
    {
        return 4.0 * (double)(d_ap.n + d_ai.n) + 8.0 * (double)(d_ap2.n + d_ax.n + d_D.n + d_head.n + d_w.n + d_x.n + d_dn.n);
    }
    // ---- the adjoint (stmmqr_ls_adjoint): made by the first call, grown on demand, never shrunk.  The plain object's int pattern of
    // A goes into d_ap / d_ai above at its first call (the damped object has it from create).
    bool last_solve_ok = false;                         // the factors and d_val belong to a solve that came to its end
    struct Adjoint {
        DevBuf<double> x, xb, z;                        // n x nrhs: the solution, its cotangent, (C'C)^-1 xbar
        DevBuf<double> v, t;                            // (n + nrhs) x nrhs: what the product with [C | Bt] takes / what its transpose gives
        DevBuf<double> rt, ut;                          // rows of C x nrhs: Bt - C x, C z
        DevBuf<double> y, cz, res, dz, nrm;             // per batch: R' \ in R's row order, C z, the refinement's residual and step; norms
        DevBuf<double> xT, zT, rtT, utT;                // the four k-fastest (nrhs > 1)
        DevBuf<double> o_ax, o_bb, o_wb, o_db;          // outputs of a call with host arrays
        bool have_z = false;                            // z belongs to a call that came to its end (stmmqr_ls_adjoint_z)
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        double bytes() const
        {
            return 8.0 * (double)(x.n + xb.n + z.n + v.n + t.n + rt.n + ut.n + y.n + cz.n + res.n + dz.n + nrm.n + xT.n + zT.n + rtT.n + utT.n +
                                  o_ax.n + o_bb.n + o_wb.n + o_db.n);
        }
    } adj;
    // ---- the robust fits (stmmqr_lsrobust.cpp): made by the first call, never shrunk
    struct Robust {
        DevBuf<int> rp, rj, rq;                         // row form of A: row pointers; by rows, the columns and the positions in A's storage
        DevBuf<double> ax;                              // the plain object: A's unweighted values (d_val holds the weighted ones)
        DevBuf<double> wax, wb;                         // the plain object: w[Ai[p]] * Ax[p] and w o b of a solve
        DevBuf<double> b, x, xprev, r, a, w, w0;        // m: b, r, a, w, w0; n: x, xprev
        DevBuf<double> part, stat, step;                // the sums' workgroup partials; the statistics [8] and the median's four; step [2]
        DevBuf<double> dd, dout, dn, res;               // host arrays of a damped call: d in, D and |D x| out; the residual norm
        DevBuf<unsigned long long> sel;                 // the selection's state and its histograms (stm_lsr_sel_words)
        bool ax_create = false;                         // ax holds the values given at create
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        double ms[4] = {0, 0, 0, 0};                    // the last reweighting: residual, selection, weights, all three
        double bytes() const
        {
            return 4.0 * (double)(rp.n + rj.n + rq.n) + 8.0 * (double)(ax.n + wax.n + wb.n + b.n + x.n + xprev.n + r.n + a.n + w.n + w0.n +
                                                                     part.n + stat.n + step.n + dd.n + dout.n + dn.n + res.n + sel.n);
        }
    } rob;
    ~stmmqr_ls()
    {
        for (auto &e : rob.ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : ev_build) if (e) (void)hipEventDestroy(e);
        for (auto &e : adj.ev) if (e) (void)hipEventDestroy(e);
        if (plan) stmmqr_plan_destroy(plan);
        if (sym) stmmqr_analysis_free(sym);
    }
};

// the plain object's int pattern of A on the device (d_ap, d_ai), once; the damped object has it from create
inline int ls_ensure_int_pattern(stmmqr_ls &L)
{
    if (L.d_ap.p) return 0;
    const stm_long n = L.n, aanz = L.anz;
    std::vector<int> ap((size_t)n + 1), ai((size_t)std::max<stm_long>(aanz, 1), 0);
    for (stm_long j = 0; j <= n; j++) ap[(size_t)j] = (int)L.Ap[(size_t)j];
    for (stm_long p = 0; p < aanz; p++) ai[(size_t)p] = (int)L.Bi[(size_t)p];
    LCHK(L.d_ap.alloc(ap.size()));
    LCHK(L.d_ai.alloc(ai.size()));
    HIPCHK(hipMemcpy(L.d_ap.p, ap.data(), ap.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.d_ai.p, ai.data(), ai.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}
