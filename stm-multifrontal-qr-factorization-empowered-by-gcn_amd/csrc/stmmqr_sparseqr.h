// stmmqr_sparseqr.h -- the SparseQR object (struct stmmqr_qr) for the translation units that work on it: stmmqr_sparseqr.cpp (host
// half, Q / R operations), stmmqr_export.cpp (LQ hands its transposition over) and stmmqr_refactor.hip (new values on the device).
// Host-only: no HIP header is needed to read it, and stmmqr_sparseqr.cpp stays buildable without the device half of the library.
// What the device side keeps for an object hangs on `ext` and is released through `ext_release`, which the destructor calls when
// set: the destructor itself never touches a device.
#pragma once
#include <algorithm>
#include <cfloat>
#include <vector>

#include "../../include/stmmqr_hip.h"

struct stmmqr_qr {
    typedef stm_long Long;
    Long m = 0, n = 0, n1rows = 0, n1cols = 0, rank = 0;
    double tol = 0;
    int ordering_used = 0;
    std::vector<Long> Q1fill, P1inv, HP1inv, R1p, R1j;        // P1inv / HP1inv / R1*: only when n1cols > 0
    std::vector<double> R1x;
    std::vector<Long> Yp, Yi;                                 // the matrix handed to the numeric phase when singletons exist
    std::vector<double> Yx;
    stmmqr_analysis *sym = nullptr;
    stmmqr_plan *plan = nullptr;
    stmmqr_stats stats = {};
    int keep_h = 1;                                           // stmmqr_sparseqr_set_keep_h: 0 = R only (no Q-apply)
    std::vector<char> Rdead;                                  // of the multifrontal part (n - n1cols)
    double ana_seconds = 0, fac_seconds = 0, sym_info[8] = {};
    const Long *Fp = nullptr, *Fi = nullptr;                  // what the numeric phase factorizes (A or Y)
    const double *Fx = nullptr;
    // ---- new values of the same pattern (stmmqr_sparseqr_refactorize) ----
    double tol_arg = 0;                                       // the `tol` argument the object was made with: its rule is applied again
    Long nz = 0;                                              // entries of the caller's matrix
    std::vector<Long> Ap0;                                    // column pointers of the matrix analysed (A, or A' for an LQ object)
    // Where the values come from, as positions in the CALLER's storage (A's own order also for an LQ object): entry t of Y, entry q
    // of R1's row form, the pivot of live singleton row k.  Built with singletons or for an LQ object (then have_maps); otherwise Y
    // is A itself.  Not built for nz >= 2^31 (maps_too_large): the tables are int, as the library's other index tables are.
    std::vector<int> ysrc, r1src, pivsrc, tsrc;               // tsrc: LQ only, storage position in A of entry q of A'
    bool have_maps = false, maps_too_large = false, is_lq = false;
    int valid = 1;                                            // 0: a refactorization failed after the old factors were given up
    int device = -1;                                          // what the numeric phase was asked for
    double rf_info[8] = {};                                   // stmmqr_sparseqr_refactor_info
    void *ext = nullptr;                                      // device side of the refactorization (stmmqr_refactor.hip)
    void (*ext_release)(void *) = nullptr;
    ~stmmqr_qr()
    {
        if (ext && ext_release) ext_release(ext);
        if (plan) stmmqr_plan_destroy(plan);
        if (sym) stmmqr_analysis_free(sym);
    }
};

// QR_DEFAULT_TOL from the largest column norm, evaluated left to right: the one expression of stm_qr_default_tol and of the
// refactorization, which gets the norm from the device
inline double stm_qr_tol_of_maxnorm(stm_long m, stm_long n, double mx) { return std::min(20.0 * ((double)m + (double)n) * DBL_EPSILON * mx, DBL_MAX); }

extern "C" {
// stmmqr_sparselq hands over its transposition (tsrc[q] = position in A of entry q of A', nz entries; NULL: nz >= 2^31): the maps of the object are
// composed with it, so that new values come in A's own order.  Before or after the numeric phase.
int stm_sparseqr_set_transposition(stmmqr_qr *qr, const int *tsrc, stm_long nz);
// what stmmqr_sparseqr_refactorize does after the factorization of the new values, as numeric_impl after its own: Rdead, HPinv,
// the scalars; rank and HP1inv rebuilt
int stm_sparseqr_after_factorization(stmmqr_qr *qr);
}
