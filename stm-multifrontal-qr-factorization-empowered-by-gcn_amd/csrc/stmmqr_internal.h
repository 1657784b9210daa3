// stmmqr_internal.h -- helpers shared by the host-side translation units of libstmmqr_hip.so (not exported: the
// library's version script keeps everything but the C ABI of include/stmmqr_hip.h local).
#pragma once
#include "../../include/stmmqr_hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

extern "C" {
// record the thread's last error (stmmqr_last_error) and return `code`
int stm_fail(int code, const char *msg);
// cc->status = code through the configured sparse_common layout (no-op for cc == NULL)
void stm_cc_set_status(stm_sparse_common *cc, int code);
// SparseCore_malloc / SparseCore_free semantics (src/core/SparseCore_common.c:603-655): counted in cc->malloc_count / memory_inuse
void *stm_cc_malloc(size_t n, size_t size, stm_sparse_common *cc);
void stm_cc_free(size_t n, size_t size, void *p, stm_sparse_common *cc);
// a device copy of a caller's CSC matrix for products with it (k_spmv; stmmqr_seminormal.cpp): stmmqr_sparseqr_solve_seminormal
typedef struct stm_aop stm_aop;
int stm_aop_create(int device, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax, stm_aop **out);
void stm_aop_destroy(stm_aop *op);
// host arrays: Y = A X (trans 0), A' X (trans 1), or with B (trans 0) Y = B - A X
int stm_aop_apply(stm_aop *op, int trans, const double *X, stm_long ldx, const double *B, stm_long ldb, double *Y, stm_long ldy,
                  stm_long nrhs);
// QR_DEFAULT_TOL of a matrix, and the column order stmmqr_sparseqr gives it (Q: [n]; orderings and refusals as stmmqr_sparseqr)
double stm_qr_default_tol(stm_long m, stm_long n, const stm_long *Ap, const double *Ax);
int stm_sparseqr_order(int ordering, double tol, stm_long m, stm_long n, const stm_long *Ap, const stm_long *Ai, const double *Ax,
                       const stm_long *Quser, stm_long *Q);
// m, n of a factorized SparseQR object (stmmqr_sparseqr.cpp)
int stm_sparseqr_dims(const stmmqr_qr *qr, stm_long *m, stm_long *n);
// stmmqr_sparseqr_min2norm with the plan's solve handed in (stmmqr_plan_solve_minnorm): the singleton stages around it (stmmqr_sparseqr.cpp)
typedef int (*stm_minnorm_fn)(stmmqr_plan *, const double *, stm_long, double *, stm_long, stm_long, int, int);
int stm_sparseqr_min2norm(stmmqr_qr *qr, const double *B, stm_long ldb, stm_long nrhs, double *X, stm_long ldx, stm_minnorm_fn solve);
}

// Row form of a sparse matrix from its nz entries in storage order (row[p], col[p]): rp [m + 1], and row by row the entries' columns
// rj and storage positions rq.  A stable counting sort: within a row the entries keep their storage order, which fixes the order
// in which k_spmv sums a row of A x.
inline void stm_row_form(long m, long nz, const int *row, const int *col, std::vector<int> &rp, std::vector<int> &rj, std::vector<int> &rq)
{
    rp.assign((size_t)m + 1, 0);
    rj.assign((size_t)std::max(1L, nz), 0); rq.assign((size_t)std::max(1L, nz), 0);
    for (long p = 0; p < nz; p++) rp[(size_t)row[p] + 1]++;
    for (long i = 0; i < m; i++) rp[(size_t)i + 1] += rp[(size_t)i];
    std::vector<int> next(rp.begin(), rp.end() - 1);
    for (long p = 0; p < nz; p++) {
        const int q = next[(size_t)row[p]]++;
        rj[(size_t)q] = col[p]; rq[(size_t)q] = (int)p;
    }
}

// What the seminormal solves report: max over the right-hand sides of |A'r| / (|A|_F (|A|_F |x| + |b|)), from |A|_F = af and the
// SQUARED norms zz = |A'r|^2, xx = |x|^2, bb = |b|^2 per right-hand side (0 / 0 counts as 0, q / 0 as infinity)
inline double stm_seminormal_info(double af, const double *zz, const double *xx, const double *bb, long nrhs)
{
    double worst = 0;
    for (long j = 0; j < nrhs; j++) {
        const double den = af * (af * std::sqrt(xx[j]) + std::sqrt(bb[j])), q = std::sqrt(zz[j]);
        worst = std::max(worst, den > 0 ? q / den : (q > 0 ? INFINITY : 0.0));
    }
    return worst;
}
