// stmmqr_internal.h -- helpers shared by the host-side translation units of libstmmqr_hip.so (not exported: the
// library's version script keeps everything but the C ABI of include/stmmqr_hip.h local).
#pragma once
#include "../../include/stmmqr_hip.h"

extern "C" {
// record the thread's last error (stmmqr_last_error) and return `code`
int stm_fail(int code, const char *msg);
// cc->status = code through the configured sparse_common layout (no-op for cc == NULL)
void stm_cc_set_status(stm_sparse_common *cc, int code);
// SparseCore_malloc / SparseCore_free semantics (src/core/SparseCore_common.c:603-655): counted in cc->malloc_count / memory_inuse
void *stm_cc_malloc(size_t n, size_t size, stm_sparse_common *cc);
void stm_cc_free(size_t n, size_t size, void *p, stm_sparse_common *cc);
// a device copy of a caller's CSC matrix for products with it (k_spmv; stmmqr_rfactor.cpp): stmmqr_sparseqr_solve_seminormal
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
}
