// The value maps of stmmqr_sparseqr_refactorize (where every entry of Y and R1 and every singleton pivot comes from in the caller's
// storage) and the object's release hook, as a stand-alone program under AddressSanitizer / UBSan.  CPU build only; built and run by
// tests/test_refactor_cpu.py:
//   g++ -fsanitize=address,undefined csrc/{stmmqr_mmio,stmmqr_symbolic,stmmqr_colamd,stmmqr_sparseqr}.cpp tests/refactor_selftest.cpp
// For every Matrix-Market file on the command line, on the host half of SparseQR() (default tolerance, default ordering):
//   Yx == Ax[ysrc] and R1x == Ax[r1src];  counts == {nz, nnz(Y), nnz(R1), n1rows};  ysrc and r1src together are a permutation of
//   0 .. nz-1;  every |Ax[pivsrc[k]]| exceeds the tolerance;  the pointers are NULL without singletons;
// the same through a transposition (the object of A' as stmmqr_sparselq makes it: the maps then speak of A's storage), and an object
// whose ext_release hook is a counting function is freed: the hook ran once.  The device entry points are stubbed: never called.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/stmmqr_hip.h"
#include "../stm-multifrontal-qr-factorization-empowered-by-gcn_amd/csrc/stmmqr_internal.h"
#include "../stm-multifrontal-qr-factorization-empowered-by-gcn_amd/csrc/stmmqr_sparseqr.h"

extern "C" int stm_fail(int code, const char *msg) { fprintf(stderr, "[refactor_selftest] library error %d: %s\n", code, msg ? msg : ""); return code; }
// device half: not part of this build
extern "C" {
stmmqr_plan *stmmqr_plan_create(const stmmqr_symbolic_view *, int, int *st) { if (st) *st = STMMQR_ERR_DEVICE; return nullptr; }
void stmmqr_plan_destroy(stmmqr_plan *) {}
int stmmqr_factorize_device(stmmqr_plan *, const stm_long *, const stm_long *, const double *, int, double, stm_long, stmmqr_stats *) { return STMMQR_ERR_DEVICE; }
int stmmqr_plan_download(stmmqr_plan *, double *, stm_long *, char *, stm_long *, double *, stm_long *, stm_long *, stm_long *, stm_long *, stm_long *, stmmqr_stats *) { return STMMQR_ERR_DEVICE; }
int stmmqr_plan_qmult(stmmqr_plan *, int, double *, stm_long, stm_long) { return STMMQR_ERR_DEVICE; }
int stmmqr_plan_rsolve(stmmqr_plan *, int, const double *, stm_long, double *, stm_long, stm_long) { return STMMQR_ERR_DEVICE; }
}

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "[refactor_selftest] FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static int released = 0;
static void count_release(void *p) { released += (p != nullptr); }

// the identities on one object; Ax is the CALLER's array (A's storage also when the object is that of A'), Fx the values of the
// matrix the object analysed (Y without singletons)
static void check_maps(const char *what, stmmqr_qr *qr, stm_long nz, const double *Ax, const double *Fx, bool lq)
{
    stm_long cnt[4] = {-1, -1, -1, -1};
    const int *ysrc = nullptr, *r1src = nullptr, *pivsrc = nullptr;
    EXPECT(stmmqr_sparseqr_refactor_maps(qr, cnt, &ysrc, &r1src, &pivsrc) == 0, "%s", what);
    double info[12] = {0};
    stmmqr_sparseqr_info(qr, info);
    const stm_long n1rows = (stm_long)info[1], n1cols = (stm_long)info[2];
    const stm_long *Yp = nullptr, *Yi = nullptr;
    const double *Yx = nullptr;
    stmmqr_sparseqr_y(qr, &Yp, &Yi, &Yx);
    const stm_long n2 = qr->n - n1cols;
    const stm_long ny = n1cols > 0 ? Yp[n2] : nz, nr1 = n1cols > 0 ? qr->R1p[(size_t)n1rows] : 0;
    EXPECT(cnt[0] == nz && cnt[1] == ny && cnt[2] == nr1 && cnt[3] == n1rows, "%s: counts %ld %ld %ld %ld", what, (long)cnt[0], (long)cnt[1], (long)cnt[2], (long)cnt[3]);
    EXPECT(ny + nr1 == nz, "%s: Y and R1 do not hold every entry", what);
    if (n1cols == 0 && !lq) {
        EXPECT(!ysrc && !r1src && !pivsrc, "%s: maps without singletons", what);
        return;
    }
    EXPECT(ysrc != nullptr, "%s: no ysrc", what);
    if (!ysrc) return;
    std::vector<char> seen((size_t)(nz > 0 ? nz : 1), 0);
    bool same = true, perm = true, piv = true;
    for (stm_long t = 0; t < ny; t++) {
        const int p = ysrc[t];
        if (p < 0 || p >= nz || seen[(size_t)p]++) { perm = false; continue; }
        if ((n1cols > 0 ? Yx[t] : Fx[t]) != Ax[p]) same = false;
    }
    if (n1cols > 0) {
        EXPECT(r1src && pivsrc, "%s: no r1src / pivsrc", what);
        if (!r1src || !pivsrc) return;
        for (stm_long q = 0; q < nr1; q++) {
            const int p = r1src[q];
            if (p < 0 || p >= nz || seen[(size_t)p]++) { perm = false; continue; }
            if (qr->R1x[(size_t)q] != Ax[p]) same = false;
        }
        const double tol = stmmqr_sparseqr_tol(qr);
        for (stm_long k = 0; k < n1rows; k++) {
            const int p = pivsrc[k];
            if (p < 0 || p >= nz || !(std::fabs(Ax[p]) > tol) || p != r1src[qr->R1p[(size_t)k]]) piv = false;
        }
    } else {
        EXPECT(!r1src && !pivsrc, "%s: R1 maps without singletons", what);
    }
    EXPECT(same, "%s: Yx / R1x are not Ax through the maps", what);
    EXPECT(perm, "%s: ysrc and r1src are no permutation of the storage positions", what);
    EXPECT(piv, "%s: a pivot position is wrong or its value does not exceed the tolerance", what);
}

int main(int argc, char **argv)
{
    int nfiles = 0, nsing = 0;
    for (int a = 1; a < argc; a++) {
        stm_long m = 0, n = 0, nnz = 0, *Ap = nullptr, *Ai = nullptr;
        double *Ax = nullptr;
        if (stmmqr_read_matrix_market(argv[a], &m, &n, &nnz, &Ap, &Ai, &Ax) != 0) { failures++; fprintf(stderr, "cannot read %s\n", argv[a]); continue; }
        nfiles++;
        stmmqr_relax rx;
        stmmqr_relax_for_qr(n, nnz, &rx);
        stmmqr_qr *qr = nullptr;
        int e = stmmqr_sparseqr_symbolic(7, -2.0, m, n, Ap, Ai, Ax, nullptr, &rx, &qr);
        EXPECT(e == 0 && qr, "%s: symbolic half", argv[a]);
        if (!e && qr) {
            if (qr->n1cols > 0) nsing++;
            check_maps(argv[a], qr, nnz, Ax, Ax, false);
            // the release hook: once, with the pointer that was set, and never for an object without one
            const int before = released;
            qr->ext = &released; qr->ext_release = count_release;
            stmmqr_sparseqr_free(qr);
            EXPECT(released == before + 1, "%s: ext_release ran %d times", argv[a], released - before);
        }
        // the object of A', the transposition handed over as stmmqr_sparselq does: the maps speak of A's storage
        {
            std::vector<stm_long> Tp((size_t)m + 1, 0), Ti((size_t)(nnz > 0 ? nnz : 1));
            std::vector<double> Tx((size_t)(nnz > 0 ? nnz : 1));
            std::vector<int> tsrc((size_t)(nnz > 0 ? nnz : 1));
            for (stm_long p = 0; p < nnz; p++) Tp[(size_t)Ai[p] + 1]++;
            for (stm_long i = 0; i < m; i++) Tp[(size_t)i + 1] += Tp[(size_t)i];
            std::vector<stm_long> w(Tp.begin(), Tp.end() - 1);
            for (stm_long j = 0; j < n; j++)
                for (stm_long p = Ap[j]; p < Ap[j + 1]; p++) { const stm_long q = w[(size_t)Ai[p]]++; Ti[(size_t)q] = j; Tx[(size_t)q] = Ax[p]; tsrc[(size_t)q] = (int)p; }
            stmmqr_relax_for_qr(m, nnz, &rx);
            stmmqr_qr *lq = nullptr;
            e = stmmqr_sparseqr_symbolic(7, -2.0, n, m, Tp.data(), Ti.data(), Tx.data(), nullptr, &rx, &lq);
            EXPECT(e == 0 && lq, "%s: symbolic half of the transpose", argv[a]);
            if (!e && lq) {
                const int before = released;
                EXPECT(stm_sparseqr_set_transposition(lq, tsrc.data(), nnz) == 0, "%s: transposition", argv[a]);
                check_maps(argv[a], lq, nnz, Ax, Tx.data(), true);
                stmmqr_sparseqr_free(lq);
                EXPECT(released == before, "%s: a release hook ran that was never set", argv[a]);
            }
        }
        printf("%s: %ld x %ld, %ld entries\n", argv[a], (long)m, (long)n, (long)nnz);
        stmmqr_free(Ap); stmmqr_free(Ai); stmmqr_free(Ax);
    }
    EXPECT(nfiles >= 1 && nsing >= 1, "no file with singletons was checked (%d files)", nfiles);
    printf("files %d, with singletons %d\n", nfiles, nsing);
    printf("ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
