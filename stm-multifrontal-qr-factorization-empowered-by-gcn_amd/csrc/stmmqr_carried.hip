// stmmqr_carried.hip -- least squares with the right-hand sides carried through the factorization (stmmqr_plan_solve_carried):
// the plan holds the R of [A B] (ntol = n: the B columns are never rank-tested), so C = Q'B sits in the last columns of R and
// x = E R11^-1 C needs no Q.  The back substitution itself is the resident-factor one (k_rsolve / k_rbig_*, stmmqr_resident.hip)
// run on a VIEW of the factorization that ends at column n: the fronts that hold B columns as pivots get fp cut back to their A
// pivots, so the B columns are "other columns" of every front, whose x the kernels read from the solution vector.  With
// x(n + j) = -1 for right-hand side j (0 for the others) and y = 0 the kernels' y - R12 x IS C(:, j) minus the A part -- no
// gather pass over the factors, no division by a diagonal entry of the B block.
//   k_carried_view   per front with B pivots: its live A pivots -> FrontNum::rank of the view; the 2-norms of the B columns
//                    below those rows (the residual norms: the triangle under C)
//   k_carried_seed   x(n + j0 + r) = -1 in vector r of a batch
// New kernels beside stmmqr_resident.hip's (no kernel there changes).
#include "stmmqr_kdev.h"

// One workgroup per front of `flist` (fronts whose pivotal columns reach beyond column n).  c: the TRUE fronts (front form).
// Column k of the front is live when HStair[k] != 0 and a row is left for its diagonal (the rule of k_rsolve / k_r_count); the R
// part of pivotal column k is rows 0 .. rm(k)-1, rm(k) = min(fm, live pivots among 0..k).  Rows 0 .. ra-1 (ra = live A pivots)
// belong to R11 | C; what a B column keeps below them is its part of the residual: resid[j] = |R(ra .. rm(k)-1, k)|_2.  Every B
// column is pivotal in exactly one front, so every resid[j] has one writer (columns without such rows keep the caller's 0).
__global__ __launch_bounds__(NT) void k_carried_view(DevCtx c, const int *__restrict__ flist, int n, FrontNum *__restrict__ view,
                                                     double *__restrict__ resid)
{
    __shared__ int s_scan[NW];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fm = c.fnum[f].fm, tid = threadIdx.x;
    const int fpa = min(s.fp, max(0, n - s.col1));            // pivotal columns of A
    const int *St = c.Stair + s.rp;
    int cnt = 0;
    for (int k = tid; k < fpa; k += NT) cnt += (St[k] != 0);
    int total;
    (void)block_incl_scan(cnt, s_scan, &total);
    const int ra = max(0, min(total, fm));
    if (tid == 0) view[f].rank = ra;
    const double *F = c.Farena + s.foff;
    for (int k = fpa + tid; k < s.fp; k += NT) {
        int q = total;
        for (int kk = fpa; kk <= k; kk++) q += (St[kk] != 0);
        const int rmk = min(fm, q);
        const double *col = F + (long long)k * s.ld;
        double ss = 0.0;
        for (int i = ra; i < rmk; i++) ss = fma(col[i], col[i], ss);
        resid[s.col1 + k - n] = sqrt(ss);
    }
}

// X: nb solution vectors at stride ldx (zeroed by the caller); vector r solves for right-hand side j0 + r
__global__ __launch_bounds__(64) void k_carried_seed(double *__restrict__ X, long long ldx, int n, int j0, int nb)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r < nb) X[(long long)r * ldx + n + j0 + r] = -1.0;
}

int stm_launch_carried_view(const DevCtx &c, const int *flist, int nfr, int n, FrontNum *view, double *resid, hipStream_t st)
{
    if (nfr <= 0) return 0;
    hipLaunchKernelGGL(k_carried_view, dim3(nfr), dim3(NT), 0, st, c, flist, n, view, resid);
    return (int)hipGetLastError();
}
int stm_launch_carried_seed(double *X, long long ldx, int n, int j0, int nb, hipStream_t st)
{
    if (nb <= 0) return 0;
    hipLaunchKernelGGL(k_carried_seed, dim3((nb + 63) / 64), dim3(64), 0, st, X, ldx, n, j0, nb);
    return (int)hipGetLastError();
}
