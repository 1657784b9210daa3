// stmmqr_leverage.hip -- leverages and single entries of ((A E)_live' (A E)_live)^-1 from the blocks of the selected inverse while
// they are resident (stmmqr_plan_leverage, stmmqr_plan_covariance_entries; the blocks: stmmqr_selinv.hip).
// After the level loop of the selected inversion the block Z_f of every front holds Z(j, k) for every pivot j of f and every column
// k of f.  A row of A makes its columns a clique of A'A and the symbolic analysis is that of A(:,Q)'A(:,Q), so for any two columns
// of one row the later one (R's order) is a column of the front where the earlier one is pivotal:
//     h_i = a_i' Z a_i = sum_{a, b in row i} a_ia a_ib Z(col_a, col_b)
// reads nothing but those blocks.
//   si_entry       Z(k1, k2) for two columns in R's order: the front of the earlier one, the local column of the later one (its own
//                  pivots: an offset; the others: a binary search of the front's ascending Rj), the position table, the block
//   k_si_leverage  one wave per row of the caller's matrix, four rows per workgroup.  For every entry a of the row (wave-uniform)
//                  the lanes stride over the entries b >= a; an off-diagonal pair counts twice.  A row need not be sorted and may
//                  name a column twice (the pair sum expands the square).  Rows are read from S = A(P,Q), the plan's row form.
//                  The cost is nnz(row)^2 lookups on ONE wave: a matrix with a dense row of tens of thousands of entries is slow
//                  here (splitting such rows over waves is not done).
//   k_si_entries   one thread per pair, the pair resolved to (front, local column, local column) on the host
// Every row's sum has a fixed order (the lane's own entries in order, then wave_sum) that depends on the row and its fronts alone:
// the same bits whatever shares the launch, no atomics on data, no LDS.
// New kernels beside stmmqr_selinv.hip's and stmmqr_resident.hip's (no kernel there changes).
#include "stmmqr_kdev.h"

// the block entry of local columns l1, l2 of front f (l1 a pivot of the view); a dead pivot or a column that was cut: 0
__device__ __forceinline__ double si_entry_at(const DevCtx &c, const SiView &v, int f, int l1, int l2)
{
    const int rp = c.fs[f].rp;
    const int p1 = v.Pos[rp + l1], p2 = v.Pos[rp + l2];
    if (p1 < 0 || p2 < 0) return 0.0;
    const SiDesc *d = v.sd + f;
    return v.Z[d->zoff + p1 + (long long)p2 * (d->rmax + d->cn)];
}

// Z(ka, kb), ka, kb < ncol in R's column order, in either order.  A pair outside the pattern (cannot happen for two columns of
// one row) raises *err = 2 and counts as 0.
__device__ __forceinline__ double si_entry(const DevCtx &c, const SiView &v, int ka, int kb, int *err)
{
    const int k1 = min(ka, kb), k2 = max(ka, kb);
    const int f = v.colfront[k1];
    const FrontSym *s = c.fs + f;
    const int col1 = s->col1, fp = s->fp;             // (the front's own pivots, not the view's: Rj lists them first)
    int l2 = k2 - col1;
    if (l2 >= fp) {
        const int *rj = v.Rj + s->rp + fp;
        const int cn = v.sd[f].cn;
        int lo = 0, hi = cn;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rj[mid] < k2) lo = mid + 1; else hi = mid;
        }
        if (lo >= cn || rj[lo] != k2) { atomicExch(err, 2); return 0.0; }
        l2 = fp + lo;
    }
    return si_entry_at(c, v, f, k1 - col1, l2);
}

__global__ __launch_bounds__(NT) void k_si_leverage(DevCtx c, SiView v, int m, int ncol, const int *__restrict__ PLinv,
                                                    const int *__restrict__ Sp, const int *__restrict__ Sj, const double *__restrict__ Sx,
                                                    double *__restrict__ lev, int *err)
{
    const int i = blockIdx.x * NW + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= m) return;                               // (the whole wave)
    const int r = PLinv[i];
    const int p0 = Sp[r], p1 = Sp[r + 1];
    double acc = 0.0;
    for (int a = p0; a < p1; a++) {
        const int ca = Sj[a];
        if (ca >= ncol) continue;                     // (a column of B)
        const double va = Sx[a];
        for (int b = a + lane; b < p1; b += 64) {
            const int cb = Sj[b];
            if (cb >= ncol) continue;
            acc += va * (b == a ? 1.0 : 2.0) * Sx[b] * si_entry(c, v, ca, cb, err);
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) lev[i] = acc;
}

// trip[3 p ..] = (front, local column of the earlier column, local column of the later one) of pair p
__global__ __launch_bounds__(NT) void k_si_entries(DevCtx c, SiView v, int npairs, const int *__restrict__ trip, double *__restrict__ out)
{
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= npairs) return;
    out[p] = si_entry_at(c, v, trip[3 * p], trip[3 * p + 1], trip[3 * p + 2]);
}

int stm_launch_si_leverage(const DevCtx &c, const SiView &v, int m, int ncol, const int *PLinv, const int *Sp, const int *Sj,
                           const double *Sx, double *lev, int *err, hipStream_t st)
{
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_si_leverage, dim3((m + NW - 1) / NW), dim3(NT), 0, st, c, v, m, ncol, PLinv, Sp, Sj, Sx, lev, err);
    return (int)hipGetLastError();
}
int stm_launch_si_entries(const DevCtx &c, const SiView &v, int npairs, const int *trip, double *out, hipStream_t st)
{
    if (npairs <= 0) return 0;
    hipLaunchKernelGGL(k_si_entries, dim3((npairs + NT - 1) / NT), dim3(NT), 0, st, c, v, npairs, trip, out);
    return (int)hipGetLastError();
}
