// stmmqr_rmult.hip -- products with R and R' on the factors resident in HBM (stmmqr_plan_rmult) and the small reductions of the
// condition estimate (stmmqr_plan_condest).  R is the whole rank x n factor, dead pivot columns included: row q of a front is its
// q-th live pivot column lc[q] (HStair != 0 and a row left, the rule of k_rsolve / k_rbig_*), and holds the front's columns
// k >= lc[q] -- later live pivots, dead pivots (which keep the R rows above them), then the non-pivotal columns.  Global row of
// R: rowbase[f] + q.  Every sum below has a fixed order that depends on the front alone: a batch gives the bits of its vectors
// one by one, whatever the launch geometry.
#include "stmmqr_kdev.h"

#define RM_NT 256                 // threads of the product kernels (block_incl_scan: NT)
#define RM_ROWS STM_RM_ROWS       // R x: rows (= threads) of a workgroup
#define RM_XC STM_RM_XC           // R x: entries of x[Rj[k]] staged in LDS per pass
#define RM_COLS STM_RM_COLS       // R' y: columns of a workgroup, a half-wave per column
static_assert(RM_NT == NT && RM_ROWS == RM_NT, "one row per thread, the 256-thread scan");
static_assert(RM_COLS % (RM_NT / 32) == 0, "every half-wave takes the same number of columns");

// ------------------------------------------------------------------------------------------------
// Y = R X.  The rows of a front depend on x alone, so a tree level is one launch: workgroup (front, slab) owns RM_ROWS rows, a
// row per thread -- consecutive threads read consecutive rows of a column (whole 256-byte segments).  x[Rj[k]] of the front's
// columns goes through LDS in chunks of RM_XC; a row walks the columns in column order from its own diagonal, one running sum.
// R vectors of a batch per workgroup (template): R is read once for all of them, per vector the arithmetic is that of R = 1.
// ------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(RM_NT) void k_rmult(DevCtx c, const int *__restrict__ flist, const int *__restrict__ Rj,
                                                 const int *__restrict__ rowbase, const double *X, double *Y, RhsBatch B, int nb)
{
    const int nr = min(R, nb - (int)blockIdx.z * R);
    X += (long long)blockIdx.z * R * B.x; Y += (long long)blockIdx.z * R * B.w;
    __shared__ int s_scan[NW];
    __shared__ int s_lc[RM_ROWS];
    __shared__ double s_x[R][RM_XC];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fp = s.fp, fn = s.fn, fm = c.fnum[f].fm;
    const int i0 = (int)blockIdx.y * RM_ROWS, tid = threadIdx.x;
    if (fp <= 0 || i0 >= min(fp, fm)) return;           // (uniform: no row of R in this slab)
    const int *St = c.Stair + s.rp;
    int rm;
    {
        const int per = (fp + RM_NT - 1) / RM_NT;
        const int k0 = min(fp, tid * per), k1 = min(fp, k0 + per);
        int cnt = 0;
        for (int k = k0; k < k1; k++) cnt += (St[k] != 0);
        int total;
        const int incl = block_incl_scan(cnt, s_scan, &total);
        int q = incl - cnt;
        for (int k = k0; k < k1; k++) {
            if (St[k] == 0) continue;
            if (q >= i0 && q < i0 + RM_ROWS && q < fm) s_lc[q - i0] = k;
            q++;
        }
        rm = min(total, fm);
    }
    __syncthreads();
    if (i0 >= rm) return;
    const int i = i0 + tid, ic = min(i, rm - 1);
    const int mylc = s_lc[ic - i0], kbeg = s_lc[0];
    const int *rj = Rj + s.rp;
    const double *F = c.Farena + s.foff;
    const long long ld = s.ld;
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    for (int kc = kbeg; kc < fn; kc += RM_XC) {
        const int len = min(RM_XC, fn - kc);
        __syncthreads();                                // (the previous chunk is done with)
        for (int e = tid; e < len; e += RM_NT) {
            const int j = rj[kc + e];
#pragma unroll
            for (int r = 0; r < R; r++) s_x[r][e] = (r < nr) ? X[(long long)r * B.x + j] : 0.0;
        }
        __syncthreads();
        const double *Fp = F + ic + (long long)kc * ld;
        int kk = 0;
        for (; kk + 8 <= len; kk += 8) {                // (eight loads in flight; the sums stay in column order)
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = Fp[(long long)(kk + u) * ld];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const bool on = kc + kk + u >= mylc;    // (below the diagonal: the reflectors, not R)
#pragma unroll
                for (int r = 0; r < R; r++) acc[r] = on ? fma(v[u], s_x[r][kk + u], acc[r]) : acc[r];
            }
        }
        for (; kk < len; kk++) {
            const double v = Fp[(long long)kk * ld];
            const bool on = kc + kk >= mylc;
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = on ? fma(v, s_x[r][kk], acc[r]) : acc[r];
        }
    }
    if (i < rm) {
#pragma unroll
        for (int r = 0; r < R; r++)
            if (r < nr) Y[(long long)r * B.w + rowbase[f] + i] = acc[r];
    }
}

// Y = R X with every row's sum carried in two doubles (a product's rounding error by fma, the sums by the error-free two-sum;
// contraction is switched off there): the result is the rounded EXACT row sum up to eps^2 sum |r_ik x_k|, which
// is what the refinement of the null-space basis needs of a residual that cancels to eps cond(R) of its terms.  k_rmult<1>'s rows, column
// order and masks; vector blockIdx.z of a batch.
__device__ __forceinline__ void dd_add_product(double v, double x, double &hi, double &lo)
{
#pragma clang fp contract(off)    // (p must stay a rounded product: fused into the sums below, its error e would be counted twice)
    const double p = v * x, e = __builtin_fma(v, x, -p);
    const double s = hi + p, bb = s - hi;
    const double err = (hi - (s - bb)) + (p - bb);
    hi = s;
    lo = lo + (err + e);
}
__global__ __launch_bounds__(RM_NT) void k_rmult_dd(DevCtx c, const int *__restrict__ flist, const int *__restrict__ Rj,
                                                    const int *__restrict__ rowbase, const double *X, double *Y, RhsBatch B)
{
    X += (long long)blockIdx.z * B.x; Y += (long long)blockIdx.z * B.w;
    __shared__ int s_scan[NW];
    __shared__ int s_lc[RM_ROWS];
    __shared__ double s_x[RM_XC];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fp = s.fp, fn = s.fn, fm = c.fnum[f].fm;
    const int i0 = (int)blockIdx.y * RM_ROWS, tid = threadIdx.x;
    if (fp <= 0 || i0 >= min(fp, fm)) return;           // (uniform: no row of R in this slab)
    const int *St = c.Stair + s.rp;
    int rm;
    {
        const int per = (fp + RM_NT - 1) / RM_NT;
        const int k0 = min(fp, tid * per), k1 = min(fp, k0 + per);
        int cnt = 0;
        for (int k = k0; k < k1; k++) cnt += (St[k] != 0);
        int total;
        const int incl = block_incl_scan(cnt, s_scan, &total);
        int q = incl - cnt;
        for (int k = k0; k < k1; k++) {
            if (St[k] == 0) continue;
            if (q >= i0 && q < i0 + RM_ROWS && q < fm) s_lc[q - i0] = k;
            q++;
        }
        rm = min(total, fm);
    }
    __syncthreads();
    if (i0 >= rm) return;
    const int i = i0 + tid, ic = min(i, rm - 1);
    const int mylc = s_lc[ic - i0], kbeg = s_lc[0];
    const int *rj = Rj + s.rp;
    const double *F = c.Farena + s.foff;
    const long long ld = s.ld;
    double hi = 0.0, lo = 0.0;
    for (int kc = kbeg; kc < fn; kc += RM_XC) {
        const int len = min(RM_XC, fn - kc);
        __syncthreads();                                // (the previous chunk is done with)
        for (int e = tid; e < len; e += RM_NT) s_x[e] = X[rj[kc + e]];
        __syncthreads();
        const double *Fp = F + ic + (long long)kc * ld;
        for (int kk = 0; kk < len; kk++)
            if (kc + kk >= mylc) dd_add_product(Fp[(long long)kk * ld], s_x[kk], hi, lo);
    }
    if (i < rm) Y[rowbase[f] + i] = hi + lo;
}

// ------------------------------------------------------------------------------------------------
// Z = R' Y scatters into columns that several fronts share: two kernels, no atomics.  k_rtmult_dots: every front writes the dot of
// its column k with its rows of y into its own slot U[Rp[f] + k] (the pass-vector array of the R' solve: one writer per slot).  A
// half-wave per column, lanes along the rows (a column of R is contiguous: the access shape of k_rtbig_step); a lane adds its rows
// in order, the lanes are added by a fixed butterfly.  Column k < fp holds the rows of the live pivots up to k, a non-pivotal
// column all rm rows.  ABS: |R| and y = 1 -- the column 1-norms.  k_rtmult_gather: z[j] = its slots in increasing slot order,
// through the transpose of Rj (cp: n + 1 offsets, slot: rjsize slots, built on the host).
// ------------------------------------------------------------------------------------------------
template <int R, bool ABS>
__global__ __launch_bounds__(RM_NT) void k_rtmult_dots(DevCtx c, const int *__restrict__ flist, const int *__restrict__ rowbase,
                                                       const double *Yv, double *U, RhsBatch B, int nb)
{
    const int nr = min(R, nb - (int)blockIdx.z * R);
    Yv += (long long)blockIdx.z * R * B.w; U += (long long)blockIdx.z * R * B.u;
    __shared__ int s_scan[NW];
    __shared__ int s_cnt[RM_COLS];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fp = s.fp, fn = s.fn, fm = max(c.fnum[f].fm, 0);
    const int c0 = (int)blockIdx.y * RM_COLS, tid = threadIdx.x;
    if (c0 >= fn) return;                               // (uniform)
    const int *St = c.Stair + s.rp;
    int rm;
    {
        const int per = (fp + RM_NT - 1) / RM_NT;
        const int k0 = min(fp, tid * per), k1 = min(fp, k0 + per);
        int cnt = 0;
        for (int k = k0; k < k1; k++) cnt += (St[k] != 0);
        int total;
        const int incl = block_incl_scan(cnt, s_scan, &total);
        int q = incl - cnt;
        for (int k = k0; k < k1; k++) {
            q += (St[k] != 0);
            if (k >= c0 && k < c0 + RM_COLS) s_cnt[k - c0] = min(q, fm);    // rows of R in column k: the live pivots up to k
        }
        rm = min(total, fm);
    }
    __syncthreads();
    const int lane32 = tid & 31, grp = tid >> 5;
    constexpr int NG = RM_NT / 32;
    const double *F = c.Farena + s.foff;
    const long long ld = s.ld;
    const double *y = Yv + rowbase[f];
    const long long ys = (nr > 1) ? B.w : 0;            // (vectors beyond the batch read the first one's y: never stored)
    for (int cc = grp; cc < RM_COLS; cc += NG) {
        const int k = c0 + cc;
        const int cnt = (k < fn) ? ((k < fp) ? s_cnt[cc] : rm) : 0;
        const double *col = F + (long long)min(k, fn - 1) * ld;
        double a[R];
#pragma unroll
        for (int r = 0; r < R; r++) a[r] = 0.0;
        int q = lane32;
        for (; q + 96 < cnt; q += 128) {                // (four loads in flight; a lane's rows are added in order)
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = col[q + 32 * u];
#pragma unroll
            for (int u = 0; u < 4; u++) {
#pragma unroll
                for (int r = 0; r < R; r++) a[r] = ABS ? a[r] + fabs(v[u]) : fma(v[u], y[(r < nr ? r : 0) * ys + q + 32 * u], a[r]);
            }
        }
        for (; q < cnt; q += 32) {
            const double v = col[q];
#pragma unroll
            for (int r = 0; r < R; r++) a[r] = ABS ? a[r] + fabs(v) : fma(v, y[(r < nr ? r : 0) * ys + q], a[r]);
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) a[r] += __shfl_xor(a[r], o, 64);
        }
        if (lane32 == 0 && k < fn) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r < nr) U[(long long)r * B.u + s.rp + k] = a[r];
        }
    }
}
__global__ __launch_bounds__(256) void k_rtmult_gather(const int *__restrict__ cp, const int *__restrict__ slot, const double *U, double *Z,
                                                       int n, long long su, long long sz)
{
    U += (long long)blockIdx.y * su; Z += (long long)blockIdx.y * sz;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double z = 0.0;
    for (int p = cp[j]; p < cp[j + 1]; p++) z += U[slot[p]];
    Z[j] = z;
}

// ------------------------------------------------------------------------------------------------
// The condition estimate's reductions: one workgroup, a thread adds its entries i = tid, tid + CE_NT, ... in order, the threads
// are combined by a fixed tree in LDS.  idx: the live pivot columns (entry i of the r-vector is a[idx[i]]), or nullptr: a[i].
//   what 0: sum |a_i|      1: sum a_i^2      2: max a_i      -> out[0]
//   what 3: max |a_i| -> out[1], the first i that attains it -> out[2], sum a_i b_i -> out[3]
// ------------------------------------------------------------------------------------------------
#define CE_NT 1024
__global__ __launch_bounds__(CE_NT) void k_ce_reduce(int what, const double *__restrict__ a, const int *__restrict__ idx,
                                                     const double *__restrict__ b, int r, double *out)
{
    __shared__ double s_v[CE_NT], s_d[CE_NT];
    __shared__ int s_j[CE_NT];
    const int tid = threadIdx.x;
    double v = 0.0, d = 0.0;
    int j = 0x7fffffff;
    for (int i = tid; i < r; i += CE_NT) {
        const double x = a[idx ? idx[i] : i];
        if (what == 0) v += fabs(x);
        else if (what == 1) v = fma(x, x, v);
        else if (what == 2) v = (i == tid) ? x : fmax(v, x);
        else {
            if (fabs(x) > v || i == tid) { v = fabs(x); j = i; }     // (strictly larger: the lowest index wins a tie)
            d = fma(x, b[i], d);
        }
    }
    if (what == 2 && tid >= r) v = -INFINITY;
    s_v[tid] = v; s_d[tid] = d; s_j[tid] = j;
    __syncthreads();
    for (int h = CE_NT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            if (what <= 1) s_v[tid] += s_v[tid + h];
            else if (what == 2) s_v[tid] = fmax(s_v[tid], s_v[tid + h]);
            else {
                const double v2 = s_v[tid + h];
                const int j2 = s_j[tid + h];
                if (j2 != 0x7fffffff && (s_j[tid] == 0x7fffffff || v2 > s_v[tid] || (v2 == s_v[tid] && j2 < s_j[tid]))) { s_v[tid] = v2; s_j[tid] = j2; }
                s_d[tid] += s_d[tid + h];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (what <= 2) out[0] = s_v[0];
        else { out[1] = s_v[0]; out[2] = (double)s_j[0]; out[3] = s_d[0]; }
    }
}
// elementwise, over the r live pivot columns idx:
//   what 0: a[idx[i]] = sign(a[idx[i]]), y >= 0 (and -0.0) giving +1          what 1: dst[idx[i]] = a[idx[i]] / d
//   what 2: dst[idx[i]] = a[i] (the r-vector into the n-vector)
__global__ __launch_bounds__(256) void k_ce_map(int what, double *a, const int *__restrict__ idx, double *dst, int r, double d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r) return;
    const int j = idx[i];
    if (what == 0) a[j] = (a[j] >= 0.0) ? 1.0 : -1.0;
    else if (what == 1) dst[j] = a[j] / d;
    else dst[j] = a[i];
}
// the null vector in the caller's column order: out[Qfill[j]] = x[j] / d, j < ncol (Qfill nullptr: identity)
__global__ __launch_bounds__(256) void k_ce_vector(const double *__restrict__ x, const int *__restrict__ qfill, double *out, int ncol, double d)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < ncol) out[qfill ? qfill[j] : j] = x[j] / d;
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int stm_launch_rmult(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, const double *X, double *Y,
                     hipStream_t st, int nb, const RhsBatch &B)
{
    if (nfr <= 0 || max_slab <= 0) return 0;
    if (nb >= 3) hipLaunchKernelGGL(k_rmult<4>, dim3(nfr, max_slab, (nb + 3) / 4), dim3(RM_NT), 0, st, c, flist, Rj, rowbase, X, Y, B, nb);
    else hipLaunchKernelGGL(k_rmult<1>, dim3(nfr, max_slab, nb), dim3(RM_NT), 0, st, c, flist, Rj, rowbase, X, Y, B, nb);
    return (int)hipGetLastError();
}
int stm_launch_rmult_dd(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, const double *X, double *Y,
                        hipStream_t st, int nb, const RhsBatch &B)
{
    if (nfr <= 0 || max_slab <= 0 || nb <= 0) return 0;
    hipLaunchKernelGGL(k_rmult_dd, dim3(nfr, max_slab, nb), dim3(RM_NT), 0, st, c, flist, Rj, rowbase, X, Y, B);
    return (int)hipGetLastError();
}
int stm_launch_rtmult_dots(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *rowbase, const double *Y, double *U, int absval,
                           hipStream_t st, int nb, const RhsBatch &B)
{
    if (nfr <= 0 || max_slab <= 0) return 0;
    if (absval) hipLaunchKernelGGL((k_rtmult_dots<1, true>), dim3(nfr, max_slab, 1), dim3(RM_NT), 0, st, c, flist, rowbase, Y, U, B, 1);
    else if (nb >= 3) hipLaunchKernelGGL((k_rtmult_dots<4, false>), dim3(nfr, max_slab, (nb + 3) / 4), dim3(RM_NT), 0, st, c, flist, rowbase, Y, U, B, nb);
    else hipLaunchKernelGGL((k_rtmult_dots<1, false>), dim3(nfr, max_slab, nb), dim3(RM_NT), 0, st, c, flist, rowbase, Y, U, B, nb);
    return (int)hipGetLastError();
}
int stm_launch_rtmult_gather(const int *cp, const int *slot, const double *U, double *Z, int n, hipStream_t st, int nb, long long su, long long sz)
{
    if (n <= 0 || nb <= 0) return 0;
    hipLaunchKernelGGL(k_rtmult_gather, dim3((n + 255) / 256, nb), dim3(256), 0, st, cp, slot, U, Z, n, su, sz);
    return (int)hipGetLastError();
}
int stm_launch_ce_reduce(int what, const double *a, const int *idx, const double *b, int r, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_ce_reduce, dim3(1), dim3(CE_NT), 0, st, what, a, idx, b, r, out);
    return (int)hipGetLastError();
}
int stm_launch_ce_map(int what, double *a, const int *idx, double *dst, int r, double d, hipStream_t st)
{
    if (r <= 0) return 0;
    hipLaunchKernelGGL(k_ce_map, dim3((r + 255) / 256), dim3(256), 0, st, what, a, idx, dst, r, d);
    return (int)hipGetLastError();
}
int stm_launch_ce_vector(const double *x, const int *qfill, double *out, int ncol, double d, hipStream_t st)
{
    if (ncol <= 0) return 0;
    hipLaunchKernelGGL(k_ce_vector, dim3((ncol + 255) / 256), dim3(256), 0, st, x, qfill, out, ncol, d);
    return (int)hipGetLastError();
}
