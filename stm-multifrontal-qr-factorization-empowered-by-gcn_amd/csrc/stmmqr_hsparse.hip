// stmmqr_hsparse.hip -- H of the factors resident in HBM as a sparse matrix in device memory (stmmqr_plan_h_sparse): one compressed
// column per live reflector, the unit diagonal stored, exact zeros dropped, rows = the permuted row ids; its Tau; the row permutation.
// The matrix is the one the host export defines (walk_packed, stmmqr_export.cpp, n1rows = 0): slot (front f, column k) of Rj has
// t = Stair[k] and h = the rows of R above its reflector -- a pivotal column the live pivots up to it (a dead one: t = h), a
// non-pivotal one min(rm + (k - fp) + 1, fm) --; it is a column of H iff t >= h and Tau[k] != 0.0, and then holds front row h - 1 as
// 1.0 and the front rows h .. t - 1 of front column k in that order.  This is the part of a front the export of R
// (stmmqr_rsparse.hip) skips, walked the same way.  Which slots are columns is known only after the count, so the scan runs over the
// slots (slot order = export order: fronts ascend and Rp ascends) and gives every slot its start AND its column number.
// Count, scan, fill -- every position comes from a scan or from a rank within a wave's ballot, no atomics: the output is the same
// bits run after run, and the bits of the host export.
//   k_hs_count   per tree level, a wave per front column: cnt[slot] = 1 + kept entries, vis[slot] = 1 + entries visited, col[slot] = 1
//                (all three 0 where the slot is no column of H)
//   k_hs_scan    one workgroup over the slots, a wave per run of them: off[slot] = the 64-bit running sum of cnt, col[slot] = the
//                running sum of col, the totals -> info
//   k_hs_cols    a thread per slot: a column writes Hp[col[slot]] = off[slot] and HTau[col[slot]] = Tau[slot]; Hp[nh] = hnz
//   k_hs_fill    the level walk again, a wave per column: lane 0 writes the unit diagonal, then 64 rows per trip: ballot of the kept
//                lanes, a lane writes at base + (kept lanes below it), the base moves on by the popcount; idx = Wmap[Hii[row]]
//   k_hs_pinv    a thread per row: HPinv[i] = Wmap[PLinv[i]]
#include "stmmqr_rsdev.h"

// what a slot of the slab holds: rows [h, t) of its front column below the unit diagonal at row h - 1, or has = false.  rmk: the
// live pivots up to column k (rs_col_rows), rm: those of the whole front
struct HsCol { int h, t; bool has; };
__device__ __forceinline__ HsCol hs_column(int t, double tau, int k, int fp, int fm, int rmk, int rm)
{
    HsCol o;
    if (k < fp) {
        o.h = rmk;
        if (t == 0) t = rmk;                            // dead pivot column: nothing below the rows of R
    } else o.h = min(rm + (k - fp) + 1, fm);
    o.t = t;
    o.has = t >= o.h && tau != 0.0 && o.h >= 1;         // (h >= 1: a reflector has a diagonal row; never false where Tau != 0)
    return o;
}
// Stair and Tau of the slab's columns -> LDS, one coalesced read (a wave then starts on a column without waiting for two loads of its
// own); before rs_col_rows, whose barriers publish them
__device__ __forceinline__ void hs_slab_cols(const int *__restrict__ St, const double *__restrict__ Tau, int c0, int fn, int *s_t, double *s_tau)
{
    const int tid = threadIdx.x;
    if (tid < RS_COLS && c0 + tid < fn) { s_t[tid] = St[c0 + tid]; s_tau[tid] = Tau[c0 + tid]; }
}

// workgroup (front, slab of RS_COLS columns)
__global__ __launch_bounds__(RS_NT) void k_hs_count(DevCtx c, const int *__restrict__ flist, int *__restrict__ cnt, int *__restrict__ vis,
                                                    int *__restrict__ colflag)
{
    __shared__ int s_scan[NW];
    __shared__ int s_cnt[RS_COLS], s_t[RS_COLS];
    __shared__ double s_tau[RS_COLS];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fp = s.fp, fn = s.fn, fm = max(c.fnum[f].fm, 0);
    const int c0 = (int)blockIdx.y * RS_COLS, tid = threadIdx.x;
    if (c0 >= fn) return;                               // (uniform)
    hs_slab_cols(c.Stair + s.rp, c.Tau + s.rp, c0, fn, s_t, s_tau);
    const int rm = rs_col_rows(c.Stair + s.rp, fp, fm, c0, s_scan, s_cnt);
    const int lane = tid & 63, wv = tid >> 6;
    const double *F = c.Farena + s.foff;
    const long long ld = s.ld;
    for (int cc = wv; cc < RS_COLS; cc += NW) {
        const int k = c0 + cc;
        if (k >= fn) break;                             // (uniform over the wave)
        const HsCol hc = hs_column(s_t[cc], s_tau[cc], k, fp, fm, (k < fp) ? s_cnt[cc] : rm, rm);
        const int rows = hc.has ? hc.t - hc.h : 0;
        const double *col = F + (long long)k * ld + hc.h;
        int nz = 0, q = lane;
        for (; q + 192 < rows; q += 256) {              // (four loads in flight)
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = col[q + 64 * u];
#pragma unroll
            for (int u = 0; u < 4; u++) nz += (v[u] != 0.0);
        }
        for (; q < rows; q += 64) nz += (col[q] != 0.0);
        nz = rs_wave_sum(nz);
        if (lane == 0) {
            cnt[s.rp + k] = hc.has ? 1 + nz : 0;
            vis[s.rp + k] = hc.has ? 1 + rows : 0;
            colflag[s.rp + k] = hc.has ? 1 : 0;
        }
    }
}

// One workgroup over the nslots slots of Rj: off[slot] = what the slots before it keep, col[slot] (1 for a column of H on entry) = the
// columns of H before it; info = {columns, entries kept, entries visited, m}.  A wave takes a run of consecutive slots and walks it 64
// slots per trip, a slot per lane (coalesced; a thread per run of slots reads a cache line per lane and trip): it adds them up, the
// waves' sums are scanned through LDS, it walks its run again with a scan of every trip by shuffles.  The sums of one trip are int (64
// slots of one front's column at most), every carry and every offset is 64-bit.
__global__ __launch_bounds__(RS_SCAN_NT) void k_hs_scan(const int *__restrict__ cnt, const int *__restrict__ vis, int *__restrict__ col,
                                                        long long *__restrict__ off, long long nslots, long long m, long long *__restrict__ info)
{
    constexpr int W = RS_SCAN_NT / 64;
    __shared__ long long s_c[W], s_v[W], s_q[W];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long per = ((nslots + W - 1) / W + 63) & ~63LL;                 // slots of a wave: whole trips
    const long long i0 = min(nslots, wid * per), i1 = min(nslots, i0 + per);
    long long sum = 0, v = 0, ncol = 0;
#pragma unroll 4
    for (long long i = i0 + lane; i < i1; i += 64) { sum += cnt[i]; v += vis[i]; ncol += col[i]; }
    sum = rs_wave_sum(sum); v = rs_wave_sum(v); ncol = rs_wave_sum(ncol);
    if (lane == 0) { s_c[wid] = sum; s_v[wid] = v; s_q[wid] = ncol; }
    __syncthreads();
    // (a lane per wave total, summed by shuffles: sixteen 64-bit triples read by every thread would take 96 registers)
    const long long sw = (lane < W) ? s_c[lane] : 0, sq = (lane < W) ? s_q[lane] : 0, sv = (lane < W) ? s_v[lane] : 0;
    long long run = rs_wave_sum((lane < wid) ? sw : 0), q = rs_wave_sum((lane < wid) ? sq : 0);    // what lies before this wave's run
    const long long tot = rs_wave_sum(sw), qtot = rs_wave_sum(sq), vtot = rs_wave_sum(sv);
#pragma unroll 1
    for (long long b = i0; b < i1; b += 256) {          // (four trips' loads in flight, their scans in order)
        int c1[4], f1[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const long long i = b + 64 * u + lane;
            c1[u] = (i < i1) ? cnt[i] : 0; f1[u] = (i < i1) ? col[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const long long i = b + 64 * u + lane;
            int x = c1[u], xq = f1[u];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o, 64), yq = __shfl_up(xq, o, 64);
                if (lane >= o) { x += y; xq += yq; }
            }
            if (i < i1) { off[i] = run + (x - c1[u]); col[i] = (int)(q + (xq - f1[u])); }
            run += __shfl(x, 63, 64); q += __shfl(xq, 63, 64);
        }
    }
    if (tid == 0) { info[0] = qtot; info[1] = tot; info[2] = vtot; info[3] = m; }
}

// a slot that is a column of H (cnt > 0: the unit diagonal is counted) -> its Hp and HTau; the end of the last column
__global__ __launch_bounds__(256) void k_hs_cols(const double *__restrict__ Tau, const int *__restrict__ cnt, const int *__restrict__ col,
                                                 const long long *__restrict__ off, int nslots, const long long *__restrict__ info,
                                                 long long *__restrict__ Hp, double *__restrict__ HTau)
{
    const int sl = blockIdx.x * 256 + threadIdx.x;
    if (sl == 0) Hp[info[0]] = info[1];
    if (sl >= nslots || cnt[sl] <= 0) return;
    const int q = col[sl];
    Hp[q] = off[sl];
    HTau[q] = Tau[sl];
}

// the walk of k_hs_count; a wave writes its column's unit diagonal and kept entries in front-row order from off[slot]
__global__ __launch_bounds__(RS_NT) void k_hs_fill(DevCtx c, const int *__restrict__ flist, const int *__restrict__ wmap,
                                                   const long long *__restrict__ off, long long *__restrict__ idx, double *__restrict__ val)
{
    __shared__ int s_scan[NW];
    __shared__ int s_cnt[RS_COLS], s_t[RS_COLS];
    __shared__ double s_tau[RS_COLS];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fp = s.fp, fn = s.fn, fm = max(c.fnum[f].fm, 0);
    const int c0 = (int)blockIdx.y * RS_COLS, tid = threadIdx.x;
    if (c0 >= fn) return;                               // (uniform)
    hs_slab_cols(c.Stair + s.rp, c.Tau + s.rp, c0, fn, s_t, s_tau);
    const int rm = rs_col_rows(c.Stair + s.rp, fp, fm, c0, s_scan, s_cnt);
    const int lane = tid & 63, wv = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;     // the lanes below this one
    const double *F = c.Farena + s.foff;
    const int *hii = c.Hii + s.hip;
    const long long ld = s.ld;
    for (int cc = wv; cc < RS_COLS; cc += NW) {
        const int k = c0 + cc;
        if (k >= fn) break;                             // (uniform over the wave)
        const HsCol hc = hs_column(s_t[cc], s_tau[cc], k, fp, fm, (k < fp) ? s_cnt[cc] : rm, rm);
        if (!hc.has) continue;                          // (uniform)
        const int rows = hc.t - hc.h;
        const double *col = F + (long long)k * ld + hc.h;
        const int *rid = hii + hc.h;
        long long base = off[s.rp + k];
        if (lane == 0) { idx[base] = wmap[hii[hc.h - 1]]; val[base] = 1.0; }
        base++;
        int i0 = 0;
        for (; i0 + 192 < rows; i0 += 256) {            // (four loads in flight; the trips are written in order)
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = col[min(i0 + 64 * u + lane, rows - 1)];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + 64 * u + lane;
                const bool keep = i < rows && v[u] != 0.0;
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
                if (keep) {
                    const long long pos = base + __popcll(mask & below);
                    idx[pos] = wmap[rid[i]]; val[pos] = v[u];
                }
                base += __popcll(mask);
            }
        }
        for (; i0 < rows; i0 += 64) {
            const int i = i0 + lane;
            const double v = col[min(i, rows - 1)];
            const bool keep = i < rows && v != 0.0;
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
            if (keep) {
                const long long pos = base + __popcll(mask & below);
                idx[pos] = wmap[rid[i]]; val[pos] = v;
            }
            base += __popcll(mask);
        }
    }
}

__global__ __launch_bounds__(256) void k_hs_pinv(const int *__restrict__ plinv, const int *__restrict__ wmap, int m, long long *__restrict__ HPinv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) HPinv[i] = wmap[plinv[i]];
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int stm_launch_hs_count(const DevCtx &c, const int *flist, int nfr, int max_slab, int *cnt, int *vis, int *col, hipStream_t st)
{
    if (nfr <= 0 || max_slab <= 0) return 0;
    hipLaunchKernelGGL(k_hs_count, dim3(nfr, max_slab), dim3(RS_NT), 0, st, c, flist, cnt, vis, col);
    return (int)hipGetLastError();
}
int stm_launch_hs_scan(const int *cnt, const int *vis, int *col, long long *off, long long nslots, long long m, long long *info, hipStream_t st)
{
    hipLaunchKernelGGL(k_hs_scan, dim3(1), dim3(RS_SCAN_NT), 0, st, cnt, vis, col, off, nslots, m, info);
    return (int)hipGetLastError();
}
int stm_launch_hs_cols(const double *Tau, const int *cnt, const int *col, const long long *off, int nslots, const long long *info, long long *Hp,
                       double *HTau, hipStream_t st)
{
    hipLaunchKernelGGL(k_hs_cols, dim3(((nslots > 0 ? nslots : 1) + 255) / 256), dim3(256), 0, st, Tau, cnt, col, off, nslots, info, Hp, HTau);
    return (int)hipGetLastError();
}
int stm_launch_hs_fill(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *wmap, const long long *off, long long *Hi, double *Hx,
                       hipStream_t st)
{
    if (nfr <= 0 || max_slab <= 0) return 0;
    hipLaunchKernelGGL(k_hs_fill, dim3(nfr, max_slab), dim3(RS_NT), 0, st, c, flist, wmap, off, Hi, Hx);
    return (int)hipGetLastError();
}
int stm_launch_hs_pinv(const int *plinv, const int *wmap, int m, long long *HPinv, hipStream_t st)
{
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_hs_pinv, dim3((m + 255) / 256), dim3(256), 0, st, plinv, wmap, m, HPinv);
    return (int)hipGetLastError();
}
