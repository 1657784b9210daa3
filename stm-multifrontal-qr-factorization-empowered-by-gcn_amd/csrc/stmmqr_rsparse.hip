// stmmqr_rsparse.hip -- R of the factors resident in HBM as a sparse matrix in device memory (stmmqr_plan_r_sparse): compressed
// columns or compressed rows, exact zeros dropped, rows below `econ` and columns below `ncol` only.  The matrix is the one the host
// export defines (walk_packed, stmmqr_export.cpp): row q of a front is its q-th live pivot column (the rule of stmmqr_rmult.hip),
// global row rowbase[f] + q; column k < fp of a front holds the rows of the live pivots up to k, a non-pivotal column all of them.
// Count, scan, fill -- every position comes from a scan or from a rank within a wave's ballot, no atomics: the output is the same
// bits run after run, and the bits of the host export.
//   columns:  k_rs_count_cols  per tree level, a wave per front column: cnt[slot] = kept entries, vis[slot] = entries visited
//             k_rs_item_sums   a thread per column of R: ptr[j + 1] = the sum over its slots (the transpose of Rj: front order =
//                              row order), the workgroup's sum of vis
//             k_rs_scan        one workgroup: ptr in place, the totals -> info
//             k_rs_slot_offsets  a thread per column: where every slot starts
//             k_rs_fill_cols   the level walk again, a wave per column, 64 rows per trip: ballot of the kept lanes, a lane writes at
//                              base + (kept lanes below it), the base moves on by the popcount
//   rows:     k_rs_rows<false> per tree level, a thread per row (the access shape of k_rmult), from the row's diagonal on: cnt / vis
//             k_rs_item_sums, k_rs_scan over the m rows
//             k_rs_rows<true>  the same walk, a row writes its entries in front order (k = 0 .. fn - 1) from ptr[row]
#include "stmmqr_rsdev.h"        // RS_NT / RS_COLS / RS_ROWS / RS_SCAN_NT, rs_col_rows, rs_wave_sum: shared with stmmqr_hsparse.hip

// ------------------------------------------------------------------------------------------------
// compressed columns
// ------------------------------------------------------------------------------------------------
// workgroup (front, slab of RS_COLS columns).  econ: at most m (the host clamps it)
__global__ __launch_bounds__(RS_NT) void k_rs_count_cols(DevCtx c, const int *__restrict__ flist, const int *__restrict__ Rj,
                                                         const int *__restrict__ rowbase, int ncol, int econ, int *__restrict__ cnt,
                                                         int *__restrict__ vis)
{
    __shared__ int s_scan[NW];
    __shared__ int s_cnt[RS_COLS];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fp = s.fp, fn = s.fn, fm = max(c.fnum[f].fm, 0);
    const int c0 = (int)blockIdx.y * RS_COLS, tid = threadIdx.x;
    if (c0 >= fn) return;                               // (uniform)
    const int rm = rs_col_rows(c.Stair + s.rp, fp, fm, c0, s_scan, s_cnt);
    const int lane = tid & 63, wv = tid >> 6;
    const int above = max(0, min(rm, econ - rowbase[f]));       // rows of the front above row econ of R
    const double *F = c.Farena + s.foff;
    const long long ld = s.ld;
    for (int cc = wv; cc < RS_COLS; cc += NW) {
        const int k = c0 + cc;
        if (k >= fn) break;                             // (uniform over the wave)
        const int j = (k < fp) ? s.col1 + k : Rj[s.rp + k];
        const int rows = (j < ncol) ? min((k < fp) ? s_cnt[cc] : rm, above) : 0;
        const double *col = F + (long long)k * ld;
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
        if (lane == 0) { cnt[s.rp + k] = nz; vis[s.rp + k] = rows; }
    }
}

// item j (a column of R through cp / slot, or with cp == nullptr a row: its own cnt / vis) -> ptr[j + 1] = its kept entries;
// part[workgroup] = the visited entries of the workgroup's items
__global__ __launch_bounds__(256) void k_rs_item_sums(const int *__restrict__ cp, const int *__restrict__ slot, const int *__restrict__ cnt,
                                                      const int *__restrict__ vis, int nitems, long long *__restrict__ ptr,
                                                      long long *__restrict__ part)
{
    __shared__ long long s_p[4];
    const int tid = threadIdx.x, j = blockIdx.x * 256 + tid;
    long long cs = 0, vs = 0;
    if (j < nitems) {
        if (cp) {
            for (int p = cp[j]; p < cp[j + 1]; p++) { const int sl = slot[p]; cs += cnt[sl]; vs += vis[sl]; }
        } else { cs = cnt[j]; vs = vis[j]; }
        ptr[j + 1] = cs;
    }
    vs = rs_wave_sum(vs);
    if ((tid & 63) == 0) s_p[tid >> 6] = vs;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = s_p[0] + s_p[1] + s_p[2] + s_p[3];
}

// One workgroup: ptr[1 .. nitems] (counts) -> their running sums, ptr[0] = 0; info = {entries kept, entries visited, rows of R, 0}.
// A thread takes a run of consecutive items: it adds them up, the threads' sums are scanned, it walks its run again.  Every offset is
// 64-bit (the largest R of the workloads has more than 2^31 entries).
__global__ __launch_bounds__(RS_SCAN_NT) void k_rs_scan(long long *__restrict__ ptr, long long nitems, const long long *__restrict__ part,
                                                        int nparts, long long rtot, long long *__restrict__ info)
{
    constexpr int W = RS_SCAN_NT / 64;
    __shared__ long long s_w[W], s_v[W];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long per = (nitems + RS_SCAN_NT - 1) / RS_SCAN_NT;
    const long long i0 = min(nitems, tid * per), i1 = min(nitems, i0 + per);
    long long sum = 0;
    for (long long i = i0; i < i1; i++) sum += ptr[1 + i];
    long long x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    long long v = 0;
    for (int p = tid; p < nparts; p += RS_SCAN_NT) v += part[p];
    v = rs_wave_sum(v);
    if (lane == 63) s_w[wid] = x;
    if (lane == 0) s_v[wid] = v;
    __syncthreads();
    long long base = 0, tot = 0, vtot = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
        const long long sw = s_w[w];
        if (w < wid) base += sw;
        tot += sw;
        vtot += s_v[w];
    }
    long long run = base + x - sum;                     // what lies before this thread's run
    for (long long i = i0; i < i1; i++) { run += ptr[1 + i]; ptr[1 + i] = run; }
    if (tid == 0) { ptr[0] = 0; info[0] = tot; info[1] = vtot; info[2] = rtot; info[3] = 0; }
}

// where the entries of every slot of column j < ncol start: its slots in slot order = its fronts in row order
__global__ __launch_bounds__(256) void k_rs_slot_offsets(const int *__restrict__ cp, const int *__restrict__ slot, const int *__restrict__ cnt,
                                                         const long long *__restrict__ ptr, long long *__restrict__ off, int ncol)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ncol) return;
    long long run = ptr[j];
    for (int p = cp[j]; p < cp[j + 1]; p++) { const int sl = slot[p]; off[sl] = run; run += cnt[sl]; }
}

// the walk of k_rs_count_cols; a wave writes its column's kept entries in row order from off[slot]
__global__ __launch_bounds__(RS_NT) void k_rs_fill_cols(DevCtx c, const int *__restrict__ flist, const int *__restrict__ Rj,
                                                        const int *__restrict__ rowbase, int ncol, int econ, const long long *__restrict__ off,
                                                        long long *__restrict__ idx, double *__restrict__ val)
{
    __shared__ int s_scan[NW];
    __shared__ int s_cnt[RS_COLS];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fp = s.fp, fn = s.fn, fm = max(c.fnum[f].fm, 0);
    const int c0 = (int)blockIdx.y * RS_COLS, tid = threadIdx.x;
    if (c0 >= fn) return;                               // (uniform)
    const int rm = rs_col_rows(c.Stair + s.rp, fp, fm, c0, s_scan, s_cnt);
    const int lane = tid & 63, wv = tid >> 6;
    const int rb = rowbase[f];
    const int above = max(0, min(rm, econ - rb));
    const unsigned long long below = (1ull << lane) - 1ull;     // the lanes below this one
    const double *F = c.Farena + s.foff;
    const long long ld = s.ld;
    for (int cc = wv; cc < RS_COLS; cc += NW) {
        const int k = c0 + cc;
        if (k >= fn) break;                             // (uniform over the wave)
        const int j = (k < fp) ? s.col1 + k : Rj[s.rp + k];
        const int rows = (j < ncol) ? min((k < fp) ? s_cnt[cc] : rm, above) : 0;
        if (rows <= 0) continue;                        // (uniform; the slot of a column >= ncol has no offset)
        const double *col = F + (long long)k * ld;
        long long base = off[s.rp + k];
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
                    idx[pos] = rb + i; val[pos] = v[u];
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
                idx[pos] = rb + i; val[pos] = v;
            }
            base += __popcll(mask);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// compressed rows: a row of R lies in one front.  Workgroup (front, slab of RS_ROWS rows), a row per thread -- consecutive threads
// read consecutive rows of a column; a row walks the front's columns in front order from its own diagonal.  FILL false: cnt[row] /
// vis[row]; true: the kept entries from ptr[row] on.
// ------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(RS_NT) void k_rs_rows(DevCtx c, const int *__restrict__ flist, const int *__restrict__ Rj,
                                                   const int *__restrict__ rowbase, int ncol, int econ, int *__restrict__ cnt,
                                                   int *__restrict__ vis, const long long *__restrict__ ptr, long long *__restrict__ idx,
                                                   double *__restrict__ val)
{
    __shared__ int s_scan[NW];
    __shared__ int s_lc[RS_ROWS];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    const int fp = s.fp, fn = s.fn, fm = c.fnum[f].fm;
    const int i0 = (int)blockIdx.y * RS_ROWS, tid = threadIdx.x;
    if (fp <= 0 || i0 >= min(fp, fm)) return;           // (uniform: no row of R in this slab)
    const int *St = c.Stair + s.rp;
    int rm;
    {
        const int per = (fp + RS_NT - 1) / RS_NT;
        const int k0 = min(fp, tid * per), k1 = min(fp, k0 + per);
        int n = 0;
        for (int k = k0; k < k1; k++) n += (St[k] != 0);
        int total;
        const int incl = block_incl_scan(n, s_scan, &total);
        int q = incl - n;
        for (int k = k0; k < k1; k++) {
            if (St[k] == 0) continue;
            if (q >= i0 && q < i0 + RS_ROWS && q < fm) s_lc[q - i0] = k;
            q++;
        }
        rm = min(total, fm);
    }
    __syncthreads();
    if (i0 >= rm) return;
    const int i = i0 + tid, ic = min(i, rm - 1);
    const int mylc = s_lc[ic - i0], kbeg = s_lc[0];
    const int row = rowbase[f] + ic;
    const bool mine = i < rm && row < econ;
    const int *rj = Rj + s.rp;
    const double *Fp = c.Farena + s.foff + ic;
    const long long ld = s.ld;
    long long pos = 0;
    if (FILL) pos = ptr[row];
    int nk = 0, nv = 0, k = kbeg;
    auto take = [&](int kk, double v) {
        const int j = (kk < fp) ? s.col1 + kk : rj[kk];
        const bool on = mine && kk >= mylc && j < ncol;           // (below the diagonal: the reflectors, not R)
        if (FILL) {
            if (on && v != 0.0) { idx[pos] = j; val[pos] = v; pos++; }
        } else { nv += on; nk += (on && v != 0.0); }
    };
    for (; k + 4 <= fn; k += 4) {                       // (four loads in flight, taken in column order)
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = Fp[(long long)(k + u) * ld];
#pragma unroll
        for (int u = 0; u < 4; u++) take(k + u, v[u]);
    }
    for (; k < fn; k++) take(k, Fp[(long long)k * ld]);
    if (!FILL && i < rm) { cnt[row] = nk; vis[row] = nv; }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int stm_launch_rs_count_cols(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, int ncol, int econ,
                             int *cnt, int *vis, hipStream_t st)
{
    if (nfr <= 0 || max_slab <= 0) return 0;
    hipLaunchKernelGGL(k_rs_count_cols, dim3(nfr, max_slab), dim3(RS_NT), 0, st, c, flist, Rj, rowbase, ncol, econ, cnt, vis);
    return (int)hipGetLastError();
}
int stm_launch_rs_fill_cols(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, int ncol, int econ,
                            const long long *off, long long *idx, double *val, hipStream_t st)
{
    if (nfr <= 0 || max_slab <= 0) return 0;
    hipLaunchKernelGGL(k_rs_fill_cols, dim3(nfr, max_slab), dim3(RS_NT), 0, st, c, flist, Rj, rowbase, ncol, econ, off, idx, val);
    return (int)hipGetLastError();
}
int stm_launch_rs_rows(const DevCtx &c, const int *flist, int nfr, int max_slab, const int *Rj, const int *rowbase, int ncol, int econ,
                       int *cnt, int *vis, const long long *ptr, long long *idx, double *val, int fill, hipStream_t st)
{
    if (nfr <= 0 || max_slab <= 0) return 0;
    if (fill) hipLaunchKernelGGL(k_rs_rows<true>, dim3(nfr, max_slab), dim3(RS_NT), 0, st, c, flist, Rj, rowbase, ncol, econ, cnt, vis, ptr, idx, val);
    else hipLaunchKernelGGL(k_rs_rows<false>, dim3(nfr, max_slab), dim3(RS_NT), 0, st, c, flist, Rj, rowbase, ncol, econ, cnt, vis, ptr, idx, val);
    return (int)hipGetLastError();
}
int stm_launch_rs_item_sums(const int *cp, const int *slot, const int *cnt, const int *vis, int nitems, long long *ptr, long long *part,
                            hipStream_t st)
{
    if (nitems <= 0) return 0;
    hipLaunchKernelGGL(k_rs_item_sums, dim3((nitems + 255) / 256), dim3(256), 0, st, cp, slot, cnt, vis, nitems, ptr, part);
    return (int)hipGetLastError();
}
int stm_launch_rs_scan(long long *ptr, long long nitems, const long long *part, int nparts, long long rtot, long long *info, hipStream_t st)
{
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(RS_SCAN_NT), 0, st, ptr, nitems, part, nparts, rtot, info);
    return (int)hipGetLastError();
}
int stm_launch_rs_slot_offsets(const int *cp, const int *slot, const int *cnt, const long long *ptr, long long *off, int ncol, hipStream_t st)
{
    if (ncol <= 0) return 0;
    hipLaunchKernelGGL(k_rs_slot_offsets, dim3((ncol + 255) / 256), dim3(256), 0, st, cp, slot, cnt, ptr, off, ncol);
    return (int)hipGetLastError();
}
