// stmmqr_rsdev.h -- device code the two sparse exports of the resident factors share (stmmqr_rsparse.hip: R, stmmqr_hsparse.hip: H):
// the shape of the level-walk kernels -- workgroup (front, slab of RS_COLS columns), a wave per column --, the prologue that gives
// every pivotal column of the slab its rows of R, and the sums over a wave.
#pragma once
#include "stmmqr_kdev.h"

#define RS_NT 256                 // threads of the level-walk kernels (block_incl_scan: NT)
#define RS_COLS STM_RM_COLS       // columns of a front per workgroup, a wave per column
#define RS_ROWS STM_RM_ROWS       // rows of a front per workgroup, a row per thread
#define RS_SCAN_NT 1024           // threads of the one-workgroup scan
static_assert(RS_NT == NT && RS_ROWS == RS_NT, "one row per thread, the 256-thread scan");
static_assert(RS_COLS % NW == 0, "every wave takes the same number of columns");

// rows of R in the columns [c0, c0 + RS_COLS) of a front's pivotal part -> s_cnt (the live pivots up to the column, at most fm); returns
// the rows of R of the front.  The prologue of k_rtmult_dots; every thread of the workgroup calls it.
__device__ __forceinline__ int rs_col_rows(const int *__restrict__ St, int fp, int fm, int c0, int *s_scan, int *s_cnt)
{
    const int tid = threadIdx.x;
    const int per = (fp + RS_NT - 1) / RS_NT;
    const int k0 = min(fp, tid * per), k1 = min(fp, k0 + per);
    int cnt = 0;
    for (int k = k0; k < k1; k++) cnt += (St[k] != 0);
    int total;
    const int incl = block_incl_scan(cnt, s_scan, &total);
    int q = incl - cnt;
    for (int k = k0; k < k1; k++) {
        q += (St[k] != 0);
        if (k >= c0 && k < c0 + RS_COLS) s_cnt[k - c0] = min(q, fm);
    }
    __syncthreads();
    return min(total, fm);
}
__device__ __forceinline__ int rs_wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long rs_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
