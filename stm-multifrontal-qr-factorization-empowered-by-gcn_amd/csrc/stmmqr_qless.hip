// stmmqr_qless.hip -- factors without H (QRsym->keepH == 0) and products with A on the device:
//   k_r_count / k_r_copy / k_r_window / k_r_unpack   qr_rhpack's keepH = 0 layout (SparseQR_factorize.c:1691-1784): the R part of
//                                                     every column only.  The offsets of the blocks (k_rh_scan) do not depend on
//                                                     the layout and are shared with the R+H path.
//   k_spmv                                           Y = A X, Y = A' X and the fused residual R = B - A X for blocks of vectors
//   k_colnorm2 / k_add_cols                          the small pieces of the seminormal solve (stmmqr_rfactor.cpp)
// New kernels beside stmmqr_pack.hip's instead of a keepH branch in those (profiles/EXPERIMENTS.md: one more path in a shared
// body made a kernel spill).
#include "stmmqr_kdev.h"

// Column lengths of the R-only block of a front -> exclusive offsets in Rhoff, the block size in FrontNum::rsize.  Column k < fp
// keeps rows 0 .. rm(k)-1, rm(k) = the live pivots among columns 0..k (at most fm), dead columns included; column k >= fp keeps the
// rm rows of R.  The bump pointer of the slab recycling is used exactly as by k_rh_count.
__global__ __launch_bounds__(NT) void k_r_count(DevCtx c, const int *__restrict__ flist)
{
    __shared__ int s_scan[NW];
    const int f = flist[blockIdx.x];
    const FrontSym s = c.fs[f];
    FrontNum *num = &c.fnum[f];
    const int tid = threadIdx.x;
    const int fm = num->fm, n = s.fn, fp = s.fp;
    const int *St = c.Stair + s.rp;
    long long *off = c.Rhoff + s.rp;
    if (fm <= 0 || n <= 0) {
        for (int k = tid; k < n; k += NT) off[k] = 0;
        if (tid == 0) num->rsize = 0;
        return;
    }
    // pass 1: rm(k), stored temporarily in off[]
    long long carry = 0;
    for (int base = 0; base < fp; base += NT) {
        const int k = base + tid;
        const int live = (k < fp && St[k] != 0) ? 1 : 0;
        int tot;
        const int incl = block_incl_scan(live, s_scan, &tot);
        if (k < fp) off[k] = min(carry + incl, (long long)fm);
        carry += tot;
    }
    __syncthreads();
    const int rm = (int)min(carry, (long long)fm);
    // pass 2: column lengths -> exclusive offsets
    carry = 0;
    for (int base = 0; base < n; base += NT) {
        const int k = base + tid;
        const int len = (k < fp) ? (int)off[k] : (k < n ? rm : 0);
        __syncthreads();
        int tot;
        const int incl = block_incl_scan(len, s_scan, &tot);
        if (k < n) off[k] = carry + incl - len;
        carry += tot;
    }
    if (tid == 0) {
        num->rsize = carry;
        if (c.rh_top) {
            const long long at = (long long)atomicAdd((unsigned long long *)c.rh_top, (unsigned long long)carry);
            if (at + carry > c.rh_cap) { c.Rboff[f] = -1; atomicExch((int *)(c.rh_top + 1), 1); }
            else c.Rboff[f] = at;
        }
    }
}

// rows of column k in the R-only block: every column is a prefix of the front's column
__device__ __forceinline__ int r_len(const long long *off, int k, int n, long long rsize)
{
    return (int)(((k + 1 < n) ? off[k + 1] : rsize) - off[k]);
}

// one wave per column, eight loads of a lane in flight before their stores (as k_rh_copy)
__device__ __forceinline__ void wave_copy(double *dst, const double *src, int len, int lane)
{
    int i = lane;
    for (; i + 7 * 64 < len; i += 8 * 64) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = src[i + 64 * u];
#pragma unroll
        for (int u = 0; u < 8; u++) dst[i + 64 * u] = v[u];
    }
    for (; i < len; i += 64) dst[i] = src[i];
}

__global__ __launch_bounds__(NT) void k_r_copy(DevCtx c, const int *__restrict__ flist, const int *__restrict__ nparts_list,
                                               double *__restrict__ RH)
{
    const int fi = blockIdx.y;
    const int nparts = nparts_list[fi];
    if ((int)blockIdx.x >= nparts) return;
    const int f = flist[fi];
    const FrontSym s = c.fs[f];
    const FrontNum *num = &c.fnum[f];
    const int n = s.fn;
    if (num->fm <= 0 || n <= 0 || c.Rboff[f] < 0) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double *F = c.Farena + s.foff;
    const long long *off = c.Rhoff + s.rp;
    double *R = RH + c.Rboff[f];
    for (int k = blockIdx.x * NW + wid; k < n; k += nparts * NW)
        wave_copy(R + off[k], F + (long long)k * s.ld, r_len(off, k, n, num->rsize), lane);
}

// download window [w0, w1) of the final layout (as k_rh_window): staged blocks are copied, kept fronts packed on the fly
__global__ __launch_bounds__(NT) void k_r_window(DevCtx c, const int *__restrict__ flist, const long long *__restrict__ fin,
                                                 const char *__restrict__ kept, const double *__restrict__ RH, long long w0, long long w1,
                                                 double *__restrict__ out)
{
    const int f = flist[blockIdx.y];
    const FrontSym s = c.fs[f];
    const FrontNum *num = &c.fnum[f];
    const long long b0 = fin[f], b1 = b0 + num->rsize;
    if (b1 <= w0 || b0 >= w1 || num->rsize <= 0) return;
    if (!kept[f]) {
        if (c.Rboff[f] < 0) return;
        const double *src = RH + c.Rboff[f];
        const long long a = max(w0, b0), b = min(w1, b1);
        for (long long i = a + (long long)blockIdx.x * NT + threadIdx.x; i < b; i += (long long)gridDim.x * NT) out[i - w0] = src[i - b0];
        return;
    }
    const int n = s.fn;
    if (num->fm <= 0 || n <= 0) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double *F = c.Farena + s.foff;
    const long long *off = c.Rhoff + s.rp;
    for (int k = blockIdx.x * NW + wid; k < n; k += gridDim.x * NW) {
        const long long d = b0 + off[k];
        const int len = r_len(off, k, n, num->rsize);
        if (d + len <= w0 || d >= w1) continue;
        const int i0 = (int)max(0LL, w0 - d), i1 = (int)min((long long)len, w1 - d);
        const double *Fk = F + (long long)k * s.ld;
        for (int i = i0 + lane; i < i1; i += 64) out[d + i - w0] = Fk[i];
    }
}

// front form of a staged R-only block in the scratch of the resident-factor operations: R where the kernels of SURVEY 8 (f1) read
// it, zeros below (k_rh_unpack's phase 0 clears the front's actual rows first: stm_launch_r_unpack)
__global__ __launch_bounds__(NT) void k_r_unpack(DevCtx c, const FrontSym *__restrict__ cs, const int *__restrict__ flist,
                                                 const char *__restrict__ kept, const double *__restrict__ RH, double *__restrict__ scratch)
{
    const int f = flist[blockIdx.y];
    if (kept[f]) return;
    const FrontSym s = cs[f];
    const FrontNum *num = &c.fnum[f];
    const int n = s.fn;
    if (num->fm <= 0 || n <= 0 || c.Rboff[f] < 0) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long long *off = c.Rhoff + s.rp;
    const double *R = RH + c.Rboff[f];
    double *F = scratch + s.foff;
    for (int k = blockIdx.x * NW + wid; k < n; k += gridDim.x * NW)
        wave_copy(F + (long long)k * s.ld, R + off[k], r_len(off, k, n, num->rsize), lane);
}

// Y(:, j) = A X(:, j) (row form of A: ptr / idx = columns / vpos = position of the value in A's own order) or A' X(:, j) (A's
// column form: vpos = nullptr), or with B: Y(:, j) = B(:, j) - A X(:, j).  One thread per output entry, its terms summed in index
// order: the same bits on every call, and column j of a batch equals the single-vector call.
__global__ __launch_bounds__(256) void k_spmv(int rows, const int *__restrict__ ptr, const int *__restrict__ idx, const int *__restrict__ vpos,
                                              const double *__restrict__ Ax, const double *__restrict__ X, long long ldx,
                                              const double *__restrict__ B, long long ldb, double *__restrict__ Y, long long ldy)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const long long j = blockIdx.y;
    const double *x = X + j * ldx;
    double acc = 0.0;
    const int q1 = ptr[i + 1];
    if (vpos)
        for (int q = ptr[i]; q < q1; q++) acc = fma(Ax[vpos[q]], x[idx[q]], acc);
    else
        for (int q = ptr[i]; q < q1; q++) acc = fma(Ax[q], x[idx[q]], acc);
    Y[i + j * ldy] = B ? B[i + j * ldb] - acc : acc;
}

// out[j] = sum of squares of column j (one workgroup per column, fixed summation order)
__global__ __launch_bounds__(256) void k_colnorm2(long long rows, const double *__restrict__ X, long long ldx, double *__restrict__ out)
{
    __shared__ double red[256];
    const double *x = X + (long long)blockIdx.x * ldx;
    double s = 0.0;
    for (long long i = threadIdx.x; i < rows; i += 256) s = fma(x[i], x[i], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// X(:, j) += D(:, j)
__global__ __launch_bounds__(256) void k_add_cols(int rows, const double *__restrict__ D, long long ldd, double *__restrict__ X, long long ldx)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const long long j = blockIdx.y;
    X[i + j * ldx] += D[i + j * ldd];
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int stm_launch_r_count(const DevCtx &c, const int *flist, int nfr, hipStream_t st)
{
    if (nfr <= 0) return 0;
    hipLaunchKernelGGL(k_r_count, dim3(nfr), dim3(NT), 0, st, c, flist);
    return (int)hipGetLastError();
}
int stm_launch_r_copy(const DevCtx &c, const int *flist, const int *nparts, int nfr, int maxparts, double *RH, hipStream_t st)
{
    if (nfr <= 0) return 0;
    hipLaunchKernelGGL(k_r_copy, dim3(maxparts, nfr), dim3(NT), 0, st, c, flist, nparts, RH);
    return (int)hipGetLastError();
}
int stm_launch_r_window(const DevCtx &c, const int *flist, int nfr, int maxparts, const long long *fin, const char *kept, const double *RH,
                        long long w0, long long w1, double *out, hipStream_t st)
{
    if (nfr <= 0 || w1 <= w0) return 0;
    hipLaunchKernelGGL(k_r_window, dim3(maxparts, nfr), dim3(NT), 0, st, c, flist, fin, kept, RH, w0, w1, out);
    return (int)hipGetLastError();
}
int stm_launch_r_unpack(const DevCtx &c, const int *flist, int nfr, int maxparts, const char *kept, const double *RH, const FrontSym *cs,
                        double *scratch, hipStream_t st)
{
    if (nfr <= 0) return 0;
    const int e = stm_launch_rh_zero(c, cs, flist, nfr, maxparts, kept, scratch, st);
    if (e) return e;
    hipLaunchKernelGGL(k_r_unpack, dim3(maxparts, nfr), dim3(NT), 0, st, c, cs, flist, kept, RH, scratch);
    return (int)hipGetLastError();
}
// nrhs vectors in launches of at most 65535 (grid y)
int stm_launch_spmv(int rows, const int *ptr, const int *idx, const int *vpos, const double *Ax, const double *X, long long ldx,
                    const double *B, long long ldb, double *Y, long long ldy, long long nrhs, hipStream_t st)
{
    if (rows <= 0 || nrhs <= 0) return 0;
    for (long long j = 0; j < nrhs; j += 65535) {
        const unsigned nb = (unsigned)(nrhs - j < 65535 ? nrhs - j : 65535);
        hipLaunchKernelGGL(k_spmv, dim3((rows + 255) / 256, nb), dim3(256), 0, st, rows, ptr, idx, vpos, Ax, X + j * ldx, ldx,
                           B ? B + j * ldb : nullptr, ldb, Y + j * ldy, ldy);
    }
    return (int)hipGetLastError();
}
int stm_launch_colnorm2(long long rows, const double *X, long long ldx, int ncols, double *out, hipStream_t st)
{
    if (ncols <= 0) return 0;
    hipLaunchKernelGGL(k_colnorm2, dim3(ncols), dim3(256), 0, st, rows, X, ldx, out);
    return (int)hipGetLastError();
}
int stm_launch_add_cols(int rows, int ncols, const double *D, long long ldd, double *X, long long ldx, hipStream_t st)
{
    if (rows <= 0 || ncols <= 0) return 0;
    hipLaunchKernelGGL(k_add_cols, dim3((rows + 255) / 256, ncols), dim3(256), 0, st, rows, D, ldd, X, ldx);
    return (int)hipGetLastError();
}
