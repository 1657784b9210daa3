// stmmqr_nullspace.hip -- the dense tall-skinny part of the minimum-norm least-squares solution on rank-deficient factors
// (stmmqr_plan_nullspace, stmmqr_plan_project_minnorm).  With pc the live and jd the d dead pivot columns among the first ncol,
// W = R11^-1 R12 and N = [-W on pc; I on jd] (ncol x d, ld = ncol, R's column order; built column by column by the passes of
// stmmqr_rfactor.cpp), R N = 0 and
//     x_min = (I - N G^-1 N') x_basic,   G = N'N = I + W'W = L L'.
//   k_null_unit / k_null_scatter   the unit vectors of a batch of dead columns; column k of N = e_jd[k] - R \ (R e_jd[k])
//   k_null_refine                  N(live rows, k) -= R \ (R N(:, k)), the residual by k_rmult_dd (stmmqr_rmult.hip): one refinement step
//   k_null_gram / k_null_gram_sum  lower 32 x 32 tiles of N'N on the matrix cores: workgroup (tile, slab) multiplies the rows of one
//                                  slab and writes a partial tile, the second kernel adds the partial tiles in slab order
//   k_null_chol_panel              right-looking Cholesky, panel of 32 columns: a workgroup per block of 32 rows at or below the
//                                  diagonal.  EVERY workgroup factorizes the diagonal block itself in LDS (the same instructions in
//                                  the same order: the same bits, no hand-off through memory) and solves its own rows against it;
//                                  the first one stores the block into Ld, the array of the diagonal blocks (G's own stays as it
//                                  was while the others read it)
//   k_null_chol_update             lower tiles of the trailing matrix minus L21 L21' on the matrix cores
//   k_null_nt / k_null_nt_sum      T = N'X: a wave per column of N and slab, STM_NULL_RV vectors of a batch at a time
//   k_null_llt                     L L' z = t blocked by 32, a workgroup per vector: the triangle in LDS by one wave, the rows below
//                                  (forwards) a row per thread, the columns' dots (backwards) a wave per eight columns
//   k_null_sub                     X -= N z, a row per thread, the dot over d in index order
//   k_null_norm2                   squared 2-norms of the columns of an array
// Every sum has an order fixed by (ncol, d, slab height) alone and there is no atomic on data: a vector of a batch carries the bits of
// the one-vector call.  Offsets into N, G and the partial sums are 64-bit.
#include "stmmqr_kdev.h"

#define NL_NB STM_NULL_NB
#define NL_RV STM_NULL_RV
#define NL_KC 64                  // rows of a slab per pass through LDS (Gram)
#define NL_LS (NL_KC + 2)         // LDS stride of a column: the 32 lanes of a half-wave read 32 distinct doubles
static_assert(NL_NB == 32 && NT == 256, "the lane maps below are written for 32 x 32 tiles and four waves");

__global__ __launch_bounds__(NT) void k_null_unit(const int *__restrict__ jd, int k0, int nb, double *X, long long ldx)
{
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v < nb) X[jd[k0 + v] + (long long)v * ldx] = 1.0;
}

// N(:, k0 + v) = e - x of vector v of the batch (x = R \ (R e): zero on every dead column, which is written as exactly 0 / 1 here)
__global__ __launch_bounds__(NT) void k_null_scatter(const double *__restrict__ Xs, long long sx, const char *__restrict__ Rdead,
                                                     const int *__restrict__ jd, int k0, int ncol, double *__restrict__ N)
{
    const int j = blockIdx.x * NT + threadIdx.x, col = k0 + blockIdx.y;
    if (j >= ncol) return;
    const double v = (j == jd[col]) ? 1.0 : (Rdead[j] ? 0.0 : 0.0 - Xs[j + (long long)blockIdx.y * sx]);
    N[j + (long long)col * ncol] = v;
}

// N(j, k0 + v) -= x_v(j) on the live columns j: the refinement's correction (the dead rows keep their exact 0 / 1)
__global__ __launch_bounds__(NT) void k_null_refine(const double *__restrict__ Xs, long long sx, const char *__restrict__ Rdead, int k0,
                                                    int ncol, double *__restrict__ N)
{
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= ncol || Rdead[j]) return;
    N[j + (long long)(k0 + blockIdx.y) * ncol] -= Xs[j + (long long)blockIdx.y * sx];
}

// partial tile (ti, tj), ti >= tj, of N'N over the rows of slab blockIdx.z: wave (wi, wj) owns a 16 x 16 quarter, D[i][j] =
// sum_k N[k][ci + i] N[k][cj + j] with A[i = l15][k = l4], B[k = l4][j = l15], D[i = l4 + 4r][j = l15]
__global__ __launch_bounds__(NT) void k_null_gram(const double *__restrict__ N, int ncol, int d, int slab, double *__restrict__ Pt)
{
    __shared__ double As[NL_NB * NL_LS], Bs[NL_NB * NL_LS];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int wi = 16 * (wid >> 1), wj = 16 * (wid & 1);
    const long long r0 = (long long)blockIdx.z * slab, r1 = min((long long)ncol, r0 + slab);
    d4 acc = {0, 0, 0, 0};
    for (long long kc = r0; kc < r1; kc += NL_KC) {
        __syncthreads();                                   // the previous chunk has been read
        const long long row = kc + (tid & 63);
        const bool in = row < r1;
#pragma unroll
        for (int q = 0; q < NL_NB / NW; q++) {
            const int c = (tid >> 6) + NW * q, ca = ti * NL_NB + c, cb = tj * NL_NB + c;
            As[c * NL_LS + (tid & 63)] = (in && ca < d) ? N[row + (long long)ca * ncol] : 0.0;
            Bs[c * NL_LS + (tid & 63)] = (in && cb < d) ? N[row + (long long)cb * ncol] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < NL_KC / 4; kk++) {
            const int k = 4 * kk + l4;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(wi + l15) * NL_LS + k], Bs[(wj + l15) * NL_LS + k], acc, 0, 0, 0);
        }
    }
    const long long t = (long long)ti * (ti + 1) / 2 + tj;
    double *P = Pt + (t * gridDim.z + blockIdx.z) * (NL_NB * NL_NB);
#pragma unroll
    for (int r = 0; r < 4; r++) P[(wi + l4 + 4 * r) + NL_NB * (wj + l15)] = acc[r];
}
__global__ __launch_bounds__(NT) void k_null_gram_sum(const double *__restrict__ Pt, int nslab, int d, double *__restrict__ G)
{
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (tj > ti) return;
    const long long t = (long long)ti * (ti + 1) / 2 + tj;
    const double *P = Pt + t * nslab * (NL_NB * NL_NB);
    for (int e = threadIdx.x; e < NL_NB * NL_NB; e += NT) {
        const int gi = ti * NL_NB + (e & 31), gj = tj * NL_NB + (e >> 5);
        if (gi >= d || gj >= d) continue;
        double s = 0.0;
        for (int sl = 0; sl < nslab; sl++) s += P[(long long)sl * (NL_NB * NL_NB) + e];
        G[gi + (long long)gj * d] = s;
    }
}

// panel p (columns c0 = 32 p .. c0 + w - 1): workgroup b owns the rows c0 + 32 b ..; a pivot that is not positive and finite raises
// *err = 3 + 4 (its column + 1) (the first one stays)
__global__ __launch_bounds__(NT) void k_null_chol_panel(double *__restrict__ G, double *__restrict__ Ld, int d, int p, int *err)
{
    __shared__ double s[NL_NB][NL_NB + 1], a[NL_NB][NL_NB + 1];
    const int tid = threadIdx.x, c0 = p * NL_NB, w = min(NL_NB, d - c0), b = blockIdx.x;
    for (int e = tid; e < NL_NB * NL_NB; e += NT) {
        const int i = e & 31, j = e >> 5;
        s[i][j] = (i < w && j < w && i >= j) ? G[(c0 + i) + (long long)(c0 + j) * d] : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int j = 0; j < w; j++) {
        const double piv = s[j][j], ljj = sqrt(piv);
        if (b == 0 && tid == 0 && (!(piv > 0.0) || !isfinite(piv))) atomicCAS(err, 0, 3 + 4 * (c0 + j + 1));
        __syncthreads();                                   // everyone has read the pivot
        if (tid < NL_NB && tid >= j) s[tid][j] = (tid == j) ? ljj : s[tid][j] / ljj;
        __syncthreads();
        for (int e = tid; e < NL_NB * NL_NB; e += NT) {
            const int i = e & 31, k = e >> 5;
            if (k > j && i >= k) s[i][k] -= s[i][j] * s[k][j];
        }
        __syncthreads();
    }
    if (b == 0) {                                          // the diagonal block of L: lower triangle, the identity beyond w
        double *D = Ld + (long long)p * (NL_NB * NL_NB);
        for (int e = tid; e < NL_NB * NL_NB; e += NT) D[e] = s[e & 31][e >> 5];
        return;
    }
    // X L' = A for the 32 rows of this block: thread i owns row i, x_ij = (a_ij - sum_{k < j} x_ik l_jk) / l_jj
    const int r0 = c0 + b * NL_NB, nr = min(NL_NB, d - r0);
    for (int e = tid; e < NL_NB * NL_NB; e += NT) {
        const int i = e & 31, j = e >> 5;
        a[i][j] = (i < nr && j < w) ? G[(r0 + i) + (long long)(c0 + j) * d] : 0.0;
    }
    __syncthreads();
    if (tid < NL_NB) {
        for (int j = 0; j < w; j++) {
            double x = a[tid][j];
            for (int k = 0; k < j; k++) x -= a[tid][k] * s[j][k];
            a[tid][j] = x / s[j][j];
        }
    }
    __syncthreads();
    for (int e = tid; e < NL_NB * NL_NB; e += NT) {
        const int i = e & 31, j = e >> 5;
        if (i < nr && j < w) G[(r0 + i) + (long long)(c0 + j) * d] = a[i][j];
    }
}

// tile (ti, tj), p < tj <= ti, of the trailing matrix -= L(ti, p) L(tj, p)': the panel behind a trailing tile is 32 columns wide
__global__ __launch_bounds__(NT) void k_null_chol_update(double *__restrict__ G, int d, int p)
{
    const int ti = p + 1 + blockIdx.x, tj = p + 1 + blockIdx.y;
    if (tj > ti) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int ib = ti * NL_NB + 16 * (wid >> 1), jb = tj * NL_NB + 16 * (wid & 1), c0 = p * NL_NB;
    const int ra = ib + l15, rb = jb + l15, cj = jb + l15;
    d4 acc;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = ib + l4 + 4 * r;
        acc[r] = (i < d && cj < d) ? G[i + (long long)cj * d] : 0.0;
    }
#pragma unroll
    for (int kk = 0; kk < NL_NB / 4; kk++) {
        const long long col = (long long)(c0 + 4 * kk + l4) * d;
        const double av = G[min(ra, d - 1) + col], bv = G[min(rb, d - 1) + col];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ra < d ? -av : 0.0, rb < d ? bv : 0.0, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = ib + l4 + 4 * r;
        if (i < d && cj < d) G[i + (long long)cj * d] = acc[r];
    }
}

// partial sums of N(:, k)' X(:, v) over the rows of slab blockIdx.y: wave = column k, lanes stride the rows, NL_RV vectors at a time
__global__ __launch_bounds__(NT) void k_null_nt(const double *__restrict__ N, int ncol, int d, int slab, const double *__restrict__ X,
                                                long long ldx, int nb, double *__restrict__ Pt)
{
    const int lane = threadIdx.x & 63, k = blockIdx.x * NW + (threadIdx.x >> 6);
    if (k >= d) return;                                    // (a whole wave; the kernel has no barrier)
    const int v0 = blockIdx.z * NL_RV, nv = min(NL_RV, nb - v0);
    const long long r0 = (long long)blockIdx.y * slab, r1 = min((long long)ncol, r0 + slab);
    const double *Nk = N + (long long)k * ncol;
    double acc[NL_RV];
#pragma unroll
    for (int q = 0; q < NL_RV; q++) acc[q] = 0.0;
    for (long long row = r0 + lane; row < r1; row += 64) {
        const double a = Nk[row];
#pragma unroll
        for (int q = 0; q < NL_RV; q++) acc[q] += a * X[row + (long long)(v0 + min(q, nv - 1)) * ldx];
    }
#pragma unroll
    for (int q = 0; q < NL_RV; q++) {
        const double sm = wave_sum(acc[q]);
        if (lane == 0 && q < nv) Pt[((long long)(v0 + q) * gridDim.y + blockIdx.y) * d + k] = sm;
    }
}
__global__ __launch_bounds__(NT) void k_null_nt_sum(const double *__restrict__ Pt, int nslab, int d, double *__restrict__ T)
{
    const int k = blockIdx.x * NT + threadIdx.x;
    if (k >= d) return;
    const double *P = Pt + (long long)blockIdx.y * nslab * d;
    double s = 0.0;
    for (int sl = 0; sl < nslab; sl++) s += P[(long long)sl * d + k];
    T[k + (long long)blockIdx.y * d] = s;
}

// z <- (L L')^-1 z for vector blockIdx.x, in place in global memory (this workgroup alone touches it)
__global__ __launch_bounds__(NT) void k_null_llt(const double *__restrict__ L, const double *__restrict__ Ld, int d, double *T)
{
    __shared__ double s_t[NL_NB][NL_NB + 1];
    __shared__ double s_z[NL_NB];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 31;
    const int nt = (d + NL_NB - 1) / NL_NB;
    double *z = T + (long long)blockIdx.x * d;
    for (int p = 0; p < nt; p++) {                          // L y = t, forwards
        const int c0 = p * NL_NB, w = min(NL_NB, d - c0);
        for (int e = tid; e < NL_NB * NL_NB; e += NT) s_t[e & 31][e >> 5] = Ld[(long long)p * (NL_NB * NL_NB) + e];
        __syncthreads();
        if (wid == 0) {
            double a = (i < w) ? z[c0 + i] : 0.0, x = 0.0;
            for (int j = 0; j < w; j++) {
                const double xj = __shfl(a, j, 64) / s_t[j][j];
                if (i > j) a -= s_t[i][j] * xj;
                if (i == j) x = xj;
            }
            if (lane < NL_NB) { s_z[lane] = x; if (lane < w) z[c0 + lane] = x; }
        }
        __syncthreads();
        for (int row = c0 + NL_NB + tid; row < d; row += NT) {   // (rows below exist: the panel is 32 wide)
            double acc = z[row];
#pragma unroll
            for (int k = 0; k < NL_NB; k++) acc -= L[row + (long long)(c0 + k) * d] * s_z[k];
            z[row] = acc;
        }
        __syncthreads();
    }
    for (int p = nt - 1; p >= 0; p--) {                     // L' z = y, backwards
        const int c0 = p * NL_NB, w = min(NL_NB, d - c0);
        {                                                   // the dots of the panel's columns with the z below it: a wave takes eight
            double acc[NL_NB / NW];                         //  columns at once (rows below exist: the panel is 32 wide), lanes stride the rows
#pragma unroll
            for (int q = 0; q < NL_NB / NW; q++) acc[q] = 0.0;
            const double *Lw = L + (long long)(c0 + wid * (NL_NB / NW)) * d;
            for (int row = c0 + NL_NB + lane; row < d; row += 64) {
                const double zr = z[row];
#pragma unroll
                for (int q = 0; q < NL_NB / NW; q++) acc[q] += Lw[row + (long long)q * d] * zr;
            }
#pragma unroll
            for (int q = 0; q < NL_NB / NW; q++) {
                const double sm = wave_sum(acc[q]);
                if (lane == 0) s_z[wid * (NL_NB / NW) + q] = sm;
            }
        }
        for (int e = tid; e < NL_NB * NL_NB; e += NT) s_t[e & 31][e >> 5] = Ld[(long long)p * (NL_NB * NL_NB) + e];
        __syncthreads();
        if (wid == 0) {
            double a = (i < w) ? z[c0 + i] - s_z[i] : 0.0, x = 0.0;
            for (int j = w - 1; j >= 0; j--) {
                const double xj = __shfl(a, j, 64) / s_t[j][j];
                if (i < j) a -= s_t[j][i] * xj;
                if (i == j) x = xj;
            }
            if (lane < w) z[c0 + lane] = x;
        }
        __syncthreads();
    }
}

// X(row, v) -= sum_k N(row, k) T(k, v), k ascending
__global__ __launch_bounds__(NT) void k_null_sub(const double *__restrict__ N, int ncol, int d, const double *__restrict__ T, int nb,
                                                 double *X, long long ldx)
{
    const int row = blockIdx.x * NT + threadIdx.x;
    if (row >= ncol) return;
    const int v0 = blockIdx.y * NL_RV, nv = min(NL_RV, nb - v0);
    double acc[NL_RV];
#pragma unroll
    for (int q = 0; q < NL_RV; q++) acc[q] = 0.0;
    for (int k = 0; k < d; k++) {
        const double a = N[row + (long long)k * ncol];
#pragma unroll
        for (int q = 0; q < NL_RV; q++) acc[q] += a * T[k + (long long)(v0 + min(q, nv - 1)) * d];
    }
#pragma unroll
    for (int q = 0; q < NL_RV; q++)
        if (q < nv) X[row + (long long)(v0 + q) * ldx] -= acc[q];
}

__global__ __launch_bounds__(NT) void k_null_norm2(const double *__restrict__ A, long long lda, int n, double *__restrict__ out)
{
    __shared__ double s_red[NW];
    const double *a = A + (long long)blockIdx.x * lda;
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) v += a[i] * a[i];
    v = block_sum<NT>(v, s_red);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

int stm_launch_null_unit(const int *jd, int k0, int nb, double *X, long long ldx, hipStream_t st)
{
    if (nb <= 0) return 0;
    hipLaunchKernelGGL(k_null_unit, dim3((nb + NT - 1) / NT), dim3(NT), 0, st, jd, k0, nb, X, ldx);
    return (int)hipGetLastError();
}
int stm_launch_null_scatter(const double *Xs, long long sx, const char *Rdead, const int *jd, int k0, int nb, int ncol, double *N, hipStream_t st)
{
    if (nb <= 0 || ncol <= 0) return 0;
    hipLaunchKernelGGL(k_null_scatter, dim3((ncol + NT - 1) / NT, nb), dim3(NT), 0, st, Xs, sx, Rdead, jd, k0, ncol, N);
    return (int)hipGetLastError();
}
int stm_launch_null_refine(const double *Xs, long long sx, const char *Rdead, int k0, int nb, int ncol, double *N, hipStream_t st)
{
    if (nb <= 0 || ncol <= 0) return 0;
    hipLaunchKernelGGL(k_null_refine, dim3((ncol + NT - 1) / NT, nb), dim3(NT), 0, st, Xs, sx, Rdead, k0, ncol, N);
    return (int)hipGetLastError();
}
int stm_launch_null_gram(const double *N, int ncol, int d, int slab, int nslab, double *Pt, double *G, hipStream_t st)
{
    if (d <= 0) return 0;
    const int nt = (d + NL_NB - 1) / NL_NB;
    hipLaunchKernelGGL(k_null_gram, dim3(nt, nt, nslab), dim3(NT), 0, st, N, ncol, d, slab, Pt);
    CK(hipGetLastError());
    hipLaunchKernelGGL(k_null_gram_sum, dim3(nt, nt), dim3(NT), 0, st, Pt, nslab, d, G);
    return (int)hipGetLastError();
}
int stm_launch_null_chol_panel(double *G, double *Ld, int d, int p, int *err, hipStream_t st)
{
    const int nt = (d + NL_NB - 1) / NL_NB;
    if (p < 0 || p >= nt) return 0;
    hipLaunchKernelGGL(k_null_chol_panel, dim3(nt - p), dim3(NT), 0, st, G, Ld, d, p, err);
    return (int)hipGetLastError();
}
int stm_launch_null_chol_update(double *G, int d, int p, hipStream_t st)
{
    const int ntr = (d + NL_NB - 1) / NL_NB - p - 1;
    if (p < 0 || ntr <= 0) return 0;
    hipLaunchKernelGGL(k_null_chol_update, dim3(ntr, ntr), dim3(NT), 0, st, G, d, p);
    return (int)hipGetLastError();
}
int stm_launch_null_nt(const double *N, int ncol, int d, int slab, int nslab, const double *X, long long ldx, int nb, double *Pt, double *T,
                       hipStream_t st)
{
    if (d <= 0 || nb <= 0) return 0;
    hipLaunchKernelGGL(k_null_nt, dim3((d + NW - 1) / NW, nslab, (nb + NL_RV - 1) / NL_RV), dim3(NT), 0, st, N, ncol, d, slab, X, ldx, nb, Pt);
    CK(hipGetLastError());
    hipLaunchKernelGGL(k_null_nt_sum, dim3((d + NT - 1) / NT, nb), dim3(NT), 0, st, Pt, nslab, d, T);
    return (int)hipGetLastError();
}
int stm_launch_null_llt(const double *L, const double *Ld, int d, double *T, int nb, hipStream_t st)
{
    if (d <= 0 || nb <= 0) return 0;
    hipLaunchKernelGGL(k_null_llt, dim3(nb), dim3(NT), 0, st, L, Ld, d, T);
    return (int)hipGetLastError();
}
int stm_launch_null_sub(const double *N, int ncol, int d, const double *T, int nb, double *X, long long ldx, hipStream_t st)
{
    if (d <= 0 || nb <= 0 || ncol <= 0) return 0;
    hipLaunchKernelGGL(k_null_sub, dim3((ncol + NT - 1) / NT, (nb + NL_RV - 1) / NL_RV), dim3(NT), 0, st, N, ncol, d, T, nb, X, ldx);
    return (int)hipGetLastError();
}
int stm_launch_null_norm2(const double *A, long long lda, int n, int nb, double *out, hipStream_t st)
{
    if (nb <= 0) return 0;
    hipLaunchKernelGGL(k_null_norm2, dim3(nb), dim3(NT), 0, st, A, lda, n, out);
    return (int)hipGetLastError();
}
