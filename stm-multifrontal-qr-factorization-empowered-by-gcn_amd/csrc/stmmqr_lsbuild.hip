// stmmqr_lsbuild.hip -- the values of [W A; D | W B; 0] for the damped least-squares object (stmmqr_ls_solve_damped), built on the
// device from (Ax, w, d, lambda, B), and |D x_j|_2 of its solution.  The matrix has m + n rows; column j of its first n holds A's
// entries in their given order and then the entry of row m + j, so entry p of A's storage (column j) sits at p + j and D_jj at
// Ap[j + 1] + j; the nrhs trailing columns are dense over all m + n rows.
//   k_lsb_values     val[p + j] = w[Ai[p]] * Ax[p] (w NULL: Ax[p]), a thread per entry of A.  One multiplication: the bits of the
//                    same product on the host.  The loads of Ax and Ai and the store run over p (the store shifted by the column
//                    number, which changes a few times per wave); w through Ai is the only gather.  The column of an entry is
//                    the last j with Ap[j] <= p, found by bisection of the int column pointers the object keeps on the device:
//                    log2(n + 1) loads of a table that stays in cache and that the neighbouring lanes read at the same places.
//                    No per-entry column table (it would double the ints the object holds) and no wave per run of columns (its
//                    balance would depend on the column lengths).
//   k_lsb_diag       D_jj = sl * s_j with s_j = d[j] or 1 (sl = sqrt(lambda), taken on the host), into D and val; a thread per column
//   k_lsb_marquardt  s_j = |W A(:, j)|_2 from the built values without the D entry, a wave per column: the largest magnitude by a
//                    butterfly, then the sum of the squared ratios (no overflow, no underflow to 0 of a column that has an entry);
//                    a zero column gets scale_min, every other norm is clamped to [scale_min, scale_max]; D_jj = sl * s_j
//   k_lsb_rhs        the B block in place after the caller's copy of B into its rows 0 .. m-1: w[i] * b for i < m, 0.0 below
//   k_lsb_dnorm      |D x_j|_2, a workgroup per column of X, the same two steps across the workgroup: lanes, then waves in order
// No atomics; every sum has a fixed order, so a call gives the same bits run after run.  Offsets into val are 64-bit.
#include <cfloat>

#include "stmmqr_kdev.h"

#define LSB_NT 256

namespace {

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(LSB_NT) void k_lsb_values(long long anz, int n, const int *__restrict__ ap, const int *__restrict__ ai,
                                                       const double *__restrict__ Ax, const double *__restrict__ w, double *__restrict__ val)
{
    const long long p = (long long)blockIdx.x * LSB_NT + threadIdx.x;
    if (p >= anz) return;
    int lo = 0, hi = n;                                 // ap[lo] <= p < ap[hi] throughout (ap[0] = 0, ap[n] = anz)
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long long)ap[mid] <= p) lo = mid; else hi = mid;
    }
    const double a = Ax[p];
    val[p + lo] = w ? w[ai[p]] * a : a;
}

__global__ __launch_bounds__(LSB_NT) void k_lsb_diag(int n, const int *__restrict__ ap, const double *d, double sl, double *D,
                                                     double *__restrict__ val)
{
    const int j = blockIdx.x * LSB_NT + threadIdx.x;
    if (j >= n) return;
    const double v = d ? sl * d[j] : sl;                // (d may be D itself: a host array of scales uploaded into it)
    D[j] = v;
    val[(long long)ap[j + 1] + j] = v;
}

__global__ __launch_bounds__(LSB_NT) void k_lsb_marquardt(int n, const int *__restrict__ ap, double sl, double smin, double smax,
                                                          double *__restrict__ D, double *val)
{
    const int j = blockIdx.x * (LSB_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n) return;                                 // (the whole wave)
    const int p0 = ap[j], p1 = ap[j + 1];
    const double *col = val + (long long)p0 + j;
    double mx = 0.0;
    for (int q = lane; q < p1 - p0; q += 64) mx = fmax(mx, fabs(col[q]));
    mx = wave_max(mx);
    double s = 0.0;
    if (mx > 0.0) {
        double ss = 0.0;
        for (int q = lane; q < p1 - p0; q += 64) { const double r = col[q] / mx; ss += r * r; }
        s = mx * sqrt(wave_sum(ss));
    }
    s = (s == 0.0) ? smin : fmin(fmax(s, smin), smax);
    if (lane == 0) {
        const double v = sl * s;
        D[j] = v;
        val[(long long)p1 + j] = v;
    }
}

__global__ __launch_bounds__(LSB_NT) void k_lsb_rhs(long long m, long long mn, const double *__restrict__ w, double *__restrict__ Bv)
{
    const long long i = (long long)blockIdx.x * LSB_NT + threadIdx.x;
    if (i >= mn) return;
    double *b = Bv + (long long)blockIdx.y * mn + i;
    if (i >= m) *b = 0.0;
    else if (w) *b = w[i] * *b;
}

__global__ __launch_bounds__(LSB_NT) void k_lsb_dnorm(int n, const double *__restrict__ D, const double *__restrict__ X, long long ldx,
                                                      double *__restrict__ out)
{
    __shared__ double s_red[LSB_NT / 64];
    const double *x = X + (long long)blockIdx.x * ldx;
    const int tid = threadIdx.x;
    double mx = 0.0;
    for (int j = tid; j < n; j += LSB_NT) mx = fmax(mx, fabs(D[j] * x[j]));
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_red[tid >> 6] = mx;
    __syncthreads();
    mx = 0.0;
#pragma unroll
    for (int k = 0; k < LSB_NT / 64; k++) mx = fmax(mx, s_red[k]);
    const double den = (mx > 0.0 && mx <= DBL_MAX) ? mx : 1.0;      // (all zero, or an infinity that stays one: unscaled)
    double ss = 0.0;
    for (int j = tid; j < n; j += LSB_NT) { const double r = (D[j] * x[j]) / den; ss += r * r; }
    ss = block_sum<LSB_NT>(ss, s_red);
    if (tid == 0) out[blockIdx.x] = den * sqrt(ss);
}

}  // namespace

int stm_launch_lsb_values(long long anz, int n, const int *ap, const int *ai, const double *Ax, const double *w, double *val, hipStream_t st)
{
    if (anz <= 0) return 0;
    hipLaunchKernelGGL(k_lsb_values, dim3((unsigned)((anz + LSB_NT - 1) / LSB_NT)), dim3(LSB_NT), 0, st, anz, n, ap, ai, Ax, w, val);
    return (int)hipGetLastError();
}

int stm_launch_lsb_diag(int n, const int *ap, const double *d, double sl, double *D, double *val, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_lsb_diag, dim3((unsigned)((n + LSB_NT - 1) / LSB_NT)), dim3(LSB_NT), 0, st, n, ap, d, sl, D, val);
    return (int)hipGetLastError();
}

int stm_launch_lsb_marquardt(int n, const int *ap, double sl, double smin, double smax, double *D, double *val, hipStream_t st)
{
    if (n <= 0) return 0;
    const int per = LSB_NT / 64;
    hipLaunchKernelGGL(k_lsb_marquardt, dim3((unsigned)((n + per - 1) / per)), dim3(LSB_NT), 0, st, n, ap, sl, smin, smax, D, val);
    return (int)hipGetLastError();
}

int stm_launch_lsb_rhs(long long m, long long n, int nrhs, const double *w, double *Bv, hipStream_t st)
{
    if (m + n <= 0 || nrhs <= 0) return 0;
    hipLaunchKernelGGL(k_lsb_rhs, dim3((unsigned)((m + n + LSB_NT - 1) / LSB_NT), (unsigned)nrhs), dim3(LSB_NT), 0, st, m, m + n, w, Bv);
    return (int)hipGetLastError();
}

int stm_launch_lsb_dnorm(int n, int nrhs, const double *D, const double *X, long long ldx, double *out, hipStream_t st)
{
    if (nrhs <= 0) return 0;
    hipLaunchKernelGGL(k_lsb_dnorm, dim3((unsigned)nrhs), dim3(LSB_NT), 0, st, n, D, X, ldx, out);
    return (int)hipGetLastError();
}
