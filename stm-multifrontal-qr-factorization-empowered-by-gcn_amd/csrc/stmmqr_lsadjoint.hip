// stmmqr_lsadjoint.hip -- the kernels of the adjoint of the least-squares solve (stmmqr_ls_adjoint, stmmqr_ls.cpp).  With C = [W A; D]
// (the plain object: C = A), Bt = [W B; 0], x the solution, z = (C'C)^-1 xbar, rt = Bt - C x and ut = C z the gradient with respect
// to the stored entry (i, j) of C is g(i, j) = sum_k rt[i, k] z[j, k] - ut[i, k] x[j, k], k over the right-hand sides.
//   k_lsa_entries    g over the entries of A's storage and, for the damped layout, over the n entries of D: item p < anz is entry p of
//                    A (row ai[p], column j = the last one with ap[j] <= p, by the bisection of k_lsb_values: empty columns never
//                    match), Axbar[p] = w[ai[p]] * g (w NULL: g); item anz + j is D_jj (row m + j), Dbar[j] = g.  A thread per item;
//                    the sum runs over k ascending in one accumulator, two fused multiply-adds per k.  The four vectors are read
//                    through two strides (item stride, k stride), and the host gives them K-FASTEST for nrhs > 1 (k_lsa_kfast:
//                    row i of rt at rt[i * nrhs ..]), as they are for nrhs = 1.  Why: the inner length is 2 nrhs <= 128 and the
//                    kernel is bound by the gather of the rows of rt and ut through ai.  Column-major, a thread touches nrhs cache
//                    lines per array and uses 8 bytes of each; k-fastest it reads nrhs * 8 contiguous bytes per array (whole lines
//                    from nrhs = 16 on), and the rows of x and z are the same for the neighbouring lanes of a column (one fetch
//                    per wave and column).  A wave per run of entries with the lanes over k would idle 63 lanes of 64 at nrhs = 1
//                    and 32 at nrhs = 32, and would sum k in the order of a butterfly, not ascending.
//   k_lsa_kfast      out[i * K + k] = in[i + k * ld]: 64 rows per workgroup through LDS, reads along the rows, writes contiguous
//   k_lsa_pad        the (n + nrhs)-vectors the product with the plan's matrix [C | Bt] takes: V = [s * src; 0] or [s * src; e_k]
//   k_lsa_bbar       Bbar[i, k] = w[i] * ut[i, k], i < m
//   k_lsa_wbar       wbar[i] = 2 * (sum_k rt[i, k] ut[i, k]) / w[i], exactly 0.0 where w[i] == 0; w NULL: all 1
//   k_lsa_resid      res = xbar - t per column and |res|^2, |xbar|^2 (a workgroup per column: lanes, then waves in order)
// No atomics; every sum has a fixed order, so a call gives the same bits run after run, and a column of a batch the bits of the
// one-column call wherever the sum does not run over k.  Offsets into the vectors and the values are 64-bit.  An output that is NULL
// is not written: the launchers skip the items of a NULL output.
#include "stmmqr_kdev.h"

#define LSA_NT 256
#define LSA_TR 64                  // rows per workgroup of k_lsa_kfast
#define LSA_KMAX 64                // = STMMQR_LS_MAX_NRHS: the widest tile of k_lsa_kfast

namespace {

__device__ __forceinline__ double lsa_g(int K, const double *__restrict__ rt, const double *__restrict__ ut, long long sk_r,
                                        const double *__restrict__ z, const double *__restrict__ x, long long sk_c)
{
    double acc = 0.0;
    for (int k = 0; k < K; k++) {
        acc = fma(rt[k * sk_r], z[k * sk_c], acc);
        acc = fma(-ut[k * sk_r], x[k * sk_c], acc);
    }
    return acc;
}

// items first .. last-1 of the anz + n; m: the row of D_00.  Vectors: entry (i, k) of rt / ut at i * si_r + k * sk_r, entry (j, k) of
// x / z at j * si_c + k * sk_c
__global__ __launch_bounds__(LSA_NT) void k_lsa_entries(long long first, long long last, long long anz, int n, long long m, int K,
                                                        const int *__restrict__ ap, const int *__restrict__ ai,
                                                        const double *__restrict__ rt, const double *__restrict__ ut, long long si_r,
                                                        long long sk_r, const double *__restrict__ x, const double *__restrict__ z,
                                                        long long si_c, long long sk_c, const double *__restrict__ w,
                                                        double *__restrict__ Axbar, double *__restrict__ Dbar)
{
    const long long p = first + (long long)blockIdx.x * LSA_NT + threadIdx.x;
    if (p >= last) return;
    if (p >= anz) {                                     // D_jj
        const long long j = p - anz;
        Dbar[j] = lsa_g(K, rt + (m + j) * si_r, ut + (m + j) * si_r, sk_r, z + j * si_c, x + j * si_c, sk_c);
        return;
    }
    int lo = 0, hi = n;                                 // ap[lo] <= p < ap[hi] throughout (ap[0] = 0, ap[n] = anz)
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long long)ap[mid] <= p) lo = mid; else hi = mid;
    }
    const long long i = ai[p];
    const double g = lsa_g(K, rt + i * si_r, ut + i * si_r, sk_r, z + (long long)lo * si_c, x + (long long)lo * si_c, sk_c);
    Axbar[p] = w ? w[i] * g : g;
}

__global__ __launch_bounds__(LSA_NT) void k_lsa_kfast(long long rows, int K, const double *__restrict__ in, long long ld,
                                                      double *__restrict__ out)
{
    __shared__ double tile[LSA_TR * (LSA_KMAX + 1)];
    const long long i0 = (long long)blockIdx.x * LSA_TR;
    const int nr = (int)((rows - i0 < LSA_TR) ? rows - i0 : LSA_TR), tid = threadIdx.x;
    const int r = tid & (LSA_TR - 1);
    if (r < nr)
        for (int k = tid / LSA_TR; k < K; k += LSA_NT / LSA_TR) tile[r * (K + 1) + k] = in[i0 + r + (long long)k * ld];
    __syncthreads();
    for (int e = tid; e < nr * K; e += LSA_NT) out[i0 * K + e] = tile[(e / K) * (K + 1) + (e % K)];
}

__global__ __launch_bounds__(LSA_NT) void k_lsa_pad(int n, int na, const double *__restrict__ src, long long lds, double s, int unit0,
                                                    double *__restrict__ V)
{
    const int j = blockIdx.x * LSA_NT + threadIdx.x;
    if (j >= na) return;
    const long long k = blockIdx.y;
    double v = 0.0;
    if (j < n) v = s * src[j + k * lds];
    else if (unit0 >= 0 && j - n == unit0 + (int)k) v = 1.0;
    V[j + k * (long long)na] = v;
}

__global__ __launch_bounds__(LSA_NT) void k_lsa_bbar(long long m, const double *__restrict__ ut, long long ldu, const double *__restrict__ w,
                                                     double *__restrict__ Bbar, long long ldbb)
{
    const long long i = (long long)blockIdx.x * LSA_NT + threadIdx.x;
    if (i >= m) return;
    const long long k = blockIdx.y;
    const double u = ut[i + k * ldu];
    Bbar[i + k * ldbb] = w ? w[i] * u : u;
}

__global__ __launch_bounds__(LSA_NT) void k_lsa_wbar(long long m, int K, const double *__restrict__ rt, const double *__restrict__ ut,
                                                     long long ld, const double *__restrict__ w, double *__restrict__ wbar)
{
    const long long i = (long long)blockIdx.x * LSA_NT + threadIdx.x;
    if (i >= m) return;
    double s = 0.0;
    for (int k = 0; k < K; k++) s = fma(rt[i + k * ld], ut[i + k * ld], s);
    const double wi = w ? w[i] : 1.0;
    wbar[i] = (wi == 0.0) ? 0.0 : 2.0 * s / wi;
}

__global__ __launch_bounds__(LSA_NT) void k_lsa_resid(int n, const double *__restrict__ xbar, long long ldxb, const double *__restrict__ t,
                                                      long long ldt, double *__restrict__ res, long long ldr, double *__restrict__ out)
{
    __shared__ double s_red[LSA_NT / 64];
    const long long k = blockIdx.x;
    double sr = 0.0, sx = 0.0;
    for (int j = threadIdx.x; j < n; j += LSA_NT) {
        const double b = xbar[j + k * ldxb], d = b - t[j + k * ldt];
        res[j + k * ldr] = d;
        sr = fma(d, d, sr);
        sx = fma(b, b, sx);
    }
    sr = block_sum<LSA_NT>(sr, s_red);
    sx = block_sum<LSA_NT>(sx, s_red);
    if (out && threadIdx.x == 0) { out[2 * k] = sr; out[2 * k + 1] = sx; }
}

}  // namespace

int stm_launch_lsa_entries(long long anz, int n, long long m, int nrhs, const int *ap, const int *ai, const double *rt, const double *ut,
                           long long si_r, long long sk_r, const double *x, const double *z, long long si_c, long long sk_c,
                           const double *w, double *Axbar, double *Dbar, hipStream_t st)
{
    const long long first = Axbar ? 0 : anz, last = Dbar ? anz + n : anz;
    if (last <= first || nrhs <= 0) return 0;
    hipLaunchKernelGGL(k_lsa_entries, dim3((unsigned)((last - first + LSA_NT - 1) / LSA_NT)), dim3(LSA_NT), 0, st, first, last, anz, n, m, nrhs,
                       ap, ai, rt, ut, si_r, sk_r, x, z, si_c, sk_c, w, Axbar, Dbar);
    return (int)hipGetLastError();
}

int stm_launch_lsa_kfast(long long rows, int nrhs, const double *in, long long ld, double *out, hipStream_t st)
{
    if (rows <= 0 || nrhs <= 0) return 0;
    if (nrhs > LSA_KMAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lsa_kfast, dim3((unsigned)((rows + LSA_TR - 1) / LSA_TR)), dim3(LSA_NT), 0, st, rows, nrhs, in, ld, out);
    return (int)hipGetLastError();
}

int stm_launch_lsa_pad(int n, int na, int nb, const double *src, long long lds, double s, int unit0, double *V, hipStream_t st)
{
    if (na <= 0 || nb <= 0) return 0;
    hipLaunchKernelGGL(k_lsa_pad, dim3((unsigned)((na + LSA_NT - 1) / LSA_NT), (unsigned)nb), dim3(LSA_NT), 0, st, n, na, src, lds, s, unit0, V);
    return (int)hipGetLastError();
}

int stm_launch_lsa_bbar(long long m, int nrhs, const double *ut, long long ldu, const double *w, double *Bbar, long long ldbb, hipStream_t st)
{
    if (m <= 0 || nrhs <= 0 || !Bbar) return 0;
    hipLaunchKernelGGL(k_lsa_bbar, dim3((unsigned)((m + LSA_NT - 1) / LSA_NT), (unsigned)nrhs), dim3(LSA_NT), 0, st, m, ut, ldu, w, Bbar, ldbb);
    return (int)hipGetLastError();
}

int stm_launch_lsa_wbar(long long m, int nrhs, const double *rt, const double *ut, long long ld, const double *w, double *wbar, hipStream_t st)
{
    if (m <= 0 || !wbar) return 0;
    hipLaunchKernelGGL(k_lsa_wbar, dim3((unsigned)((m + LSA_NT - 1) / LSA_NT)), dim3(LSA_NT), 0, st, m, nrhs, rt, ut, ld, w, wbar);
    return (int)hipGetLastError();
}

int stm_launch_lsa_resid(int n, int nb, const double *xbar, long long ldxb, const double *t, long long ldt, double *res, long long ldr,
                         double *out, hipStream_t st)
{
    if (nb <= 0) return 0;
    hipLaunchKernelGGL(k_lsa_resid, dim3((unsigned)nb), dim3(LSA_NT), 0, st, n, xbar, ldxb, t, ldt, res, ldr, out);
    return (int)hipGetLastError();
}
