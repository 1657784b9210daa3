// stmmqr_lsrobust.hip -- robust least squares by iteratively reweighted solves (stmmqr_ls_solve_robust, stmmqr_ls_robust_weights,
// stmmqr_median_abs): everything between two solves, on the device.
//   k_lsr_resid    r_i = b_i - sum_j A_ij x_j with A's UNWEIGHTED values, a thread per row over the row form the feature keeps (row
//                  pointers; by rows the columns and the positions in A's storage).  A row is summed in ascending column order in
//                  one accumulator.  A thread per row, as k_spmv: the rows of a least-squares matrix hold a handful of entries (the
//                  one-entry rows of syn_star beside its one row of 54), so a wave per row would leave nearly all of its lanes
//                  idle on nearly every row, and its lane sums would need a butterfly per row; the one long row (54 entries in
//                  syn_star) costs one lane 54 dependent steps while the kernel is bound by the gathers of the other rows anyway.
//   k_lsr_abs      a_i = |w0_i * r_i| (w0 NULL: |r_i|), one multiplication
//   k_lsr_hist / k_lsr_pick / k_lsr_above / k_lsr_median   the exact order statistics lo = a_(floor((c - 1) / 2)) and
//                  hi = a_(floor(c / 2)) over the c entries whose mask is not 0, by a radix select on the 64-bit pattern of the
//                  non-negative doubles (monotone): 8 passes of 8 bits from the top.  A pass is two launches chained on the stream:
//                  k_lsr_hist counts the digit of every key that shares the prefix chosen so far (read from device memory) into 256
//                  bins, k_lsr_pick (one wave) finds the bin that holds the rank, extends the prefix and leaves the rank inside
//                  that bin.  No workgroup waits for another.  The keys of a fit share their exponent, so in the leading passes a
//                  wave sees one to three digits: the wave counts by digit -- up to 4 rounds of (digit of the first lane left,
//                  ballot of its equals, ONE LDS add of the population count by that lane) -- and only lanes still left after
//                  those add for themselves.  The workgroup's 256 counts go to the pass's global bins with one integer atomic per
//                  non-empty bin: counts do not depend on the order.  The select keeps the number of keys below lo and equal to lo,
//                  so hi = lo when (below + equal) > floor(c / 2); otherwise hi is the smallest key above lo (k_lsr_above: an
//                  integer minimum).  k_lsr_median writes 0.5 * (lo + hi), lo, hi, c.  NaNs sort last and are not searched for.
//   k_lsr_weights  u = a / sigma, w_i = w0_i * f(u), rho(u) for the five losses (L2, Huber, Cauchy, Tukey, smoothed L1), with
//                  sigma = max(mad_factor * median, sigma_min) read from the selection's result, or a given one; sigma == 0: w = w0
//                  and rho = 0, no division is formed.  Per workgroup: the sum of rho (lanes by wave_sum, waves in order) and the
//                  two counts (rows with w == 0 although w0 != 0; rows with f == 1).
//   k_lsr_wsum     the partial sums in a fixed order by one workgroup; the eight statistics of a reweighting
//   k_lsr_step     max |x - xprev| and max |x| as the bits of non-negative doubles (integer maxima: order-independent)
//   k_lsr_scale    dst[p] = w[idx[p]] * src[p] (idx NULL: w[p]): the weighted values and right-hand side of the plain object
// No atomics on doubles; every floating-point sum has a fixed order, so a call gives the same bits run after run.  The weight
// functions are evaluated without contraction to fused multiply-adds: the same operations in the same order on the host give the
// same bits (divisions and square roots are correctly rounded), log1p to its last bits.
#include <algorithm>
#include <cfloat>

#include "stmmqr_kdev.h"

#define LSR_NT 256
#define LSR_BINS 256                    // == LSR_NT: a thread per bin
#define LSR_PASSES 8
#define LSR_ROUNDS 4
// the selection's words (unsigned long long): [0] the leading 8 * pass bits of lo found so far, [1] the rank inside the keys that
// share them, [2] c, [3] keys below them, [4] keys that share them, [5] the smallest key above lo, [6..7] spare, then the bins of
// the eight passes
#define LSR_HDR 8

namespace {

__device__ __forceinline__ unsigned long long key_of(double v) { return (unsigned long long)__double_as_longlong(v); }

__global__ __launch_bounds__(LSR_NT) void k_lsr_resid(long long m, const int *__restrict__ rp, const int *__restrict__ rj,
                                                      const int *__restrict__ rq, const double *__restrict__ Ax,
                                                      const double *__restrict__ x, const double *__restrict__ b, double *__restrict__ r)
{
    const long long i = (long long)blockIdx.x * LSR_NT + threadIdx.x;
    if (i >= m) return;
    double s = 0.0;
    for (int q = rp[i]; q < rp[i + 1]; q++) s += Ax[(long long)rq[q]] * x[rj[q]];
    r[i] = b[i] - s;
}

__global__ __launch_bounds__(LSR_NT) void k_lsr_abs(long long m, const double *__restrict__ w0, const double *__restrict__ r,
                                                    double *__restrict__ a)
{
    const long long i = (long long)blockIdx.x * LSR_NT + threadIdx.x;
    if (i >= m) return;
    a[i] = fabs(w0 ? w0[i] * r[i] : r[i]);
}

__global__ __launch_bounds__(LSR_NT) void k_lsr_hist(long long len, const double *__restrict__ a, const double *__restrict__ mask, int pass,
                                                     unsigned long long *sel)
{
    __shared__ unsigned int s_h[LSR_BINS];
    const int tid = threadIdx.x, lane = tid & 63;
    s_h[tid] = 0;
    __syncthreads();
    const unsigned long long prefix = sel[0];
    const int shift = 56 - 8 * pass;
    for (long long i0 = (long long)blockIdx.x * LSR_NT; i0 < len; i0 += (long long)gridDim.x * LSR_NT) {      // (uniform in the workgroup)
        const long long i = i0 + tid;
        bool live = i < len;
        unsigned long long key = 0;
        if (live) {
            key = key_of(a[i]);
            live = (!mask || mask[i] != 0.0) && (pass == 0 || (key >> (shift + 8)) == prefix);
        }
        const int d = (int)((key >> shift) & (LSR_BINS - 1));
        unsigned long long todo = __ballot(live);
        for (int round = 0; round < LSR_ROUNDS && todo; round++) {                                        // (uniform in the wave)
            const int src = __ffsll((long long)todo) - 1;
            const int d0 = __shfl(d, src, 64);
            const unsigned long long same = __ballot(live && d == d0);
            if (lane == src) atomicAdd(&s_h[d0], (unsigned int)__popcll(same));
            live = live && d != d0;
            todo &= ~same;
        }
        if (live) atomicAdd(&s_h[d], 1u);
    }
    __syncthreads();
    const unsigned int c = s_h[tid];
    if (c) atomicAdd(&sel[LSR_HDR + LSR_BINS * pass + tid], (unsigned long long)c);
}

// one wave: lane l holds the bins 4 l .. 4 l + 3
__global__ __launch_bounds__(64) void k_lsr_pick(int pass, unsigned long long *sel)
{
    const int lane = threadIdx.x;
    const unsigned long long *h = sel + LSR_HDR + LSR_BINS * pass + 4 * lane;
    const unsigned long long c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3], s = c0 + c1 + c2 + c3;
    unsigned long long inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    const unsigned long long total = __shfl(inc, 63, 64);
    unsigned long long rank = total ? (total - 1) / 2 : 0, prefix = 0, below = 0;
    if (pass > 0) { prefix = sel[0]; rank = sel[1]; below = sel[3]; }
    unsigned long long e = inc - s;
    if (pass == 0 && lane == 0) { sel[2] = total; sel[5] = ~0ull; }
    if (total && rank >= e && rank < inc) {                 // one lane
        int d = 4 * lane;
        unsigned long long cnt = c0;
        if (rank >= e + cnt) { e += cnt; d++; cnt = c1; }
        if (rank >= e + cnt) { e += cnt; d++; cnt = c2; }
        if (rank >= e + cnt) { e += cnt; d++; cnt = c3; }
        sel[0] = (prefix << 8) | (unsigned long long)d;
        sel[1] = rank - e;
        sel[3] = below + e;
        sel[4] = cnt;
    }
}

__global__ __launch_bounds__(LSR_NT) void k_lsr_above(long long len, const double *__restrict__ a, const double *__restrict__ mask,
                                                      unsigned long long *sel)
{
    __shared__ unsigned long long s_mn[LSR_NT / 64];
    const unsigned long long lo = sel[0], c = sel[2];
    if (c == 0 || sel[3] + sel[4] > c / 2) return;          // hi == lo (every workgroup alike)
    const int tid = threadIdx.x;
    unsigned long long mn = ~0ull;
    for (long long i = (long long)blockIdx.x * LSR_NT + tid; i < len; i += (long long)gridDim.x * LSR_NT) {
        const unsigned long long key = key_of(a[i]);
        if ((!mask || mask[i] != 0.0) && key > lo && key < mn) mn = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(mn, o, 64);
        if (y < mn) mn = y;
    }
    if ((tid & 63) == 0) s_mn[tid >> 6] = mn;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < LSR_NT / 64; k++) if (s_mn[k] < mn) mn = s_mn[k];
        if (mn != ~0ull) atomicMin(&sel[5], mn);
    }
}

__global__ void k_lsr_median(const unsigned long long *__restrict__ sel, double *__restrict__ out)
{
    const unsigned long long c = sel[2];
    double lo = 0.0, hi = 0.0;
    if (c > 0) {
        lo = __longlong_as_double((long long)sel[0]);
        hi = (sel[3] + sel[4] > c / 2) ? lo : __longlong_as_double((long long)sel[5]);
    }
    out[0] = 0.5 * (lo + hi); out[1] = lo; out[2] = hi; out[3] = (double)c;
}

// f(u) and rho(u) of the five losses; no contraction (see the head of the file)
__device__ __forceinline__ void loss_of(int loss, double cc, double u, double &f, double &rho)
{
#pragma clang fp contract(off)
    const double t = u / cc, t2 = t * t;
    switch (loss) {
    case 1:
        f = (u <= cc) ? 1.0 : sqrt(cc / u);
        rho = (u <= cc) ? (u * u) / 2.0 : cc * (u - cc / 2.0);
        break;
    case 2:
        f = 1.0 / sqrt(1.0 + t2);
        rho = ((cc * cc) / 2.0) * log1p(t2);
        break;
    case 3: {
        const double g = 1.0 - t2;
        f = (u < cc) ? g : 0.0;
        rho = (u < cc) ? ((cc * cc) / 6.0) * (1.0 - (g * g) * g) : (cc * cc) / 6.0;
        break;
    }
    case 4:
        f = 1.0 / sqrt(fmax(u, cc));
        rho = (u >= cc) ? u : (u * u) / (2.0 * cc) + cc / 2.0;
        break;
    default:
        f = 1.0;
        rho = (u * u) / 2.0;
    }
}

__global__ __launch_bounds__(LSR_NT) void k_lsr_weights(long long m, const double *__restrict__ a, const double *__restrict__ w0,
                                                        const double *__restrict__ med, double sigma_given, double mad_factor,
                                                        double sigma_min, int loss, double cc, double *__restrict__ w,
                                                        double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double s_red[LSR_NT / 64];
    const double sigma = fmax(med ? mad_factor * med[0] : sigma_given, sigma_min);
    const long long i = (long long)blockIdx.x * LSR_NT + threadIdx.x;
    double rho = 0.0, rej = 0.0, unit = 0.0;
    if (i < m) {
        const double w0i = w0 ? w0[i] : 1.0;
        double f = 1.0;
        if (sigma != 0.0) loss_of(loss, cc, a[i] / sigma, f, rho);
        const double wi = w0i * f;
        w[i] = wi;
        rej = (wi == 0.0 && w0i != 0.0) ? 1.0 : 0.0;
        unit = (f == 1.0) ? 1.0 : 0.0;
    }
    rho = block_sum<LSR_NT>(rho, s_red);
    rej = block_sum<LSR_NT>(rej, s_red);                    // (whole numbers: exact)
    unit = block_sum<LSR_NT>(unit, s_red);
    if (threadIdx.x == 0) {
        double *p = part + 3 * (long long)blockIdx.x;
        p[0] = rho; p[1] = rej; p[2] = unit;
    }
}

__global__ __launch_bounds__(LSR_NT) void k_lsr_wsum(long long nb, const double *__restrict__ part, const double *__restrict__ med,
                                                     double sigma_given, double mad_factor, double sigma_min, double *__restrict__ stat)
{
#pragma clang fp contract(off)
    __shared__ double s_red[LSR_NT / 64];
    double rho = 0.0, rej = 0.0, unit = 0.0;
    for (long long k = threadIdx.x; k < nb; k += LSR_NT) { rho += part[3 * k]; rej += part[3 * k + 1]; unit += part[3 * k + 2]; }
    rho = block_sum<LSR_NT>(rho, s_red);
    rej = block_sum<LSR_NT>(rej, s_red);
    unit = block_sum<LSR_NT>(unit, s_red);
    if (threadIdx.x == 0) {
        const double sigma = fmax(med ? mad_factor * med[0] : sigma_given, sigma_min);
        stat[0] = sigma;
        stat[1] = med ? med[1] : 0.0; stat[2] = med ? med[2] : 0.0; stat[3] = med ? med[3] : 0.0;
        stat[4] = rho; stat[5] = rej; stat[6] = unit;
        stat[7] = (sigma == 0.0) ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(LSR_NT) void k_lsr_step(long long n, const double *__restrict__ x, const double *__restrict__ xprev,
                                                     unsigned long long *out)
{
    __shared__ unsigned long long s_mx[2][LSR_NT / 64];
    const int tid = threadIdx.x;
    unsigned long long dx = 0, ax = 0;
    for (long long j = (long long)blockIdx.x * LSR_NT + tid; j < n; j += (long long)gridDim.x * LSR_NT) {
        const double xj = x[j];
        const unsigned long long kd = key_of(fabs(xj - xprev[j])), ka = key_of(fabs(xj));
        if (kd > dx) dx = kd;
        if (ka > ax) ax = ka;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long yd = __shfl_xor(dx, o, 64), ya = __shfl_xor(ax, o, 64);
        if (yd > dx) dx = yd;
        if (ya > ax) ax = ya;
    }
    if ((tid & 63) == 0) { s_mx[0][tid >> 6] = dx; s_mx[1][tid >> 6] = ax; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < LSR_NT / 64; k++) {
            if (s_mx[0][k] > dx) dx = s_mx[0][k];
            if (s_mx[1][k] > ax) ax = s_mx[1][k];
        }
        if (dx) atomicMax(&out[0], dx);
        if (ax) atomicMax(&out[1], ax);
    }
}

__global__ __launch_bounds__(LSR_NT) void k_lsr_scale(long long len, const int *__restrict__ idx, const double *__restrict__ w,
                                                      const double *__restrict__ src, double *__restrict__ dst)
{
    const long long p = (long long)blockIdx.x * LSR_NT + threadIdx.x;
    if (p >= len) return;
    dst[p] = w[idx ? (long long)idx[p] : p] * src[p];
}

__global__ __launch_bounds__(LSR_NT) void k_lsr_fill(long long len, double v, double *__restrict__ dst)
{
    const long long p = (long long)blockIdx.x * LSR_NT + threadIdx.x;
    if (p < len) dst[p] = v;
}

inline unsigned blocks_of(long long len) { return (unsigned)((len + LSR_NT - 1) / LSR_NT); }
inline unsigned capped_blocks(long long len) { return (unsigned)std::max<long long>(1, std::min<long long>((len + LSR_NT - 1) / LSR_NT, 1024)); }

}  // namespace

long long stm_lsr_sel_words() { return LSR_HDR + (long long)LSR_BINS * LSR_PASSES; }
long long stm_lsr_part_doubles(long long m) { return 3 * std::max<long long>(1, (m + LSR_NT - 1) / LSR_NT); }

int stm_launch_lsr_resid(long long m, const int *rp, const int *rj, const int *rq, const double *Ax, const double *x, const double *b,
                         double *r, hipStream_t st)
{
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_lsr_resid, dim3(blocks_of(m)), dim3(LSR_NT), 0, st, m, rp, rj, rq, Ax, x, b, r);
    return (int)hipGetLastError();
}

int stm_launch_lsr_abs(long long m, const double *w0, const double *r, double *a, hipStream_t st)
{
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_lsr_abs, dim3(blocks_of(m)), dim3(LSR_NT), 0, st, m, w0, r, a);
    return (int)hipGetLastError();
}

int stm_launch_lsr_select(long long len, const double *a, const double *mask, unsigned long long *sel, double *out, hipStream_t st)
{
    CK(hipMemsetAsync(sel, 0, (size_t)stm_lsr_sel_words() * sizeof(unsigned long long), st));
    const unsigned nb = capped_blocks(len);
    for (int pass = 0; pass < LSR_PASSES; pass++) {
        hipLaunchKernelGGL(k_lsr_hist, dim3(nb), dim3(LSR_NT), 0, st, len, a, mask, pass, sel);
        hipLaunchKernelGGL(k_lsr_pick, dim3(1), dim3(64), 0, st, pass, sel);
    }
    hipLaunchKernelGGL(k_lsr_above, dim3(nb), dim3(LSR_NT), 0, st, len, a, mask, sel);
    hipLaunchKernelGGL(k_lsr_median, dim3(1), dim3(1), 0, st, sel, out);
    return (int)hipGetLastError();
}

int stm_launch_lsr_weights(long long m, const double *a, const double *w0, const double *med, double sigma_given, double mad_factor,
                           double sigma_min, int loss, double cc, double *w, double *part, double *stat, hipStream_t st)
{
    const long long nb = m > 0 ? (long long)blocks_of(m) : 0;
    if (nb > 0)
        hipLaunchKernelGGL(k_lsr_weights, dim3((unsigned)nb), dim3(LSR_NT), 0, st, m, a, w0, med, sigma_given, mad_factor, sigma_min, loss, cc, w,
                           part);
    hipLaunchKernelGGL(k_lsr_wsum, dim3(1), dim3(LSR_NT), 0, st, nb, part, med, sigma_given, mad_factor, sigma_min, stat);
    return (int)hipGetLastError();
}

int stm_launch_lsr_step(long long n, const double *x, const double *xprev, double *out, hipStream_t st)
{
    CK(hipMemsetAsync(out, 0, 2 * sizeof(double), st));
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_lsr_step, dim3(capped_blocks(n)), dim3(LSR_NT), 0, st, n, x, xprev, (unsigned long long *)out);
    return (int)hipGetLastError();
}

int stm_launch_lsr_scale(long long len, const int *idx, const double *w, const double *src, double *dst, hipStream_t st)
{
    if (len <= 0) return 0;
    hipLaunchKernelGGL(k_lsr_scale, dim3(blocks_of(len)), dim3(LSR_NT), 0, st, len, idx, w, src, dst);
    return (int)hipGetLastError();
}

int stm_launch_lsr_fill(long long len, double v, double *dst, hipStream_t st)
{
    if (len <= 0) return 0;
    hipLaunchKernelGGL(k_lsr_fill, dim3(blocks_of(len)), dim3(LSR_NT), 0, st, len, v, dst);
    return (int)hipGetLastError();
}
