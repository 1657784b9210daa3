// stmmqr_selinv.hip -- diag((A'A)^-1) by selected inversion of R'R on the resident factors (stmmqr_plan_covariance_diag).
// The Takahashi / Erisman-Tinney recurrence walks the frontal tree from the root to the leaves.  Per front, with rm live pivots
// (compact list lc: the rule of k_rsolve / k_rbig_prep) and cn non-pivotal columns, R11 = F[0:rm, lc], R12 = F[0:rm, fp:fp+cn]:
//     Z_NN    gathered from the parent's block through Rjrel and the parent's position table (dead parent pivot: zero row / column)
//     [G | S] = R11^-1 [I | R12]
//     Z_PN    = -S Z_NN
//     Z_PP    = G G' - Z_PN S'
// and var[column of live pivot i] = Z_PP[i, i].  The front's block Z_f is (rm + cn)^2, column-major with ld = SiDesc::rmax + cn,
// live pivots first; [G | S] lives in a workspace of the tree level (ld = max(rmax, 1)).
//   k_si_prep    per front: lc, rm, the position table (live pivot: compact index, non-pivotal: rm + cj, anything else -1)
//   k_si_load    W = [I | R12]
//   k_si_gather  Z_NN from the parent's block
//   k_si_trsm    blocked back substitution, block rows of STM_SI_NB from the bottom up, a workgroup per strip of STM_SI_NB columns:
//                the diagonal triangle is solved in LDS (two columns per wave at a time), the rows above are updated on the matrix
//                cores.  The G strip of columns j.. starts at block row j: the rows below are zero and are never visited.
//   k_si_prod    tiled MFMA product, mode 0: Z_PN (and its mirror Z_NP), mode 1: Z_PP (tiles on and above the diagonal, mirrored)
//   k_si_diag    var[Qfill[Rj[..]]] = Z_PP[i, i]
// One launch per kernel and tree level (blockIdx.x: the front of the level, .y / .z: its strip or tile); a workgroup whose strip or tile lies outside its
// front returns at once.  Every sum has a fixed order (k ascending inside a tile, block rows descending in the substitution) that
// depends on the front alone: the same bits whatever shares the launch, no atomics on data.
// New kernels beside stmmqr_resident.hip's (no kernel there changes).
#include "stmmqr_kdev.h"

#define SI_NB STM_SI_NB
#define SI_T STM_SI_TILE
#define SI_KC STM_SI_KC
#define SI_LS (SI_T + 16)        // LDS row stride of the operand chunks: the 16-lane groups of an MFMA operand read fall on distinct banks
static_assert(SI_NB == 32 && SI_T == 64 && SI_KC == 16, "the lane maps below are written for these sizes");

__global__ __launch_bounds__(NT) void k_si_prep(DevCtx c, const SiDesc *__restrict__ sd, int *__restrict__ Lc, int *__restrict__ Pos,
                                                int *__restrict__ Rm, int *err)
{
    __shared__ int s_scan[NW];
    const int f = blockIdx.x, tid = threadIdx.x;
    const SiDesc d = sd[f];
    const FrontSym s = c.fs[f];
    const FrontNum nm = c.fnum[f];
    const int fp = d.fp, fm = nm.fm;
    const int *St = c.Stair + s.rp;
    int *lc = Lc + s.rp, *pos = Pos + s.rp;
    const int per = (fp + NT - 1) / NT;
    const int k0 = min(fp, tid * per), k1 = min(fp, k0 + per);
    int cnt = 0;
    for (int k = k0; k < k1; k++) cnt += (St[k] != 0);
    int total;
    const int incl = block_incl_scan(cnt, s_scan, &total);
    int q = incl - cnt;
    for (int k = k0; k < k1; k++) {
        const bool live = St[k] != 0 && q < fm;
        if (live) lc[q] = k;
        pos[k] = live ? q : -1;
        q += (St[k] != 0);
    }
    const int rm = max(0, min(total, fm));
    // (columns behind the view's pivots: the non-pivotal ones that take part, then whatever the ncol cut leaves out)
    for (int k = fp + tid; k < s.fn; k += NT) pos[k] = (k >= s.fp && k - s.fp < d.cn) ? rm + (k - s.fp) : -1;
    if (tid == 0) {
        Rm[f] = rm;
        if (d.check && rm != nm.rank) atomicExch(err, 1);   // (cannot happen: same rule as the factorization)
    }
}

// W (rm x (rm + cn)) = [I | R12]; blockIdx.y strides over the columns
__global__ __launch_bounds__(NT) void k_si_load(DevCtx c, const int *__restrict__ flist, const SiDesc *__restrict__ sd,
                                                const int *__restrict__ Rm, double *__restrict__ Wl)
{
    const int f = flist[blockIdx.x];
    const SiDesc d = sd[f];
    const FrontSym s = c.fs[f];
    const int rm = Rm[f], ncols = rm + d.cn;
    if (rm <= 0) return;
    const double *F = c.Farena + s.foff;
    double *W = Wl + d.woff;
    const long long ld = s.ld, ldw = max(d.rmax, 1);
    for (int col = blockIdx.y; col < ncols; col += gridDim.y) {
        if (col < rm) {
            for (int i = threadIdx.x; i < rm; i += NT) W[i + col * ldw] = (i == col) ? 1.0 : 0.0;
        } else {
            const double *src = F + (long long)(s.fp + col - rm) * ld;
            for (int i = threadIdx.x; i < rm; i += NT) W[i + col * ldw] = src[i];
        }
    }
}

// Z_NN of the front from its parent's block: column cj of the front's non-pivotal part is the parent's local column
// Rjrel[Rp[f] + fp + cj] (the map of k_rtsolve), whose position in the parent's block is Pos of the parent
__global__ __launch_bounds__(NT) void k_si_gather(DevCtx c, const int *__restrict__ flist, const SiDesc *__restrict__ sd,
                                                  const int *__restrict__ Rm, const int *__restrict__ Pos, double *__restrict__ Z)
{
    const int f = flist[blockIdx.x];
    const SiDesc d = sd[f];
    const int cn = d.cn;
    if (cn <= 0) return;
    const FrontSym s = c.fs[f];
    const int rm = Rm[f];
    const long long ldz = d.rmax + cn;
    double *Zf = Z + d.zoff;
    const int par = s.parent;
    const int *rel = c.Rjrel + s.rp + s.fp;
    const int *ppos = nullptr;
    const double *Zp = nullptr;
    long long ldp = 0;
    if (par >= 0) {
        const SiDesc pd = sd[par];
        ppos = Pos + c.fs[par].rp;
        Zp = Z + pd.zoff;
        ldp = pd.rmax + pd.cn;
    }
    for (int cj = blockIdx.y; cj < cn; cj += gridDim.y) {
        const int pj = ppos ? ppos[rel[cj]] : -1;
        for (int ci = threadIdx.x; ci < cn; ci += NT) {
            const int pi = ppos ? ppos[rel[ci]] : -1;
            Zf[(rm + ci) + (rm + cj) * ldz] = (pi >= 0 && pj >= 0) ? Zp[pi + pj * ldp] : 0.0;
        }
    }
}

// [G | S] = R11^-1 [I | R12] in place in W.  Workgroup (x, y): strip y of SI_NB columns of front x of the level.
__global__ __launch_bounds__(NT) void k_si_trsm(DevCtx c, const int *__restrict__ flist, const SiDesc *__restrict__ sd,
                                                const int *__restrict__ Rm, const int *__restrict__ Lc, double *__restrict__ Wl)
{
    __shared__ double s_tri[SI_NB][SI_NB + 1];
    __shared__ double s_x[SI_NB][SI_NB + 1];               // [row of the block][column of the strip]
    const int f = flist[blockIdx.x];
    const SiDesc d = sd[f];
    const int rm = Rm[f], ncols = rm + d.cn;
    const int c0 = blockIdx.y * SI_NB;
    if (rm <= 0 || c0 >= ncols) return;
    const FrontSym s = c.fs[f];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int ncs = min(SI_NB, ncols - c0);
    const double *F = c.Farena + s.foff;
    const int *lc = Lc + s.rp;
    double *W = Wl + d.woff;
    const long long ld = s.ld, ldw = max(d.rmax, 1);
    const int kb0 = (c0 < rm) ? c0 : ((rm - 1) / SI_NB) * SI_NB;
    for (int kb = kb0; kb >= 0; kb -= SI_NB) {
        const int nbk = min(SI_NB, rm - kb);
        for (int e = tid; e < SI_NB * SI_NB; e += NT) {
            const int i = e % SI_NB, j = e / SI_NB;
            // (unit diagonal beyond the block's rows: no division by zero, their x stays 0)
            s_tri[i][j] = (i < nbk && j < nbk && i <= j) ? F[(kb + i) + (long long)lc[kb + j] * ld] : (i == j ? 1.0 : 0.0);
            s_x[i][j] = (i < nbk && j < ncs) ? W[(kb + i) + (long long)(c0 + j) * ldw] : 0.0;
        }
        __syncthreads();
        // the triangle: half a wave per column, lane i owns row i; x_j for j = nbk-1 .. 0 (as k_rsolve)
#pragma unroll 1
        for (int pass = 0; pass < SI_NB / (2 * NW); pass++) {
            const int col = pass * 2 * NW + wid * 2 + (lane >> 5), i = lane & 31;
            double a = s_x[i][col], x = 0.0;
            for (int j = nbk - 1; j >= 0; j--) {
                const double aj = __shfl(a, (lane & 32) + j, 64);
                const double xj = aj / s_tri[j][j];
                if (i < j) a -= s_tri[i][j] * xj;
                if (i == j) x = xj;
            }
            s_x[i][col] = x;
        }
        __syncthreads();
        for (int e = tid; e < SI_NB * SI_NB; e += NT) {
            const int i = e % SI_NB, j = e / SI_NB;
            if (i < nbk && j < ncs) W[(kb + i) + (long long)(c0 + j) * ldw] = s_x[i][j];
        }
        // rows above the block: W(0:kb, strip) -= R11(0:kb, block) X, as D' = (-X)' R11' on the matrix cores: A[i = strip column][k],
        // B[k][j = row], D[i = l4 + 4r][j = l15] -- a wave takes 16 rows and both halves of the strip
        for (int it = wid; it < kb / 16; it += NW) {
            const int row = 16 * it + l15;
            d4 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j0 = l4 + 4 * r, j1 = 16 + l4 + 4 * r;
                acc0[r] = (j0 < ncs) ? W[row + (long long)(c0 + j0) * ldw] : 0.0;
                acc1[r] = (j1 < ncs) ? W[row + (long long)(c0 + j1) * ldw] : 0.0;
            }
#pragma unroll
            for (int kk = 0; kk < SI_NB / 4; kk++) {
                const int k = 4 * kk + l4;
                const double bv = F[row + (long long)lc[min(kb + k, rm - 1)] * ld];
                const double b = (k < nbk) ? bv : 0.0;
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-s_x[k][l15], b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-s_x[k][16 + l15], b, acc1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j0 = l4 + 4 * r, j1 = 16 + l4 + 4 * r;
                if (j0 < ncs) W[row + (long long)(c0 + j0) * ldw] = acc0[r];
                if (j1 < ncs) W[row + (long long)(c0 + j1) * ldw] = acc1[r];
            }
        }
        __syncthreads();                                   // (the next block row reads what the other waves stored)
    }
}

// C(i, j) = sum_k A(i, k) B(k, j), both operands with their first index contiguous: A(i, k) = pa[i + k lda], B(k, j) = pb[j + k ldb];
// `neg`: -A.  One K-chunk of SI_KC goes through registers into LDS (the next one is loaded while this one is multiplied).
struct SiOp { const double *pa, *pb; long long lda, ldb; int k0, k1, neg; };
struct SiChunk { double a[4], b[4]; };
__device__ __forceinline__ void si_chunk_load(SiChunk &ck, const SiOp &o, int kc, int i0, int j0, int M, int N, int tid)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int idx = tid + NT * q, x = idx & (SI_T - 1), k = kc + (idx >> 6);
        const bool kin = k < o.k1;
        const double av = (kin && i0 + x < M) ? o.pa[(i0 + x) + (long long)k * o.lda] : 0.0;
        ck.a[q] = o.neg ? -av : av;
        ck.b[q] = (kin && j0 + x < N) ? o.pb[(j0 + x) + (long long)k * o.ldb] : 0.0;
    }
}
__device__ __forceinline__ void si_product(const SiOp &o, int i0, int j0, int M, int N, double *As, double *Bs, d4 &c00, d4 &c01, d4 &c10,
                                           d4 &c11)
{
    if (o.k0 >= o.k1) return;                              // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int wi = 32 * (wid >> 1), wj = 32 * (wid & 1);
    SiChunk ck;
    si_chunk_load(ck, o, o.k0, i0, j0, M, N, tid);
    for (int kc = o.k0; kc < o.k1; kc += SI_KC) {
        __syncthreads();                                   // the previous chunk has been read
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int idx = tid + NT * q, x = idx & (SI_T - 1), k = idx >> 6;
            As[k * SI_LS + x] = ck.a[q];
            Bs[k * SI_LS + x] = ck.b[q];
        }
        __syncthreads();
        if (kc + SI_KC < o.k1) si_chunk_load(ck, o, kc + SI_KC, i0, j0, M, N, tid);
#pragma unroll
        for (int kk = 0; kk < SI_KC / 4; kk++) {
            const int k = 4 * kk + l4;
            const double a0 = As[k * SI_LS + wi + l15], a1 = As[k * SI_LS + wi + 16 + l15];
            const double b0 = Bs[k * SI_LS + wj + l15], b1 = Bs[k * SI_LS + wj + 16 + l15];
            c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c00, 0, 0, 0);
            c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c01, 0, 0, 0);
            c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c10, 0, 0, 0);
            c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c11, 0, 0, 0);
        }
    }
}
// store one 16 x 16 result (D[i = l4 + 4r][j = l15]) at C(i, j) = Zc[i + j ldz] and its mirror at Zm[j + i ldz]; `upper`: a tile on the
// diagonal of a symmetric block keeps i <= j only, so that both triangles hold the same bits
__device__ __forceinline__ void si_store(const d4 &v, int ib, int jb, int M, int N, double *Zc, double *Zm, long long ldz, bool upper, int lane)
{
    const int j = jb + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = ib + (lane >> 4) + 4 * r;
        if (i < M && j < N && (!upper || i <= j)) {
            Zc[i + (long long)j * ldz] = v[r];
            Zm[j + (long long)i * ldz] = v[r];
        }
    }
}

// mode 0: Z_PN = -S Z_NN (rm x cn) and its mirror.  Z_NN is read through its transpose: the block is symmetric to the bit (every
//         off-diagonal entry of a block is stored together with its mirror, and the gather copies entries).
// mode 1: Z_PP = G G' - Z_PN S' (rm x rm), tiles with tj >= ti; G(j, k) = 0 for k < j, so the first product starts at the tile's column.
// Workgroup (x, y, z): tile (y, z) of front x of the level.
__global__ __launch_bounds__(NT) void k_si_prod(DevCtx c, const int *__restrict__ flist, const SiDesc *__restrict__ sd,
                                                const int *__restrict__ Rm, const double *__restrict__ Wl, double *__restrict__ Z, int mode)
{
    __shared__ double As[SI_KC * SI_LS], Bs[SI_KC * SI_LS];
    const int f = flist[blockIdx.x];
    const SiDesc d = sd[f];
    const int rm = Rm[f], cn = d.cn;
    const int M = rm, N = mode ? rm : cn;
    const int i0 = blockIdx.y * SI_T, j0 = blockIdx.z * SI_T;
    if (i0 >= M || j0 >= N || (mode && j0 < i0)) return;
    const long long ldz = d.rmax + cn, ldw = max(d.rmax, 1);
    const double *W = Wl + d.woff;
    double *Zf = Z + d.zoff;
    const double *S = W + rm * ldw;                        // S(i, k) = S[i + k ldw]
    d4 c00 = {0, 0, 0, 0}, c01 = c00, c10 = c00, c11 = c00;
    SiOp o;
    if (mode == 0) {
        o.pa = S; o.lda = ldw; o.pb = Zf + rm + rm * ldz; o.ldb = ldz; o.k0 = 0; o.k1 = cn; o.neg = 1;
        si_product(o, i0, j0, M, N, As, Bs, c00, c01, c10, c11);
    } else {
        o.pa = W; o.lda = ldw; o.pb = W; o.ldb = ldw; o.k0 = j0; o.k1 = rm; o.neg = 0;
        si_product(o, i0, j0, M, N, As, Bs, c00, c01, c10, c11);
        o.pa = Zf + rm * ldz; o.lda = ldz; o.pb = S; o.ldb = ldw; o.k0 = 0; o.k1 = cn; o.neg = 1;
        si_product(o, i0, j0, M, N, As, Bs, c00, c01, c10, c11);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int ib = i0 + 32 * (wid >> 1), jb = j0 + 32 * (wid & 1);
    double *Zc = mode ? Zf : Zf + rm * ldz;                // C(i, j): Z_PP at (i, j), Z_PN at (i, rm + j)
    double *Zm = mode ? Zf : Zf + rm;                      // mirror:  Z_PP at (j, i), Z_NP at (rm + j, i)
    const bool up = mode && i0 == j0;
    si_store(c00, ib, jb, M, N, Zc, Zm, ldz, up, lane);
    si_store(c01, ib, jb + 16, M, N, Zc, Zm, ldz, up, lane);
    si_store(c10, ib + 16, jb, M, N, Zc, Zm, ldz, up, lane);
    si_store(c11, ib + 16, jb + 16, M, N, Zc, Zm, ldz, up, lane);
}

// var[caller's column of live pivot i] = Z_PP[i, i]
__global__ __launch_bounds__(NT) void k_si_diag(DevCtx c, const int *__restrict__ flist, const SiDesc *__restrict__ sd,
                                                const int *__restrict__ Rm, const int *__restrict__ Lc, const int *__restrict__ Rj,
                                                const int *__restrict__ Qfill, const double *__restrict__ Z, double *__restrict__ var)
{
    const int f = flist[blockIdx.x];
    const SiDesc d = sd[f];
    const FrontSym s = c.fs[f];
    const int i = blockIdx.y * NT + threadIdx.x;
    if (i >= Rm[f]) return;
    const long long ldz = d.rmax + d.cn;
    const int col = Rj[s.rp + Lc[s.rp + i]];
    var[Qfill ? Qfill[col] : col] = Z[d.zoff + i + i * ldz];
}

int stm_launch_si_prep(const DevCtx &c, int nf, const SiDesc *sd, int *Lc, int *Pos, int *Rm, int *err, hipStream_t st)
{
    if (nf <= 0) return 0;
    hipLaunchKernelGGL(k_si_prep, dim3(nf), dim3(NT), 0, st, c, sd, Lc, Pos, Rm, err);
    return (int)hipGetLastError();
}
// one tree level: max_r / max_cn = the largest SiDesc::rmax / cn of its fronts (grid sizes; symbolic)
int stm_launch_si_level(const DevCtx &c, const int *flist, int nfr, int max_r, int max_cn, const SiDesc *sd, const int *Rm, const int *Lc,
                        const int *Pos, const int *Rj, const int *Qfill, double *W, double *Z, double *var, hipStream_t st)
{
    if (nfr <= 0) return 0;
    if (max_cn > 0) {
        hipLaunchKernelGGL(k_si_gather, dim3(nfr, max_cn < 1024 ? max_cn : 1024), dim3(NT), 0, st, c, flist, sd, Rm, Pos, Z);
        CK(hipGetLastError());
    }
    if (max_r <= 0) return 0;
    const int tr = (max_r + SI_T - 1) / SI_T, tn = (max_cn + SI_T - 1) / SI_T;
    hipLaunchKernelGGL(k_si_load, dim3(nfr, max_r + max_cn < 1024 ? max_r + max_cn : 1024), dim3(NT), 0, st, c, flist, sd, Rm, W);
    CK(hipGetLastError());
    hipLaunchKernelGGL(k_si_trsm, dim3(nfr, (max_r + max_cn + SI_NB - 1) / SI_NB), dim3(NT), 0, st, c, flist, sd, Rm, Lc, W);
    CK(hipGetLastError());
    if (max_cn > 0) {
        hipLaunchKernelGGL(k_si_prod, dim3(nfr, tr, tn), dim3(NT), 0, st, c, flist, sd, Rm, W, Z, 0);
        CK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_si_prod, dim3(nfr, tr, tr), dim3(NT), 0, st, c, flist, sd, Rm, W, Z, 1);
    CK(hipGetLastError());
    hipLaunchKernelGGL(k_si_diag, dim3(nfr, (max_r + NT - 1) / NT), dim3(NT), 0, st, c, flist, sd, Rm, Lc, Rj, Qfill, Z, var);
    return (int)hipGetLastError();
}
