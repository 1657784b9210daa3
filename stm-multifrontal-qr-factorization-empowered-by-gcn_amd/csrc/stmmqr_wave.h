// Wave64 reduction primitives for gfx950 (DPP + v_permlane{16,32}_swap; no LDS crossbar traffic).
// Used by the Householder panel kernels: every column step of qr_front's dlarfg/dlarf pair (reference
// STMMQR/qr/qr_kernel.c:1359-1381, 1434-1609) needs one norm and up to seven v'c dot products summed over the
// whole workgroup, and that reduction is the critical path of the step.
#pragma once
#include <hip/hip_runtime.h>

// one DPP step of an fp64 butterfly: v + (v moved by the DPP control), both 32-bit halves moved separately
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi2, lo2);
}
template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) { return v + dpp_mov<CTRL>(v); }

// v(l) + v(l ^ 16): v_permlane16_swap exchanges the odd rows of one operand with the even rows of the other
__device__ __forceinline__ double xor16_add(double v)
{
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}
// v(l) + v(l ^ 32)
__device__ __forceinline__ double xor32_add(double v)
{
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}

// sum over the 64 lanes of a wave, result in every lane.  quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror give every lane the total of its row of 16; two permlane swaps combine the four rows.
__device__ __forceinline__ double wave_sum(double v)
{
    v = dpp_add<0xB1>(v);
    v = dpp_add<0x4E>(v);
    v = dpp_add<0x141>(v);
    v = dpp_add<0x140>(v);
    v = xor16_add(v);
    return xor32_add(v);
}

// sum over the lanes that share (lane & 7): row_ror:8 inside the rows of 16, then the two row exchanges
__device__ __forceinline__ double wave_sum_stride8(double v)
{
    v = dpp_add<0x128>(v);
    v = xor16_add(v);
    return xor32_add(v);
}

// Eight sums at once.  Each halving step exchanges one half of the values with a partner lane and keeps the
// other half (7 exchange-adds instead of 8 x 3); afterwards lane l holds the sum over its group of 8 lanes of
// value number  idx(l) = ((l>>1)&1) + 2*(l&1) + 4*((l>>2)&1),  and wave_sum_stride8 finishes the job:
// every lane l ends with the wave total of value idx(l).
__device__ __forceinline__ int red8_idx(int lane) { return ((lane >> 1) & 1) + 2 * (lane & 1) + 4 * ((lane >> 2) & 1); }
__device__ __forceinline__ constexpr int red8_lane(int x) { return ((x >> 1) & 1) + 2 * (x & 1) + 4 * ((x >> 2) & 1); }

// maximum of an int over the 64 lanes of the wave, in every lane
__device__ __forceinline__ int wave_max_int(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

//
// NV sizes the butterfly to the sums a caller has: v[NV .. 7] are zero by the caller's CODE (padding, not data) and are never
// read.  One exchange-add pairs a lower member (kept by the lanes on side 0) with an upper member (kept by side 1):
//   both live        : keep = side ? up : lo, send = side ? lo : up, keep + moved(send)   -- 4 selects, 2 DPP moves, 1 add
//   upper one zero   : lo + moved(lo) in EVERY lane                                       -- 2 DPP moves, 1 add
//   both zero        : the pair does not exist
// Side 0 of the middle form computes lo(l) + lo(partner), the expression the full form has there (its partner sends lo), so the
// lanes l with red8_idx(l) < NV end with the bits of the unsized butterfly.  Side 1, where the full form has 0 + 0, holds a
// value nobody may read: lanes with red8_idx(l) >= NV are UNSPECIFIED after wave_reduce8<NV>.  They never reach a specified
// lane: the side of a lane in a pair is one of the bits 0-2 of its number, and every later partner (l ^ 1, l ^ 2, row_ror:8,
// l ^ 16, l ^ 32) keeps the bit of an earlier pair.
// Instructions of the butterfly for NV = 8 .. 1: 49, 45, 41, 37, 33, 26, 19, 9.
template <int CTRL, bool HAVE_UP>
__device__ __forceinline__ double red8_pair(bool side, double lo, double up)
{
    if constexpr (HAVE_UP) {
        const double keep = side ? up : lo;
        const double send = side ? lo : up;
        return keep + dpp_mov<CTRL>(send);
    } else
        return dpp_add<CTRL>(lo);
}
template <int NV = 8>
__device__ __forceinline__ double wave_reduce8_partial(const double (&v)[8])
{
    static_assert(NV >= 1 && NV <= 8, "one to eight live sums");
    const int lane = threadIdx.x & 63;
    const bool sA = (lane >> 2) & 1, sB = lane & 1, sC = (lane >> 1) & 1;
    constexpr int N4 = NV < 4 ? NV : 4, N2 = NV < 2 ? NV : 2;      // live values after the first / second halving
    double n4[4] = {0.0, 0.0, 0.0, 0.0}, n2[2] = {0.0, 0.0};       // (entries past N4 / N2 are never read)
    // partner 7 - (l & 7): the other quad
    if constexpr (N4 > 0) n4[0] = red8_pair<0x141, (4 < NV)>(sA, v[0], v[4]);
    if constexpr (N4 > 1) n4[1] = red8_pair<0x141, (5 < NV)>(sA, v[1], v[5]);
    if constexpr (N4 > 2) n4[2] = red8_pair<0x141, (6 < NV)>(sA, v[2], v[6]);
    if constexpr (N4 > 3) n4[3] = red8_pair<0x141, (7 < NV)>(sA, v[3], v[7]);
    // partner l ^ 1
    if constexpr (N2 > 0) n2[0] = red8_pair<0xB1, (2 < N4)>(sB, n4[0], n4[2]);
    if constexpr (N2 > 1) n2[1] = red8_pair<0xB1, (3 < N4)>(sB, n4[1], n4[3]);
    // partner l ^ 2
    return red8_pair<0x4E, (1 < N2)>(sC, n2[0], n2[1]);
}
template <int NV = 8>
__device__ __forceinline__ double wave_reduce8(const double (&v)[8])
{
    return wave_sum_stride8(wave_reduce8_partial<NV>(v));
}
// The same with the count as a VALUE, for the index of a fully unrolled loop (not a constant expression of the language, a
// constant by the time the switch is simplified: one case is left in each copy of the loop body).
__device__ __forceinline__ double wave_reduce8_n(const double (&v)[8], int nv)
{
    switch (nv) {
    case 1: return wave_reduce8<1>(v);
    case 2: return wave_reduce8<2>(v);
    case 3: return wave_reduce8<3>(v);
    case 4: return wave_reduce8<4>(v);
    case 5: return wave_reduce8<5>(v);
    case 6: return wave_reduce8<6>(v);
    case 7: return wave_reduce8<7>(v);
    default: return wave_reduce8<8>(v);
    }
}

// A value that is the same in every lane although the compiler cannot prove it (loaded by every lane from one address,
// computed by every lane from the same operands), moved to scalar registers: what depends on it becomes scalar arithmetic
// and scalar branches, and a load it comes from is settled where the move stands.  (Only where that holds: the int and double
// forms return the first active lane's value, the bool form whether any active lane has it set.)
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double wave_uniform(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ bool wave_uniform(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; }
// Load of a double that nothing writes while the kernel runs, through the scalar cache into scalar registers (the
// constant address space: the address must be wave-uniform).
__device__ __forceinline__ double ld_uniform_const(const double *p)
{
    return *(const __attribute__((address_space(4))) double *)(unsigned long long)p;
}

// value of lane SRC (compile-time) in every lane, as a wave-uniform value
template <int SRC>
__device__ __forceinline__ double lane_bcast(double v)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), SRC),
                            __builtin_amdgcn_readlane(__double2loint(v), SRC));
}
