// Self-test of the sized eight-sum butterfly (csrc/stmmqr_wave.h, wave_reduce8<NV>): built and run by
// tests/test_gpu_wave_sized.py.  One 64-thread workgroup; for NV = 1 .. 8 the sized and the unsized form reduce the same
// vectors, whose entries v[NV..7] are zero in the DATA (the unsized form cannot know it), and every lane l with
// red8_idx(l) < NV and every broadcast lane_bcast<red8_lane(x)>, x < NV, must hold the same bytes.  The entries are not
// integers and span 16 decades with mixed signs, so another order of the additions would round differently.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "stmmqr_wave.h"   // -I <package>/csrc

#define NVEC 384

template <int NV>
__global__ void k(const double *in, double *out_s, double *out_u, double *bc_s, double *bc_u)
{
    const int l = threadIdx.x;
    for (int e = 0; e < NVEC; e++) {
        double v[8];
        for (int x = 0; x < 8; x++) v[x] = in[((size_t)e * 64 + l) * 8 + x];
        const double rs = wave_reduce8<NV>(v), ru = wave_reduce8<8>(v);
        out_s[e * 64 + l] = rs;
        out_u[e * 64 + l] = ru;
        double *bs = bc_s + ((size_t)e * 64 + l) * 8, *bu = bc_u + ((size_t)e * 64 + l) * 8;
        for (int x = 0; x < 8; x++) bs[x] = bu[x] = 0.0;
        if constexpr (NV > 0) { bs[0] = lane_bcast<red8_lane(0)>(rs); bu[0] = lane_bcast<red8_lane(0)>(ru); }
        if constexpr (NV > 1) { bs[1] = lane_bcast<red8_lane(1)>(rs); bu[1] = lane_bcast<red8_lane(1)>(ru); }
        if constexpr (NV > 2) { bs[2] = lane_bcast<red8_lane(2)>(rs); bu[2] = lane_bcast<red8_lane(2)>(ru); }
        if constexpr (NV > 3) { bs[3] = lane_bcast<red8_lane(3)>(rs); bu[3] = lane_bcast<red8_lane(3)>(ru); }
        if constexpr (NV > 4) { bs[4] = lane_bcast<red8_lane(4)>(rs); bu[4] = lane_bcast<red8_lane(4)>(ru); }
        if constexpr (NV > 5) { bs[5] = lane_bcast<red8_lane(5)>(rs); bu[5] = lane_bcast<red8_lane(5)>(ru); }
        if constexpr (NV > 6) { bs[6] = lane_bcast<red8_lane(6)>(rs); bu[6] = lane_bcast<red8_lane(6)>(ru); }
        if constexpr (NV > 7) { bs[7] = lane_bcast<red8_lane(7)>(rs); bu[7] = lane_bcast<red8_lane(7)>(ru); }
    }
}

#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); return 2; } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double rnd01()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;      // xorshift64
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

template <int NV>
static int run(const double *d_in, double *d_s, double *d_u, double *d_bs, double *d_bu, const std::vector<double> &h,
               int &bad, int &inexact)
{
    const size_t n1 = (size_t)NVEC * 64, n8 = n1 * 8;
    std::vector<double> hin(h), rs(n1), ru(n1), bs(n8), bu(n8);
    for (size_t i = 0; i < n8; i++)
        if ((int)(i % 8) >= NV) hin[i] = 0.0;
    CHECK(hipMemcpy((void *)d_in, hin.data(), n8 * sizeof(double), hipMemcpyHostToDevice));
    k<NV><<<1, 64>>>(d_in, d_s, d_u, d_bs, d_bu);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(rs.data(), d_s, n1 * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ru.data(), d_u, n1 * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(bs.data(), d_bs, n8 * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(bu.data(), d_bu, n8 * sizeof(double), hipMemcpyDeviceToHost));
    for (int e = 0; e < NVEC; e++) {
        for (int l = 0; l < 64; l++) {
            const int idx = ((l >> 1) & 1) + 2 * (l & 1) + 4 * ((l >> 2) & 1);
            const size_t o = (size_t)e * 64 + l;
            if (idx < NV && memcmp(&rs[o], &ru[o], sizeof(double)) != 0) bad++;
            if (memcmp(&bs[o * 8], &bu[o * 8], 8 * sizeof(double)) != 0) bad++;          // (x >= NV: both written as zero)
            // the unsized form itself: every lane of a value holds one total, close to the plain sum and finite
            if (!std::isfinite(ru[o])) bad++;
            if (idx < NV && memcmp(&bu[o * 8 + idx], &ru[o], sizeof(double)) != 0) bad++;
        }
        // how often the data can tell two orders of addition apart: the left-to-right sum against the butterfly's
        for (int x = 0; x < NV; x++) {
            double s = 0.0;
            for (int l = 0; l < 64; l++) s += hin[((size_t)e * 64 + l) * 8 + x];
            const double got = bu[(size_t)e * 64 * 8 + x];
            if (s != got) inexact++;
            double mx = 0.0;
            for (int l = 0; l < 64; l++) mx = fmax(mx, fabs(hin[((size_t)e * 64 + l) * 8 + x]));
            if (fabs(s - got) > 64.0 * 2.3e-16 * 64.0 * mx) bad++;     // 63 additions of terms <= mx, twice over
        }
    }
    return 0;
}

int main()
{
    const size_t n1 = (size_t)NVEC * 64, n8 = n1 * 8;
    std::vector<double> h(n8);
    for (size_t i = 0; i < n8; i++) {
        const double mag = pow(10.0, -8.0 + 16.0 * rnd01());
        h[i] = ((rnd01() < 0.5) ? -1.0 : 1.0) * mag * (0.5 + 0.5 * rnd01());
    }
    double *d_in, *d_s, *d_u, *d_bs, *d_bu;
    CHECK(hipMalloc(&d_in, n8 * sizeof(double))); CHECK(hipMalloc(&d_s, n1 * sizeof(double))); CHECK(hipMalloc(&d_u, n1 * sizeof(double)));
    CHECK(hipMalloc(&d_bs, n8 * sizeof(double))); CHECK(hipMalloc(&d_bu, n8 * sizeof(double)));
    int bad = 0, inexact = 0, rc = 0;
    rc |= run<1>(d_in, d_s, d_u, d_bs, d_bu, h, bad, inexact); rc |= run<2>(d_in, d_s, d_u, d_bs, d_bu, h, bad, inexact);
    rc |= run<3>(d_in, d_s, d_u, d_bs, d_bu, h, bad, inexact); rc |= run<4>(d_in, d_s, d_u, d_bs, d_bu, h, bad, inexact);
    rc |= run<5>(d_in, d_s, d_u, d_bs, d_bu, h, bad, inexact); rc |= run<6>(d_in, d_s, d_u, d_bs, d_bu, h, bad, inexact);
    rc |= run<7>(d_in, d_s, d_u, d_bs, d_bu, h, bad, inexact); rc |= run<8>(d_in, d_s, d_u, d_bs, d_bu, h, bad, inexact);
    if (rc) return rc;
    // (of 36 * NVEC sums nearly all round differently in another order; a data set of exact sums would prove nothing)
    if (inexact < 18 * NVEC) { printf("sizedtest: the data does not separate orders of addition (%d)\n", inexact); return 3; }
    printf("sizedtest bad=%d (%d vectors per NV, %d of %d sums differ from the left-to-right order)\n", bad, NVEC, inexact, 36 * NVEC);
    return bad != 0;
}
