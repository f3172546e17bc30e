// k_lim.h -- the device helpers the limiter's kernel files share (k_lim.hip, k_limtp.hip): the exact division, the
// 64-bit product of one sample, and a stream seen as one sequence across the seam between its history slot and the
// run's slot (k_lim.hip describes the decomposition).
#ifndef CMHIP_K_LIM_H
#define CMHIP_K_LIM_H

#include "cmhip_device.h"

namespace cmhip {

constexpr u32 LIM_R = (LIM_TILE_MAX + LIM_HALO_MAX) / LIM_BLOCK;     // 26 elements per thread at most

// floor(num / pr) for num = T << 15 (15 significant bits: exact as a float), T < pr <= 2^21 (exact as a float; the
// sample detector stays at or below 2^19, the true-peak detector below 2^21): the quotient is below 2^15, the reciprocal
// instruction (v_rcp_f32 / v_rcp_iflag_f32) is within one ulp and the product rounds once, so the estimate is less than
// 2^-6 away from the quotient and its floor at most one off, either way; one correction step each way makes it exact
// (tests/test_lim_host.py and tests/test_limtp_host.py run this form over every pr of their range for nine thresholds,
// the reciprocal one ulp low, exact, high)
__device__ __forceinline__ u32 lim_div(u32 num, u32 pr)
{
    u32 q = (u32)((float)num * __builtin_amdgcn_rcpf((float)pr));
    const int r = (int)(num - q * pr);               // in (-pr, 2 pr)
    if (r < 0)
        q -= 1u;
    else if ((u32)r >= pr)
        q += 1u;
    return q;
}

__device__ __forceinline__ u32 lim_abs(int x) { return (u32)(x < 0 ? -x : x); }
__device__ __forceinline__ int lim_lo(u32 w) { return (int)(short)(w & 0xffffu); }
__device__ __forceinline__ int lim_hi(u32 w) { return (int)w >> 16; }

// one sample: the 64-bit product (v_mad_i64_i32), exact; |y| <= T, so nothing is clamped
__device__ __forceinline__ u32 lim_apply(int x, u32 c)
{
    const long long y = ((long long)x * (long long)(int)c + (1ll << 26)) >> 27;
    return (u32)(int)y & 0xffffu;
}

// vector vv of the stream as a tile sees it: the history slot below 0, the run's slot from 0 on, zeros past the count
__device__ __forceinline__ void lim_load(u32 (&x)[4], const int16_t *ins, const int16_t *hs, u32 hv, int vv, u32 nfull,
                                         u32 ntail)
{
    if (vv < 0) {
        const u32x4 w = reinterpret_cast<const u32x4 *>(hs)[hv + vv];
        x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
    } else {
        const u32 v = (u32)vv;
        load_vec(x, ins, v, v < nfull, v == nfull && ntail != 0, ntail);
    }
}
// sample q of the same sequence (q >= -halo * C, below the count)
__device__ __forceinline__ int lim_sample(const int16_t *ins, const int16_t *hs, u32 hsamp, int q)
{
    return q < 0 ? hs[hsamp + q] : ins[q];
}

// the other history slot: the last halo frames of (old slot, the run's F frames)
__device__ __forceinline__ void lim_write_hist(const int16_t *ins, const int16_t *hs, int16_t *hn, u32 hsamp, u32 F, u32 C)
{
    const int first = (int)(F * C) - (int)hsamp;     // sample of the sequence that becomes sample 0 of the slot
    for (u32 i = threadIdx.x; i < hsamp; i += LIM_BLOCK)
        hn[i] = (int16_t)lim_sample(ins, hs, hsamp, first + (int)i);
}

}  // namespace cmhip
#endif
