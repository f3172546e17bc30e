// k_lim.h -- the device helpers of the limiter's tile (k_lim_tile.h, which k_lim.hip, k_limtp.hip and k_limrel.hip
// instantiate): the exact division, the two detectors' gain of one frame (the sample detector's lim_gain, the true-peak
// detector's FIR in pair form and limtp_gain), the 64-bit product of one sample, and a stream seen as one sequence across
// the seam between its history slot and the run's slot (k_lim_tile.h describes the decomposition).
#ifndef CMHIP_K_LIM_H
#define CMHIP_K_LIM_H

#include "cmhip_device.h"

namespace cmhip {

constexpr u32 LIM_R = (LIM_TILE_MAX + LIM_HALO_MAX) / LIM_BLOCK;     // without a release: 26 elements per thread at most

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

// the sample detector: g of a frame whose largest magnitude is `peak`
__device__ __forceinline__ u32 lim_gain(u32 peak, u32 drive, u32 T)
{
    const u32 pr = (peak * drive + 4095u) >> 12;     // <= 65535 * 32768 + 4095 < 2^31
    return pr <= T ? LIM_UNITY : lim_div(T << 15, pr);
}

__device__ __forceinline__ u32 lim_abs(int x) { return (u32)(x < 0 ? -x : x); }
__device__ __forceinline__ int lim_lo(u32 w) { return (int)(short)(w & 0xffffu); }
__device__ __forceinline__ int lim_hi(u32 w) { return (int)w >> 16; }

// the true-peak detector (k_lim_tile.h describes the pair form)
constexpr u32 limtp_pair(unsigned p, unsigned i)
{
    return (u32)(uint16_t)tp_h(p, 2 * i + 1) | ((u32)(uint16_t)tp_h(p, 2 * i) << 16);
}

__device__ __forceinline__ int limtp_dot2(u32 x, u32 k, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, k), acc, false);
}

// t <= 16571 * 32768 < 2^30; drive * t < 2^46 (v_mad_u64_u32); pr <= 1 060 528 < 2^21
__device__ __forceinline__ u32 limtp_gain(u32 t, u32 drive, u32 T)
{
    const u32 pr = (u32)(((u64)drive * (u64)t + ((1ull << 25) - 1ull)) >> 25);
    return pr <= T ? LIM_UNITY : lim_div(T << 15, pr);
}

// max(|y_0|, .., |y_3|) at local frame t of the dwords d, channel c (pair(t, c): x_c[t-1] | x_c[t] << 16)
template <class Pair>
__device__ __forceinline__ u32 limtp_fir(Pair pair, u32 t, u32 c)
{
    int y[4] = {0, 0, 0, 0};
#pragma unroll
    for (u32 i = 0; i < TP_TAPS / 2; i++) {
        const u32 pr = pair(t - 2u * i, c);
        y[0] = limtp_dot2(pr, limtp_pair(0, i), y[0]);
        y[1] = limtp_dot2(pr, limtp_pair(1, i), y[1]);
        y[2] = limtp_dot2(pr, limtp_pair(2, i), y[2]);
        y[3] = limtp_dot2(pr, limtp_pair(3, i), y[3]);
    }
    return max(max(lim_abs(y[0]), lim_abs(y[1])), max(lim_abs(y[2]), lim_abs(y[3])));
}

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

// the g of vector w's frames (8 mono, 4 stereo) into LDS, 16 bytes at a time
template <int CT>
__device__ __forceinline__ void lim_put_g(u32 *L, u32 w, const u32 *g)
{
    u32x4 *Lv = reinterpret_cast<u32x4 *>(L);
    const u32x4 g0 = {g[0], g[1], g[2], g[3]};
    if constexpr (CT == 1) {
        const u32x4 g1 = {g[4], g[5], g[6], g[7]};
        Lv[2 * w] = g0;
        Lv[2 * w + 1] = g1;
    } else {
        Lv[w] = g0;
    }
}

// output vector v8 of the stream: whole where the count covers it, the ragged end through store_tail, nothing past it
__device__ __forceinline__ void lim_store(int16_t *outs, u32 v8, const u32 (&o)[4], u32 nfull, u32 ntail)
{
    if (v8 < nfull) {
        const u32x4 ov = {o[0], o[1], o[2], o[3]};
        __builtin_nontemporal_store(ov, reinterpret_cast<u32x4 *>(outs) + v8);
    } else if (v8 == nfull) {
        store_tail(outs, v8, o, ntail);
    }
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
