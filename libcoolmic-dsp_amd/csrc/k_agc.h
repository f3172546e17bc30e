// k_agc.h -- the leveller's tile bodies (k_agc.hip has the decomposition): a tile's context from the run's record, the
// energy pass and the apply pass.  k_agc.hip instantiates them for the leveller, k_automix.hip for the automixer, whose
// record keeps the count and the position in the leveller's places and whose gain nodes have the leveller's form.
// k_failover.hip instantiates the energy pass alone, with SLOTS: its rows' records name the input slot they read.
#pragma once

#include "cmhip_device.h"

namespace cmhip {

struct AgcTileCtx {                                  // a tile (wave-uniform)
    const int16_t *ins;
    int16_t *outs;
    AgcTile tl;
    AgcSpan sp;
    u32 s;
};

// false: the workgroup has no frames (uniform).  SLOTS (the failover switch's energy pass): row s of the records reads the
// input slot its record names in AREC_SLOT; its table row is still row s.
template <bool SLOTS = false>
__device__ __forceinline__ bool agc_tile_ctx(const AgcArgs &a, u32 C, AgcTileCtx &c)
{
    c.s = blockIdx.x / a.chunks;
    const u32 t = blockIdx.x - c.s * a.chunks;
    const u32 *rec = a.rec + (u64)c.s * AGC_REC;
    const u32 count = uniform(rec[AREC_COUNT]), pos_lo = uniform(rec[AREC_POS_LO]);
    c.tl = agc_tile(pos_lo, count, a.w, a.tile_log2, t);
    if (c.tl.fa >= c.tl.fb)
        return false;
    c.sp = agc_tile_span(c.tl.fa, c.tl.fb, C);
    if constexpr (SLOTS)
        c.ins = a.in + (u64)uniform(rec[AREC_SLOT]) * a.in_stride;
    else
        c.ins = a.in + (u64)c.s * a.in_stride;
    c.outs = a.out + (u64)c.s * a.out_stride;
    return true;
}

__device__ __forceinline__ u64 agc_sq(int x) { return (u64)(u32)(x * x); }

// ---------------------------------------------------------------------------
// energy.  CT: the channel count of the fast forms, 0 for the any-channel-count form.  NT threads, NV vectors each.
// lds (CT == 0 only): u64 [C][NT], a slot per thread and channel
template <int CT, u32 NT, u32 NV, bool SLOTS = false>
__device__ __forceinline__ void agc_energy_body(const AgcArgs &a, u64 *lds)
{
    const u32 C = CT ? (u32)CT : a.channels;
    AgcTileCtx c;
    if (!agc_tile_ctx<SLOTS>(a, C, c))
        return;
    const u32 tid = threadIdx.x;
    const AgcSpan sp = c.sp;
    const u32x4 *vin = reinterpret_cast<const u32x4 *>(c.ins);
    u64 *row = a.table + ((u64)c.s * a.nw + c.tl.win) * C;
    const u32 nh = sp.hend - sp.sa, nt = sp.sb - sp.tb;

    u32x4 x[NV];
#pragma unroll
    for (u32 j = 0; j < NV; j++) {
        const u32 v = sp.vb + tid + NT * j;
        x[j] = u32x4{0, 0, 0, 0};
        if (v < sp.ve)
            x[j] = __builtin_nontemporal_load(vin + v);
    }

    if constexpr (CT != 0) {
        u64 acc0 = 0, acc1 = 0;                      // (mono: acc0 alone)
#pragma unroll
        for (u32 j = 0; j < NV; j++) {
#pragma unroll
            for (u32 d = 0; d < 4; d++) {
                const u32 dw = x[j][d];
                const u64 lo = agc_sq((int)(short)dw), hi = agc_sq((int)dw >> 16);
                acc0 += lo;
                if constexpr (CT == 1)
                    acc0 += hi;
                else
                    acc1 += hi;
            }
        }
        // the ragged ends, a sample per lane
        u32 e = 0xffffffffu;
        if (tid < nh)
            e = sp.sa + tid;
        else if (tid - nh < nt)
            e = sp.tb + (tid - nh);
        if (e != 0xffffffffu) {
            const u64 q = agc_sq((int)c.ins[e]);
            if (CT == 1 || (e & 1u) == 0)
                acc0 += q;
            else
                acc1 += q;
        }
        const u64 t0 = wave_add_u40(acc0);           // (at most 34 squares per lane: below 2^36)
        if (tid == 0 && t0)
            atomicAdd(row, t0);
        if constexpr (CT == 2) {
            const u64 t1 = wave_add_u40(acc1);
            if (tid == 0 && t1)
                atomicAdd(row + 1, t1);
        }
    } else {
        for (u32 ch = 0; ch < C; ch++)
            lds[ch * NT + tid] = 0;
#pragma unroll
        for (u32 j = 0; j < NV; j++) {
            const u32 v = sp.vb + tid + NT * j;
            if (v < sp.ve) {
                u32 ch = (v * 8u) % C;
#pragma unroll
                for (u32 i = 0; i < 8; i++) {
                    const int xi = (int)(short)(x[j][i >> 1] >> (16u * (i & 1u)));
                    lds[ch * NT + tid] += agc_sq(xi);
                    ch = ch + 1u == C ? 0u : ch + 1u;
                }
            }
        }
        u32 e = 0xffffffffu;
        if (tid < nh)
            e = sp.sa + tid;
        else if (tid - nh < nt)
            e = sp.tb + (tid - nh);
        if (e != 0xffffffffu)
            lds[(e % C) * NT + tid] += agc_sq((int)c.ins[e]);
        __syncthreads();
        // a wave per channel in turn: the 256 slots of the channel, four per lane (below 2^37), then the wave
        const u32 wave = tid >> 6, lane = tid & 63u;
        for (u32 ch = wave; ch < C; ch += NT / 64u) {
            u64 v = 0;
#pragma unroll
            for (u32 q = 0; q < NT / 64u; q++)
                v += lds[ch * NT + lane + 64u * q];
            const u64 tot = wave_add_u40(v);
            if (lane == 0 && tot)
                atomicAdd(row + ch, tot);
        }
    }
}

// ---------------------------------------------------------------------------
// apply

// one sample of run frame f: the gain between the tile's nodes, the product, the clamp
__device__ __forceinline__ int agc_out(int x, u32 f, const AgcTile &tl, int a0, int diff, u32 w, u32 &clips)
{
    const int g = a0 + ((diff * (int)(tl.j + (f - tl.fa))) >> w);
    u32 clip;
    const int y = agc_sample(x, g, &clip);
    clips += clip;
    return y;
}

// lds (CT == 0 only): u32 [NT / 64], the waves' clip counts
template <int CT, u32 NT, u32 NV>
__device__ __forceinline__ void agc_apply_body(const AgcArgs &a, u32 *lds)
{
    const u32 C = CT ? (u32)CT : a.channels;
    AgcTileCtx c;
    if (!agc_tile_ctx(a, C, c))
        return;
    const u32 tid = threadIdx.x;
    const AgcSpan sp = c.sp;
    const u32x4 *vin = reinterpret_cast<const u32x4 *>(c.ins);
    u32x4 *vout = reinterpret_cast<u32x4 *>(c.outs);
    const u32 nh = sp.hend - sp.sa, nt = sp.sb - sp.tb;

    u32x4 x[NV];
#pragma unroll
    for (u32 j = 0; j < NV; j++) {
        const u32 v = sp.vb + tid + NT * j;
        x[j] = u32x4{0, 0, 0, 0};
        if (v < sp.ve)
            x[j] = __builtin_nontemporal_load(vin + v);
    }
    // the ragged ends, a sample per lane
    u32 e = 0xffffffffu;
    if (tid < nh)
        e = sp.sa + tid;
    else if (tid - nh < nt)
        e = sp.tb + (tid - nh);
    int xe = 0;
    if (e != 0xffffffffu)
        xe = (int)c.ins[e];

    // the window's two nodes, read only now: the tile's loads depend on the record alone and are on their way
    const u32 *nd = a.nodes + ((u64)c.s * (a.nw + 1u) + c.tl.win);
    const int a0 = (int)uniform(nd[0]), diff = (int)uniform(nd[1]) - a0;
    u32 clips = 0;

#pragma unroll
    for (u32 j = 0; j < NV; j++) {
        const u32 v = sp.vb + tid + NT * j;
        if (v < sp.ve) {
            u32 f = CT == 1 ? v * 8u : CT == 2 ? v * 4u : (v * 8u) / C;          // the frame of the vector's first sample
            u32 ch = CT ? 0u : v * 8u - f * C;
            u32 y[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 i = 0; i < 8; i++) {
                const int xi = (int)(short)(x[j][i >> 1] >> (16u * (i & 1u)));
                const u32 fi = CT == 1 ? f + i : CT == 2 ? f + (i >> 1) : f;
                const int yi = agc_out(xi, fi, c.tl, a0, diff, a.w, clips);
                y[i >> 1] |= ((u32)yi & 0xffffu) << (16u * (i & 1u));
                if constexpr (CT == 0) {
                    if (++ch == C) {
                        ch = 0;
                        f++;
                    }
                }
            }
            const u32x4 ov = {y[0], y[1], y[2], y[3]};
            __builtin_nontemporal_store(ov, vout + v);
        }
    }
    if (e != 0xffffffffu) {
        const u32 f = CT == 1 ? e : CT == 2 ? e >> 1 : e / C;
        c.outs[e] = (int16_t)agc_out(xe, f, c.tl, a0, diff, a.w, clips);
    }

    // clips: the wave, then the workgroup, then one add
    u32 total = wave_add_u32(clips);
    if constexpr (CT == 0) {
        if ((tid & 63u) == 0)
            lds[tid >> 6] = total;
        __syncthreads();
        total = 0;
#pragma unroll
        for (u32 q = 0; q < NT / 64u; q++)
            total += lds[q];
    }
    if (tid == 0 && total)
        atomicAdd(a.clips + c.s, (u64)total);
}

}  // namespace cmhip
