// k_dyn.h -- the device side of the dynamics stage's kernels (k_dyn.hip): the helpers and the tile body of the
// decomposition k_dyn.hip describes, with the detector's source and the detector as compile-time parameters (k_dyn.hip,
// "RMS", says why step 2 sums the squares in two halves).  KEYED = false: the level follows the stream's own frames
// (k_dyn<CT, DET>).  KEYED = true: step 1 takes its run slot, history slot and history vector base from stream key[s]
// (k_dynk<CT, DET>); step 3, step 4, the copy of a stream without frames, the curve and the meter stay stream s's own.
// A keyed stream and its key have equal counts (the host refuses a run otherwise), so one count bounds both.
#ifndef CMHIP_K_DYN_H
#define CMHIP_K_DYN_H

#include "cmhip_device.h"

namespace cmhip {

constexpr u32 DYN_R = (DYN_TILE_MAX + DYN_HALO_MAX) / DYN_BLOCK;     // 30 elements per thread at most

__device__ __forceinline__ u32 dyn_abs(int x) { return (u32)(x < 0 ? -x : x); }
__device__ __forceinline__ int dyn_lo(u32 w) { return (int)(short)(w & 0xffffu); }
__device__ __forceinline__ int dyn_hi(u32 w) { return (int)w >> 16; }

// one sample: |x * s| <= 2^15 * 2^15, the product and the rounding fit 32 bits; |y| <= |x|, so nothing is clamped
__device__ __forceinline__ u32 dyn_apply(int x, u32 s)
{
    const int y = (x * (int)s + (1 << 14)) >> 15;
    return (u32)y & 0xffffu;
}

// curve(l) from the packed table in LDS: dword k holds T[k] | T[k+1] << 16
__device__ __forceinline__ u32 dyn_lookup(const u32 *cv, u32 l)
{
    const DynIndex i = dyn_index(l);
    const u32 w = cv[i.idx];
    const int t0 = (int)(w & 0xffffu), t1 = (int)(w >> 16);
    return (u32)(t0 + (((t1 - t0) * (int)i.frac) >> i.sh));       // |product| < 2^27
}

// vector vv of the stream as a tile sees it: the history slot below 0, the run's slot from 0 on, zeros past the count
__device__ __forceinline__ void dyn_load(u32 (&x)[4], const int16_t *ins, const int16_t *hs, u32 hv, int vv, u32 nfull,
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
__device__ __forceinline__ int dyn_sample(const int16_t *ins, const int16_t *hs, u32 hsamp, int q)
{
    return q < 0 ? hs[hsamp + q] : ins[q];
}

// the other history slot: the last halo frames of (old slot, the run's F frames)
__device__ __forceinline__ void dyn_write_hist(const int16_t *ins, const int16_t *hs, int16_t *hn, u32 hsamp, u32 F, u32 C)
{
    const int first = (int)(F * C) - (int)hsamp;     // sample of the sequence that becomes sample 0 of the slot
    for (u32 i = threadIdx.x; i < hsamp; i += DYN_BLOCK)
        hn[i] = (int16_t)dyn_sample(ins, hs, hsamp, first + (int)i);
}

// the stream's curve into LDS, packed (threads 0..122; entry 123 is read into the high half of dword 122 and never used)
__device__ __forceinline__ void dyn_stage_curve(const uint16_t *c, u32 *cv)
{
    const u32 tid = threadIdx.x;
    if (tid < DYN_CURVE_USED)
        cv[tid] = (u32)c[tid] | (u32)c[tid + 1u] << 16;
}

// C: 1 or 2, or 0 for a run-time channel count; KEYED: the detector reads stream key[s] (key: uint32 [S], else unused);
// DET: DYN_DETECT_MEAN or DYN_DETECT_RMS
template <int CT, bool KEYED, u32 DET = DYN_DETECT_MEAN>
__device__ __forceinline__ void dyn_tile(const DynArgs &a, const u32 *key, u32 *L, u32 *cv, u32 *red)
{
    const u32 C = CT ? (u32)CT : a.channels;
    const u32 tid = threadIdx.x, tile = a.tile_frames, halo = a.halo;
    const u32 s = blockIdx.x / a.chunks;             // stream
    const u32 k = blockIdx.x - s * a.chunks;         // tile inside the stream
    u32 ks = s;                                      // the stream whose frames the detector reads
    if constexpr (KEYED)
        ks = key[s];                                 // (read first: the tile's loads wait for nothing else from memory)
    const u32 F = a.nframes ? a.nframes[s] : a.frames;
    const u32 f0 = k * tile;
    const u32 hsamp = halo * C, hv = hsamp >> 3;
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    int16_t *outs = a.out + (u64)s * a.out_stride;
    const int16_t *hs = a.hist + ((u64)a.parity * a.streams + s) * hsamp;
    int16_t *hn = a.hist + ((u64)(a.parity ^ 1u) * a.streams + s) * hsamp;
    const int16_t *kin = ins, *kh = hs;              // step 1's run slot and history slot
    if constexpr (KEYED) {
        kin = a.in + (u64)ks * a.in_stride;
        kh = a.hist + ((u64)a.parity * a.streams + ks) * hsamp;
    }
    if (f0 >= F) {                                   // (uniform)
        if (F == 0 && k == 0)                        // a stream without frames keeps its history across the flip
            dyn_write_hist(ins, hs, hn, hsamp, 0, C);
        return;
    }
    const u32 nt = min(tile, F - f0);                // the tile's frames
    const u32 N = halo + tile;
    const u32 ns = F * C, nfull = ns >> 3, ntail = ns & 7u;
    const uint16_t *curve = a.curve + (u64)s * DYN_CURVE;

    // ---- 1. e of frames f0 - halo .. f0 + tile - 1
    if constexpr (CT != 0) {
        constexpr u32 FPV = 8u / (u32)CT;            // frames per vector
        constexpr u32 VPT = (DYN_R * (u32)CT + 7u) / 8u;     // vectors per thread at most: 4 (mono), 8 (stereo)
        const u32 NV = N / FPV;
        const int vbase = (int)((f0 * C) >> 3) - (int)hv;
        u32 x[VPT][4];
#pragma unroll
        for (u32 i = 0; i < VPT; i++) {
            const u32 w = tid + DYN_BLOCK * i;
            x[i][0] = x[i][1] = x[i][2] = x[i][3] = 0;
            if (w < NV)
                dyn_load(x[i], kin, kh, hv, vbase + (int)w, nfull, ntail);
        }
        // the stream's curve, read only now: the tile's loads depend on kernel arguments alone and are on their way
        __builtin_amdgcn_sched_barrier(0);
        dyn_stage_curve(curve, cv);
        u32x4 *Lv = reinterpret_cast<u32x4 *>(L);
#pragma unroll
        for (u32 i = 0; i < VPT; i++) {
            const u32 w = tid + DYN_BLOCK * i;
            if (w < NV) {
                u32 e[8];
#pragma unroll
                for (u32 d = 0; d < 4; d++) {
                    const u32 lo = dyn_abs(dyn_lo(x[i][d])), hi = dyn_abs(dyn_hi(x[i][d]));
                    if constexpr (CT == 1) {
                        e[2 * d] = lo;
                        e[2 * d + 1] = hi;
                    } else {
                        e[d] = max(lo, hi);
                    }
                }
                const u32x4 e0 = {e[0], e[1], e[2], e[3]};
                if constexpr (CT == 1) {
                    const u32x4 e1 = {e[4], e[5], e[6], e[7]};
                    Lv[2 * w] = e0;
                    Lv[2 * w + 1] = e1;
                } else {
                    Lv[w] = e0;
                }
            }
        }
    } else {
        dyn_stage_curve(curve, cv);
        for (u32 j = tid; j < N; j += DYN_BLOCK) {
            const int p = (int)(f0 + j) - (int)halo;         // frame
            u32 peak = 0;
            if (p < (int)F)
                for (u32 c = 0; c < C; c++)
                    peak = max(peak, dyn_abs(dyn_sample(kin, kh, hsamp, p * (int)C + (int)c)));
            L[j] = peak;
        }
    }
    __syncthreads();

    // ---- 2. boxcar sum over A, sliding maximum over W, the curve, boxcar sum over B: doubling, own elements in registers
    u32 v[DYN_R];
#pragma unroll
    for (u32 i = 0; i < DYN_R; i++) {
        const u32 j = tid + DYN_BLOCK * i;
        v[i] = j < N ? L[j] : 0u;
    }
    // (at entry LDS holds v and every thread is past its reads; the last pass of a sum shifts; a read needs no guard,
    // only the index is clamped: what an element without a partner or a slot past N takes reaches no frame of the tile)
    auto pass = [&](u32 dist, auto is_max, u32 shift) {
        u32 o[DYN_R];
#pragma unroll
        for (u32 i = 0; i < DYN_R; i++) {
            const u32 j = min(tid + DYN_BLOCK * i, N - 1u);
            o[i] = L[max(j, dist) - dist];
        }
        __syncthreads();
#pragma unroll
        for (u32 i = 0; i < DYN_R; i++) {
            const u32 j = tid + DYN_BLOCK * i;
            v[i] = (decltype(is_max)::value ? max(v[i], o[i]) : v[i] + o[i]) >> shift;
            if (j < N)
                L[j] = v[i];
        }
        __syncthreads();
    };
    const u32 W = a.W, la = a.a, lb = a.b;
    if constexpr (DET == DYN_DETECT_RMS) {
        // the mean square from two 32-bit sums: e^2 = hi * 2^15 + lo; the low halves go through the a passes first while e
        // waits in registers, then the high halves while sum_lo waits there; the two meet in dyn_mean_square, and the
        // root leaves L.  An element without a partner or a slot past N takes the same entries in both rounds, so it too
        // is a mean of A squares, at most 2^30.
        u32 w[DYN_R];
#pragma unroll
        for (u32 i = 0; i < DYN_R; i++) {
            const u32 j = tid + DYN_BLOCK * i;
            w[i] = v[i];
            v[i] = (w[i] * w[i]) & ((1u << DYN_SQ_SPLIT) - 1u);
            if (j < N)
                L[j] = v[i];
        }
        __syncthreads();
        for (u32 d = 1; d < (1u << la); d *= 2u)
            pass(d, std::false_type{}, 0);                   // sums below 2^25
#pragma unroll
        for (u32 i = 0; i < DYN_R; i++) {
            const u32 j = tid + DYN_BLOCK * i;
            const u32 hi = (w[i] * w[i]) >> DYN_SQ_SPLIT;
            w[i] = v[i];
            v[i] = hi;
            if (j < N)
                L[j] = v[i];
        }
        __syncthreads();
        for (u32 d = 1; d < (1u << la); d *= 2u)
            pass(d, std::false_type{}, 0);                   // sums at most 2^25
#pragma unroll
        for (u32 i = 0; i < DYN_R; i++) {
            const u32 j = tid + DYN_BLOCK * i;
            v[i] = dyn_isqrt(dyn_mean_square(v[i], w[i], la));
            if (j < N)
                L[j] = v[i];
        }
        __syncthreads();
    } else {
        for (u32 d = 1; d < (1u << la); d *= 2u)
            pass(d, std::false_type{}, 2u * d == (1u << la) ? la : 0u);     // sums below 2^26; leaves L
    }
    u32 P = 1;
    for (; 2u * P <= W; P *= 2u)
        pass(P, std::true_type{}, 0);
    if (W > P)
        pass(W - P, std::true_type{}, 0);                    // leaves l
#pragma unroll
    for (u32 i = 0; i < DYN_R; i++) {
        const u32 j = tid + DYN_BLOCK * i;
        v[i] = dyn_lookup(cv, min(v[i], DYN_UNITY));         // (the bound holds by construction; it keeps the index inside the table)
        if (j < N)
            L[j] = v[i];
    }
    __syncthreads();
    for (u32 d = 1; d < (1u << lb); d *= 2u)
        pass(d, std::false_type{}, 2u * d == (1u << lb) ? lb : 0u);     // sums at most 2^24; leaves s

    // ---- the gain meter: minimum of s over the tile's frames, one atomic per workgroup
    {
        u32 red_max = 0;                             // of 32768 - s
#pragma unroll
        for (u32 i = 0; i < DYN_R; i++) {
            const u32 j = tid + DYN_BLOCK * i;
            if (j >= halo && j < halo + nt)
                red_max = max(red_max, DYN_UNITY - v[i]);
        }
        red_max = wave_max_u32(red_max);
        if ((tid & 63u) == 0)
            red[tid >> 6] = red_max;
        __syncthreads();
        if (tid == 0) {
            const u32 m = max(max(red[0], red[1]), max(red[2], red[3]));
            if (m)
                atomicMin(a.gmin + s, DYN_UNITY - m);
        }
    }

    // ---- 3. y[n] = x[n - D] * s[n]: output vectors f0*C/8 .. of the tile
    const u32 D = (1u << lb) - 1u;
    const u32 vb = (f0 * C) >> 3, nv = (nt * C + 7u) >> 3;
    u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
    const u32 *Ls = L + halo;                        // s of the tile's frames
    if constexpr (CT != 0) {
        constexpr u32 FPV = 8u / (u32)CT;
        const u32 back = ((D + 1u) * C) >> 3;        // the delayed samples of vector v: CT of vector v - back ...
        for (u32 w = tid; w < nv; w += DYN_BLOCK) {
            const u32 v8 = vb + w;
            u32 x0[4], x1[4];
            dyn_load(x0, ins, hs, hv, (int)v8 - (int)back, nfull, ntail);
            dyn_load(x1, ins, hs, hv, (int)v8 - (int)back + 1, nfull, ntail);     // ... and the first 8 - CT of the next
            const u32x4 *sv = reinterpret_cast<const u32x4 *>(Ls + w * FPV);
            u32 o[4];
            if constexpr (CT == 1) {
                const u32x4 s0 = sv[0], s1 = sv[1];
                const u32 sf[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                const u32 xs[5] = {x0[0], x0[1], x0[2], x0[3], x1[0]};
#pragma unroll
                for (u32 d = 0; d < 4; d++)          // output samples 2d, 2d + 1 are input samples 2d + 1, 2d + 2
                    o[d] = dyn_apply(dyn_hi(xs[d]), sf[2 * d]) | dyn_apply(dyn_lo(xs[d + 1]), sf[2 * d + 1]) << 16;
            } else {
                const u32x4 s0 = sv[0];
                const u32 sf[4] = {s0.x, s0.y, s0.z, s0.w};
                const u32 xs[4] = {x0[1], x0[2], x0[3], x1[0]};
#pragma unroll
                for (u32 d = 0; d < 4; d++)
                    o[d] = dyn_apply(dyn_lo(xs[d]), sf[d]) | dyn_apply(dyn_hi(xs[d]), sf[d]) << 16;
            }
            if (v8 < nfull) {
                const u32x4 ov = {o[0], o[1], o[2], o[3]};
                __builtin_nontemporal_store(ov, dst + v8);
            } else if (v8 == nfull) {
                store_tail(outs, v8, o, ntail);
            }
        }
    } else {
        for (u32 w = tid; w < nv; w += DYN_BLOCK) {
            const u32 v8 = vb + w;
            u32 o[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 e = 0; e < 8; e++) {
                const u32 q = v8 * 8u + e;           // output sample of the stream
                if (q < ns) {
                    const u32 n = q / C;
                    const int x = dyn_sample(ins, hs, hsamp, (int)q - (int)(D * C));
                    o[e >> 1] |= dyn_apply(x, Ls[n - f0]) << (16u * (e & 1u));
                }
            }
            if (v8 < nfull) {
                const u32x4 ov = {o[0], o[1], o[2], o[3]};
                __builtin_nontemporal_store(ov, dst + v8);
            } else if (v8 == nfull) {
                store_tail(outs, v8, o, ntail);
            }
        }
    }

    // ---- 4. the stream's last tile leaves the history of the next run
    if (F <= f0 + tile)
        dyn_write_hist(ins, hs, hn, hsamp, F, C);
}

}  // namespace cmhip
#endif
