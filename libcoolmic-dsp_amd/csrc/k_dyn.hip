// k_dyn.hip -- gfx950 (MI355X, wave64) dynamics stage, compressor and gate: S streams of C interleaved int16 channels
// in, the same out, delayed by D = B - 1 frames and multiplied by a gain of at most unity that follows the level through
// a per-stream curve, in exact integers (include/coolmic_hip.h, "dynamics", has the arithmetic to the bit;
// csrc/dyn_plan.h the geometry and the curve's index function):
//     e = max_c |x[n][c]|                              L = (sum of e over the last A frames) >> a
//     l = max of L over the last W frames              g = curve(l)
//     s = (sum of g over the last B frames) >> b       y[n][ch] = (x[n-D][ch] * s[n] + 2^14) >> 15
//
//   k_dyn_fast<C>   C in {1, 2}: the tile's frames come in and leave as whole 16-byte vectors
//   k_dyn_any       3..16 channels: sample by sample; no speed goal
//   k_dyn_set       writes one curve, handed over as a kernel argument, into a range of streams
//
// The decomposition is k_lim.hip's.  A workgroup of 256 threads takes one stream and a tile of tile_frames frames, and
// evaluates N = halo + tile_frames frames: the tile's own and the halo in front of them, which are the stream's history
// slot where the tile is the run's first and the run's own input otherwise (tile_frames >= halo).  Seen from a tile a
// stream is ONE sequence of 16-byte vectors: vector v >= 0 is vector v of the run's slot, vector v < 0 is vector
// halo*C/8 + v of the history slot (halo is a multiple of 8 frames, so the seam is a vector edge for every channel count).
//   1. e of all N frames goes to LDS, one dword per frame (index j = frame - (f0 - halo)); frames at or past the
//      stream's count are zeros: a window only looks back, so they reach no output of the run.  The stream's curve goes
//      to LDS behind the tile's loads, 123 dwords of T[k] | T[k+1] << 16: a lookup is one LDS read.
//   2. Thread t keeps elements j = t + 256 i, i < 30, in registers.  Boxcar sum by doubling: a passes v[j] += v[j - 2^k],
//      then v >>= a: L.  Sliding maximum by doubling: p = floor(log2 W) passes v[j] = max(v[j], v[j - 2^k]) give the
//      maximum over 2^p frames, one more pass at distance W - 2^p (two overlapping power-of-two windows) the maximum
//      over W: l.  The lookup, in registers: g.  b more add passes and v >>= b: s.  A pass reads its partner from LDS
//      (consecutive lanes, consecutive dwords), a barrier, writes its own element back, a barrier.  The read is
//      unconditional: an element without a partner (j < distance) takes element 0, an element slot past N the partner of
//      N - 1.  Neither reaches a frame of the tile -- element j is right after all passes when j >= HIST, whatever lies
//      below its window, and halo >= HIST -- and both stay inside the bounds: after k passes an element is a sum (or a
//      maximum) of at most 2^k of the original entries.
//   3. s stays in LDS; the tile's delayed samples x[n - D] are read again from global memory (the two vectors an output
//      vector's samples lie in: D * C = -C mod 8), multiplied by s[n] in 32 bits, and leave as whole 16-byte non-temporal
//      vectors, the stream's ragged end through store_tail.  The minimum of s over the tile is reduced over the
//      workgroup and merged with ONE atomicMin, skipped when nothing was reduced.
//   4. The stream's last tile writes the other history slot: the last halo frames of (old slot, run's input).
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

// C: 1 or 2, or 0 for a run-time channel count
template <int CT>
__device__ __forceinline__ void dyn_tile(const DynArgs &a, u32 *L, u32 *cv, u32 *red)
{
    const u32 C = CT ? (u32)CT : a.channels;
    const u32 tid = threadIdx.x, tile = a.tile_frames, halo = a.halo;
    const u32 s = blockIdx.x / a.chunks;             // stream
    const u32 k = blockIdx.x - s * a.chunks;         // tile inside the stream
    const u32 F = a.nframes ? a.nframes[s] : a.frames;
    const u32 f0 = k * tile;
    const u32 hsamp = halo * C, hv = hsamp >> 3;
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    int16_t *outs = a.out + (u64)s * a.out_stride;
    const int16_t *hs = a.hist + ((u64)a.parity * a.streams + s) * hsamp;
    int16_t *hn = a.hist + ((u64)(a.parity ^ 1u) * a.streams + s) * hsamp;
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
                dyn_load(x[i], ins, hs, hv, vbase + (int)w, nfull, ntail);
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
                    peak = max(peak, dyn_abs(dyn_sample(ins, hs, hsamp, p * (int)C + (int)c)));
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
    for (u32 d = 1; d < (1u << la); d *= 2u)
        pass(d, std::false_type{}, 2u * d == (1u << la) ? la : 0u);     // sums below 2^26; leaves L
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

template <int C>
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_fast(DynArgs a)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<C>(a, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_any(DynArgs a)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<0>(a, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

// one curve (a kernel argument: it travels with the launch) into streams first .. first + count - 1, dword by dword
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_set(u32 *curve, u32 first, u32 count, DynCurveArg c)
{
    constexpr u32 WORDS = DYN_CURVE / 2u;
    const u64 i = (u64)blockIdx.x * DYN_BLOCK + threadIdx.x;
    if (i < (u64)count * WORDS)
        curve[(u64)first * WORDS + i] = c.w[i & (WORDS - 1u)];
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_dyn(const DynArgs &a, hipStream_t st)
{
    const DynPlan p = plan_dyn(a.streams, a.channels, a.a, a.b, a.W - (1u << a.b), a.frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    DynArgs b = a;
    b.halo = p.halo;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    switch (a.channels) {
    case 1: hipLaunchKernelGGL((k_dyn_fast<1>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    case 2: hipLaunchKernelGGL((k_dyn_fast<2>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    default: hipLaunchKernelGGL(k_dyn_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    }
    return hipGetLastError();
}

hipError_t launch_dyn_set(uint16_t *curve, uint32_t first, uint32_t count, const uint16_t *table, hipStream_t st)
{
    if (count == 0)
        return hipSuccess;
    DynCurveArg c;
    for (u32 k = 0; k < DYN_CURVE / 2u; k++)
        c.w[k] = (u32)table[2 * k] | (u32)table[2 * k + 1] << 16;
    const u64 words = (u64)count * (DYN_CURVE / 2u);
    hipLaunchKernelGGL(k_dyn_set, dim3((u32)((words + DYN_BLOCK - 1u) / DYN_BLOCK)), dim3(DYN_BLOCK), 0, st,
                       reinterpret_cast<u32 *>(curve), first, count, c);
    return hipGetLastError();
}

// test hook: the plan of a dynamics run whose longest stream has `frames` frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_dyn(uint32_t streams, uint32_t channels, uint32_t detector_log2, uint32_t smooth_log2,
                                    uint32_t hold, uint32_t frames, DynPlan *plan)
{
    if (plan)
        *plan = plan_dyn(streams, channels, detector_log2, smooth_log2, hold, frames);
}

}  // namespace cmhip
