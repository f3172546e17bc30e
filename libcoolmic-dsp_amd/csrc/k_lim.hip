// k_lim.hip -- gfx950 (MI355X, wave64) look-ahead peak limiter: S streams of C interleaved int16 channels in, the same
// out, delayed by D = A - 1 frames and held under a ceiling T, in exact integers (include/coolmic_hip.h, "peak
// limiter", has the arithmetic to the bit; csrc/lim_plan.h the geometry):
//     pr = (drive * max_c |x[n][c]| + 4095) >> 12       g = pr <= T ? 32768 : floor(T * 32768 / pr)
//     m  = min of g over the last W frames              s = (sum of m over the last A frames) >> a
//     y[n][ch] = (x[n-D][ch] * (drive * s[n]) + 2^26) >> 27
//
//   k_lim_fast<C>   C in {1, 2}: the tile's frames come in and leave as whole 16-byte vectors
//   k_lim_any       3..16 channels: sample by sample; no speed goal
//   k_lim_set       writes one parameter word, handed over as a kernel argument, into a range of streams
//
// A workgroup of 256 threads takes one stream and a tile of tile_frames frames, and evaluates N = halo + tile_frames
// frames: the tile's own and the halo in front of them, which are the stream's history slot where the tile is the
// run's first and the run's own input otherwise (tile_frames >= halo).  Seen from a tile a stream is ONE sequence of
// 16-byte vectors: vector v >= 0 is vector v of the run's slot, vector v < 0 is vector halo*C/8 + v of the history
// slot (halo is a multiple of 8 frames, so the seam is a vector edge for every channel count).
//   1. g of all N frames goes to LDS, one dword per frame (index j = frame - (f0 - halo)); frames at or past the
//      stream's count are zeros, g = 32768: a window only looks back, so they reach no output of the run.
//   2. Thread t keeps elements j = t + 256 i, i < 26, in registers.  Sliding minimum by doubling: p = floor(log2 W)
//      passes v[j] = min(v[j], v[j - 2^k]) give the minimum over 2^p frames, one more pass at distance W - 2^p (two
//      overlapping power-of-two windows) the minimum over W.  Boxcar sum by doubling: a passes v[j] += v[j - 2^k].
//      A pass reads its partner from LDS (consecutive lanes, consecutive dwords), a barrier, writes its own element
//      back, a barrier.  Element j is right after all passes when j >= HIST; halo >= HIST, so every frame of the tile is.
//   3. s = v >> a stays in LDS; the tile's delayed samples x[n - D] are read again from global memory (the two
//      vectors an output vector's samples lie in), multiplied by drive * s[n] in 64 bits, and leave as whole 16-byte
//      non-temporal vectors, the stream's ragged end through store_tail.  The minimum of s over the tile is reduced
//      over the workgroup and merged with ONE atomicMin.
//   4. The stream's last tile writes the other history slot: the last halo frames of (old slot, run's input).
#include "k_lim.h"

namespace cmhip {

// C: 1 or 2, or 0 for a run-time channel count
// (k_limtp.hip's limtp_tile and k_limrel.hip's limrel_tile carry copies of steps 2 to 4 and the meter: a change to them
// goes into all three)
template <int CT>
__device__ __forceinline__ void lim_tile(const LimArgs &a, u32 *L, u32 *red)
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
            lim_write_hist(ins, hs, hn, hsamp, 0, C);
        return;
    }
    const u32 nt = min(tile, F - f0);                // the tile's frames
    const u32 N = halo + tile;
    const u32 ns = F * C, nfull = ns >> 3, ntail = ns & 7u;
    u32 T, drive;

    // ---- 1. g of frames f0 - halo .. f0 + tile - 1
    if constexpr (CT != 0) {
        constexpr u32 FPV = 8u / (u32)CT;            // frames per vector
        constexpr u32 VPT = (LIM_R * (u32)CT + 7u) / 8u;     // vectors per thread at most: 4 (mono), 7 (stereo)
        const u32 NV = N / FPV;
        const int vbase = (int)((f0 * C) >> 3) - (int)hv;
        u32 x[VPT][4];
#pragma unroll
        for (u32 i = 0; i < VPT; i++) {
            const u32 w = tid + LIM_BLOCK * i;
            x[i][0] = x[i][1] = x[i][2] = x[i][3] = 0;
            if (w < NV)
                lim_load(x[i], ins, hs, hv, vbase + (int)w, nfull, ntail);
        }
        // the stream's parameters, read only now: the tile's loads depend on kernel arguments alone and are on their
        // way (k_mix_fast); one dword at offset 0 of an address computed in full
        __builtin_amdgcn_sched_barrier(0);
        const u32 pw = uniform(*(a.par + s));
        T = pw & 0xffffu;
        drive = pw >> 16;
        u32x4 *Lv = reinterpret_cast<u32x4 *>(L);
#pragma unroll
        for (u32 i = 0; i < VPT; i++) {
            const u32 w = tid + LIM_BLOCK * i;
            if (w < NV) {
                u32 g[8];
#pragma unroll
                for (u32 d = 0; d < 4; d++) {
                    const u32 lo = lim_abs(lim_lo(x[i][d])), hi = lim_abs(lim_hi(x[i][d]));
                    if constexpr (CT == 1) {
                        g[2 * d] = lim_gain(lo, drive, T);
                        g[2 * d + 1] = lim_gain(hi, drive, T);
                    } else {
                        g[d] = lim_gain(max(lo, hi), drive, T);
                    }
                }
                const u32x4 g0 = {g[0], g[1], g[2], g[3]};
                if constexpr (CT == 1) {
                    const u32x4 g1 = {g[4], g[5], g[6], g[7]};
                    Lv[2 * w] = g0;
                    Lv[2 * w + 1] = g1;
                } else {
                    Lv[w] = g0;
                }
            }
        }
    } else {
        const u32 pw = uniform(*(a.par + s));
        T = pw & 0xffffu;
        drive = pw >> 16;
        for (u32 j = tid; j < N; j += LIM_BLOCK) {
            const int p = (int)(f0 + j) - (int)halo;         // frame
            u32 peak = 0;
            if (p < (int)F)
                for (u32 c = 0; c < C; c++)
                    peak = max(peak, lim_abs(lim_sample(ins, hs, hsamp, p * (int)C + (int)c)));
            L[j] = lim_gain(peak, drive, T);
        }
    }
    __syncthreads();

    // ---- 2. sliding minimum over W, boxcar sum over A: doubling, own elements in registers
    u32 v[LIM_R];
#pragma unroll
    for (u32 i = 0; i < LIM_R; i++) {
        const u32 j = tid + LIM_BLOCK * i;
        v[i] = j < N ? L[j] : LIM_UNITY;
    }
    // (at entry LDS holds v and every thread is past its reads)
    auto pass = [&](u32 dist, auto is_min, u32 shift) {
        u32 o[LIM_R];
#pragma unroll
        for (u32 i = 0; i < LIM_R; i++) {
            const u32 j = tid + LIM_BLOCK * i;
            o[i] = j < N && j >= dist ? L[j - dist] : (decltype(is_min)::value ? LIM_UNITY : 0u);
        }
        __syncthreads();
#pragma unroll
        for (u32 i = 0; i < LIM_R; i++) {
            const u32 j = tid + LIM_BLOCK * i;
            v[i] = decltype(is_min)::value ? min(v[i], o[i]) : v[i] + o[i];
            if (j < N)
                L[j] = v[i] >> shift;
        }
        __syncthreads();
    };
    const u32 W = a.W, la = a.a;
    u32 P = 1;
    for (; 2u * P <= W; P *= 2u)
        pass(P, std::true_type{}, 0);
    if (W > P)
        pass(W - P, std::true_type{}, 0);
    for (u32 d = 1; d < (1u << la); d *= 2u)
        pass(d, std::false_type{}, 2u * d == (1u << la) ? la : 0u);     // the last pass leaves s = S >> a in LDS

    // ---- the gain-reduction meter: minimum of s over the tile's frames, one atomic per workgroup
    {
        u32 red_max = 0;                             // of 32768 - s
#pragma unroll
        for (u32 i = 0; i < LIM_R; i++) {
            const u32 j = tid + LIM_BLOCK * i;
            if (j >= halo && j < halo + nt)
                red_max = max(red_max, LIM_UNITY - (v[i] >> la));
        }
        red_max = wave_max_u32(red_max);
        if ((tid & 63u) == 0)
            red[tid >> 6] = red_max;
        __syncthreads();
        if (tid == 0) {
            const u32 m = max(max(red[0], red[1]), max(red[2], red[3]));
            if (m)
                atomicMin(a.gmin + s, LIM_UNITY - m);
        }
    }

    // ---- 3. y[n] = x[n - D] * (drive * s[n]): output vectors f0*C/8 .. of the tile
    const u32 D = (1u << la) - 1u;
    const u32 vb = (f0 * C) >> 3, nv = (nt * C + 7u) >> 3;
    u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
    const u32 *Ls = L + halo;                        // s of the tile's frames
    if constexpr (CT != 0) {
        constexpr u32 FPV = 8u / (u32)CT;
        const u32 back = ((D + 1u) * C) >> 3;        // the delayed samples of vector v: CT of vector v - back ...
        for (u32 w = tid; w < nv; w += LIM_BLOCK) {
            const u32 v8 = vb + w;
            u32 x0[4], x1[4];
            lim_load(x0, ins, hs, hv, (int)v8 - (int)back, nfull, ntail);
            lim_load(x1, ins, hs, hv, (int)v8 - (int)back + 1, nfull, ntail);     // ... and the first 8 - CT of the next
            const u32x4 *sv = reinterpret_cast<const u32x4 *>(Ls + w * FPV);
            u32 o[4];
            if constexpr (CT == 1) {
                const u32x4 s0 = sv[0], s1 = sv[1];
                const u32 sf[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                const u32 xs[5] = {x0[0], x0[1], x0[2], x0[3], x1[0]};
#pragma unroll
                for (u32 d = 0; d < 4; d++)          // output samples 2d, 2d + 1 are input samples 2d + 1, 2d + 2
                    o[d] = lim_apply(lim_hi(xs[d]), drive * sf[2 * d]) | lim_apply(lim_lo(xs[d + 1]), drive * sf[2 * d + 1]) << 16;
            } else {
                const u32x4 s0 = sv[0];
                const u32 sf[4] = {s0.x, s0.y, s0.z, s0.w};
                const u32 xs[4] = {x0[1], x0[2], x0[3], x1[0]};
#pragma unroll
                for (u32 d = 0; d < 4; d++)
                    o[d] = lim_apply(lim_lo(xs[d]), drive * sf[d]) | lim_apply(lim_hi(xs[d]), drive * sf[d]) << 16;
            }
            if (v8 < nfull) {
                const u32x4 ov = {o[0], o[1], o[2], o[3]};
                __builtin_nontemporal_store(ov, dst + v8);
            } else if (v8 == nfull) {
                store_tail(outs, v8, o, ntail);
            }
        }
    } else {
        for (u32 w = tid; w < nv; w += LIM_BLOCK) {
            const u32 v8 = vb + w;
            u32 o[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 e = 0; e < 8; e++) {
                const u32 q = v8 * 8u + e;           // output sample of the stream
                if (q < ns) {
                    const u32 n = q / C;
                    const int x = lim_sample(ins, hs, hsamp, (int)q - (int)(D * C));
                    o[e >> 1] |= lim_apply(x, drive * Ls[n - f0]) << (16u * (e & 1u));
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
        lim_write_hist(ins, hs, hn, hsamp, F, C);
}

template <int C>
__global__ __launch_bounds__(LIM_BLOCK) void k_lim_fast(LimArgs a)
{
    extern __shared__ u32x4 lim_lds[];
    __shared__ u32 red[4];
    lim_tile<C>(a, reinterpret_cast<u32 *>(lim_lds), red);
}

__global__ __launch_bounds__(LIM_BLOCK) void k_lim_any(LimArgs a)
{
    extern __shared__ u32x4 lim_lds[];
    __shared__ u32 red[4];
    lim_tile<0>(a, reinterpret_cast<u32 *>(lim_lds), red);
}

// one parameter word (a kernel argument: it travels with the launch) into streams first .. first + count - 1
__global__ __launch_bounds__(LIM_BLOCK) void k_lim_set(u32 *par, u32 first, u32 count, u32 word)
{
    const u32 i = blockIdx.x * LIM_BLOCK + threadIdx.x;
    if (i < count)
        par[(u64)first + i] = word;
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_lim(const LimArgs &a, hipStream_t st)
{
    const LimPlan p = plan_lim(a.streams, a.channels, a.a, a.W - (1u << a.a), a.frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    LimArgs b = a;
    b.halo = p.halo;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    switch (a.channels) {
    case 1: hipLaunchKernelGGL((k_lim_fast<1>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    case 2: hipLaunchKernelGGL((k_lim_fast<2>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    default: hipLaunchKernelGGL(k_lim_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    }
    return hipGetLastError();
}

hipError_t launch_lim_set(uint32_t *par, uint32_t first, uint32_t count, uint32_t threshold, uint32_t drive, hipStream_t st)
{
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_lim_set, dim3((count + LIM_BLOCK - 1u) / LIM_BLOCK), dim3(LIM_BLOCK), 0, st, par, first, count,
                       threshold | drive << 16);
    return hipGetLastError();
}

// test hook: the plan of a limiter run whose longest stream has `frames` frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_lim(uint32_t streams, uint32_t channels, uint32_t lookahead_log2, uint32_t hold,
                                    uint32_t frames, LimPlan *plan)
{
    if (plan)
        *plan = plan_lim(streams, channels, lookahead_log2, hold, frames);
}

}  // namespace cmhip
