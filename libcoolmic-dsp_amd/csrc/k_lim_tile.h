// k_lim_tile.h -- the ONE tile body of the limiter's kernels (k_lim.hip, k_limtp.hip, k_limrel.hip instantiate it; the
// small helpers are k_lim.h's) and the launch helper their launchers share.
//
// A workgroup of 256 threads takes one stream and a tile of tile_frames frames, and evaluates N = halo + tile_frames
// frames: the tile's own and the halo in front of them, which are the stream's history slot where the tile is the
// run's first and the run's own input otherwise (tile_frames >= halo).  Seen from a tile a stream is ONE sequence of
// 16-byte vectors: vector v >= 0 is vector v of the run's slot, vector v < 0 is vector halo*C/8 + v of the history
// slot (halo is a multiple of 8 frames, so the seam is a vector edge for every channel count).
//   1. g of all N frames goes to LDS, one dword per frame (index j = frame - (f0 - halo)); frames at or past the
//      stream's count are zeros, g = 32768: a window only looks back, so they reach no output of the run.  Three forms:
//      the sample detector's fast form (whole vectors, thread t takes vectors t + 256 i), the true-peak detector's fast
//      form (below) and the any-channel-count form, sample by sample for either detector.
//   2. Thread t keeps elements j = t + 256 i, i < SLOTS, in registers.  Sliding minimum by doubling: p = floor(log2 W)
//      passes v[j] = min(v[j], v[j - 2^k]) give the minimum over 2^p frames, one more pass at distance W - 2^p (two
//      overlapping power-of-two windows) the minimum over W.  The release ramp (REL) and the boxcar sum by doubling: a
//      passes v[j] += v[j - 2^k].  A pass reads its partner from LDS (consecutive lanes, consecutive dwords), a
//      barrier, writes its own element back, a barrier.  Element j is right after all passes when j >= HIST;
//      halo >= HIST, so every frame of the tile is.
//   3. s = v >> a stays in LDS; the tile's delayed samples x[n - D] are read again from global memory (the two
//      vectors an output vector's samples lie in: D + 1 is a multiple of 8 frames for both detectors), multiplied by
//      drive * s[n] in 64 bits, and leave as whole 16-byte non-temporal vectors, the stream's ragged end through
//      store_tail.  The minimum of s over the tile is reduced over the workgroup and merged with ONE atomicMin.
//   4. The stream's last tile writes the other history slot: the last halo frames of (old slot, run's input).
//
// Step 1 of the true-peak detector.  g[n] needs the 13 frames in front of frame n, so a tile reads 13 frames in front
// of its evaluated range; where they would lie in front of the history slot (the run's first tile) they are zeros: the
// elements they make wrong are j < 13 <= HIST, which reach no output.  Fast forms: the evaluated range is
// NV = N * C / 8 vectors; thread t owns the cnt = ceil(NV / 256) CONSECUTIVE vectors from t * cnt on and loads, besides
// them, the 16 frames in front of its first one again from global memory (2 vectors mono, 4 stereo: its neighbour's,
// L1 / L2 hits; nothing is staged through LDS and nothing spills).  All of it is loaded before the parameter word is
// read.  Pairs of consecutive samples of one channel sit in a dword, P[t] = x[t-1] | x[t] << 16, and one v_dot2 does
// two taps: y_p[t] = sum_{i<6} dot2(P[t - 2i], K[p][i]), K[p][i] = H[p][2i+1] | H[p][2i] << 16, 24 literal constants.
// drive * t is one v_mad_u64_u32; a vector's g leave as 16-byte LDS stores.
//
// The release (REL) is a min-plus convolution with a ramp, and a ramp doubles as a window does: after k passes
//     v[j] = min over i < 2^k of (m[j-i] + i*q),    pass k:  v[j] = min(v[j], v[j - 2^k] + (q << k)),
// k = 0 .. rho - 1.  A partner in front of element 0 counts as 32768: with the added q << k > 0 it never wins, which is
// what "no earlier frame" means.  (R - 1) * q < 32768 = R * q, so a window of R frames is the whole ramp: an m further
// back would have to be below zero to matter.  Element j is right after all passes when j >= HIST.
#ifndef CMHIP_K_LIM_TILE_H
#define CMHIP_K_LIM_TILE_H

#include "k_lim.h"

namespace cmhip {

struct LimRelArgs : LimArgs {
    uint32_t rho;                                    // release_log2, 1..11
};

// TP: the true-peak detector.  REL: the release stage (Args is LimRelArgs).  SLOTS: elements per thread at most,
// N <= 256 * SLOTS.  CT: 1 or 2, or 0 for a run-time channel count
template <bool TP, bool REL, u32 SLOTS, int CT, class Args>
__device__ __forceinline__ void lim_tile(const Args &a, u32 *L, u32 *red)
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
    const u32 N = halo + tile;                       // <= 256 * SLOTS
    const u32 ns = F * C, nfull = ns >> 3, ntail = ns & 7u;
    u32 T, drive;

    // ---- 1. g of frames f0 - halo .. f0 + tile - 1
    if constexpr (CT != 0 && !TP) {
        constexpr u32 FPV = 8u / (u32)CT;            // frames per vector
        constexpr u32 VPT = (SLOTS * (u32)CT + 7u) / 8u;     // vectors per thread at most
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
                lim_put_g<CT>(L, w, g);
            }
        }
    } else if constexpr (CT != 0) {
        constexpr u32 FPV = 8u / (u32)CT;            // frames per vector
        constexpr u32 VPT = (SLOTS * (u32)CT + 7u) / 8u;     // own vectors per thread at most
        constexpr u32 HV = 16u / FPV;                // vectors in front of them: 16 frames, 13 needed
        constexpr u32 H0 = HV * FPV;                 // local index of the thread's first own frame
        const u32 NV = N / FPV;
        const u32 cnt = (NV + LIM_BLOCK - 1u) / LIM_BLOCK;   // (uniform) own vectors per thread, <= VPT
        const u32 w0 = tid * cnt;                    // the first of them, counted in the evaluated range
        const int vbase = (int)((f0 * C) >> 3) - (int)hv;
        u32 d[(HV + VPT) * 4];
#pragma unroll
        for (u32 i = 0; i < HV + VPT; i++) {
            u32 x[4] = {0, 0, 0, 0};
            const int w = (int)(w0 + i) - (int)HV;   // vector of the evaluated range; below 0: in front of it
            const int vv = vbase + w;                // ... of the stream's sequence; below -hv: in front of the slot
            if (i < HV + cnt && w < (int)NV && vv >= -(int)hv)
                lim_load(x, ins, hs, hv, vv, nfull, ntail);
            d[4 * i] = x[0]; d[4 * i + 1] = x[1]; d[4 * i + 2] = x[2]; d[4 * i + 3] = x[3];
        }
        __builtin_amdgcn_sched_barrier(0);           // (the parameter word after the loads, as above)
        const u32 pw = uniform(*(a.par + s));
        T = pw & 0xffffu;
        drive = pw >> 16;
        auto pair = [&](u32 t, u32 c) -> u32 {       // x_c[t-1] | x_c[t] << 16 (k_tpeak.hip)
            if constexpr (CT == 1) {
                (void)c;
                return (t & 1u) ? d[t >> 1] : __builtin_amdgcn_alignbit(d[t >> 1], d[(t >> 1) - 1u], 16);
            } else {
                return __builtin_amdgcn_perm(d[t], d[t - 1u], c == 0 ? 0x05040100u : 0x07060302u);
            }
        };
        auto sample = [&](u32 t, u32 c) -> int {     // x_c[t]
            if constexpr (CT == 1) {
                (void)c;
                return (t & 1u) ? lim_hi(d[t >> 1]) : lim_lo(d[t >> 1]);
            } else {
                return c == 0 ? lim_lo(d[t]) : lim_hi(d[t]);
            }
        };
#pragma unroll
        for (u32 i = 0; i < VPT; i++) {
            const u32 w = w0 + i;
            if (i < cnt && w < NV) {
                u32 g[FPV];
#pragma unroll
                for (u32 f = 0; f < FPV; f++) {
                    const u32 t = H0 + i * FPV + f;  // local frame of element n: y at n - 2, the sample at n - 8
                    u32 pk = 0;
#pragma unroll
                    for (u32 c = 0; c < (u32)CT; c++) {
                        pk = max(pk, lim_abs(sample(t - 8u, c)) << 13);
                        pk = max(pk, limtp_fir(pair, t - 2u, c));
                        // (one FIR at a time: left to itself the scheduler interleaves the tile's dot chains)
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    g[f] = limtp_gain(pk, drive, T);
                }
                lim_put_g<CT>(L, w, g);
            }
        }
    } else {
        const u32 pw = uniform(*(a.par + s));
        T = pw & 0xffffu;
        drive = pw >> 16;
        for (u32 j = tid; j < N; j += LIM_BLOCK) {
            const int n = (int)(f0 + j) - (int)halo;             // frame
            u32 pk = 0;
            if constexpr (!TP) {
                if (n < (int)F)
                    for (u32 c = 0; c < C; c++)
                        pk = max(pk, lim_abs(lim_sample(ins, hs, hsamp, n * (int)C + (int)c)));
                L[j] = lim_gain(pk, drive, T);
            } else {
                for (u32 c = 0; c < C; c++) {
                    int x[LIM_TP_FRONT];             // x[i] is frame n - 13 + i: zeros in front of the slot and past the count
#pragma unroll
                    for (u32 i = 0; i < LIM_TP_FRONT; i++) {
                        const int p = n - (int)LIM_TP_FRONT + (int)i;
                        x[i] = p >= -(int)halo && p < (int)F ? lim_sample(ins, hs, hsamp, p * (int)C + (int)c) : 0;
                    }
                    pk = max(pk, lim_abs(x[LIM_TP_FRONT - 8u]) << 13);
#pragma unroll
                    for (u32 ph = 0; ph < 4; ph++) {
                        int y = 0;
#pragma unroll
                        for (u32 t = 0; t < TP_TAPS; t++)
                            y += (int)tp_h(ph, t) * x[LIM_TP_FRONT - 2u - t];
                        pk = max(pk, lim_abs(y));
                    }
                }
                L[j] = limtp_gain(pk, drive, T);
            }
        }
    }
    __syncthreads();

    // ---- 2. sliding minimum over W, release ramp over R, boxcar sum over A: doubling, own elements in registers
    u32 v[SLOTS];
#pragma unroll
    for (u32 i = 0; i < SLOTS; i++) {
        const u32 j = tid + LIM_BLOCK * i;
        v[i] = j < N ? L[j] : LIM_UNITY;
    }
    // (at entry LDS holds v and every thread is past its reads)
    // kind 0: v = min(v, partner); 1: v = min(v, partner + add); 2: v += partner, v >> shift goes to LDS
    auto pass = [&](u32 dist, auto kind, u32 add, u32 shift) {
        constexpr int K = decltype(kind)::value;
        u32 o[SLOTS];
#pragma unroll
        for (u32 i = 0; i < SLOTS; i++) {
            const u32 j = tid + LIM_BLOCK * i;
            o[i] = j < N && j >= dist ? L[j - dist] : (K == 2 ? 0u : LIM_UNITY);
        }
        __syncthreads();
#pragma unroll
        for (u32 i = 0; i < SLOTS; i++) {
            const u32 j = tid + LIM_BLOCK * i;
            if constexpr (K == 0)
                v[i] = min(v[i], o[i]);
            else if constexpr (K == 1)
                v[i] = min(v[i], o[i] + add);
            else
                v[i] = v[i] + o[i];
            if (j < N)
                L[j] = v[i] >> shift;
        }
        __syncthreads();
    };
    using k_min = std::integral_constant<int, 0>;
    using k_rel = std::integral_constant<int, 1>;
    using k_sum = std::integral_constant<int, 2>;
    const u32 W = a.W, la = a.a;
    u32 P = 1;
    for (; 2u * P <= W; P *= 2u)
        pass(P, k_min{}, 0, 0);
    if (W > P)
        pass(W - P, k_min{}, 0, 0);
    if constexpr (REL) {
        const u32 rho = a.rho, q = LIM_UNITY >> rho;
        for (u32 e = 0; e < rho; e++)
            pass(1u << e, k_rel{}, q << e, 0);
    }
    for (u32 d = 1; d < (1u << la); d *= 2u)
        pass(d, k_sum{}, 0, 2u * d == (1u << la) ? la : 0u);         // the last pass leaves s = S >> a in LDS

    // ---- the gain-reduction meter: minimum of s over the tile's frames, one atomic per workgroup
    {
        u32 red_max = 0;                             // of 32768 - s
#pragma unroll
        for (u32 i = 0; i < SLOTS; i++) {
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
    const u32 D = (1u << la) - 1u + (TP ? LIM_TP_LAG : 0u);          // D + 1 is a multiple of 8 frames for both
    const u32 vb = (f0 * C) >> 3, nv = (nt * C + 7u) >> 3;
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
            lim_store(outs, v8, o, nfull, ntail);
        }
    } else {
        for (u32 w = tid; w < nv; w += LIM_BLOCK) {
            const u32 v8 = vb + w;
            u32 o[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 e = 0; e < 8; e++) {
                const u32 qs = v8 * 8u + e;          // output sample of the stream
                if (qs < ns) {
                    const u32 n = qs / C;
                    const int x = lim_sample(ins, hs, hsamp, (int)qs - (int)(D * C));
                    o[e >> 1] |= lim_apply(x, drive * Ls[n - f0]) << (16u * (e & 1u));
                }
            }
            lim_store(outs, v8, o, nfull, ntail);
        }
    }

    // ---- 4. the stream's last tile leaves the history of the next run
    if (F <= f0 + tile)
        lim_write_hist(ins, hs, hn, hsamp, F, C);
}

// the launch every limiter launcher ends in: the plan's geometry into the arguments, then the mono, the stereo or the
// any-channel-count kernel
template <class Args>
inline hipError_t lim_launch(const LimPlan &p, Args b, hipStream_t st, void (*mono)(Args), void (*stereo)(Args),
                             void (*any)(Args))
{
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    b.halo = p.halo;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    hipLaunchKernelGGL(b.channels == 1 ? mono : b.channels == 2 ? stereo : any, dim3(p.grid), dim3(p.block), p.lds_bytes,
                       st, b);
    return hipGetLastError();
}

}  // namespace cmhip
#endif
