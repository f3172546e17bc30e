// k_limtp.hip -- gfx950 (MI355X, wave64) look-ahead limiter with the TRUE-PEAK detector: k_lim.hip's tile with another
// step 1 (include/coolmic_hip.h, "peak limiter", "true-peak detector", has the arithmetic to the bit; csrc/lim_plan.h
// the geometry):
//     y_p[n][c] = sum_{k<12} H[p][k] * x[n-k][c]        p = 0..3: BS.1770 Annex 2's 4x oversampling, exact int32
//     t[n]  = max_c max(|x[n-8][c]| << 13, max_p |y_p[n-2][c]|)
//     pr    = (drive * t[n] + 2^25 - 1) >> 25           g = pr <= T ? 32768 : floor(T * 32768 / pr)
//     m, s as in k_lim.hip                              y[n][ch] = (x[n-Dtp][ch] * (drive * s[n]) + 2^26) >> 27
// with Dtp = A + 7 and HIST = A + W - 2 + 13.
//
//   k_limtp_fast<C>   C in {1, 2}: whole 16-byte vectors in and out, the FIR in k_tpeak.hip's pair-dword dot form
//   k_limtp_any       3..16 channels: sample by sample in plain multiply-adds; no speed goal
//
// The tile, its N = halo + tile_frames elements, the seam between the history slot and the run's slot, steps 2 to 4 and
// the meter are k_lim.hip's, restated here (the helpers come from k_lim.h; the tile body is a second copy because
// k_lim.hip's generated code is kept as it is).  Step 3 reads x[n - Dtp]: Dtp + 1 = A + 8 is a multiple of 8 frames as
// D + 1 = A is there, so "the two vectors an output vector's samples lie in" holds unchanged.
//
// Step 1.  g[n] needs the 13 frames in front of frame n, so a tile reads 13 frames in front of its evaluated range;
// where they would lie in front of the history slot (the run's first tile) they are zeros: the elements they make wrong
// are j < 13 <= HIST, which reach no output.  Fast forms: the evaluated range is NV = N * C / 8 vectors; thread t owns
// the cnt = ceil(NV / 256) CONSECUTIVE vectors from t * cnt on (at most 4 mono, 7 stereo) and loads, besides them, the
// 16 frames in front of its first one again from global memory (2 vectors mono, 4 stereo: its neighbour's, L1 / L2
// hits; nothing is staged through LDS and nothing spills).  All of it is loaded before the parameter word is read.
// Pairs of consecutive samples of one channel sit in a dword, P[t] = x[t-1] | x[t] << 16, and one v_dot2 does two taps:
// y_p[t] = sum_{i<6} dot2(P[t - 2i], K[p][i]), K[p][i] = H[p][2i+1] | H[p][2i] << 16, 24 literal constants.  drive * t
// is one v_mad_u64_u32; a vector's g leave as 16-byte LDS stores.
#include "k_lim.h"

namespace cmhip {

// C: 1 or 2, or 0 for a run-time channel count
template <int CT>
__device__ __forceinline__ void limtp_tile(const LimArgs &a, u32 *L, u32 *red)
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
        constexpr u32 VPT = (LIM_R * (u32)CT + 7u) / 8u;     // own vectors per thread at most: 4 (mono), 7 (stereo)
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
        // the stream's parameters, read only now: the tile's loads depend on kernel arguments alone and are on their
        // way (k_lim_fast); one dword at offset 0 of an address computed in full
        __builtin_amdgcn_sched_barrier(0);
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
        u32x4 *Lv = reinterpret_cast<u32x4 *>(L);
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
            const int n = (int)(f0 + j) - (int)halo;             // frame
            u32 pk = 0;
            for (u32 c = 0; c < C; c++) {
                int x[LIM_TP_FRONT];                 // x[i] is frame n - 13 + i: zeros in front of the slot and past the count
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
    const u32 D = (1u << la) - 1u + LIM_TP_LAG;     // Dtp = A + 7: D + 1 is a multiple of 8 frames, as it is there
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
__global__ __launch_bounds__(LIM_BLOCK) void k_limtp_fast(LimArgs a)
{
    extern __shared__ u32x4 limtp_lds[];
    __shared__ u32 red[4];
    limtp_tile<C>(a, reinterpret_cast<u32 *>(limtp_lds), red);
}

__global__ __launch_bounds__(LIM_BLOCK) void k_limtp_any(LimArgs a)
{
    extern __shared__ u32x4 limtp_lds[];
    __shared__ u32 red[4];
    limtp_tile<0>(a, reinterpret_cast<u32 *>(limtp_lds), red);
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_limtp(const LimArgs &a, hipStream_t st)
{
    const LimPlan p = plan_limtp(a.streams, a.channels, a.a, a.W - (1u << a.a), a.frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    LimArgs b = a;
    b.halo = p.halo;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    switch (a.channels) {
    case 1: hipLaunchKernelGGL((k_limtp_fast<1>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    case 2: hipLaunchKernelGGL((k_limtp_fast<2>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    default: hipLaunchKernelGGL(k_limtp_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    }
    return hipGetLastError();
}

// test hook: the plan of a true-peak limiter run whose longest stream has `frames` frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_limtp(uint32_t streams, uint32_t channels, uint32_t lookahead_log2, uint32_t hold,
                                      uint32_t frames, LimPlan *plan)
{
    if (plan)
        *plan = plan_limtp(streams, channels, lookahead_log2, hold, frames);
}

}  // namespace cmhip
