// ubench_corr.hip -- where k_corr_fast's time goes on MI355X, on the config-2 shape: 4096 stereo streams
// x 65536 frames, one wave per 8 KiB tile, gains 750 / 1250 over 1000 and the channel swap.  Two layouts of the tile's
// loads -- a line per lane (lane owns 8 consecutive 16-byte vectors: k_tpeak.hip's, which its FIR needs) and coalesced
// (lane owns vectors lane, lane + 64, ...: k_corr.hip's) -- each in five forms:
//   dots        the three products as v_dot2c_i32_i16 against masked copies of the frame's dword (k_corr.hip's form)
//   mads        the same products as v_mad_i32_i16 with op_sel (no masks, no start-of-chain moves; inline assembly)
//   no atomics  the dot form without the three atomicAdd per wave
//   gain only   loads, map and gain
//   loads only
// Kernel time between HIP events, median / min / max of 15 launches after 5; the sums of the forms that produce them are
// compared with the first form's.
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Iinclude tools/ubench_corr.hip -o tools/ubench_corr
#include "../libcoolmic-dsp_amd/csrc/cmhip_device.h"
#include <stdio.h>
#include <string.h>
#include <vector>
#include <algorithm>

using namespace cmhip;

constexpr u32 U = 8, TILE_V = 64 * U, LF = U * 4, BIAS = 0x7fff0000u;

__device__ __forceinline__ u32 dot2(u32 x, u32 y, u32 acc)
{
    return (u32)__builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, y), (int)acc, false);
}
__device__ __forceinline__ u32 mad_ll(u32 w, u32 acc)
{
    u32 r;
    asm("v_mad_i32_i16 %0, %1, %1, %2 op_sel:[0,0,0,0]" : "=v"(r) : "v"(w), "v"(acc));
    return r;
}
__device__ __forceinline__ u32 mad_hh(u32 w, u32 acc)
{
    u32 r;
    asm("v_mad_i32_i16 %0, %1, %1, %2 op_sel:[1,1,0,0]" : "=v"(r) : "v"(w), "v"(acc));
    return r;
}
__device__ __forceinline__ u32 mad_lh(u32 w, u32 acc)
{
    u32 r;
    asm("v_mad_i32_i16 %0, %1, %1, %2 op_sel:[0,1,0,0]" : "=v"(r) : "v"(w), "v"(acc));
    return r;
}
__device__ __forceinline__ u32 mad_ll0(u32 w)
{
    u32 r;
    asm("v_mad_i32_i16 %0, %1, %1, 0 op_sel:[0,0,0,0]" : "=v"(r) : "v"(w));
    return r;
}
__device__ __forceinline__ u32 mad_hh0(u32 w)
{
    u32 r;
    asm("v_mad_i32_i16 %0, %1, %1, 0 op_sel:[1,1,0,0]" : "=v"(r) : "v"(w));
    return r;
}
__device__ __forceinline__ u32 mad_lhb(u32 w, u32 bias)
{
    u32 r;
    asm("v_mad_i32_i16 %0, %1, %1, %2 op_sel:[0,1,0,0]" : "=v"(r) : "v"(w), "s"(bias));
    return r;
}

// V: 0 dots, 1 v_mad_i32_i16, 2 dots without the atomics, 3 load + gain only, 4 loads only; COAL: the loads' layout
template <int V, bool COAL = false>
__global__ __launch_bounds__(64) void k(CorrArgs a)
{
    const u32 s = blockIdx.x / a.chunks, kk = blockIdx.x - s * a.chunks;
    const u32 lane = threadIdx.x & 63u;
    const u32 vl = kk * TILE_V + lane * U;
    const int16_t *ins = a.in + (u64)s * a.stride;
    const u32x4 *src = reinterpret_cast<const u32x4 *>(ins);
    u32 d[LF];
#pragma unroll
    for (u32 i = 0; i < U; i++) {
        u32x4 w = __builtin_nontemporal_load(COAL ? src + kk * TILE_V + 64u * i + lane : src + vl + i);
        d[4 * i] = w.x; d[4 * i + 1] = w.y; d[4 * i + 2] = w.z; d[4 * i + 3] = w.w;
    }
    __builtin_amdgcn_sched_barrier(0);
    const StreamParam *p = a.param + s;
    const u32 perm2 = p->perm2, mi01 = p->mi01, mf0 = p->mf[0], mf1 = p->mf[1];
    const u32 bias = uniform(BIAS);
    u64 ea = 0, eb = 0, xb = 0;
#pragma unroll
    for (u32 i = 0; i < LF; i += 2) {
        u32 w[2];
#pragma unroll
        for (u32 j = 0; j < 2; j++) {
            u32 x = d[i + j];
            if constexpr (V != 4) {
                x = __builtin_amdgcn_perm(x, x, perm2);
                (void)gain2<true>(x, mi01, mf0, mf1, w[j]);
            } else {
                w[j] = x;
            }
        }
        if constexpr (V == 0 || V == 2) {
            ea += dot2(w[1], w[1] & 0xffffu, dot2(w[0], w[0] & 0xffffu, 0u));
            eb += dot2(w[1], w[1] & 0xffff0000u, dot2(w[0], w[0] & 0xffff0000u, 0u));
            xb += dot2(w[1], w[1] >> 16, dot2(w[0], w[0] >> 16, BIAS));
        } else if constexpr (V == 1) {
            ea += mad_ll(w[1], mad_ll0(w[0]));
            eb += mad_hh(w[1], mad_hh0(w[0]));
            xb += mad_lh(w[1], mad_lhb(w[0], bias));
        } else {
            ea += w[0] ^ w[1]; eb += w[0] & 0xffu; xb += w[1] & 0xffu;
        }
    }
    const u64 sa = wave_add_u40(ea), sb = wave_add_u40(eb);
    const u64 sx = wave_add_u40(xb) - 64ull * (LF / 2) * BIAS;
    if (lane == 0) {
        unsigned long long *win = a.sums + (u64)s * (CORR_MAX_PAIRS * CORR_SUMS);
        if constexpr (V == 0 || V == 1) {
            if (sa) atomicAdd(win, sa);
            if (sb) atomicAdd(win + 1, sb);
            if (sx) atomicAdd(win + 2, sx);
        } else {
            if (sa == 0x123456789abcull && sb == 77 && sx == 3)      // (never: keeps the sums alive)
                win[0] = sa;
        }
    }
}

__global__ void fill(u32 *p, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        u32 x = (u32)i * 2654435761u + 12345u;
        x ^= x >> 13; x *= 0x5bd1e995u; x ^= x >> 15;
        p[i] = x;
    }
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

template <int V, bool COAL = false>
static int run(const char *name, CorrArgs a, u32 grid, std::vector<unsigned long long> *keep)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const size_t words = (size_t)a.streams * CORR_MAX_PAIRS * CORR_SUMS;
    for (int i = 0; i < 5; i++)
        hipLaunchKernelGGL((k<V, COAL>), dim3(grid), dim3(64), 0, 0, a);
    CK(hipDeviceSynchronize());
    CK(hipMemset(a.sums, 0, words * 8));
    std::vector<float> ms;
    for (int i = 0; i < 15; i++) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((k<V, COAL>), dim3(grid), dim3(64), 0, 0, a);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t; CK(hipEventElapsedTime(&t, e0, e1));
        ms.push_back(t);
    }
    CK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    std::vector<unsigned long long> h(words);
    CK(hipMemcpy(h.data(), a.sums, words * 8, hipMemcpyDeviceToHost));
    int same = -1;
    if (keep) {
        if (keep->empty()) *keep = h; else same = (*keep == h);
    }
    printf("%-28s median %.4f ms  min %.4f  max %.4f  sums[0..2] %llu %llu %lld  equal_to_first %d\n", name, ms[7], ms[0],
           ms[14], h[0] / 15, h[1] / 15, (long long)h[2] / 15, same);
    fflush(stdout);
    return 0;
}

int main()
{
    const u32 S = 4096, T = 65536;
    CorrArgs a{};
    a.streams = S; a.channels = 2; a.frames = T; a.npairs = 1; a.stride = (u64)T * 2;
    a.chunks = (T * 2 / 8) / TILE_V;
    const u32 grid = S * a.chunks;
    int16_t *in; StreamParam *par; unsigned long long *sums;
    const size_t bytes = (size_t)S * T * 2 * 2;
    CK(hipMalloc((void **)&in, bytes));
    CK(hipMalloc((void **)&par, sizeof(StreamParam) * S));
    CK(hipMalloc((void **)&sums, (size_t)S * CORR_MAX_PAIRS * CORR_SUMS * 8));
    hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, (u32 *)in, bytes / 4);
    std::vector<StreamParam> hp(S);
    for (u32 s = 0; s < S; s++) {
        StreamParam &p = hp[s];
        memset(&p, 0, sizeof(p));
        p.mode = GAIN_GENERAL;
        p.perm2 = 0x01000302u;                   // swap
        // gains 750 / 1250 over 1000: mi = gain / scale, mf = ceil((gain % scale) * 2^32 / scale)
        const u32 g[2] = {750, 1250};
        for (int c = 0; c < 2; c++) {
            p.mi[c] = (uint16_t)(g[c] / 1000);
            p.mf[c] = (u32)((((unsigned long long)(g[c] % 1000) << 32) + 999) / 1000);
        }
        p.mi01 = p.mi[0] | ((u32)p.mi[1] << 16);
        p.chmap[0] = 1; p.chmap[1] = 0;
    }
    CK(hipMemcpy(par, hp.data(), sizeof(StreamParam) * S, hipMemcpyHostToDevice));
    CK(hipDeviceSynchronize());
    a.in = in; a.param = par; a.sums = sums;
    std::vector<unsigned long long> keep;
    for (int rep = 0; rep < 2; rep++) {
        if (run<0>("dots, a line per lane", a, grid, &keep)) return 1;
        if (run<1>("mads, a line per lane", a, grid, &keep)) return 1;
        if (run<2>("dots, no atomics, line", a, grid, nullptr)) return 1;
        if (run<3>("gain only, line", a, grid, nullptr)) return 1;
        if (run<4>("loads only, line", a, grid, nullptr)) return 1;
        if ((run<0, true>("dots, coalesced", a, grid, &keep))) return 1;
        if ((run<1, true>("mads, coalesced", a, grid, &keep))) return 1;
        if ((run<2, true>("dots, coalesced, no atomics", a, grid, nullptr))) return 1;
        if ((run<3, true>("gain only, coalesced", a, grid, nullptr))) return 1;
        if ((run<4, true>("loads only, coalesced", a, grid, nullptr))) return 1;
    }
    return 0;
}
