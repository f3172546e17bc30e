// k_iirramp.hip -- gfx950 (MI355X, wave64) kernels of the filter's coefficient ramps: a section moves from c0 to c1 over
// R frames, every frame with a section c(p) of its own (include/coolmic_hip.h, "filter", has the arithmetic to the bit;
// csrc/iir_ramp.h the position and the section between two ends as code).  Launched instead of k_iir.hip's kernels for a
// run at whose start some section ramps; the table behind the run's counts then holds IIR_RAMP_WORDS per section: both
// ends, done and R.
//
//   k_iirr_fast<C, NP>  k_iir_fast's decomposition: a lane is (row, section) and keeps its section's two ends, their
//                       sums and its clock (done, inc) in registers
//   k_iirr_any          k_iir_any's: a lane is a row and loops over its sections; the workgroup's ends lie in LDS beside
//                       the tiles, staged once, and a lane reads a section's twelve words back per frame
//
// Tiles, the DPP hand-over, the empty pipeline at every tile's end and the order of a frame's steps are k_iir.hip's (the
// tile movers: k_iir.h; the step: iir_plan.h).  What is new stands beside the recurrence, not in it: a frame's position
// depends on the frame's index alone and its five coefficients on the position alone, so neither waits for v.  A
// section at rest takes the same path: its clock says "over", p = 32768 and c(32768) = c1.
#include "k_iir.h"

namespace cmhip {

// a lane's section between its ends
struct IirRamped {
    IirSec c0 = IIR_UNITY, c1 = IIR_UNITY;
    int32_t s0 = IIR_ONE, s1 = IIR_ONE;
    IirRampClock clock = {2u, 1u << 31};             // at rest
    __device__ __forceinline__ void load(const int32_t *e)
    {
        c0 = iir_load_sec(e);
        c1 = iir_load_sec(e + IIR_SEC_WORDS);
        s0 = iir_ramp_sum(c0);
        s1 = iir_ramp_sum(c1);
        clock = iir_ramp_clock((u32)e[10], (u32)e[11]);
    }
    // frame f of the run
    __device__ __forceinline__ IirSec at(u32 f) const { return iir_ramp_section(c0, c1, s0, s1, iir_ramp_at(clock, f)); }
};

// ---------------------------------------------------------------------------
template <int C, int NP>
__global__ __launch_bounds__(IIR_BLOCK) void k_iirr_fast(IirArgs a)
{
    __shared__ __attribute__((aligned(4))) int16_t lds[IIR_LDS_SAMPLES];
    constexpr u32 SPW = IIR_BLOCK / (u32)(C * NP);
    const u32 lane = threadIdx.x, k = lane % (u32)NP, r = lane / (u32)NP, j = r / (u32)C, c = r % (u32)C;
    const u32 s0 = blockIdx.x * SPW, s = s0 + j, N = a.sections;
    const bool live = s < a.streams, real = live && k < N;
    const u32 count = live ? a.counts[s] : 0u;
    const u32 most = wave_max_u32(count);
    if (most == 0)                                   // (uniform) streams given no frames keep everything
        return;
    IirRamped rs;                                    // sections N..NP-1: the identity at rest, e stays 0
    IirState st = {0, 0, 0, 0, 0};
    IirState *home = a.state + ((u64)s * (u32)C + c) * N + k;
    if (real) {
        rs.load(a.coef + ((u64)s * N + k) * IIR_RAMP_WORDS);
        st = *home;
    }
    int16_t *row = lds + j * iir_lds_pitch((u32)C) + c;
    u64 clips = 0, overs = 0;
    int vprev = 0;
    const u32 tiles = (most + IIR_TILE - 1u) / IIR_TILE;
    u32x4 ahead[IIR_MOVE];
    iir_tile_fetch(a, ahead, s0, SPW, (u32)C, 0);
    for (u32 t = 0; t < tiles; t++) {
        iir_tile_commit(a, ahead, lds, s0, SPW, (u32)C, t);
        __syncthreads();
        if (t + 1u < tiles)                          // (uniform) the next tile's loads fly while this one is walked
            iir_tile_fetch(a, ahead, s0, SPW, (u32)C, t + 1u);
        const u32 len = iir_tile_frames(count, t);
        const u32 steps = iir_tile_frames(most, t) + (u32)NP - 1u;
        u32 cl = 0, ov = 0;
        for (u32 i0 = 0; i0 < steps; i0 += IIR_UNROLL) {         // (steps past the last are past every len)
            int x[IIR_UNROLL], y[IIR_UNROLL];
            IirSec cf[IIR_UNROLL];
#pragma unroll
            for (u32 q = 0; q < IIR_UNROLL; q++) {
                x[q] = 0;
                if (k == 0 && i0 + q < len)
                    x[q] = row[(i0 + q) * (u32)C];
                cf[q] = rs.at(t * IIR_TILE + (i0 + q - k));      // (a frame below 0 or past len: some section, not used)
            }
#pragma unroll
            for (u32 q = 0; q < IIR_UNROLL; q++) {
                int u = iir_input(x[q]);
                if constexpr (NP > 1) {
                    const int below = __builtin_amdgcn_update_dpp(0, vprev, 0x111, 0xf, 0xf, true);     // row_shr:1
                    u = k == 0 ? u : below;
                }
                const u32 f = i0 + q - k;                // (wraps below frame 0: not below len)
                IirState nx = st;
                u32 over, clip;
                const int v = iir_section(cf[q], u, nx, &over);
                y[q] = iir_output(v, &clip);
                if (f < len) {
                    st = nx;
                    vprev = v;
                    ov += over;
                    cl += k == (u32)NP - 1u ? clip : 0u;
                }
            }
            if (k == (u32)NP - 1u) {
#pragma unroll
                for (u32 q = 0; q < IIR_UNROLL; q++) {
                    const u32 f = i0 + q - k;
                    if (f < len)
                        row[f * (u32)C] = (int16_t)y[q];
                }
            }
        }
        clips += cl;
        overs += ov;
        __syncthreads();
        iir_tile_store(a, lds, s0, SPW, (u32)C, t);
        __syncthreads();
    }
    if (real && count != 0)
        *home = st;
    if (live) {
        iir_count(a.clips + s, clips);
        iir_count(a.overs + s, overs);
    }
}

// ---------------------------------------------------------------------------
// The any form's ends in LDS: the launcher takes this kernel for C >= 3 only, so a workgroup has at most 21 streams of at
// most 8 sections.  A section is twelve words there -- c0, c1, and its clock (done, inc) in place of (done, R) -- read
// back as three 16-byte vectors; a stream's sections lie 12 N + 4 words apart, so that the up to six streams of a
// 16-lane group, each of which reads its own address, start in different banks whatever N is.
constexpr u32 IIRR_MAX_SPW = IIR_BLOCK / 3u;
constexpr u32 IIRR_PITCH_MAX = IIR_RAMP_WORDS * IIR_MAX_SEC + 4u;
__device__ __forceinline__ u32 iirr_pitch(u32 N) { return IIR_RAMP_WORDS * N + 4u; }

__global__ __launch_bounds__(IIR_BLOCK) void k_iirr_any(IirArgs a)
{
    __shared__ __attribute__((aligned(4))) int16_t lds[IIR_LDS_SAMPLES];
    __shared__ __attribute__((aligned(16))) int32_t ends[IIRR_MAX_SPW * IIRR_PITCH_MAX];
    const u32 C = a.channels, N = a.sections, spw = IIR_BLOCK / C;
    const u32 lane = threadIdx.x, j = lane / C, c = lane - j * C;
    const u32 s0 = blockIdx.x * spw, s = s0 + j;
    const bool live = j < spw && s < a.streams;
    const u32 count = live ? a.counts[s] : 0u;
    const u32 most = wave_max_u32(count);
    if (most == 0 || spw > IIRR_MAX_SPW)             // (uniform; the second never: plan_iir sends C <= 2 to the fast form)
        return;
    // the workgroup's sections into LDS: entry i is section i % N of stream s0 + i / N
    const u32 here = a.streams - s0 < spw ? a.streams - s0 : spw;
    for (u32 i = lane; i < here * N; i += IIR_BLOCK) {
        const int32_t *e = a.coef + ((u64)s0 * N + i) * IIR_RAMP_WORDS;
        int32_t *l = ends + (i / N) * iirr_pitch(N) + (i % N) * IIR_RAMP_WORDS;
#pragma unroll
        for (u32 w = 0; w < 10u; w++)
            l[w] = e[w];
        const IirRampClock clock = iir_ramp_clock((u32)e[10], (u32)e[11]);
        l[10] = (int32_t)clock.done;
        l[11] = (int32_t)clock.inc;
    }
    const int32_t *mine = ends + (live ? j : 0u) * iirr_pitch(N);
    IirState st[IIR_MAX_SEC];
    IirState *home = a.state + ((u64)s * C + c) * N;
#pragma unroll
    for (u32 k = 0; k < IIR_MAX_SEC; k++) {
        st[k] = IirState{0, 0, 0, 0, 0};
        if (live && k < N)
            st[k] = home[k];
    }
    int16_t *row = lds + j * iir_lds_pitch(C) + c;
    u64 clips = 0, overs = 0;
    const u32 tiles = (most + IIR_TILE - 1u) / IIR_TILE;
    u32x4 ahead[IIR_MOVE];
    iir_tile_fetch(a, ahead, s0, spw, C, 0);
    for (u32 t = 0; t < tiles; t++) {
        iir_tile_commit(a, ahead, lds, s0, spw, C, t);
        __syncthreads();                             // (also: the ends are in LDS)
        if (t + 1u < tiles)
            iir_tile_fetch(a, ahead, s0, spw, C, t + 1u);
        const u32 len = iir_tile_frames(count, t);
        u32 cl = 0, ov = 0;
        for (u32 i0 = 0; i0 < len; i0 += IIR_UNROLL) {
            int x[IIR_UNROLL];
#pragma unroll
            for (u32 q = 0; q < IIR_UNROLL; q++) {
                x[q] = 0;
                if (i0 + q < len)
                    x[q] = row[(i0 + q) * C];
            }
#pragma unroll
            for (u32 q = 0; q < IIR_UNROLL; q++) {
                if (i0 + q < len) {
                    int u = iir_input(x[q]);
#pragma unroll
                    for (u32 k = 0; k < IIR_MAX_SEC; k++) {
                        if (k < N) {                     // (uniform)
                            const int4 *e = reinterpret_cast<const int4 *>(mine + k * IIR_RAMP_WORDS);
                            const int4 e0 = e[0], e1 = e[1], e2 = e[2];
                            const IirSec c0 = {e0.x, e0.y, e0.z, e0.w, e1.x}, c1 = {e1.y, e1.z, e1.w, e2.x, e2.y};
                            const IirRampClock clock = {(u32)e2.z, (u32)e2.w};
                            const IirSec cf = iir_ramp_section(c0, c1, iir_ramp_at(clock, t * IIR_TILE + i0 + q));
                            u32 over;
                            u = iir_section(cf, u, st[k], &over);
                            ov += over;
                        }
                    }
                    u32 clip;
                    x[q] = iir_output(u, &clip);
                    cl += clip;
                }
            }
#pragma unroll
            for (u32 q = 0; q < IIR_UNROLL; q++)
                if (i0 + q < len)
                    row[(i0 + q) * C] = (int16_t)x[q];
        }
        clips += cl;
        overs += ov;
        __syncthreads();
        iir_tile_store(a, lds, s0, spw, C, t);
        __syncthreads();
    }
    if (live && count != 0) {
#pragma unroll
        for (u32 k = 0; k < IIR_MAX_SEC; k++)
            if (k < N)
                home[k] = st[k];
    }
    if (live) {
        iir_count(a.clips + s, clips);
        iir_count(a.overs + s, overs);
    }
}

// ---------------------------------------------------------------------------
// launcher

template <int C>
static void launch_iirr_fast(const IirArgs &a, const IirPlan &p, hipStream_t st)
{
    switch (p.np) {
    case 1: hipLaunchKernelGGL((k_iirr_fast<C, 1>), dim3(p.grid), dim3(p.block), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_iirr_fast<C, 2>), dim3(p.grid), dim3(p.block), 0, st, a); break;
    case 4: hipLaunchKernelGGL((k_iirr_fast<C, 4>), dim3(p.grid), dim3(p.block), 0, st, a); break;
    default: hipLaunchKernelGGL((k_iirr_fast<C, 8>), dim3(p.grid), dim3(p.block), 0, st, a); break;
    }
}

void launch_iir_ramp(const IirArgs &a, const IirPlan &p, hipStream_t st)
{
    if (!p.fast)
        hipLaunchKernelGGL(k_iirr_any, dim3(p.grid), dim3(p.block), 0, st, a);
    else if (a.channels == 1)
        launch_iirr_fast<1>(a, p, st);
    else
        launch_iirr_fast<2>(a, p, st);
}

// test hooks (host logic, need no GPU): the section between two ends and the position, as the kernels compute them
extern "C" void cmhip_test_iir_ramp_at(const int32_t *c0, const int32_t *c1, uint32_t done, uint32_t R, uint32_t f,
                                       int32_t *out, uint32_t *p)
{
    if (!c0 || !c1 || !out)
        return;
    const IirSec a = {c0[0], c0[1], c0[2], c0[3], c0[4]}, b = {c1[0], c1[1], c1[2], c1[3], c1[4]};
    const uint32_t at = iir_ramp_at(iir_ramp_clock(done, R), f);
    const IirSec c = iir_ramp_section(a, b, at);
    out[0] = c.b0; out[1] = c.b1; out[2] = c.b2; out[3] = c.a1; out[4] = c.a2;
    if (p)
        *p = at;
}

}  // namespace cmhip
