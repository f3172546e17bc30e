// k_iir.hip -- gfx950 (MI355X, wave64) filter kernels: S streams of C interleaved int16 channels through a cascade of
// N biquad sections in exact integers (include/coolmic_hip.h, "filter", has the arithmetic to the bit; csrc/iir_plan.h
// the section, the output step and the tiles as code).  One launch per run:
//
//   k_iir_fast<C, NP>   C in {1, 2}: a lane is (row, section), NP = N rounded up to 1, 2, 4, 8 lanes per row
//   k_iir_any           every channel count up to 16: a lane is a row and loops over its sections
//
// Time is a recurrence and the floor is not linear, so nothing is parallel along a stream: the parallelism is the rows
// (a channel of a stream) and, in the fast form, the sections.  A workgroup is one wave and owns whole streams
// (iir_plan's spw), so exactly one lane owns a section's state in a launch: read at the start, written at the end, no
// atomics but the two counters'.
//
// The interleaved PCM enters and leaves in 16-byte vectors through an LDS tile of IIR_TILE frames per stream, worked on
// in place: the lanes deal the workgroup's vectors among themselves, a vector that the stream's count cuts goes sample
// by sample, one past it not at all (iir_tile_vec).  A tile's whole vectors are loaded into registers, all at once, while
// the tile before it is walked, so no global latency stands between two tiles.  The streams' tiles lie iir_lds_pitch
// apart in LDS: all rows of a wave access their frame i in the same instruction, and at a pitch of B C samples -- a
// multiple of the 128 bytes that the 32 banks span -- every one of them would hit the same bank.  Between the two moves every row walks its tile frame by frame with
// 2-byte LDS accesses, four frames' reads in front of their four chains and the four writes behind them: one wait for
// LDS per four frames.
//
// Fast form: at step i of a tile section k works on frame i - k, on what the lane below it -- section k - 1 of the same
// row -- made at step i - 1, handed over by a DPP row shift (NP divides a DPP row of 16 lanes: the neighbour is never in
// another row).  A tile of f frames takes f + NP - 1 steps, so the pipeline is empty at the end of every tile: a run's
// cut changes nothing.  The DPP move stands outside every divergent branch.
#include "k_iir.h"

namespace cmhip {

// (the tile between the slots and LDS: k_iir.h, shared with the ramp kernels of k_iirramp.hip)

// ---------------------------------------------------------------------------
template <int C, int NP>
__global__ __launch_bounds__(IIR_BLOCK) void k_iir_fast(IirArgs a)
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
    IirSec cf = IIR_UNITY;                           // sections N..NP-1: the identity, e stays 0
    IirState st = {0, 0, 0, 0, 0};
    IirState *home = a.state + ((u64)s * (u32)C + c) * N + k;
    if (real) {
        cf = iir_load_sec(a.coef + ((u64)s * N + k) * IIR_SEC_WORDS);
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
#pragma unroll
            for (u32 q = 0; q < IIR_UNROLL; q++) {
                x[q] = 0;
                if (k == 0 && i0 + q < len)
                    x[q] = row[(i0 + q) * (u32)C];
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
                const int v = iir_section(cf, u, nx, &over);
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
__global__ __launch_bounds__(IIR_BLOCK) void k_iir_any(IirArgs a)
{
    __shared__ __attribute__((aligned(4))) int16_t lds[IIR_LDS_SAMPLES];
    const u32 C = a.channels, N = a.sections, spw = IIR_BLOCK / C;
    const u32 lane = threadIdx.x, j = lane / C, c = lane - j * C;
    const u32 s0 = blockIdx.x * spw, s = s0 + j;
    const bool live = j < spw && s < a.streams;
    const u32 count = live ? a.counts[s] : 0u;
    const u32 most = wave_max_u32(count);
    if (most == 0)
        return;
    IirSec cf[IIR_MAX_SEC];
    IirState st[IIR_MAX_SEC];
    IirState *home = a.state + ((u64)s * C + c) * N;
#pragma unroll
    for (u32 k = 0; k < IIR_MAX_SEC; k++) {
        cf[k] = IIR_UNITY;
        st[k] = IirState{0, 0, 0, 0, 0};
        if (live && k < N) {
            cf[k] = iir_load_sec(a.coef + ((u64)s * N + k) * IIR_SEC_WORDS);
            st[k] = home[k];
        }
    }
    int16_t *row = lds + j * iir_lds_pitch(C) + c;
    u64 clips = 0, overs = 0;
    const u32 tiles = (most + IIR_TILE - 1u) / IIR_TILE;
    u32x4 ahead[IIR_MOVE];
    iir_tile_fetch(a, ahead, s0, spw, C, 0);
    for (u32 t = 0; t < tiles; t++) {
        iir_tile_commit(a, ahead, lds, s0, spw, C, t);
        __syncthreads();
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
                            u32 over;
                            u = iir_section(cf[k], u, st[k], &over);
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
static void launch_iir_fast(const IirArgs &a, const IirPlan &p, hipStream_t st)
{
    switch (p.np) {
    case 1: hipLaunchKernelGGL((k_iir_fast<C, 1>), dim3(p.grid), dim3(p.block), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_iir_fast<C, 2>), dim3(p.grid), dim3(p.block), 0, st, a); break;
    case 4: hipLaunchKernelGGL((k_iir_fast<C, 4>), dim3(p.grid), dim3(p.block), 0, st, a); break;
    default: hipLaunchKernelGGL((k_iir_fast<C, 8>), dim3(p.grid), dim3(p.block), 0, st, a); break;
    }
}

hipError_t launch_iir(const IirArgs &a, uint32_t frames, bool ramp, hipStream_t st)
{
    const IirPlan p = plan_iir(a.streams, a.channels, a.sections, frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    if (ramp)
        launch_iir_ramp(a, p, st);
    else if (!p.fast)
        hipLaunchKernelGGL(k_iir_any, dim3(p.grid), dim3(p.block), 0, st, a);
    else if (a.channels == 1)
        launch_iir_fast<1>(a, p, st);
    else
        launch_iir_fast<2>(a, p, st);
    return hipGetLastError();
}

// test hooks (host logic, need no GPU): the plan of a run whose longest stream has `frames` frames, a tile's vector,
// and the section and the output step as code
extern "C" void cmhip_test_plan_iir(uint32_t streams, uint32_t channels, uint32_t sections, uint32_t frames, IirPlan *plan)
{
    if (plan)
        *plan = plan_iir(streams, channels, sections, frames);
}

extern "C" void cmhip_test_iir_tile_vec(uint32_t count, uint32_t channels, uint32_t t, uint32_t q, uint32_t *off, uint32_t *n)
{
    const IirVec v = iir_tile_vec(count, channels, t, q);
    if (off)
        *off = v.off;
    if (n)
        *n = v.n;
}

// one frame through one section: sec int32 [5], state int32 [5] (u1, u2, v1, v2, e) updated in place -> v
extern "C" int32_t cmhip_test_iir_section(const int32_t *sec, int32_t u, int32_t *state, uint32_t *over)
{
    if (!sec || !state)
        return 0;
    IirState s = {state[0], state[1], state[2], state[3], (uint32_t)state[4]};
    uint32_t o;
    const int32_t v = iir_section(IirSec{sec[0], sec[1], sec[2], sec[3], sec[4]}, u, s, &o);
    state[0] = s.u1; state[1] = s.u2; state[2] = s.v1; state[3] = s.v2; state[4] = (int32_t)s.e;
    if (over)
        *over = o;
    return v;
}

extern "C" int32_t cmhip_test_iir_output(int32_t v, uint32_t *clip)
{
    uint32_t c;
    const int32_t y = iir_output(v, &c);
    if (clip)
        *clip = c;
    return y;
}

}  // namespace cmhip
