// k_corr.hip -- gfx950 (MI355X, wave64) phase-correlation kernels: per stream and channel pair (a, b) the sums of
// x_a^2, x_b^2 and x_a * x_b over the TRANSFORMED stream (channel map, gain, saturation), in exact 64-bit integers.
// A pass of its own, launched ahead of the block kernel of the same run: it reads the run's INPUT slots and transforms
// them itself with the block kernels' arithmetic (cmhip_device.h), so the samples are bit-identical to theirs and an
// in-place batch needs nothing special.
//
//   k_corr_fast   stereo with the one pair (0, 1) / (1, 0): one wave per 8 KiB tile of one stream
//   k_corr_any    every other case (3..16 channels, or stereo with several pairs): one workgroup per 1024 frames
//
// k_tpeak.hip's front end (load, map, gain, the tile cut, the ragged tile masked by the stream's count) without its
// halo and history: a frame's contribution depends on that frame alone.  Integer sums merged by integer atomics do
// not depend on the order the waves arrive in: the windows are reproducible to the bit.  DESIGN 4.16.
#include "cmhip_device.h"

namespace cmhip {

// ---------------------------------------------------------------------------
// Stereo, one pair.
//
// A wave owns a contiguous tile of CORR_U * 64 16-byte vectors of one stream (2048 frames); a lane owns the vectors
// lane, lane + 64, ... of it (32 frames), so each of the CORR_U load instructions reads 1 KiB in one piece.  (Frames
// are independent here: k_tpeak.hip's line per lane, which its FIR needs, has every load instruction touch 64 lines
// and measured 0.45 ms against 0.21 ms for 4096 x 65536 frames in this kernel)  A frame is one dword w = L | R << 16 after map and
// gain, and its three products are three v_dot2_i32_i16 of w against masked copies of itself:
//     L*L = dot2(w, w & 0xffff)      R*R = dot2(w, w & 0xffff0000)      L*R = dot2(w, w >> 16)
// (never 2*L*R in one dot: L = R = -32768 gives 2^31).  The dots chain through their accumulator over TWO frames, as
// 32-bit patterns (the instruction adds modulo 2^32), and what a chain holds is argued to be the exact sum:
//     squares   one is at most 2^30 (-32768 squared), two at most 2^31: below 2^32, the pattern is the sum as uint32.
//               (Three would still fit, four would not; 32 frames per lane divide by two.)
//     cross     one lies in [-2^30 + 2^15, 2^30], two in [-2^31 + 2^16, 2^31]: 2^31 is no int32.  The chain starts
//               from CORR_BIAS = 2^31 - 2^16 instead of 0, which moves the range to [0, 2^32 - 2^16]: the pattern is
//               bias + sum as uint32, no carry lost.  The biases (16 per lane, whatever the frames hold -- a frame
//               past the stream's count is a zero dword) come off the wave's total.
// Each chain's result is added to a 64-bit sum per lane (at most 16 * 2^32 = 2^36), the lanes' sums are reduced over
// the wave (wave_add_u40: below 2^40 per lane), and lane 0 issues one 64-bit atomicAdd per sum that is not zero.
constexpr u32 CORR_U = 8;                        // 16-byte vectors per lane
constexpr u32 CORR_TILE_VEC = 64 * CORR_U;       // vectors per wave: 8 KiB of PCM, 2048 stereo frames
constexpr u32 CORR_LANE_FRAMES = CORR_U * 4;     // stereo frames per lane
constexpr u32 CORR_BIAS = 0x7fff0000u;           // 2^31 - 2^16
static_assert(CORR_LANE_FRAMES % 2 == 0, "the dot chains take two frames");

__device__ __forceinline__ u32 corr_dot2(u32 x, u32 y, u32 acc)
{
    return (u32)__builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, y), (int)acc, false);
}

// FULL: every frame of the tile lies inside the stream's count -- no bounds tests.  Otherwise vectors past the
// count are not loaded and frames past it are zero dwords (what lies there is not the stream's).
template <bool FULL>
__device__ __forceinline__ void corr_tile(const CorrArgs &a, u32 s, u32 k, u32 nfr, u32 nvec, const int16_t *ins)
{
    const u32 lane = threadIdx.x & 63u;
    const u32 vl = k * CORR_TILE_VEC + lane;     // the lane's first vector; its others follow 64 apart
    const u32x4 *src = reinterpret_cast<const u32x4 *>(ins);

    u32 d[CORR_LANE_FRAMES];
#pragma unroll
    for (u32 i = 0; i < CORR_U; i++) {
        u32x4 w = {0, 0, 0, 0};
        if (FULL || vl + 64u * i < nvec)
            w = __builtin_nontemporal_load(src + vl + 64u * i);
        d[4 * i] = w.x; d[4 * i + 1] = w.y; d[4 * i + 2] = w.z; d[4 * i + 3] = w.w;
    }

    // the stream's parameters, read behind the tile's loads (as tp_tile does, k_tpeak.hip)
    __builtin_amdgcn_sched_barrier(0);
    const StreamParam *p = a.param + s;
    const u32 perm2 = p->perm2;
    const u32 mi01 = p->mi01;
    const u32 mf0 = p->mf[0], mf1 = p->mf[1];

    const u32 f0 = vl * 4u;                      // the lane's first frame in the stream; dword n of d is frame
                                                 // f0 + 256 * (n / 4) + n % 4
    u64 ea = 0, eb = 0, xb = 0;
#pragma unroll
    for (u32 i = 0; i < CORR_LANE_FRAMES; i += 2) {
        u32 w[2];
#pragma unroll
        for (u32 j = 0; j < 2; j++) {
            u32 x = d[i + j];
            if constexpr (!FULL)                 // (a select, not a branch; the gain of a zero sample is zero)
                x = f0 + 256u * ((i + j) >> 2) + ((i + j) & 3u) < nfr ? x : 0u;
            x = __builtin_amdgcn_perm(x, x, perm2);              // stereo channel map
            (void)gain2<true>(x, mi01, mf0, mf1, w[j]);
        }
        ea += corr_dot2(w[1], w[1] & 0xffffu, corr_dot2(w[0], w[0] & 0xffffu, 0u));
        eb += corr_dot2(w[1], w[1] & 0xffff0000u, corr_dot2(w[0], w[0] & 0xffff0000u, 0u));
        xb += corr_dot2(w[1], w[1] >> 16, corr_dot2(w[0], w[0] >> 16, CORR_BIAS));
    }

    const u64 sa = wave_add_u40(ea), sb = wave_add_u40(eb);
    const u64 sx = wave_add_u40(xb) - 64ull * (CORR_LANE_FRAMES / 2) * CORR_BIAS;    // (two's complement)
    if (lane == 0) {
        unsigned long long *win = a.sums + (u64)s * (CORR_MAX_PAIRS * CORR_SUMS);
        if (sa)
            atomicAdd(win, sa);
        if (sb)
            atomicAdd(win + 1, sb);
        if (sx)
            atomicAdd(win + 2, sx);
    }
}

__global__ __launch_bounds__(64) void k_corr_fast(CorrArgs a)
{
    const u32 s = blockIdx.x / a.chunks;         // stream
    const u32 k = blockIdx.x - s * a.chunks;     // tile inside the stream
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    const u32 nsamp = nfr * 2u;
    const u32 nvec = (nsamp + 7u) >> 3;          // 16-byte vectors that hold a sample of the stream
    const u32 v0 = k * CORR_TILE_VEC;
    const int16_t *ins = a.in + (u64)s * a.stride;
    if (v0 >= nvec)
        return;
    if (v0 + CORR_TILE_VEC <= (nsamp >> 3))
        corr_tile<true>(a, s, k, nfr, nvec, ins);
    else
        corr_tile<false>(a, s, k, nfr, nvec, ins);
}

// ---------------------------------------------------------------------------
// Any channel count, up to CORR_MAX_PAIRS pairs.  A workgroup of 256 threads takes CORR_ANY_FRAMES frames of one
// stream, its threads stride over them; pair by pair a thread transforms the two samples of its frames with gain1
// and sums the three products in 64 bits (a cross product moved by 2^30 to stay non-negative through the wave's
// reduction), the waves' totals meet in LDS and one global atomic per sum that is not zero follows.  The stream's
// map and gains go through LDS first: the pairs' channels are uniform run-time values, and a table in LDS is
// indexed without a scalar load at a register offset.  Bit-exact by the same integer arithmetic; no speed goal.
constexpr u32 CORR_ANY_FRAMES = 1024;
constexpr u32 CORR_ANY_PER = CORR_ANY_FRAMES / 256;          // frames per thread

__global__ __launch_bounds__(256) void k_corr_any(CorrArgs a, u64 pa, u64 pb)
{
    __shared__ unsigned long long lsum[CORR_MAX_PAIRS * CORR_SUMS];
    __shared__ u32 lmf[MAX_CH], lmi[MAX_CH], lmap[MAX_CH];
    const u32 C = a.channels;
    const u32 s = blockIdx.x / a.chunks;
    const u32 k = blockIdx.x - s * a.chunks;
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    const u32 f0 = k * CORR_ANY_FRAMES;          // the tile's first frame
    if (f0 >= nfr)                               // (uniform)
        return;
    const int16_t *ins = a.in + (u64)s * a.stride;
    const StreamParam *p = a.param + s;
    if (threadIdx.x < CORR_MAX_PAIRS * CORR_SUMS)
        lsum[threadIdx.x] = 0;
    if (threadIdx.x < C) {
        lmf[threadIdx.x] = p->mf[threadIdx.x];
        lmi[threadIdx.x] = p->mi[threadIdx.x];
        lmap[threadIdx.x] = p->chmap[threadIdx.x];
    }
    __syncthreads();

    for (u32 i = 0; i < a.npairs; i++) {         // (uniform)
        const u32 ca = (u32)(pa >> (8u * i)) & 0xffu, cb = (u32)(pb >> (8u * i)) & 0xffu;
        const u32 ia = lmap[ca], ib = lmap[cb];
        const u32 mia = lmi[ca], mib = lmi[cb], mfa = lmf[ca], mfb = lmf[cb];
        u64 ea = 0, eb = 0, xb = 0;              // per lane at most 4 * 2^30, 4 * 2^31
#pragma unroll
        for (u32 j = 0; j < CORR_ANY_PER; j++) {
            const u32 f = f0 + j * 256u + threadIdx.x;
            int xa = 0, xc = 0;
            if (f < nfr) {
                xa = gain1(ins[(u64)f * C + ia], mia, mfa);
                xc = gain1(ins[(u64)f * C + ib], mib, mfb);
            }
            ea += (u32)(xa * xa);                // at most 2^30
            eb += (u32)(xc * xc);
            xb += (u32)(xa * xc) + (1u << 30);   // [-2^30 + 2^15, 2^30] moved to [2^15, 2^31]
        }
        // (every lane of every wave arrives here: the DPP reductions see a full wave)
        const u64 sa = wave_add_u40(ea), sb = wave_add_u40(eb);
        const u64 sx = wave_add_u40(xb) - (64ull * CORR_ANY_PER << 30);      // (two's complement)
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(&lsum[i * CORR_SUMS], sa);
            atomicAdd(&lsum[i * CORR_SUMS + 1], sb);
            atomicAdd(&lsum[i * CORR_SUMS + 2], sx);
        }
    }
    __syncthreads();
    if (threadIdx.x < a.npairs * CORR_SUMS && lsum[threadIdx.x])
        atomicAdd(&a.sums[(u64)s * (CORR_MAX_PAIRS * CORR_SUMS) + threadIdx.x], lsum[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// launcher

CorrPlan plan_corr(const CorrArgs &a)
{
    CorrPlan p{};
    p.err = hipSuccess;
    if (a.streams == 0 || a.frames == 0 || a.channels < 2 || a.channels > MAX_CH || a.npairs == 0 ||
        a.npairs > CORR_MAX_PAIRS)
        return p;
    p.fast = a.channels == 2 && a.npairs == 1 ? 1u : 0u;
    const u64 nvec = ((u64)a.frames * 2 + 7) / 8;
    const u64 tiles = p.fast ? (nvec + CORR_TILE_VEC - 1) / CORR_TILE_VEC
                             : ((u64)a.frames + CORR_ANY_FRAMES - 1) / CORR_ANY_FRAMES;
    if (tiles * a.streams >= (1ull << 31)) {     // (as plan_run: no grid of 2^31 workgroups)
        CorrPlan refused{};
        refused.err = hipErrorInvalidValue;
        return refused;
    }
    p.chunks = (u32)tiles;
    p.grid = a.streams * p.chunks;
    p.block = p.fast ? 64u : 256u;
    return p;
}

hipError_t launch_corr(const CorrArgs &a, hipStream_t st)
{
    const CorrPlan p = plan_corr(a);
    if (p.grid == 0)
        return p.err;
    CorrArgs b = a;
    b.chunks = p.chunks;
    if (p.fast) {
        hipLaunchKernelGGL(k_corr_fast, dim3(p.grid), dim3(p.block), 0, st, b);
    } else {
        u64 pa = 0, pb = 0;                      // the pairs' channels, pair i in byte i
        for (u32 i = 0; i < a.npairs; i++) {
            pa |= (u64)a.a[i] << (8u * i);
            pb |= (u64)a.b[i] << (8u * i);
        }
        hipLaunchKernelGGL(k_corr_any, dim3(p.grid), dim3(p.block), 0, st, b, pa, pb);
    }
    return hipGetLastError();
}

// test hook: the plan of a correlation pass (host logic, needs no GPU)
extern "C" void cmhip_test_plan_corr(uint32_t streams, uint32_t channels, uint32_t frames, uint32_t npairs,
                                     CorrPlan *plan)
{
    CorrArgs a{};
    a.streams = streams;
    a.channels = channels;
    a.frames = frames;
    a.npairs = npairs;
    if (plan)
        *plan = plan_corr(a);
}

}  // namespace cmhip
