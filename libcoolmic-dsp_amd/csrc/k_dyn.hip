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
// The decomposition is the limiter's (k_lim_tile.h).
// A workgroup of 256 threads takes one stream and a tile of tile_frames frames, and
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
// The helpers and the tile body are csrc/k_dyn.h's, shared with k_dynkey.hip (the side-chain: the detector reads another
// stream); this file instantiates the unkeyed form.
#include "k_dyn.h"

namespace cmhip {

template <int C>
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_fast(DynArgs a)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<C, false>(a, nullptr, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_any(DynArgs a)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<0, false>(a, nullptr, reinterpret_cast<u32 *>(dyn_lds), cv, red);
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
