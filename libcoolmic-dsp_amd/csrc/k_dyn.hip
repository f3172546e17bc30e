// k_dyn.hip -- gfx950 (MI355X, wave64) dynamics stage, compressor and gate: S streams of C interleaved int16 channels
// in, the same out, delayed by D = B - 1 frames and multiplied by a gain of at most unity that follows the level through
// a per-stream curve, in exact integers (include/coolmic_hip.h, "dynamics", has the arithmetic to the bit;
// csrc/dyn_plan.h the geometry and the curve's index function):
//     e = max_c |x_k[n][c]|, k = key[s] or s itself    L = (sum of e over the last A frames) >> a, or
//                                                      L = isqrt((sum of e^2 over the last A frames) >> a)
//     l = max of L over the last W frames              g = curve_s(l)
//     s = (sum of g over the last B frames) >> b       y[n][ch] = (x_s[n-D][ch] * s[n] + 2^14) >> 15
//
//   k_dyn<CT, DET>   CT in {1, 2}: the tile's frames come in and leave as whole 16-byte vectors; CT = 0: 3..16 channels,
//                    sample by sample, no speed goal.  DET: DYN_DETECT_MEAN or DYN_DETECT_RMS
//   k_dynk<CT, DET>  the same with side-chain keys: the detector of stream s reads stream key[s] (uint32 [S])
//   k_dyn_set        writes one curve, handed over as a kernel argument, into a range of streams
//   k_dynk_set       writes the key of a range of streams into the map; the key is a kernel argument
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
//
// Keys.  A workgroup reads key[s] before anything else, so that step 1's loads depend on it and on kernel arguments
// alone and the curve still follows them.  Step 1 reads the key's run slot and the key's history slot: both hold raw
// input frames, the history in the slot the host's parity selects for reading, which no workgroup of the run writes --
// so a tile of s may read the history of k while k's last tile writes k's other slot.
//
// RMS.  e^2 reaches 2^30 and a sum over A = 1024 frames 2^40, past the 32 bits a pass adds in.  The square is split,
//     e^2 = hi * 2^15 + lo,  lo < 2^15,  hi <= 2^15,
// so each half sums to at most 2^25 over A frames and step 2's add pass runs unchanged once per half.  Then
// M = (sum_hi << (15 - a)) + (sum_lo >> a) -- exact, because a <= 10 < 15 makes sum_hi * 2^15 a multiple of 2^a -- and
// L = dyn_isqrt(M) (csrc/dyn_plan.h: a float seed and an integer repair that holds for every 32-bit value).
// The other form, 64-bit elements for the a passes, would have cost a second dword of LDS per frame (61 440 B at the
// largest geometry: one workgroup per CU where two dwords stay, and ds_read_b64 moves twice the bytes per pass) to save
// a passes out of 20 to 37; the split form costs a passes and 30 registers and leaves the LDS and the plan alone.
#include "k_dyn.h"

namespace cmhip {

template <int CT, u32 DET>
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn(DynArgs a)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<CT, false, DET>(a, nullptr, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

template <int CT, u32 DET>
__global__ __launch_bounds__(DYN_BLOCK) void k_dynk(DynArgs a, const u32 *key)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<CT, true, DET>(a, key, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

// one curve (a kernel argument: it travels with the launch) into streams first .. first + count - 1, dword by dword
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_set(u32 *curve, u32 first, u32 count, DynCurveArg c)
{
    constexpr u32 WORDS = DYN_CURVE / 2u;
    const u64 i = (u64)blockIdx.x * DYN_BLOCK + threadIdx.x;
    if (i < (u64)count * WORDS)
        curve[(u64)first * WORDS + i] = c.w[i & (WORDS - 1u)];
}

// the key of streams first .. first + count - 1: `key`, or each stream itself where own != 0
__global__ __launch_bounds__(DYN_BLOCK) void k_dynk_set(u32 *map, u32 first, u32 count, u32 key, u32 own)
{
    const u32 i = blockIdx.x * DYN_BLOCK + threadIdx.x;
    if (i < count)
        map[first + i] = own ? first + i : key;
}

// ---------------------------------------------------------------------------
// launchers

// one detector's mono, stereo or any-channel-count kernel, keyed where there is a map
template <u32 DET>
static void dyn_launch(const DynPlan &p, const DynArgs &b, const u32 *key, hipStream_t st)
{
    const u32 C = b.channels;
    if (key)
        hipLaunchKernelGGL(C == 1 ? (k_dynk<1, DET>) : C == 2 ? (k_dynk<2, DET>) : (k_dynk<0, DET>), dim3(p.grid),
                           dim3(p.block), p.lds_bytes, st, b, key);
    else
        hipLaunchKernelGGL(C == 1 ? (k_dyn<1, DET>) : C == 2 ? (k_dyn<2, DET>) : (k_dyn<0, DET>), dim3(p.grid),
                           dim3(p.block), p.lds_bytes, st, b);
}

hipError_t launch_dyn(const DynArgs &a, uint32_t detector, const uint32_t *key, hipStream_t st)
{
    const DynPlan p = plan_dyn(a.streams, a.channels, a.a, a.b, a.W - (1u << a.b), a.frames, detector);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    DynArgs b = a;
    b.halo = p.halo;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    if (detector == DYN_DETECT_RMS)
        dyn_launch<DYN_DETECT_RMS>(p, b, key, st);
    else
        dyn_launch<DYN_DETECT_MEAN>(p, b, key, st);
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

hipError_t launch_dyn_set_key(uint32_t *map, uint32_t first, uint32_t count, uint32_t key, bool own, hipStream_t st)
{
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_dynk_set, dim3((count + DYN_BLOCK - 1u) / DYN_BLOCK), dim3(DYN_BLOCK), 0, st, map, first, count,
                       key, own ? 1u : 0u);
    return hipGetLastError();
}

// test hooks (host logic, need no GPU): the plan of a dynamics run whose longest stream has `frames` frames, with the
// mean and with the RMS detector, and the root the kernels take
extern "C" void cmhip_test_plan_dyn(uint32_t streams, uint32_t channels, uint32_t detector_log2, uint32_t smooth_log2,
                                    uint32_t hold, uint32_t frames, DynPlan *plan)
{
    if (plan)
        *plan = plan_dyn(streams, channels, detector_log2, smooth_log2, hold, frames);
}

extern "C" void cmhip_test_plan_dynrms(uint32_t streams, uint32_t channels, uint32_t detector_log2, uint32_t smooth_log2,
                                       uint32_t hold, uint32_t frames, DynPlan *plan)
{
    if (plan)
        *plan = plan_dyn(streams, channels, detector_log2, smooth_log2, hold, frames, DYN_DETECT_RMS);
}

extern "C" uint32_t cmhip_test_dyn_isqrt(uint32_t v) { return dyn_isqrt(v); }

}  // namespace cmhip
