// k_dynrms.hip -- gfx950 (MI355X, wave64) dynamics stage with the RMS detector: the level is the root of the mean square
// of the loudest channel over the last A frames, in exact integers (include/coolmic_hip.h, "dynamics", "RMS detector",
// has the arithmetic to the bit).  Only the second line of the arithmetic changes:
//     M = (sum of e^2 over the last A frames) >> a       L = isqrt(M), the largest r with r * r <= M
//     e, l, g = curve(l), s and y = (x[n-D] * s[n] + 2^14) >> 15 as before; with a key, e is the key's
//
//   k_dynrms_fast<C>    C in {1, 2}
//   k_dynrms_any        3..16 channels
//   k_dynrmsk_fast<C>   the same with side-chain keys (the detector reads stream key[s])
//   k_dynrmsk_any
//
// The decomposition is k_dyn.hip's and the body is csrc/k_dyn.h's with DET = DYN_DETECT_RMS; the plan, the tile, the
// LDS (one dword per frame, 30 720 B at most) and the grid are the mean detector's.  What is new is the sum of squares:
// e^2 reaches 2^30 and a sum over A = 1024 frames 2^40, past the 32 bits a pass adds in.  The square is split,
//     e^2 = hi * 2^15 + lo,  lo < 2^15,  hi <= 2^15,
// so each half sums to at most 2^25 over A frames, and step 2's add pass runs unchanged once per half: first the a
// passes over lo, with e kept in registers beside the running sums, then the a passes over hi, with sum_lo kept there.
// Then M = (sum_hi << (15 - a)) + (sum_lo >> a) -- exact, because a <= 10 < 15 makes sum_hi * 2^15 a multiple of 2^a --
// and L = dyn_isqrt(M) (csrc/dyn_plan.h: a float seed and an integer repair that holds for every 32-bit value), once per
// element and tile.  From there on the sliding maximum, the curve, the ramp, the meter, steps 3 and 4 are the same text.
// The other form, 64-bit elements for the a passes, would have cost a second dword of LDS per frame (61 440 B at the
// largest geometry: one workgroup per CU where two dwords stay, and ds_read_b64 moves twice the bytes per pass) to save
// a passes out of 20 to 37; the split form costs a passes and 30 registers and leaves the LDS and the plan alone.
// The unguarded reads stay harmless: an element without a partner, or a slot past N, takes the same entries in both
// rounds, so its two sums belong to one set of at most A squares and its M is at most 2^30 like everybody's.
// The keyed kernels are launched only while a key is set (cmhip_dyn_run decides, as for the mean detector).
#include "k_dyn.h"

namespace cmhip {

template <int C>
__global__ __launch_bounds__(DYN_BLOCK) void k_dynrms_fast(DynArgs a)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<C, false, DYN_DETECT_RMS>(a, nullptr, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

__global__ __launch_bounds__(DYN_BLOCK) void k_dynrms_any(DynArgs a)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<0, false, DYN_DETECT_RMS>(a, nullptr, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

template <int C>
__global__ __launch_bounds__(DYN_BLOCK) void k_dynrmsk_fast(DynArgs a, const u32 *key)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<C, true, DYN_DETECT_RMS>(a, key, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

__global__ __launch_bounds__(DYN_BLOCK) void k_dynrmsk_any(DynArgs a, const u32 *key)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<0, true, DYN_DETECT_RMS>(a, key, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

// ---------------------------------------------------------------------------
// launcher

// key == nullptr: the unkeyed kernels
hipError_t launch_dynrms(const DynArgs &a, const uint32_t *key, hipStream_t st)
{
    const DynPlan p = plan_dyn(a.streams, a.channels, a.a, a.b, a.W - (1u << a.b), a.frames, DYN_DETECT_RMS);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    DynArgs b = a;
    b.halo = p.halo;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    if (key) {
        switch (a.channels) {
        case 1: hipLaunchKernelGGL((k_dynrmsk_fast<1>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b, key); break;
        case 2: hipLaunchKernelGGL((k_dynrmsk_fast<2>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b, key); break;
        default: hipLaunchKernelGGL(k_dynrmsk_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b, key); break;
        }
    } else {
        switch (a.channels) {
        case 1: hipLaunchKernelGGL((k_dynrms_fast<1>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
        case 2: hipLaunchKernelGGL((k_dynrms_fast<2>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
        default: hipLaunchKernelGGL(k_dynrms_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
        }
    }
    return hipGetLastError();
}

// test hooks (host logic, need no GPU): the plan of a run with the RMS detector, and the root the kernels take
extern "C" void cmhip_test_plan_dynrms(uint32_t streams, uint32_t channels, uint32_t detector_log2, uint32_t smooth_log2,
                                       uint32_t hold, uint32_t frames, DynPlan *plan)
{
    if (plan)
        *plan = plan_dyn(streams, channels, detector_log2, smooth_log2, hold, frames, DYN_DETECT_RMS);
}

extern "C" uint32_t cmhip_test_dyn_isqrt(uint32_t v) { return dyn_isqrt(v); }

}  // namespace cmhip
