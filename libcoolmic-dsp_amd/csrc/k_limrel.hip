// k_limrel.hip -- gfx950 (MI355X, wave64) look-ahead limiter with the RELEASE STAGE, for both detectors: the limiter's
// tile with 32 element slots per thread and rho release passes between the minimum passes and the sum passes
// (include/coolmic_hip.h, "peak limiter", "release stage", has the arithmetic to the bit; csrc/lim_plan.h the geometry;
// csrc/k_lim_tile.h the tile, its steps and why the ramp doubles as a window does):
//     g, m as in k_lim.hip (the sample detector) or k_limtp.hip (the true-peak detector)
//     r[n] = min over 0 <= k < R of (m[n-k] + k*q)         R = 2^rho frames, q = 32768 >> rho per frame
//     s    = (sum of r over the last A frames) >> a         y[n][ch] = (x[n-D][ch] * (drive * s[n]) + 2^26) >> 27
// with HIST = A + W - 2 + (R - 1) (+ 13 for the true-peak detector) <= 4096 and D as without the stage.
//
//   k_limrel_fast<C>, k_limrel_any       the sample detector
//   k_limtprel_fast<C>, k_limtprel_any   the true-peak detector
//
// A limiter with rho = 0 never comes here: it launches k_lim.hip's or k_limtp.hip's kernels (launch_limrel).
//
// The tile is 4096 frames for every geometry and a workgroup evaluates N = halo + 4096 <= 8192 elements, one dword of
// dynamic LDS each (32 KiB at most); thread t keeps elements j = t + 256 i, i < LIMREL_SLOTS = 32, and a fast form takes
// at most 4 (mono), 8 (stereo) vectors per thread in step 1.
#include "k_lim_tile.h"

namespace cmhip {

template <int C>
__global__ __launch_bounds__(LIM_BLOCK) void k_limrel_fast(LimRelArgs a)
{
    extern __shared__ u32x4 limrel_lds[];
    __shared__ u32 red[4];
    lim_tile<false, true, LIMREL_SLOTS, C>(a, reinterpret_cast<u32 *>(limrel_lds), red);
}

__global__ __launch_bounds__(LIM_BLOCK) void k_limrel_any(LimRelArgs a)
{
    extern __shared__ u32x4 limrel_lds[];
    __shared__ u32 red[4];
    lim_tile<false, true, LIMREL_SLOTS, 0>(a, reinterpret_cast<u32 *>(limrel_lds), red);
}

template <int C>
__global__ __launch_bounds__(LIM_BLOCK) void k_limtprel_fast(LimRelArgs a)
{
    extern __shared__ u32x4 limrel_lds[];
    __shared__ u32 red[4];
    lim_tile<true, true, LIMREL_SLOTS, C>(a, reinterpret_cast<u32 *>(limrel_lds), red);
}

__global__ __launch_bounds__(LIM_BLOCK) void k_limtprel_any(LimRelArgs a)
{
    extern __shared__ u32x4 limrel_lds[];
    __shared__ u32 red[4];
    lim_tile<true, true, LIMREL_SLOTS, 0>(a, reinterpret_cast<u32 *>(limrel_lds), red);
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_limrel(const LimArgs &a, uint32_t detector, uint32_t release_log2, hipStream_t st)
{
    if (release_log2 == 0)                           // the limiter without the stage: the kernels it always had
        return detector == LIM_DETECT_TRUE_PEAK ? launch_limtp(a, st) : launch_lim(a, st);
    const LimPlan p = plan_limrel(detector, a.streams, a.channels, a.a, a.W - (1u << a.a), release_log2, a.frames);
    LimRelArgs b;
    static_cast<LimArgs &>(b) = a;
    b.rho = release_log2;
    if (detector == LIM_DETECT_TRUE_PEAK)
        return lim_launch<LimRelArgs>(p, b, st, k_limtprel_fast<1>, k_limtprel_fast<2>, k_limtprel_any);
    return lim_launch<LimRelArgs>(p, b, st, k_limrel_fast<1>, k_limrel_fast<2>, k_limrel_any);
}

// test hook: the plan of a run of a limiter with a release stage (host logic, needs no GPU)
extern "C" void cmhip_test_plan_limrel(uint32_t detector, uint32_t streams, uint32_t channels, uint32_t lookahead_log2,
                                       uint32_t hold, uint32_t release_log2, uint32_t frames, LimPlan *plan)
{
    if (plan)
        *plan = plan_limrel(detector, streams, channels, lookahead_log2, hold, release_log2, frames);
}

}  // namespace cmhip
