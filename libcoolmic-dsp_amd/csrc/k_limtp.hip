// k_limtp.hip -- gfx950 (MI355X, wave64) look-ahead limiter with the TRUE-PEAK detector: the limiter's tile with the
// true-peak step 1 (include/coolmic_hip.h, "peak limiter", "true-peak detector", has the arithmetic to the bit;
// csrc/lim_plan.h the geometry; csrc/k_lim_tile.h the tile, its steps and the pair-dword form of the FIR):
//     y_p[n][c] = sum_{k<12} H[p][k] * x[n-k][c]        p = 0..3: BS.1770 Annex 2's 4x oversampling, exact int32
//     t[n]  = max_c max(|x[n-8][c]| << 13, max_p |y_p[n-2][c]|)
//     pr    = (drive * t[n] + 2^25 - 1) >> 25           g = pr <= T ? 32768 : floor(T * 32768 / pr)
//     m, s as in k_lim.hip                              y[n][ch] = (x[n-Dtp][ch] * (drive * s[n]) + 2^26) >> 27
// with Dtp = A + 7 and HIST = A + W - 2 + 13.  Dtp + 1 = A + 8 is a multiple of 8 frames as D + 1 = A is in k_lim.hip,
// so step 3's "the two vectors an output vector's samples lie in" holds unchanged.
//
//   k_limtp_fast<C>   C in {1, 2}: whole 16-byte vectors in and out, the FIR in k_tpeak.hip's pair-dword dot form;
//                     a thread owns at most 4 (mono), 7 (stereo) consecutive vectors
//   k_limtp_any       3..16 channels: sample by sample in plain multiply-adds; no speed goal
//
// No release stage, LIM_R = 26 element slots per thread.
#include "k_lim_tile.h"

namespace cmhip {

template <int C>
__global__ __launch_bounds__(LIM_BLOCK) void k_limtp_fast(LimArgs a)
{
    extern __shared__ u32x4 limtp_lds[];
    __shared__ u32 red[4];
    lim_tile<true, false, LIM_R, C>(a, reinterpret_cast<u32 *>(limtp_lds), red);
}

__global__ __launch_bounds__(LIM_BLOCK) void k_limtp_any(LimArgs a)
{
    extern __shared__ u32x4 limtp_lds[];
    __shared__ u32 red[4];
    lim_tile<true, false, LIM_R, 0>(a, reinterpret_cast<u32 *>(limtp_lds), red);
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_limtp(const LimArgs &a, hipStream_t st)
{
    return lim_launch<LimArgs>(plan_limtp(a.streams, a.channels, a.a, a.W - (1u << a.a), a.frames), a, st,
                               k_limtp_fast<1>, k_limtp_fast<2>, k_limtp_any);
}

// test hook: the plan of a true-peak limiter run whose longest stream has `frames` frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_limtp(uint32_t streams, uint32_t channels, uint32_t lookahead_log2, uint32_t hold,
                                      uint32_t frames, LimPlan *plan)
{
    if (plan)
        *plan = plan_limtp(streams, channels, lookahead_log2, hold, frames);
}

}  // namespace cmhip
