// k_lim.hip -- gfx950 (MI355X, wave64) look-ahead peak limiter: S streams of C interleaved int16 channels in, the same
// out, delayed by D = A - 1 frames and held under a ceiling T, in exact integers (include/coolmic_hip.h, "peak
// limiter", has the arithmetic to the bit; csrc/lim_plan.h the geometry; csrc/k_lim_tile.h the tile and its steps):
//     pr = (drive * max_c |x[n][c]| + 4095) >> 12       g = pr <= T ? 32768 : floor(T * 32768 / pr)
//     m  = min of g over the last W frames              s = (sum of m over the last A frames) >> a
//     y[n][ch] = (x[n-D][ch] * (drive * s[n]) + 2^26) >> 27
//
//   k_lim_fast<C>   C in {1, 2}: the tile's frames come in and leave as whole 16-byte vectors
//   k_lim_any       3..16 channels: sample by sample; no speed goal
//   k_lim_set       writes one parameter word, handed over as a kernel argument, into a range of streams
//
// The tile is the sample detector's, without a release stage, with LIM_R = 26 element slots per thread.
#include "k_lim_tile.h"

namespace cmhip {

template <int C>
__global__ __launch_bounds__(LIM_BLOCK) void k_lim_fast(LimArgs a)
{
    extern __shared__ u32x4 lim_lds[];
    __shared__ u32 red[4];
    lim_tile<false, false, LIM_R, C>(a, reinterpret_cast<u32 *>(lim_lds), red);
}

__global__ __launch_bounds__(LIM_BLOCK) void k_lim_any(LimArgs a)
{
    extern __shared__ u32x4 lim_lds[];
    __shared__ u32 red[4];
    lim_tile<false, false, LIM_R, 0>(a, reinterpret_cast<u32 *>(lim_lds), red);
}

// one parameter word (a kernel argument: it travels with the launch) into streams first .. first + count - 1
__global__ __launch_bounds__(LIM_BLOCK) void k_lim_set(u32 *par, u32 first, u32 count, u32 word)
{
    const u32 i = blockIdx.x * LIM_BLOCK + threadIdx.x;
    if (i < count)
        par[(u64)first + i] = word;
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_lim(const LimArgs &a, hipStream_t st)
{
    return lim_launch<LimArgs>(plan_lim(a.streams, a.channels, a.a, a.W - (1u << a.a), a.frames), a, st, k_lim_fast<1>,
                               k_lim_fast<2>, k_lim_any);
}

hipError_t launch_lim_set(uint32_t *par, uint32_t first, uint32_t count, uint32_t threshold, uint32_t drive, hipStream_t st)
{
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_lim_set, dim3((count + LIM_BLOCK - 1u) / LIM_BLOCK), dim3(LIM_BLOCK), 0, st, par, first, count,
                       threshold | drive << 16);
    return hipGetLastError();
}

// test hook: the plan of a limiter run whose longest stream has `frames` frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_lim(uint32_t streams, uint32_t channels, uint32_t lookahead_log2, uint32_t hold,
                                    uint32_t frames, LimPlan *plan)
{
    if (plan)
        *plan = plan_lim(streams, channels, lookahead_log2, hold, frames);
}

}  // namespace cmhip
