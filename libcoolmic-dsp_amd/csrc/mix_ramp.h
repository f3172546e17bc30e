// mix_ramp.h -- the arithmetic of a matrix ramp and the host's mirror of the streams' ramps (include/coolmic_hip.h,
// "matrix ramps").  Host only, plain C++17, no HIP: tests/cpp/mix_ramp_test.cpp compiles it with g++ alone.
//
//   inc  = ceil(2^32 / R)                       R in 2..2^20: inc <= 2^31
//   p(n) = min(32768, (n * inc) >> 17)          n = 1..R the ramp's frame, p in units of 2^-15, p(0) = 0
//   N    = w0 * (32768 - p) + w1 * p            |N| <= 2^30
//   w(p) = sgn(N) * (|N| >> 15)                 truncated towards zero: |w(p)| <= |N| / 32768, so a row's sum |w| is at
//                                               most the convex combination of the two ends' sums (<= 65535)
// A stream ramps while done < R: frame f (from 0) of its next run uses w(p(done + f + 1)), frames past the ramp W1.
// The device keeps the same four numbers per stream (k_mixramp.hip) and advances them by the same counts, so the
// mirror answers cmhip_mix_ramp_state without asking the device.
#ifndef CMHIP_MIX_RAMP_H
#define CMHIP_MIX_RAMP_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace cmhip {

constexpr uint32_t MIX_RAMP_MAX = 1u << 20;          // frames of a ramp at most
constexpr uint32_t MIX_RAMP_ONE = 32768;             // p at the ramp's end

inline uint32_t mix_ramp_inc(uint32_t R) { return (uint32_t)(((1ull << 32) + R - 1u) / R); }     // R >= 2

// p(n); n above R counts as R, R below 2 is a step (0 before it, the end from frame 1 on)
inline uint32_t mix_ramp_position(uint32_t n, uint32_t R)
{
    if (n == 0)
        return 0;
    if (R < 2)
        return MIX_RAMP_ONE;
    if (n > R)
        n = R;
    const uint64_t q = ((uint64_t)n * mix_ramp_inc(R)) >> 17;
    return q < MIX_RAMP_ONE ? (uint32_t)q : MIX_RAMP_ONE;
}

// w(p); p above 32768 counts as 32768
inline int16_t mix_ramp_weight(int16_t w0, int16_t w1, uint32_t p)
{
    if (p > MIX_RAMP_ONE)
        p = MIX_RAMP_ONE;
    const int32_t N = (int32_t)w0 * (int32_t)(MIX_RAMP_ONE - p) + (int32_t)w1 * (int32_t)p;
    const int32_t a = (N < 0 ? -N : N) >> 15;
    return (int16_t)(N < 0 ? -a : a);
}

// The streams' ramps as the host knows them: W0 and W1 int16 [S][n] (n = C_out * C_in entries), done and R per
// stream.  R = 0: the stream does not ramp and W1 is its matrix.
struct MixRampMirror {
    size_t n = 0;
    std::vector<int16_t> w0, w1;
    std::vector<uint32_t> done, R;
    size_t active = 0;                               // streams with done < R

    // every stream at rest on its matrix W[s] (int16 [S][n]); may throw std::bad_alloc
    void init(size_t streams, size_t entries, const int16_t *W)
    {
        n = entries;
        w0.assign(W, W + streams * entries);
        w1.assign(W, W + streams * entries);
        done.assign(streams, 0);
        R.assign(streams, 0);
        active = 0;
    }
    bool ramping(size_t s) const { return done[s] < R[s]; }
    bool any() const { return active != 0; }
    // the matrix in force: w(p(done)) while the stream ramps, its target otherwise
    void now(size_t s, int16_t *W) const
    {
        const uint32_t p = ramping(s) ? mix_ramp_position(done[s], R[s]) : MIX_RAMP_ONE;
        for (size_t i = 0; i < n; i++)
            W[i] = mix_ramp_weight(w0[s * n + i], w1[s * n + i], p);
    }
    // a ramp of `frames` >= 2 frames to W, from the matrix in force (a retarget when one is running)
    void start(size_t s, const int16_t *W, uint32_t frames)
    {
        now(s, &w0[s * n]);                          // (entry i of W0 is read before it is written)
        for (size_t i = 0; i < n; i++)
            w1[s * n + i] = W[i];
        if (!ramping(s))
            active++;
        done[s] = 0;
        R[s] = frames;
    }
    // a step to W: whatever ramp runs is over
    void cancel(size_t s, const int16_t *W)
    {
        if (ramping(s))
            active--;
        done[s] = R[s] = 0;
        for (size_t i = 0; i < n; i++)
            w0[s * n + i] = w1[s * n + i] = W[i];
    }
    // the stream was given `count` frames
    void advance(size_t s, uint32_t count)
    {
        if (!ramping(s))
            return;
        done[s] = count >= R[s] - done[s] ? R[s] : done[s] + count;
        if (!ramping(s))
            active--;
    }
};

}  // namespace cmhip
#endif
