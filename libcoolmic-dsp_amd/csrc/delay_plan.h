// delay_plan.h -- the ring geometry, the position arithmetic, the tile classes, the host's mirror and the launch plan of
// the delay stage (include/coolmic_hip.h, "delay").  Plain C++17, no HIP: tests/cpp/delay_plan_test.cpp compiles it with
// g++ alone; the kernels (k_delay.hip) use the same class and index functions.
//
//   S streams of C interleaved int16 channels, a delay d_s in 0..max_delay frames per stream.
//   The state is a ring per stream: `cap` frames, cap = max_delay + max_frames rounded up to 8, so a stream's ring is
//   whole 16-byte vectors for every channel count.  pos in 0..cap-1 is the frame the next run's first frame goes to.
//
// Everything the kernels do is in SAMPLES, the frame numbers times C: a delay of d frames shifts the interleaved stream by
// D = d * C samples whatever C is.  CAP = cap * C, P = pos * C, N = count * C.  A run writes the ring samples
// [P, P + N) and reads [P - D, P), both modulo CAP; D + N <= CAP, so the two ranges never meet and one launch is free
// of races between workgroups.  Output sample e of the run is in[e - D] for e >= D and ring[(P + e - D) mod CAP] before.
//
// A tile is a stretch of output samples between 16-byte edges.  Its class for one tap (delay_tap):
//     DELAY_BEHIND   wholly behind D: the samples in[q ...], q = e0 - D
//     DELAY_FRONT    wholly in front of D and its stretch of the ring does not wrap: ring[q ...]
//     DELAY_MIXED    on the seam or on the ring's wrap: every 16-byte vector of the tile is classified again by itself
//                    (delay_tap over its 8 samples), and a vector that is still DELAY_MIXED goes sample by sample;
//                    class and shift are then per vector: (-D) mod 8 behind the seam, (P - D) mod 8 in front of it
// q is 2-byte aligned at best; q mod 8 is the same for every vector of such a tile, so the first two classes are aligned
// 16-byte loads and one funnel shift by a uniform amount.
//
// A run's per-stream record (DELAY_REC dwords, sent through the counts ring with every run): count, pos, d1, d0, R,
// done, inc.  The stream ramps while done < R: frame f of the run crossfades the taps d0 and d1 at p(done + f + 1)
// (csrc/mix_ramp.h).  The device keeps no position of its own: the host sees every count and hands the positions down.
#ifndef CMHIP_DELAY_PLAN_H
#define CMHIP_DELAY_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define CMHIP_DELAY_HD __host__ __device__
#else
#define CMHIP_DELAY_HD
#endif

namespace cmhip {

constexpr uint32_t DELAY_MAX_CH = 16;
constexpr uint32_t DELAY_RAMP_MAX = 1u << 20;        // frames of a crossfade at most (MIX_RAMP_MAX)
constexpr uint32_t DELAY_FAST_BLOCK = 64;            // mono / stereo: one wave per tile ...
constexpr uint32_t DELAY_FAST_VECS = 256;            // ... of four 16-byte vectors per lane
constexpr uint32_t DELAY_ANY_BLOCK = 256;            // any channel count: 256 threads per tile ...
constexpr uint32_t DELAY_ANY_FRAMES = 256;           // ... of 256 frames, 32 C vectors
constexpr uint32_t DELAY_REC = 8;                    // dwords of a stream's record
constexpr uint32_t DREC_COUNT = 0, DREC_POS = 1, DREC_D1 = 2, DREC_D0 = 3, DREC_R = 4, DREC_DONE = 5, DREC_INC = 6;

enum DelayClass : uint32_t { DELAY_BEHIND = 0, DELAY_FRONT = 1, DELAY_MIXED = 2 };

// frames of a stream's ring
constexpr uint64_t delay_ring_frames(uint64_t max_delay, uint64_t max_frames) { return (max_delay + max_frames + 7u) & ~7ull; }

// what cmhip_delay_new accepts: (max_delay + max_frames) * C below 2^31, so every sample index of a ring fits 32 bits
constexpr bool delay_geometry_ok(uint64_t streams, uint64_t channels, uint64_t max_delay, uint64_t max_frames)
{
    return streams != 0 && channels >= 1 && channels <= DELAY_MAX_CH && max_frames != 0 && max_delay < (1ull << 31) &&
           max_frames < (1ull << 31) && (max_delay + max_frames) * channels < (1ull << 31);
}

// v below 3 CAP -> v mod CAP
CMHIP_DELAY_HD constexpr uint32_t delay_wrap(uint64_t v, uint32_t CAP)
{
    if (v >= CAP)
        v -= CAP;
    if (v >= CAP)
        v -= CAP;
    return (uint32_t)v;
}

// the ring sample that holds sample j of the run, j in -CAP .. CAP - 1 (negative: history)
CMHIP_DELAY_HD constexpr uint32_t delay_ring_index(uint32_t P, uint32_t CAP, int64_t j)
{
    return delay_wrap((uint64_t)((int64_t)P + (int64_t)CAP + j), CAP);
}

struct DelayTap {
    uint32_t cls;              // DelayClass
    uint32_t q;                // the first source sample: of the input (DELAY_BEHIND), of the ring (DELAY_FRONT)
};

// the class of output samples [e0, e0 + len) at a delay of D samples; len >= 1, D <= CAP, P < CAP
CMHIP_DELAY_HD constexpr DelayTap delay_tap(uint32_t e0, uint32_t len, uint32_t D, uint32_t P, uint32_t CAP)
{
    if (e0 >= D)
        return DelayTap{DELAY_BEHIND, e0 - D};
    if ((uint64_t)e0 + len <= D) {
        const uint32_t q = delay_ring_index(P, CAP, (int64_t)e0 - (int64_t)D);
        if ((uint64_t)q + len <= CAP)
            return DelayTap{DELAY_FRONT, q};
    }
    return DelayTap{DELAY_MIXED, 0u};
}

// the run's samples [0, h) go into the ring one by one, h = delay_ring_head(P): behind them the ring's 16-byte
// granules are those of the run's samples h, h + 8, ...
CMHIP_DELAY_HD constexpr uint32_t delay_ring_head(uint32_t P) { return (8u - (P & 7u)) & 7u; }

inline uint32_t delay_ramp_inc(uint32_t R) { return (uint32_t)(((1ull << 32) + R - 1u) / R); }       // mix_ramp_inc

// The streams as the host knows them.  d1: the last accepted target.  A stream ramps while done < R; outside a ramp
// R = done = 0 and d0 = d1.
struct DelayMirror {
    uint32_t cap = 0;
    std::vector<uint32_t> pos, d1, d0, R, done;

    void init(size_t streams, uint32_t ring_frames)              // may throw std::bad_alloc
    {
        cap = ring_frames;
        pos.assign(streams, 0);
        d1.assign(streams, 0);
        d0.assign(streams, 0);
        R.assign(streams, 0);
        done.assign(streams, 0);
    }
    bool ramping(size_t s) const { return done[s] < R[s]; }
    void set(size_t s, uint32_t d)
    {
        d0[s] = d1[s] = d;
        R[s] = done[s] = 0;
    }
    void ramp(size_t s, uint32_t d, uint32_t frames)             // frames >= 2, the stream does not ramp
    {
        d0[s] = d1[s];
        d1[s] = d;
        R[s] = frames;
        done[s] = 0;
    }
    // the record of a run that gives the stream `count` frames
    void record(size_t s, uint32_t count, uint32_t *rec) const
    {
        rec[DREC_COUNT] = count;
        rec[DREC_POS] = pos[s];
        rec[DREC_D1] = d1[s];
        rec[DREC_D0] = d0[s];
        rec[DREC_R] = R[s];
        rec[DREC_DONE] = done[s];
        rec[DREC_INC] = ramping(s) ? delay_ramp_inc(R[s]) : 0u;
        rec[7] = 0;
    }
    // the stream was given `count` frames (count <= cap)
    void advance(size_t s, uint32_t count)
    {
        pos[s] = delay_wrap((uint64_t)pos[s] + count, cap);
        if (!ramping(s))
            return;
        done[s] = count >= R[s] - done[s] ? R[s] : done[s] + count;
        if (!ramping(s))
            set(s, d1[s]);
    }
};

struct DelayPlan {
    int      err;                  // 1: refused, the grid would reach 2^31 workgroups
    uint32_t fast;                 // the mono / stereo kernel
    uint32_t grid, block;          // grid 0: nothing to launch (or refused)
    uint32_t chunks;               // tiles per stream
    uint32_t tile_frames;          // frames per tile
    uint32_t tile_vecs;            // 16-byte vectors per tile
    uint32_t ring_frames;          // frames of a stream's ring
};

// frames: the run's largest count
static inline DelayPlan plan_delay(uint32_t streams, uint32_t channels, uint32_t max_delay, uint32_t max_frames,
                                   uint32_t frames)
{
    DelayPlan p{};
    if (!delay_geometry_ok(streams, channels, max_delay, max_frames))
        return p;
    p.ring_frames = (uint32_t)delay_ring_frames(max_delay, max_frames);
    if (frames == 0)
        return p;
    const uint32_t fast = channels <= 2 ? 1u : 0u;
    const uint32_t tile = fast ? DELAY_FAST_VECS * 8u / channels : DELAY_ANY_FRAMES;
    const uint64_t tiles = ((uint64_t)frames + tile - 1u) / tile;
    if (tiles * streams >= (1ull << 31)) {
        p.err = 1;
        return p;
    }
    p.fast = fast;
    p.block = fast ? DELAY_FAST_BLOCK : DELAY_ANY_BLOCK;
    p.chunks = (uint32_t)tiles;
    p.grid = streams * p.chunks;
    p.tile_frames = tile;
    p.tile_vecs = tile * channels / 8u;
    return p;
}

}  // namespace cmhip
#endif
