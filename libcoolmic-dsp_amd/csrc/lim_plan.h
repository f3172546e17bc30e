// lim_plan.h -- the geometry and the launch plan of the peak limiter (include/coolmic_hip.h, "peak limiter").  Host
// only, plain C++17, no HIP: tests/cpp/lim_plan_test.cpp compiles it with g++ alone.
//
//   a = lookahead_log2 in 3..9, A = 2^a, D = A - 1 (the delay), H = hold, W = A + H <= 2048,
//   HIST = A + W - 2: the earlier frames an output depends on.
//   halo = HIST rounded up to 8 frames: what a stream's history slot holds and what a tile evaluates in front of its own
//   frames -- a multiple of 8 so that a slot is whole 16-byte vectors for every channel count and lines up with the
//   stream's vectors (frame -1 of a run is the slot's last frame).
//   A workgroup of 256 threads takes one stream and a tile of tile_frames frames: the largest power of two <= 4096 that
//   is >= halo (so the frames in front of a tile never reach past the previous tile) and whose per-frame dwords,
//   (tile_frames + halo) * 4 bytes of dynamic LDS, fit 64 KiB (no per-device limit is raised).
//
// The true-peak detector (LIM_DETECT_TRUE_PEAK; k_limtp.hip) looks at the 4x oversampled signal: its g of frame n covers
// sample n - 8 and the interval behind it and needs the 13 frames x[n-13 .. n-1].  D = A + 7 (so that D + 1 stays a
// multiple of 8 frames), HIST = A + W - 2 + 13; hold >= 1, so that an interval's gain also covers the interval's second
// end sample, and A + W <= 2549, so that HIST <= 2560 = LIM_HALO_MAX: lim_geom_tp / plan_limtp.  The rest is the same.
//
// The release stage (release_log2 = rho in 1..11, R = 2^rho; k_limrel.hip) puts a min-plus convolution with a ramp of
// slope q = 32768 >> rho between the minimum and the sum: HIST grows by R - 1 and may reach 4096 = LIMREL_HIST_MAX, the
// tile, so the tile is always 4096 frames and a workgroup evaluates up to 8192 elements, LIMREL_SLOTS = 32 per thread,
// 32 KiB of dynamic LDS: lim_geom_rel / plan_limrel.  rho = 0 is the limiter without the stage: lim_geom_rel and
// plan_limrel then give what lim_geom_of and plan_lim_of give, and the launchers take k_lim.hip's and k_limtp.hip's
// kernels (LIM_R = 26 slots per thread, csrc/k_lim.h).  The slot counts are arguments of the one tile template
// (csrc/k_lim_tile.h).
#ifndef CMHIP_LIM_PLAN_H
#define CMHIP_LIM_PLAN_H

#include <stdint.h>

namespace cmhip {

constexpr uint32_t LIM_BLOCK = 256;
constexpr uint32_t LIM_TILE_MAX = 4096;
constexpr uint32_t LIM_LDS_LIMIT = 64u * 1024u;
constexpr uint32_t LIM_MAX_CH = 16;
constexpr uint32_t LIM_A_MIN = 3, LIM_A_MAX = 9;
constexpr uint32_t LIM_W_MAX = 2048;
constexpr uint32_t LIM_HALO_MAX = 2560;              // a = 9, W = 2048: HIST = 2558
constexpr uint32_t LIM_T_MAX = 32767;
constexpr uint32_t LIM_DRIVE_MAX = 65535;
constexpr uint32_t LIM_UNITY = 32768;                // Q15
constexpr uint32_t LIM_DETECT_SAMPLE = 0, LIM_DETECT_TRUE_PEAK = 1;
constexpr uint32_t LIM_TP_FRONT = 13;                // frames in front of frame n that the true-peak g[n] reads
constexpr uint32_t LIM_TP_LAG = 8;                   // what the true-peak detector adds to the delay
constexpr uint32_t LIM_TP_AW_MAX = LIM_HALO_MAX + 2u - LIM_TP_FRONT;     // 2549: A + W at most
constexpr uint32_t LIMREL_RHO_MAX = 11;              // release_log2 at most: R = 2048 frames
constexpr uint32_t LIMREL_HIST_MAX = LIM_TILE_MAX;   // HIST with a release: a history halo never exceeds the tile
constexpr uint32_t LIMREL_SLOTS = (LIM_TILE_MAX + LIMREL_HIST_MAX) / LIM_BLOCK;      // 32 elements per thread at most

struct LimGeom {
    uint32_t a, A, D, H, W, hist, halo;
};

// false: lookahead_log2 or hold out of range (g is not written)
inline bool lim_geom(uint32_t lookahead_log2, uint32_t hold, LimGeom *g)
{
    if (lookahead_log2 < LIM_A_MIN || lookahead_log2 > LIM_A_MAX)
        return false;
    const uint32_t A = 1u << lookahead_log2;
    if (hold > LIM_W_MAX - A)
        return false;
    if (g) {
        g->a = lookahead_log2;
        g->A = A;
        g->D = A - 1u;
        g->H = hold;
        g->W = A + hold;
        g->hist = A + g->W - 2u;
        g->halo = (g->hist + 7u) & ~7u;
    }
    return true;
}

// the same for the true-peak detector: also false for hold 0 and for A + W > 2549
inline bool lim_geom_tp(uint32_t lookahead_log2, uint32_t hold, LimGeom *g)
{
    LimGeom t;
    if (hold == 0 || !lim_geom(lookahead_log2, hold, &t) || t.A + t.W > LIM_TP_AW_MAX)
        return false;
    if (g) {
        t.D += LIM_TP_LAG;
        t.hist += LIM_TP_FRONT;
        t.halo = (t.hist + 7u) & ~7u;
        *g = t;
    }
    return true;
}

inline bool lim_geom_of(uint32_t detector, uint32_t lookahead_log2, uint32_t hold, LimGeom *g)
{
    return detector == LIM_DETECT_SAMPLE      ? lim_geom(lookahead_log2, hold, g)
           : detector == LIM_DETECT_TRUE_PEAK ? lim_geom_tp(lookahead_log2, hold, g)
                                              : false;
}

// the same with a release stage of 2^release_log2 frames: also false for release_log2 > 11 and for HIST > 4096
// (release_log2 0: lim_geom_of)
inline bool lim_geom_rel(uint32_t detector, uint32_t lookahead_log2, uint32_t hold, uint32_t release_log2, LimGeom *g)
{
    LimGeom t;
    if (release_log2 > LIMREL_RHO_MAX || !lim_geom_of(detector, lookahead_log2, hold, &t))
        return false;
    t.hist += (1u << release_log2) - 1u;
    if (t.hist > LIMREL_HIST_MAX)
        return false;
    t.halo = (t.hist + 7u) & ~7u;
    if (g)
        *g = t;
    return true;
}

inline bool lim_params_ok(uint32_t threshold, uint32_t drive)
{
    return threshold >= 1u && threshold <= LIM_T_MAX && drive >= 1u && drive <= LIM_DRIVE_MAX;
}

struct LimPlan {
    int      err;                  // 1: refused, the grid would reach 2^31 workgroups
    uint32_t fast;                 // the mono / stereo kernel; otherwise the any-channel-count kernel
    uint32_t grid, block;          // grid 0: nothing to launch (or refused, or bad geometry)
    uint32_t chunks;               // tiles per stream
    uint32_t tile_frames;
    uint32_t lds_bytes;            // dynamic LDS of the launch
    uint32_t halo;
};

// what every plan ends in, the geometry known: the tiles of a run whose longest stream has `frames` frames
inline LimPlan lim_plan_tiles(uint32_t streams, uint32_t channels, uint32_t frames, uint32_t halo, uint32_t tile)
{
    LimPlan p{};
    const uint64_t tiles = ((uint64_t)frames + tile - 1u) / tile;
    if (tiles * streams >= (1ull << 31)) {
        p.err = 1;
        return p;
    }
    p.fast = channels <= 2u ? 1u : 0u;
    p.block = LIM_BLOCK;
    p.tile_frames = tile;
    p.lds_bytes = (tile + halo) * 4u;
    p.halo = halo;
    p.chunks = (uint32_t)tiles;
    p.grid = streams * p.chunks;
    return p;
}

inline bool lim_run_ok(uint32_t streams, uint32_t channels, uint32_t frames)
{
    return streams != 0 && frames != 0 && channels != 0 && channels <= LIM_MAX_CH;
}

// the plan of a run whose longest stream has `frames` frames, for either detector
inline LimPlan plan_lim_of(uint32_t detector, uint32_t streams, uint32_t channels, uint32_t lookahead_log2, uint32_t hold,
                           uint32_t frames)
{
    LimGeom g;
    if (!lim_run_ok(streams, channels, frames) || !lim_geom_of(detector, lookahead_log2, hold, &g))
        return LimPlan{};
    uint32_t tile = LIM_TILE_MAX;
    while (tile / 2u >= g.halo && tile / 2u >= 8u && (tile + g.halo) * 4u > LIM_LDS_LIMIT)
        tile >>= 1;                                   // (never taken today: 4096 + 2560 frames are 26 KiB)
    return lim_plan_tiles(streams, channels, frames, g.halo, tile);
}

inline LimPlan plan_lim(uint32_t streams, uint32_t channels, uint32_t lookahead_log2, uint32_t hold, uint32_t frames)
{
    return plan_lim_of(LIM_DETECT_SAMPLE, streams, channels, lookahead_log2, hold, frames);
}

inline LimPlan plan_limtp(uint32_t streams, uint32_t channels, uint32_t lookahead_log2, uint32_t hold, uint32_t frames)
{
    return plan_lim_of(LIM_DETECT_TRUE_PEAK, streams, channels, lookahead_log2, hold, frames);
}

// the plan of a run of a limiter with a release stage, for either detector: the tile is 4096 frames for every geometry
// (halo <= 4096 <= tile, (4096 + 4096) * 4 bytes are 32 KiB); release_log2 0 gives plan_lim_of's plan
inline LimPlan plan_limrel(uint32_t detector, uint32_t streams, uint32_t channels, uint32_t lookahead_log2, uint32_t hold,
                           uint32_t release_log2, uint32_t frames)
{
    LimGeom g;
    if (release_log2 == 0)
        return plan_lim_of(detector, streams, channels, lookahead_log2, hold, frames);
    if (!lim_run_ok(streams, channels, frames) || !lim_geom_rel(detector, lookahead_log2, hold, release_log2, &g))
        return LimPlan{};
    return lim_plan_tiles(streams, channels, frames, g.halo, LIM_TILE_MAX);
}

}  // namespace cmhip
#endif
