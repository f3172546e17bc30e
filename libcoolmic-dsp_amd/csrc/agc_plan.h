// agc_plan.h -- the arithmetic, the run's window plan, the tiles, the host's mirror and the launch plan of the leveller
// (include/coolmic_hip.h, "leveller").  Plain C++17, no HIP: tests/cpp/agc_plan_test.cpp compiles it with g++ alone; the
// kernels (k_agc.hip) use the same step, gain, sample and tile functions.
//
//   S streams of C interleaved int16 channels.  w = window_log2 in 6..14, W = 2^w.  A stream's frames are counted since
//   creation or the last reset: n, 64 bits.  Window k = n >> w, j = n & (W - 1).
//
// A run gives a stream `count` frames from position pos.  It touches the windows pos >> w .. (pos + count - 1) >> w:
// at most NW = max_frames / W + 2 of them (a carried partial one in front, a partial one behind).  Window i of the run is
// entry i of the stream's row in the energy table, uint64 [S][NW][C], and has the gain nodes i and i + 1 of the stream's
// row in the nodes table, uint32 [S][NW + 1].
//
// A tile is a stretch of 2^tile_log2 frames between multiples of that number in the stream's ABSOLUTE position,
// tile_log2 <= w, so a tile never straddles a window: its energy goes to one table entry and its two gain nodes are
// uniform.  A run's first and last tile are cut by the run's ends.  In the run's own samples a tile begins and ends
// anywhere in a 16-byte vector: whole vectors inside it are the body, the up to 7 samples in front and behind go one by
// one (agc_tile_span).
//
// A run's per-stream record (AGC_REC dwords, sent through the counts ring with every run): count, pos (two dwords) and
// the parameters in force, packed.  The device keeps no position and no parameters: the host sees every count and every
// set, and hands them down.
#ifndef CMHIP_AGC_PLAN_H
#define CMHIP_AGC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dyn_plan.h"

#if defined(__HIPCC__)
#define CMHIP_AGC_HD __host__ __device__
#else
#define CMHIP_AGC_HD
#endif

namespace cmhip {

constexpr uint32_t AGC_MAX_CH = 16;
constexpr uint32_t AGC_W_MIN = 6, AGC_W_MAX = 14;
constexpr uint32_t AGC_UNITY = 4096;                 // 2^12, the limiter's drive unit
constexpr uint32_t AGC_FAST_BLOCK = 64;              // mono / stereo: one wave per tile ...
constexpr uint32_t AGC_FAST_VECS = 256;              // ... of at most four 16-byte vectors per lane
constexpr uint32_t AGC_ANY_BLOCK = 256;              // any channel count: 256 threads per tile ...
constexpr uint32_t AGC_ANY_TILE_LOG2 = 8;            // ... of at most 256 frames, 32 C vectors: two per thread
constexpr uint32_t AGC_ANY_VECS = 2;
constexpr uint32_t AGC_STEP_BLOCK = 64;              // k_agc_step: one lane per stream
constexpr uint32_t AGC_REC = 8;                      // dwords of a stream's record
constexpr uint32_t AREC_COUNT = 0, AREC_POS_LO = 1, AREC_POS_HI = 2, AREC_P0 = 3, AREC_P1 = 4, AREC_P2 = 5, AREC_P3 = 6;

// cmhip_agc_params_t, field by field (cmhip_agc.hip holds the two layouts against each other)
struct AgcParams {
    uint16_t target, gate, gain_min, gain_max, rise, fall, initial;
};

CMHIP_AGC_HD constexpr bool agc_window_ok(uint32_t w) { return w >= AGC_W_MIN && w <= AGC_W_MAX; }
CMHIP_AGC_HD constexpr bool agc_params_ok(const AgcParams &p)
{
    return p.target >= 1 && p.target <= 32767 && p.gate <= 32767 && p.gain_min >= 1 && p.gain_min <= p.gain_max &&
           p.initial >= p.gain_min && p.initial <= p.gain_max;
}

// the parameters as a record carries them, and back
CMHIP_AGC_HD inline void agc_pack(const AgcParams &p, uint32_t *rec)
{
    rec[AREC_P0] = (uint32_t)p.target | ((uint32_t)p.gate << 16);
    rec[AREC_P1] = (uint32_t)p.gain_min | ((uint32_t)p.gain_max << 16);
    rec[AREC_P2] = (uint32_t)p.rise | ((uint32_t)p.fall << 16);
    rec[AREC_P3] = (uint32_t)p.initial;
}
CMHIP_AGC_HD inline AgcParams agc_unpack(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3)
{
    AgcParams p;
    p.target = (uint16_t)p0;
    p.gate = (uint16_t)(p0 >> 16);
    p.gain_min = (uint16_t)p1;
    p.gain_max = (uint16_t)(p1 >> 16);
    p.rise = (uint16_t)p2;
    p.fall = (uint16_t)(p2 >> 16);
    p.initial = (uint16_t)p3;
    return p;
}

// the level of a complete window from its loudest channel's sum of squares: E <= W * 2^30, so E >> w fits 32 bits
CMHIP_AGC_HD inline uint32_t agc_level(uint64_t E, uint32_t w) { return dyn_isqrt((uint32_t)(E >> w)); }

// the header's step(A, L): the gain node behind A, given the level L (0..32768) of the last complete window.
// (T << 12) / L < 2^27; A * rise < 2^32.
CMHIP_AGC_HD inline uint32_t agc_step(uint32_t A, uint32_t L, const AgcParams &p)
{
    if (L == 0 || L < p.gate)
        return A;
    uint32_t D = ((uint32_t)p.target << 12) / L;
    D = D < p.gain_min ? p.gain_min : D > p.gain_max ? p.gain_max : D;
    if (D > A && p.rise) {
        uint32_t d = (A * (uint32_t)p.rise) >> 16;
        d = d ? d : 1u;
        return D < A + d ? D : A + d;
    }
    if (D < A && p.fall) {
        uint32_t d = (A * (uint32_t)p.fall) >> 16;
        d = d ? d : 1u;
        return A - d > D ? A - d : D;                // (d < A: d <= A * 65535 >> 16 < A, or d = 1 <= D < A)
    }
    return A;
}

// the gain of frame j of a window between its nodes: |a1 - a0| < 2^16 and j < 2^14, so the product fits int32
CMHIP_AGC_HD inline int32_t agc_gain(uint32_t a0, uint32_t a1, uint32_t j, uint32_t w)
{
    return (int32_t)a0 + ((((int32_t)a1 - (int32_t)a0) * (int32_t)j) >> w);
}

// one sample: |x g| + 2048 < 2^31.  *clip: 1 where the clamp changed the value
CMHIP_AGC_HD inline int32_t agc_sample(int32_t x, int32_t g, uint32_t *clip)
{
    const int32_t v = (x * g + 2048) >> 12;
    const int32_t y = v < -32768 ? -32768 : v > 32767 ? 32767 : v;
    *clip = y != v ? 1u : 0u;
    return y;
}

// ---- a run's windows
struct AgcRun {
    uint64_t first;            // the window the run's first frame lies in
    uint32_t nwin;             // windows the run touches (0 for no frames)
    uint32_t complete;         // ... of which so many end inside the run: the first `complete` of them
    uint32_t head;             // frames in front of the run's first window edge that belong to a window begun earlier
    uint32_t tail;             // frames of a window begun in this run and left open
};
CMHIP_AGC_HD inline AgcRun agc_run(uint64_t pos, uint32_t count, uint32_t w)
{
    const uint32_t W = 1u << w, j0 = (uint32_t)pos & (W - 1u);
    AgcRun r;
    r.first = pos >> w;
    r.nwin = count ? (uint32_t)(((uint64_t)j0 + count - 1u) >> w) + 1u : 0u;
    r.complete = (uint32_t)(((uint64_t)j0 + count) >> w);
    r.head = j0 ? (count < W - j0 ? count : W - j0) : 0u;
    r.tail = (count - r.head) & (W - 1u);
    return r;
}
// windows a run of at most max_frames frames touches at most: the rows of the two tables
CMHIP_AGC_HD constexpr uint32_t agc_table_windows(uint64_t max_frames, uint32_t w) { return (uint32_t)(max_frames >> w) + 2u; }

// ---- tiles
struct AgcTile {
    uint32_t fa, fb;           // the run's frames [fa, fb); fa >= fb: the tile lies behind the stream's count
    uint32_t win;              // its window, counted from the run's first
    uint32_t j;                // frame fa's place in that window
};
// tile t of a run of `count` frames from position pos (its low 32 bits: W divides 2^32)
CMHIP_AGC_HD inline AgcTile agc_tile(uint32_t pos_lo, uint32_t count, uint32_t w, uint32_t tile_log2, uint32_t t)
{
    const uint32_t TF = 1u << tile_log2, W = 1u << w;
    const uint32_t off = pos_lo & (TF - 1u);         // frames of tile 0 in front of the run
    const uint64_t lo = (uint64_t)t << tile_log2;    // the tile's first frame, counted from tile 0's
    AgcTile r;
    const uint64_t a = lo > off ? lo - off : 0u, b = lo + TF - off;
    r.fa = a < count ? (uint32_t)a : count;
    r.fb = b < count ? (uint32_t)b : count;
    const uint32_t jj = (pos_lo & (W - 1u)) + r.fa;
    r.win = jj >> w;
    r.j = jj & (W - 1u);
    return r;
}

// a tile's samples [sa, sb) of the run, cut at the run's 16-byte vectors: [sa, hend) one by one, the vectors
// [vb, ve) whole, [tb, sb) one by one.  Where the tile lies inside one vector everything is head.
struct AgcSpan {
    uint32_t sa, hend, vb, ve, tb, sb;
};
CMHIP_AGC_HD inline AgcSpan agc_tile_span(uint32_t fa, uint32_t fb, uint32_t C)
{
    AgcSpan s;
    s.sa = fa * C;
    s.sb = fb * C;
    const uint32_t up = (s.sa + 7u) & ~7u;
    s.hend = up < s.sb ? up : s.sb;
    s.vb = (s.hend + 7u) >> 3;
    s.ve = s.sb >> 3;
    if (s.ve < s.vb)
        s.ve = s.vb;
    s.tb = s.hend > (s.sb & ~7u) ? s.hend : (s.sb & ~7u);
    return s;
}

// ---- the streams as the host knows them
struct AgcMirror {
    std::vector<uint64_t> pos;
    std::vector<AgcParams> par;

    void init(size_t streams, const AgcParams &p)                  // may throw std::bad_alloc
    {
        pos.assign(streams, 0);
        par.assign(streams, p);
    }
    void record(size_t s, uint32_t count, uint32_t *rec) const
    {
        rec[AREC_COUNT] = count;
        rec[AREC_POS_LO] = (uint32_t)pos[s];
        rec[AREC_POS_HI] = (uint32_t)(pos[s] >> 32);
        agc_pack(par[s], rec);
        rec[7] = 0;
    }
};

// ---- the launch plan
struct AgcPlan {
    int      err;                  // 1: refused, the grid would reach 2^31 workgroups
    uint32_t fast;                 // the mono / stereo kernels
    uint32_t grid, block;          // of k_agc_energy and k_agc_apply; grid 0: nothing to launch (or refused)
    uint32_t chunks;               // tiles per stream
    uint32_t tile_log2;            // frames per tile, as a power of two
    uint32_t nw;                   // NW: windows per stream in the tables
    uint32_t step_grid;            // workgroups of k_agc_step
};

constexpr bool agc_geometry_ok(uint64_t streams, uint64_t channels, uint64_t w, uint64_t max_frames)
{
    return streams != 0 && streams < (1ull << 31) && channels >= 1 && channels <= AGC_MAX_CH && w >= AGC_W_MIN &&
           w <= AGC_W_MAX && max_frames != 0 && max_frames < (1ull << 31) && max_frames * channels < (1ull << 31);
}

// frames: the run's largest count
static inline AgcPlan plan_agc(uint32_t streams, uint32_t channels, uint32_t w, uint64_t max_frames, uint32_t frames)
{
    AgcPlan p{};
    if (!agc_geometry_ok(streams, channels, w, max_frames))
        return p;
    p.nw = agc_table_windows(max_frames, w);
    if (frames == 0)
        return p;
    p.fast = channels <= 2 ? 1u : 0u;
    const uint32_t most = p.fast ? (channels == 1 ? 11u : 10u) : AGC_ANY_TILE_LOG2;      // 256 vectors : 256 frames
    p.tile_log2 = w < most ? w : most;
    // (tile 0 may begin up to a tile less a frame in front of the run)
    const uint64_t tiles = (((uint64_t)frames + (1u << p.tile_log2) - 1u) >> p.tile_log2) + 1u;
    if (tiles * streams >= (1ull << 31)) {
        p.err = 1;
        return p;
    }
    p.block = p.fast ? AGC_FAST_BLOCK : AGC_ANY_BLOCK;
    p.chunks = (uint32_t)tiles;
    p.grid = streams * p.chunks;
    p.step_grid = (streams + AGC_STEP_BLOCK - 1u) / AGC_STEP_BLOCK;
    return p;
}

}  // namespace cmhip
#endif
