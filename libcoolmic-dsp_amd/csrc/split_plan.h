// split_plan.h -- the geometry, the tap groups, the kernel's table and the launch plan of the band split
// (include/coolmic_hip.h, "band split").  Host only, plain C++17, no HIP: tests/cpp/split_plan_test.cpp compiles it with
// g++ alone.
//
//   B bands in 2..8, B - 1 filters g_b[T], T odd in 3..1023, q_b in 14..20, D = (T - 1) / 2.
//   Tp = T + 1 rounded up to 8: the taps as the kernel walks them, zero taps behind T, in blocks of 8 (four pairs).
//
// Exactness (the idea of csrc/bus_route.h).  The kernel adds tap PAIRS with the dot instruction into an int32.  A chain
// of pairs whose sum |g| is at most 65535 stays below 2^31 against any int16 input (65535 * 32768 = 2^31 - 32768), so
// each filter's pairs are cut into consecutive GROUPS within that bound, greedily from tap 0; the kernel adds a finished
// group into an int64 and starts the next from zero.  A group ends on a pair, that is, on an even tap.  One pair can pass
// the bound on its own in exactly one way, both taps -32768 (sum |g| = 65536): it is a group of its own, and the one
// sum of it that leaves int32, +2^31 from two samples of -32768, comes back from the instruction as -2^31, which no
// group can reach otherwise (the least sum of any group is -65536 * 32767 > -2^31): the kernel reads -2^31 as +2^31.
//
// The kernel's table (SplitArgs::table), dwords, nf = B - 1 filters:
//     [nf][Tp/2]  pair kk of filter b: g_b[2kk+1] | g_b[2kk] << 16 -- the order the dot instruction meets a pair of
//                 samples (older, newer) in
//     [nf][Tp/8]  block j of filter b: bit p (of 4) set when a group ends behind pair 4j + p and another follows; the
//                 upper half counts the blocks j, j + 1, ... in a row whose four bits are all clear (0 when block j's
//                 are not): the kernel runs those in a loop of its own
//     [nf]        q_b
//
// A workgroup of 256 threads takes one stream and a tile of SPLIT_TILE / C frames for mono and stereo (a lane owns eight
// consecutive frames of one channel), of SPLIT_TILE frames and one channel after the other otherwise.  The planes of
// a tile in LDS: per channel `row` = tile + Tp + 8 samples, twice (plain, and delayed by one sample, as k_src.hip's).
#ifndef CMHIP_SPLIT_PLAN_H
#define CMHIP_SPLIT_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

namespace cmhip {

constexpr uint32_t SPLIT_BLOCK = 256;
constexpr uint32_t SPLIT_LANE_FRAMES = 8;            // consecutive frames of one channel a lane owns
constexpr uint32_t SPLIT_TILE = SPLIT_BLOCK * SPLIT_LANE_FRAMES;
constexpr uint32_t SPLIT_MAX_CH = 16;
constexpr uint32_t SPLIT_BANDS_MIN = 2, SPLIT_BANDS_MAX = 8;
constexpr uint32_t SPLIT_T_MIN = 3, SPLIT_T_MAX = 1023;
constexpr uint32_t SPLIT_Q_MIN = 14, SPLIT_Q_MAX = 20;
constexpr uint32_t SPLIT_GROUP_BOUND = 65535;
constexpr uint32_t SPLIT_LDS_LIMIT = 64u * 1024u;

constexpr uint32_t split_tp(uint32_t T) { return (T + 1u + 7u) & ~7u; }
constexpr bool split_geometry_ok(uint32_t bands, uint32_t taps)
{
    return bands >= SPLIT_BANDS_MIN && bands <= SPLIT_BANDS_MAX && taps >= SPLIT_T_MIN && taps <= SPLIT_T_MAX && (taps & 1u);
}
constexpr uint32_t split_table_words(uint32_t bands, uint32_t taps)
{
    return (bands - 1u) * (split_tp(taps) / 2u + split_tp(taps) / 8u + 1u);
}

static inline uint32_t split_abs(int16_t v) { return (uint32_t)abs((int)v); }

// The groups of one filter: ends[i] is the tap behind group i (even, or T for the last); groups cover 0 .. T - 1 once.
static inline void split_groups(const int16_t *g, uint32_t T, std::vector<uint32_t> *ends)
{
    ends->clear();
    uint32_t sum = 0;
    for (uint32_t k = 0; k < T; k += 2) {
        const uint32_t pair = split_abs(g[k]) + (k + 1 < T ? split_abs(g[k + 1]) : 0u);
        if (k != 0 && sum + pair > SPLIT_GROUP_BOUND) {
            ends->push_back(k);
            sum = 0;
        }
        sum += pair;
    }
    ends->push_back(T);
}

// the table in the kernel's form: split_table_words(bands, taps) dwords at `out`
static inline void split_compile(uint32_t bands, uint32_t taps, const int16_t *g, const uint8_t *q, uint32_t *out)
{
    const uint32_t nf = bands - 1u, Tp = split_tp(taps);
    uint32_t *pairs = out, *masks = out + (size_t)nf * (Tp / 2u), *qs = masks + (size_t)nf * (Tp / 8u);
    std::vector<uint32_t> ends;
    for (uint32_t b = 0; b < nf; b++) {
        const int16_t *gb = g + (size_t)b * taps;
        for (uint32_t kk = 0; kk < Tp / 2u; kk++) {
            const uint32_t k = 2u * kk;
            const uint16_t newer = k < taps ? (uint16_t)gb[k] : 0, older = k + 1u < taps ? (uint16_t)gb[k + 1u] : 0;
            pairs[(size_t)b * (Tp / 2u) + kk] = (uint32_t)older | (uint32_t)newer << 16;
        }
        for (uint32_t j = 0; j < Tp / 8u; j++)
            masks[(size_t)b * (Tp / 8u) + j] = 0;
        split_groups(gb, taps, &ends);
        for (size_t i = 0; i + 1 < ends.size(); i++) {          // (the last group ends the filter: the kernel adds it anyway)
            const uint32_t kk = ends[i] / 2u - 1u;              // the pair the group ends behind
            masks[(size_t)b * (Tp / 8u) + kk / 4u] |= 1u << (kk & 3u);
        }
        for (uint32_t j = Tp / 8u, run = 0; j-- > 0;) {
            uint32_t &w = masks[(size_t)b * (Tp / 8u) + j];
            run = w ? 0u : run + 1u;
            w |= run << 16;
        }
        qs[b] = q[b];
    }
}

struct SplitPlan {
    int      err;                  // 1: refused, the grid would reach 2^31 workgroups
    uint32_t fast;                 // the mono / stereo kernel
    uint32_t grid, block;          // grid 0: nothing to launch (or refused)
    uint32_t chunks;               // tiles per stream
    uint32_t tile_frames;          // frames per tile
    uint32_t tp;                   // split_tp(taps)
    uint32_t row;                  // samples between the planes of a tile in LDS
    uint32_t table_words;          // dwords of the table, copied into LDS in front of the planes
    uint32_t lds_bytes;            // dynamic LDS of the launch
};

// frames: the run's largest count
static inline SplitPlan plan_split(uint32_t streams, uint32_t channels, uint32_t bands, uint32_t taps, uint32_t frames)
{
    SplitPlan p{};
    if (streams == 0 || frames == 0 || channels == 0 || channels > SPLIT_MAX_CH || !split_geometry_ok(bands, taps))
        return p;
    const uint32_t fast = channels <= 2 ? 1u : 0u;
    const uint32_t tile = fast ? SPLIT_TILE / channels : SPLIT_TILE;
    const uint32_t planes = fast ? channels : 1u;
    const uint32_t tp = split_tp(taps), row = tile + tp + 8u;
    const uint32_t words = (split_table_words(bands, taps) + 3u) & ~3u;
    const uint64_t tiles = ((uint64_t)frames + tile - 1u) / tile;
    if (tiles * streams >= (1ull << 31)) {
        p.err = 1;
        return p;
    }
    p.fast = fast;
    p.block = SPLIT_BLOCK;
    p.chunks = (uint32_t)tiles;
    p.grid = streams * p.chunks;
    p.tile_frames = tile;
    p.tp = tp;
    p.row = row;
    p.table_words = words;
    p.lds_bytes = words * 4u + 2u * planes * row * 2u;
    return p;
}
static_assert(((split_table_words(SPLIT_BANDS_MAX, SPLIT_T_MAX) + 3u) & ~3u) * 4u +
                      2u * 2u * (SPLIT_TILE / 2u + split_tp(SPLIT_T_MAX) + 8u) * 2u <= SPLIT_LDS_LIMIT &&
                  ((split_table_words(SPLIT_BANDS_MAX, SPLIT_T_MAX) + 3u) & ~3u) * 4u +
                      2u * (SPLIT_TILE + split_tp(SPLIT_T_MAX) + 8u) * 2u <= SPLIT_LDS_LIMIT,
              "the largest table and tile fit the LDS a workgroup may take");

}  // namespace cmhip
#endif
