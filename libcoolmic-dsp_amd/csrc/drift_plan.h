// drift_plan.h -- the table check, the kernel's table, the counts, the host's mirror, the servo and the launch plan of
// the drift stage (include/coolmic_hip.h, "clock-drift compensation").  Host only, plain C++17, no HIP:
// tests/cpp/drift_plan_test.cpp compiles it with g++ alone.
//
// The kernel's table (DriftArgs::table), dwords: [P + 1][T/2 + 1], row P appended here.  Dword kk of row p is
// H[p][2kk+1] | H[p][2kk] << 16 -- the order the dot instruction meets a pair of samples (older, newer) in -- and the
// last dword of a row is padding.  The padding makes the row stride an ODD number of dwords: at |delta| = 2^24 the
// phase moves by P/256 rows per output, so up to 32 lanes of a half wave read up to 32 different rows at one tap, and
// ds_read_b32 has 32 banks; an odd stride spreads consecutive rows over all of them, where T/2 = 16 would put every
// second row on one bank.  Rows p and p + 1 are adjacent: a lane's two rows are one contiguous read of T + 1 dwords.
//
// A workgroup of 256 threads takes one stream and a tile of tile_out output frames.  The planes of a tile in LDS: per
// channel `row` samples, twice (plain, and delayed by one sample, as k_src.hip's).  For mono and stereo the second copy
// lies C * row / 2 dwords behind the first, and row is chosen so that this is 16 modulo 32: neighbouring stereo
// outputs read neighbouring frames, one from each copy, and then never meet on a bank.
//
// Per run and stream DRIFT_REC dwords travel to the device through the counts ring: the count F, the output count K,
// delta, and pos (low, high).  The device keeps no position of its own.
#ifndef CMHIP_DRIFT_PLAN_H
#define CMHIP_DRIFT_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

namespace cmhip {

constexpr uint32_t DRIFT_BLOCK = 256;
constexpr uint32_t DRIFT_MAX_CH = 16;
constexpr uint32_t DRIFT_PHI_MIN = 5, DRIFT_PHI_MAX = 8;
constexpr uint32_t DRIFT_T_MIN = 4, DRIFT_T_MAX = 64;
constexpr int32_t  DRIFT_DELTA_MAX = 1 << 24;
constexpr uint32_t DRIFT_LDS_LIMIT = 64u * 1024u;        // what a workgroup may take without raising the device's limit
constexpr uint32_t DRIFT_TABLE_LDS_MAX = 45u * 1024u;    // the resampler's rule: a larger table is read through the caches
constexpr uint32_t DRIFT_TILE_MAX = 2048;                // output frames per tile
constexpr uint32_t DRIFT_REC = 5;                        // dwords per stream and run: F, K, delta, pos low, pos high
constexpr uint64_t DRIFT_ONE = 1ull << 32;

constexpr bool drift_geometry_ok(uint32_t phi, uint32_t T)
{
    return phi >= DRIFT_PHI_MIN && phi <= DRIFT_PHI_MAX && T >= DRIFT_T_MIN && T <= DRIFT_T_MAX && !(T & 1u);
}
constexpr bool drift_delta_ok(int64_t delta) { return delta >= -DRIFT_DELTA_MAX && delta <= DRIFT_DELTA_MAX; }
constexpr uint32_t drift_row_words(uint32_t T) { return T / 2u + 1u; }
// (rounded up to 16 bytes: the kernel copies the table in 16-byte vectors and the planes follow it)
constexpr uint32_t drift_table_words(uint32_t phi, uint32_t T) { return (((1u << phi) + 1u) * drift_row_words(T) + 3u) & ~3u; }

enum DriftTableError : int {
    DRIFT_TABLE_OK = 0,
    DRIFT_TABLE_GEOMETRY,      // phi outside 5..8, T outside 4..64 or odd
    DRIFT_TABLE_FIRST,         // H[0][0] != 0
    DRIFT_TABLE_SUM,           // a row has sum |h| above 65535            (*where: the row)
};
static inline DriftTableError drift_table_check(uint32_t phi, uint32_t T, const int16_t *h, uint32_t *where)
{
    if (!drift_geometry_ok(phi, T))
        return DRIFT_TABLE_GEOMETRY;
    if (h[0] != 0)
        return DRIFT_TABLE_FIRST;
    for (uint32_t p = 0; p < (1u << phi); p++) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < T; k++)
            sum += (uint32_t)abs((int)h[(size_t)p * T + k]);
        if (sum > 65535u) {
            if (where)
                *where = p;
            return DRIFT_TABLE_SUM;
        }
    }
    return DRIFT_TABLE_OK;
}

// tap k of row p of the (P + 1)-row table: row P is row 0 moved by one tap
static inline int16_t drift_tap(uint32_t phi, uint32_t T, const int16_t *h, uint32_t p, uint32_t k)
{
    if (p < (1u << phi))
        return h[(size_t)p * T + k];
    return k + 1u < T ? h[k + 1u] : (int16_t)0;
}

// the table in the kernel's form: drift_table_words(phi, T) dwords at `out`
static inline void drift_compile(uint32_t phi, uint32_t T, const int16_t *h, uint32_t *out)
{
    const uint32_t rw = drift_row_words(T), words = drift_table_words(phi, T);
    for (uint32_t i = 0; i < words; i++)
        out[i] = 0;
    for (uint32_t p = 0; p <= (1u << phi); p++)
        for (uint32_t kk = 0; kk < T / 2u; kk++) {
            const uint16_t newer = (uint16_t)drift_tap(phi, T, h, p, 2u * kk);
            const uint16_t older = (uint16_t)drift_tap(phi, T, h, p, 2u * kk + 1u);
            out[(size_t)p * rw + kk] = (uint32_t)older | (uint32_t)newer << 16;
        }
}

// K = ceil((F * 2^32 - pos) / step), 0 when pos >= F * 2^32 (or delta out of range)
static inline uint32_t drift_out_frames(uint64_t pos, int32_t delta, uint32_t frames)
{
    const uint64_t end = (uint64_t)frames << 32;
    if (!drift_delta_ok(delta) || pos >= end)
        return 0;
    const uint64_t step = DRIFT_ONE + (uint64_t)(int64_t)delta;
    return (uint32_t)((end - pos + step - 1u) / step);
}
// pos' = pos + K * step - F * 2^32, in 0 .. step - 1 whenever pos < step
static inline uint64_t drift_next_pos(uint64_t pos, int32_t delta, uint32_t frames)
{
    const uint64_t step = DRIFT_ONE + (uint64_t)(int64_t)delta;
    return pos + (uint64_t)drift_out_frames(pos, delta, frames) * step - ((uint64_t)frames << 32);
}

// What the host knows of every stream: it sees every run's counts, every set, seek and reset.
struct DriftMirror {
    std::vector<int32_t>  delta;
    std::vector<uint64_t> pos, in_total, out_total;

    void init(size_t streams)
    {
        delta.assign(streams, 0);
        pos.assign(streams, 0);
        in_total.assign(streams, 0);
        out_total.assign(streams, 0);
    }
    void reset(size_t s) { pos[s] = in_total[s] = out_total[s] = 0; }
    uint32_t out_frames(size_t s, uint32_t frames) const { return drift_out_frames(pos[s], delta[s], frames); }
    // the stream's record of a run that gives it `frames` frames (DRIFT_REC dwords)
    void record(size_t s, uint32_t frames, uint32_t *rec) const
    {
        rec[0] = frames;
        rec[1] = out_frames(s, frames);
        rec[2] = (uint32_t)delta[s];
        rec[3] = (uint32_t)pos[s];
        rec[4] = (uint32_t)(pos[s] >> 32);
    }
    // ... once the run is queued -> its output count
    uint32_t advance(size_t s, uint32_t frames)
    {
        const uint32_t k = out_frames(s, frames);
        pos[s] = drift_next_pos(pos[s], delta[s], frames);
        in_total[s] += frames;
        out_total[s] += k;
        return k;
    }
};

// The servo (cmhip_drift_servo_t has this layout)
struct DriftServo {
    int64_t  target, integ;
    uint32_t kp_log2, ki_log2;
    int32_t  limit, delta;
    uint32_t clamped;
};
constexpr uint32_t DRIFT_SERVO_SHIFT_MAX = 24;
static inline bool drift_servo_init(DriftServo *v, uint32_t target, uint32_t kp_log2, uint32_t ki_log2, int32_t limit)
{
    if (target > 0x7fffffffu || kp_log2 > DRIFT_SERVO_SHIFT_MAX || ki_log2 > DRIFT_SERVO_SHIFT_MAX || limit < 1 ||
        limit > DRIFT_DELTA_MAX)
        return false;
    *v = DriftServo{(int64_t)target, 0, kp_log2, ki_log2, limit, 0, 0u};
    return true;
}
static inline void drift_servo_reset(DriftServo *v)
{
    v->integ = 0;
    v->delta = 0;
    v->clamped = 0;
}
static inline int32_t drift_servo_step(DriftServo *v, int64_t fill)
{
    if (fill < 0 || fill > 0x7fffffff)
        return v->delta;
    const int64_t e = fill - v->target;
    const int64_t raw = e * ((int64_t)1 << v->kp_log2) + (v->integ + e) * ((int64_t)1 << v->ki_log2);
    if (raw >= -(int64_t)v->limit && raw <= (int64_t)v->limit) {
        v->integ += e;
        v->delta = (int32_t)raw;
        v->clamped = 0;
    } else {
        v->delta = raw < 0 ? -v->limit : v->limit;
        v->clamped = 1;
    }
    return v->delta;
}

struct DriftPlan {
    int      err;                  // 1: refused, the grid would reach 2^31 workgroups (or nothing fits)
    uint32_t fast;                 // the mono / stereo kernel
    uint32_t grid, block;          // grid 0: nothing to launch (or refused)
    uint32_t chunks;               // tiles per stream
    uint32_t tile_out;             // output frames per tile
    uint32_t tile_in;              // input frames a tile stages at most, its halo included
    uint32_t row;                  // samples between the planes of a tile in LDS
    uint32_t table_lds;            // the table is copied into LDS in front of the planes
    uint32_t table_words;          // dwords of the table
    uint32_t lds_bytes;            // dynamic LDS of the launch
};

// A tile of tile_out outputs reads at most floor((tile_out - 1) * (2^32 + 2^24) / 2^32) + 2 input frames of its own
// (floor(x + y) - floor(x) <= floor(y) + 1) behind a halo of T - 1.
static inline uint32_t drift_tile_in(uint32_t tile_out, uint32_t T)
{
    return (uint32_t)(((uint64_t)(tile_out - 1u) * (DRIFT_ONE + (uint64_t)DRIFT_DELTA_MAX)) >> 32) + 2u + (T - 1u);
}
// samples per plane: the frames staged and one more for the delayed copy, even, and for mono / stereo with
// C * row = 32 modulo 64 samples (the second copy 16 dwords modulo 32 behind the first)
static inline uint32_t drift_row(uint32_t tile_in, uint32_t channels)
{
    uint32_t row = (tile_in + 2u) & ~1u;
    if (channels <= 2u)
        while ((channels * row) % 64u != 32u)
            row += 2u;
    return row;
}

// out_frames: what the run gives its longest stream.  The table goes into LDS when it fits (always, for phi <= 8 and
// T <= 64) and a tile reads at least as many rows as the table has: every tile copies the whole table, which a run of
// a few packet-sized frames would pay for without using it.
static inline DriftPlan plan_drift(uint32_t streams, uint32_t channels, uint32_t phi, uint32_t T, uint32_t out_frames)
{
    DriftPlan p{};
    if (streams == 0 || out_frames == 0 || channels == 0 || channels > DRIFT_MAX_CH || !drift_geometry_ok(phi, T))
        return p;
    const uint32_t words = drift_table_words(phi, T), rows = (1u << phi) + 1u;
    uint32_t tile = DRIFT_TILE_MAX, row = 0, table_lds = 0;
    uint64_t lds = 0;
    for (;; tile >>= 1) {
        const uint32_t most = out_frames < tile ? out_frames : tile;
        table_lds = words * 4u <= DRIFT_TABLE_LDS_MAX && 2u * most >= rows ? 1u : 0u;
        row = drift_row(drift_tile_in(tile, T), channels);
        lds = (table_lds ? words * 4ull : 0ull) + 2ull * channels * row * sizeof(int16_t);
        if (lds <= DRIFT_LDS_LIMIT || tile == 2u)
            break;
    }
    const uint64_t tiles = ((uint64_t)out_frames + tile - 1u) / tile;
    if (lds > DRIFT_LDS_LIMIT || tiles * streams >= (1ull << 31)) {
        p.err = 1;
        return p;
    }
    p.fast = channels <= 2 ? 1u : 0u;
    p.block = DRIFT_BLOCK;
    p.chunks = (uint32_t)tiles;
    p.grid = streams * p.chunks;
    p.tile_out = tile;
    p.tile_in = drift_tile_in(tile, T);
    p.row = row;
    p.table_lds = table_lds;
    p.table_words = words;
    p.lds_bytes = (uint32_t)lds;
    return p;
}

}  // namespace cmhip
#endif
