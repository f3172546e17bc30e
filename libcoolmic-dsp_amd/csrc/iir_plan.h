// iir_plan.h -- the arithmetic, the tiles and the launch plan of the filter stage (include/coolmic_hip.h, "filter").
// Plain C++17, no HIP: tests/cpp/iir_plan_test.cpp compiles it with g++ alone; the kernels (k_iir.hip) use the same
// section, output and tile functions.
//
//   S streams of C interleaved int16 channels, N = 1..8 biquad sections per stream, coefficients in units of 2^-26.
//   A ROW is one channel of one stream; a row's sections each keep u1, u2, v1, v2 and the remainder e (IirState).
//
// Time is a recurrence and the floor is not linear: nothing is parallel along a stream.  A workgroup is one wave and
// owns `spw` whole streams.  It walks them in tiles of IIR_TILE frames: tile t of a stream is the run's frames
// [t B, min((t + 1) B, count)), B C samples from a 16-byte boundary of the slot, so it is B C / 8 whole vectors of which
// the last one or more may be ragged or empty (iir_tile_vec).  The tile goes through LDS: vectors in, the recurrence
// frame by frame in place, vectors out; the streams' tiles lie iir_lds_pitch samples apart there.
//
//   fast (C <= 2): a lane is (row, section), NP = N rounded up to 1, 2, 4, 8 lanes per row (sections N..NP-1 are unity
//     and keep no state).  At step i of a tile section k works on frame i - k and takes its input from the lane below,
//     which made it one step earlier; a tile of f frames takes f + NP - 1 steps, so the pipeline is empty at every
//     tile's and therefore every run's end.
//   any: a lane is a row and loops over its sections.
#ifndef CMHIP_IIR_PLAN_H
#define CMHIP_IIR_PLAN_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CMHIP_IIR_HD __host__ __device__
#else
#define CMHIP_IIR_HD
#endif

namespace cmhip {

constexpr uint32_t IIR_MAX_CH = 16;
constexpr uint32_t IIR_MAX_SEC = 8;
constexpr int32_t  IIR_ONE = 1 << 26;                // a coefficient of 1.0
constexpr int32_t  IIR_COEF_MAX = 1 << 28;           // |c| <= 4.0
constexpr uint32_t IIR_FRAC = 12;                    // fraction bits of the signal between the sections
constexpr int32_t  IIR_V_MAX = 0x7fffffff;           // |v| <= 2^31 - 1
constexpr uint32_t IIR_BLOCK = 64;                   // one wave per workgroup
constexpr uint32_t IIR_TILE = 64;                    // B: frames per tile and stream
constexpr uint32_t IIR_SEC_WORDS = 5;

// cmhip_iir_section_t, field by field (cmhip_iir.hip holds the two layouts against each other)
struct IirSec {
    int32_t b0, b1, b2, a1, a2;
};
// a section of a row between two frames
struct IirState {
    int32_t  u1, u2, v1, v2;
    uint32_t e;                                      // 0 <= e < 2^26
};

constexpr IirSec IIR_UNITY = {IIR_ONE, 0, 0, 0, 0};

// the stability triangle on the integers, and |c| <= 2^28
CMHIP_IIR_HD constexpr bool iir_section_ok(const IirSec &c)
{
    const int64_t one = IIR_ONE, lim = IIR_COEF_MAX;
    const int64_t v[5] = {c.b0, c.b1, c.b2, c.a1, c.a2};
    for (int i = 0; i < 5; i++)
        if (v[i] > lim || v[i] < -lim)
            return false;
    const int64_t a1 = c.a1 < 0 ? -(int64_t)c.a1 : (int64_t)c.a1, a2 = c.a2;
    return a2 < one && a2 > -one && a1 < one + a2;
}

// one frame through one section: |c| <= 2^28 and |state| < 2^31, so |acc| < 5 * 2^59 + 2^26 < 2^62.  The term of v1,
// which the frame before has made last, is added last.  *over: 1 where the clamp changed v.
CMHIP_IIR_HD inline int32_t iir_section(const IirSec &c, int32_t u, IirState &s, uint32_t *over)
{
    int64_t acc = (int64_t)c.b0 * u + (int64_t)c.b1 * s.u1 + (int64_t)c.b2 * s.u2 - (int64_t)c.a2 * s.v2;
    acc += (int64_t)s.e;
    acc -= (int64_t)c.a1 * s.v1;
    s.e = (uint32_t)acc & (uint32_t)(IIR_ONE - 1);
    const int64_t q = acc >> 26;                     // arithmetic: floor
    const int32_t v = q < -(int64_t)IIR_V_MAX ? -IIR_V_MAX : q > (int64_t)IIR_V_MAX ? IIR_V_MAX : (int32_t)q;
    *over = (int64_t)v != q ? 1u : 0u;
    s.u2 = s.u1;
    s.u1 = u;
    s.v2 = s.v1;
    s.v1 = v;
    return v;
}

// a sample into the first section
CMHIP_IIR_HD inline int32_t iir_input(int32_t x) { return (int32_t)((uint32_t)x << IIR_FRAC); }

// the last section's v as a sample: (v + 2048) >> 12 without leaving int32, clamped.  *clip: 1 where the clamp
// changed the value
CMHIP_IIR_HD inline int32_t iir_output(int32_t v, uint32_t *clip)
{
    const int32_t r = (v >> IIR_FRAC) + ((v >> (IIR_FRAC - 1u)) & 1);
    const int32_t y = r < -32768 ? -32768 : r > 32767 ? 32767 : r;
    *clip = y != r ? 1u : 0u;
    return y;
}

// ---- tiles
// lanes per row of the fast form
CMHIP_IIR_HD constexpr uint32_t iir_np(uint32_t sections)
{
    return sections <= 1 ? 1u : sections <= 2 ? 2u : sections <= 4 ? 4u : 8u;
}
// 16-byte vectors of a stream's tile
CMHIP_IIR_HD constexpr uint32_t iir_tile_vecs(uint32_t C) { return IIR_TILE * C / 8u; }
// samples between two streams' tiles in LDS: B C and ceil(C / 2) dwords, so that the rows of a wave -- which all read
// and write their frame i at the same time -- start in different banks instead of all in one
CMHIP_IIR_HD constexpr uint32_t iir_lds_pitch(uint32_t C) { return IIR_TILE * C + 2u * ((C + 1u) / 2u); }
// frames of tile t of a stream that got `count` frames
CMHIP_IIR_HD inline uint32_t iir_tile_frames(uint32_t count, uint32_t t)
{
    const uint64_t lo = (uint64_t)t * IIR_TILE;
    return lo >= count ? 0u : count - lo < IIR_TILE ? (uint32_t)(count - lo) : IIR_TILE;
}
// vector q of tile t: its first sample in the slot, and how many of its 8 samples lie below the stream's count (8: the
// vector goes whole, 1..7: sample by sample, 0: not at all)
struct IirVec {
    uint32_t off, n;
};
CMHIP_IIR_HD inline IirVec iir_tile_vec(uint32_t count, uint32_t C, uint32_t t, uint32_t q)
{
    IirVec r;
    const uint64_t off = ((uint64_t)t * iir_tile_vecs(C) + q) * 8u, end = (uint64_t)count * C;      // (below 2^31)
    r.off = (uint32_t)off;
    r.n = off >= end ? 0u : end - off < 8u ? (uint32_t)(end - off) : 8u;
    return r;
}

// ---- the launch plan
struct IirPlan {
    int      err;                  // 1: refused
    uint32_t fast;                 // k_iir_fast<C, NP>
    uint32_t np;                   // lanes per row (1 in the any form)
    uint32_t spw;                  // streams per workgroup
    uint32_t grid, block;          // grid 0: nothing to launch (or refused)
    uint32_t tile;                 // B
    uint32_t tiles;                // of the run's longest stream
    uint32_t lds_bytes;            // the workgroup's tiles
};

constexpr bool iir_geometry_ok(uint64_t streams, uint64_t channels, uint64_t sections, uint64_t max_frames)
{
    return streams != 0 && streams < (1ull << 31) && channels >= 1 && channels <= IIR_MAX_CH && sections >= 1 &&
           sections <= IIR_MAX_SEC && max_frames != 0 && max_frames < (1ull << 31) && max_frames * channels < (1ull << 31);
}

// frames: the run's largest count
static inline IirPlan plan_iir(uint32_t streams, uint32_t channels, uint32_t sections, uint32_t frames)
{
    IirPlan p{};
    if (!iir_geometry_ok(streams, channels, sections, 1))
        return p;
    p.fast = channels <= 2 ? 1u : 0u;
    p.np = p.fast ? iir_np(sections) : 1u;
    p.spw = IIR_BLOCK / (channels * p.np);
    p.tile = IIR_TILE;
    p.block = IIR_BLOCK;
    p.lds_bytes = p.spw * iir_lds_pitch(channels) * 2u;
    if (frames == 0)
        return p;
    p.tiles = (uint32_t)(((uint64_t)frames + IIR_TILE - 1u) / IIR_TILE);
    p.grid = (streams + p.spw - 1u) / p.spw;
    return p;
}

}  // namespace cmhip
#endif
