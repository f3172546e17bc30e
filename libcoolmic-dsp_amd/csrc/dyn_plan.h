// dyn_plan.h -- the geometry, the curve's index function and the launch plan of the dynamics stage
// (include/coolmic_hip.h, "dynamics").  Plain C++17, no HIP: tests/cpp/dyn_plan_test.cpp and tests/cpp/dyn_rms_test.cpp
// compile it with g++ alone; the kernels (k_dyn.hip) use the same index function and the same root.
//
//   a = detector_log2 in 3..10, A = 2^a: the level window.  b = smooth_log2 in 3..9, B = 2^b: the gain's ramp; D = B - 1
//   (the delay).  H = hold, W = B + H <= 2048.  HIST = (A - 1) + (W - 1) + (B - 1): the earlier frames an output depends on.
//   halo = HIST rounded up to 8 frames: what a stream's history slot holds and what a tile evaluates in front of its own
//   frames -- a multiple of 8 so that a slot is whole 16-byte vectors for every channel count and lines up with the
//   stream's vectors (frame -1 of a run is the slot's last frame).
//   A workgroup of 256 threads takes one stream and a tile of tile_frames frames: the largest power of two <= 4096 that
//   is >= halo (so the frames in front of a tile never reach past the previous tile) and whose per-frame dwords,
//   (tile_frames + halo) * 4 bytes of dynamic LDS, fit 64 KiB (no per-device limit is raised).
#ifndef CMHIP_DYN_PLAN_H
#define CMHIP_DYN_PLAN_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CMHIP_DYN_HD __host__ __device__
#else
#define CMHIP_DYN_HD
#endif

namespace cmhip {

constexpr uint32_t DYN_BLOCK = 256;
constexpr uint32_t DYN_TILE_MAX = 4096;
constexpr uint32_t DYN_LDS_LIMIT = 64u * 1024u;
constexpr uint32_t DYN_MAX_CH = 16;
constexpr uint32_t DYN_A_MIN = 3, DYN_A_MAX = 10;
constexpr uint32_t DYN_B_MIN = 3, DYN_B_MAX = 9;
constexpr uint32_t DYN_W_MAX = 2048;
constexpr uint32_t DYN_HALO_MAX = 3584;              // a = 10, b = 9, W = 2048: HIST = 3581
constexpr uint32_t DYN_UNITY = 32768;                // Q15
constexpr uint32_t DYN_CURVE = 128;                  // entries of a curve (CMHIP_DYN_CURVE)
constexpr uint32_t DYN_CURVE_USED = 123;             // entries 0..122 are read
constexpr uint32_t DYN_KNOT_MAX = 121;               // level 32768: the largest index a lookup reaches
constexpr uint32_t DYN_DETECT_MEAN = 0;              // CMHIP_DYN_DETECT_*: L is the mean magnitude over A frames ...
constexpr uint32_t DYN_DETECT_RMS = 1;               // ... or the root of the mean square
constexpr uint32_t DYN_SQ_SPLIT = 15;                // e^2 = hi * 2^15 + lo: the halves the RMS detector sums apart

struct DynGeom {
    uint32_t a, A, b, B, D, H, W, hist, halo;
};

// false: detector_log2, smooth_log2 or hold out of range (g is not written)
inline bool dyn_geom(uint32_t detector_log2, uint32_t smooth_log2, uint32_t hold, DynGeom *g)
{
    if (detector_log2 < DYN_A_MIN || detector_log2 > DYN_A_MAX || smooth_log2 < DYN_B_MIN || smooth_log2 > DYN_B_MAX)
        return false;
    const uint32_t A = 1u << detector_log2, B = 1u << smooth_log2;
    if (hold > DYN_W_MAX - B)
        return false;
    if (g) {
        g->a = detector_log2;
        g->A = A;
        g->b = smooth_log2;
        g->B = B;
        g->D = B - 1u;
        g->H = hold;
        g->W = B + hold;
        g->hist = (A - 1u) + (g->W - 1u) + (B - 1u);
        g->halo = (g->hist + 7u) & ~7u;
    }
    return true;
}

// every used entry of a curve is a gain of at most unity; entries 123..127 are ignored
inline bool dyn_curve_ok(const uint16_t *curve)
{
    for (uint32_t k = 0; k < DYN_CURVE_USED; k++)
        if (curve[k] > DYN_UNITY)
            return false;
    return true;
}

// Where level l (0..32768) lies on the curve's grid, 8 knots per octave: curve(l) = T[idx] + ((T[idx+1] - T[idx]) * frac
// >> sh).  With E = floor(log2 l) and l normalised to bit 15, the three bits below the leading one are the knot inside
// the octave for E >= 3 (l >> (E - 3)) and for E < 3 (l << (3 - E)) alike, so neither case needs a branch; l == 0 is one
// select.
struct DynIndex {
    uint32_t idx, frac, sh;
};
CMHIP_DYN_HD inline DynIndex dyn_index(uint32_t l)
{
    const uint32_t E = 31u - (uint32_t)__builtin_clz(l | 1u);      // (l == 0: E = 0, and idx is taken as 0 below)
    const uint32_t norm = l << (15u - E);                         // the leading one at bit 15
    DynIndex r;
    r.sh = E > 3u ? E - 3u : 0u;
    r.frac = l & ((1u << r.sh) - 1u);
    r.idx = l ? 1u + 8u * E + ((norm >> 12) & 7u) : 0u;
    return r;
}

// the curve at level l, on the host (the kernels read T[idx] and T[idx+1] as one packed dword)
inline uint32_t dyn_curve_at(const uint16_t *T, uint32_t l)
{
    const DynIndex i = dyn_index(l);
    const int t0 = (int)T[i.idx], t1 = (int)T[i.idx + 1u];
    return (uint32_t)(t0 + (((t1 - t0) * (int)i.frac) >> i.sh));
}

// The RMS detector's root: the largest r with r * r <= v, for every v below 2^32.  The seed is a float root and the result
// does not rest on how it rounds: (float)v is off by at most v * 2^-24, a root of a few units in the last place keeps the
// relative error of the seed below 2^-21, and the root is at most 65536, so the seed lies within 2^-5 of sqrt(v) and its
// integer part within 1 of the answer.  One step down and one step up, compared in integers, repair that.  The seed is
// clamped to 65535 first, so r * r and v - r * r stay inside 32 bits.
CMHIP_DYN_HD inline uint32_t dyn_isqrt(uint32_t v)
{
    uint32_t r = (uint32_t)__builtin_sqrtf((float)v);
    r = r > 65535u ? 65535u : r;
    if (r * r > v)
        r--;
    if (v - r * r > 2u * r)                           // (r + 1)^2 <= v
        r++;
    return r;
}

// The RMS detector's sum of squares from its two halves: with e^2 = hi * 2^15 + lo, lo < 2^15, and the sums of hi and of
// lo over A = 2^a frames (each at most 2^25), (sum_hi * 2^15 + sum_lo) >> a without 64 bits: a <= 10 < 15, so the first
// term is a multiple of 2^a and the shift splits.  At most 2^30.
CMHIP_DYN_HD inline uint32_t dyn_mean_square(uint32_t sum_hi, uint32_t sum_lo, uint32_t a)
{
    return (sum_hi << (DYN_SQ_SPLIT - a)) + (sum_lo >> a);
}

struct DynPlan {
    int      err;                  // 1: refused, the grid would reach 2^31 workgroups
    uint32_t fast;                 // the mono / stereo kernel; otherwise the any-channel-count kernel
    uint32_t grid, block;          // grid 0: nothing to launch (or refused, or bad geometry)
    uint32_t chunks;               // tiles per stream
    uint32_t tile_frames;
    uint32_t lds_bytes;            // dynamic LDS of the launch
    uint32_t halo;
    uint32_t passes;               // a + floor(log2 W) + (W not a power of two) + b; the RMS detector: a more
};

// the plan of a run whose longest stream has `frames` frames.  The RMS detector has the mean detector's tile, grid and
// LDS: the two halves of a square go through the same dword per frame one after the other (a more add passes).
inline DynPlan plan_dyn(uint32_t streams, uint32_t channels, uint32_t detector_log2, uint32_t smooth_log2, uint32_t hold,
                        uint32_t frames, uint32_t detector = DYN_DETECT_MEAN)
{
    DynPlan p{};
    DynGeom g;
    if (streams == 0 || frames == 0 || channels == 0 || channels > DYN_MAX_CH ||
        detector > DYN_DETECT_RMS || !dyn_geom(detector_log2, smooth_log2, hold, &g))
        return p;
    uint32_t tile = DYN_TILE_MAX;
    while (tile / 2u >= g.halo && tile / 2u >= 8u && (tile + g.halo) * 4u > DYN_LDS_LIMIT)
        tile >>= 1;                                   // (never taken today: 4096 + 3584 frames are 30 KiB)
    const uint64_t tiles = ((uint64_t)frames + tile - 1u) / tile;
    if (tiles * streams >= (1ull << 31)) {
        p.err = 1;
        return p;
    }
    p.fast = channels <= 2u ? 1u : 0u;
    p.block = DYN_BLOCK;
    p.tile_frames = tile;
    p.lds_bytes = (tile + g.halo) * 4u;
    p.halo = g.halo;
    p.chunks = (uint32_t)tiles;
    p.grid = streams * p.chunks;
    uint32_t P = 1, lw = 0;
    for (; 2u * P <= g.W; P *= 2u)
        lw++;
    p.passes = g.a + lw + (g.W > P ? 1u : 0u) + g.b + (detector == DYN_DETECT_RMS ? g.a : 0u);
    return p;
}

}  // namespace cmhip
#endif
