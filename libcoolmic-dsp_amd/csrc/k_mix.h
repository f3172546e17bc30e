// k_mix.h -- what the mixer's kernel files share (k_mix.hip, k_mixramp.hip; k_busramp.hip takes the ramp's steps from here): the workgroup and LDS geometry of the
// any-channel-count form, the dot and pack steps, and the tile geometry of the mono / stereo form.
#ifndef CMHIP_K_MIX_H
#define CMHIP_K_MIX_H

#include "cmhip_device.h"

namespace cmhip {

constexpr u32 MIX_BLOCK = 256;
constexpr u32 MIX_LDS_LIMIT = 64u * 1024u;       // what a workgroup may take without raising the device's limit
constexpr u32 MIX_TILE_MAX = 1024;               // frames of a k_mix_any tile at most: four per thread

__host__ __device__ constexpr u32 mix_cp(u32 ci) { return (ci + 1u) / 2u; }
// LDS of k_mix_any: the matrix (rounded up to whole 16-byte vectors), CP planes of tile dwords, the output tile
__host__ __device__ constexpr u32 mix_wk_lds(u32 ci, u32 co) { return (co * mix_cp(ci) + 3u) & ~3u; }
__host__ __device__ constexpr u32 mix_lds_bytes(u32 ci, u32 co, u32 tile)
{
    return 4u * mix_wk_lds(ci, co) + 4u * mix_cp(ci) * tile + 2u * co * tile;
}

__device__ __forceinline__ int mix_dot2(u32 x, u32 k, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, k), acc, false);
}
// two accumulators (rounding included) -> one dword of output: shift, then clamp and pack
__device__ __forceinline__ u32 mix_pack(int a0, int a1)
{
    return __builtin_bit_cast(u32, __builtin_amdgcn_cvt_pk_i16(a0 >> 14, a1 >> 14));
}

// ---- a ramp's position and weights (k_mixramp.hip, k_busramp.hip; csrc/mix_ramp.h is the same on the host)
// n is clamped to R first: then n * inc <= R * ceil(2^32 / R) < 2^32 + R, and the shifted product fits 32 bits
__device__ __forceinline__ u32 mixr_pos(u32 n, u32 R, u32 inc)
{
    const u64 q = (u64)min(n, R) * inc;
    return min((u32)(q >> 17), 32768u);
}
// one entry: |N| <= 2^30; adding 32767 to a negative N turns the arithmetic shift into truncation towards zero
__device__ __forceinline__ int mixr_w(int w0, int w1, u32 p)
{
    const int N = w0 * (int)(32768u - p) + w1 * (int)p;
    return (N + ((N >> 31) & 32767)) >> 15;
}
// both halves of a kernel-form dword
__device__ __forceinline__ u32 mixr_wk(u32 k0, u32 k1, u32 p)
{
    const int lo = mixr_w((int)(short)k0, (int)(short)k1, p);
    const int hi = mixr_w((int)k0 >> 16, (int)k1 >> 16, p);
    return ((u32)lo & 0xffffu) | ((u32)hi << 16);
}

// the mono / stereo form's geometry (k_mix.hip, "Form 1", explains the units)
template <int CI, int CO>
struct MixFast {
    static constexpr u32 UF = 8u / (u32)(CI < CO ? CI : CO);
    static constexpr u32 VI = UF * (u32)CI / 8u, VO = UF * (u32)CO / 8u;
    static constexpr u32 NU = 4u / (VI > VO ? VI : VO);
    static constexpr u32 TILE_FRAMES = 64u * NU * UF;
};

}  // namespace cmhip
#endif
