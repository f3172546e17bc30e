// k_mix.h -- what the mixer's and the mix bus's kernel files share (k_mix.hip, k_mixramp.hip; k_bus.h takes the geometry
// and the small steps from here): the workgroup and LDS geometry of the any-channel-count form and its scatter step, the
// dot and pack steps, a ramp's arithmetic, the ONE tile body of the mixer's mono / stereo form with the plain and the
// ramp path (RAMP), and the tile plan.
#ifndef CMHIP_K_MIX_H
#define CMHIP_K_MIX_H

#include "cmhip_device.h"

namespace cmhip {

constexpr u32 MIX_BLOCK = 256;
constexpr u32 MIX_LDS_LIMIT = 64u * 1024u;       // what a workgroup may take without raising the device's limit
constexpr u32 MIX_TILE_MAX = 1024;               // frames of an any-channel-count tile at most: four per thread

__host__ __device__ constexpr u32 mix_cp(u32 ci) { return (ci + 1u) / 2u; }
// LDS of k_mix_any: the matrix (rounded up to whole 16-byte vectors), CP planes of tile dwords, the output tile;
// k_mixr_any has W0 and W1 behind the matrix
__host__ __device__ constexpr u32 mix_wk_lds(u32 ci, u32 co) { return (co * mix_cp(ci) + 3u) & ~3u; }
__host__ __device__ constexpr u32 mix_lds_bytes(u32 ci, u32 co, u32 tile)
{
    return 4u * mix_wk_lds(ci, co) + 4u * mix_cp(ci) * tile + 2u * co * tile;
}
__host__ __device__ constexpr u32 mixr_lds_bytes(u32 ci, u32 co, u32 tile)
{
    return mix_lds_bytes(ci, co, tile) + 8u * mix_wk_lds(ci, co);
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
__device__ __forceinline__ int mix_sat16(long long v)
{
    return (int)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
}

// load_vec (cmhip_device.h) with the load's cache policy a parameter: a stream that feeds many buses (mix-minus) is
// read again by other waves, which a non-temporal load does not favour
template <bool NT>
__device__ __forceinline__ void mix_load_vec(u32 (&x)[4], const int16_t *ins, u32 v, bool full, bool tail, u32 ntail)
{
    u32x4 w = {0, 0, 0, 0};
    if (full) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(ins) + v;
        w = NT ? __builtin_nontemporal_load(p) : *p;
    }
    x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
    if (tail) {
        for (u32 j = 0; j < ntail; j++) {
            const u32 val = (u32)(uint16_t)ins[(u64)v * 8 + j];
#pragma unroll
            for (u32 i = 0; i < 4; i++)
                if (i == (j >> 1))
                    x[i] |= val << (16u * (j & 1u));
        }
    }
}

// ---- a ramp's position and weights (csrc/mix_ramp.h is the same on the host)
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

// ---------------------------------------------------------------------------
// Form 1: mono / stereo on both sides.  A lane works in UNITS of UF frames, the fewest that are whole 16-byte vectors
// on both sides: VI input vectors and VO output vectors.  NU units per lane make four vectors on the wider side:
//     1 -> 1   UF 8, 1 in, 1 out, NU 4: a tile of 2048 frames      2 -> 1   UF 8, 2 in, 1 out, NU 2: 1024 frames
//     2 -> 2   UF 4, 1 in, 1 out, NU 4: 1024 frames                1 -> 2   UF 8, 1 in, 2 out, NU 2: 1024 frames
// Unit j of a lane is unit n0 + 64 j + lane of the stream, so a wave's instruction covers 64 consecutive units.
template <int CI, int CO>
struct MixFast {
    static constexpr u32 UF = 8u / (u32)(CI < CO ? CI : CO);
    static constexpr u32 VI = UF * (u32)CI / 8u, VO = UF * (u32)CO / 8u;
    static constexpr u32 NU = 4u / (VI > VO ? VI : VO);
    static constexpr u32 TILE_FRAMES = 64u * NU * UF;
    static constexpr u32 NOUT = NU * VO * 8u;        // output samples of a lane
};

// The tile of k_mix_fast (RAMP = false) and k_mixr_fast.  Every output sample is ONE dot instruction on an input dword.
// Stereo in: the dword is a frame, the weight dword the row.  Mono in: the dword holds two frames, and the row's weight
// sits in the half of the frame it belongs to (the other half is zero), so no sample is extracted from its dword.
// RAMP: per frame of a unit one position (a 32 x 32 -> 64 multiply, a funnel shift, two mins), per matrix entry two
// multiply-adds and the shift, and the row's dword is packed as the dot instruction wants it; with mono input the two
// halves of an input dword now belong to different frames and meet different weights.
template <int CI, int CO, bool FULL, bool RAMP>
__device__ __forceinline__ void mixr_fast_tile(const MixArgs &a, const u32 *rec, u32 R, u32 done, u32 s, u32 k, u32 F,
                                               const int16_t *a_in, int16_t *a_out, u64 in_stride, u64 out_stride)
{
    using G = MixFast<CI, CO>;
    constexpr u32 VI = G::VI, VO = G::VO, NU = G::NU, UF = G::UF;
    const u32 lane = threadIdx.x & 63u;
    const int16_t *ins = a_in + (u64)s * in_stride;
    int16_t *outs = a_out + (u64)s * out_stride;
    const u32 ns_in = F * (u32)CI, ns_out = F * (u32)CO;
    const u32 nfull_in = ns_in >> 3, ntail_in = ns_in & 7u;
    const u32 nfull_out = ns_out >> 3, ntail_out = ns_out & 7u;
    const u32 n0 = k * 64u * NU;

    // ---- load: every vector of the tile, before the matrices are read
    u32 x[NU][VI][4];
#pragma unroll
    for (u32 j = 0; j < NU; j++) {
#pragma unroll
        for (u32 i = 0; i < VI; i++) {
            const u32 v = (n0 + 64u * j + lane) * VI + i;
            load_vec(x[j][i], ins, v, FULL || v < nfull_in, !FULL && ntail_in && v == nfull_in, ntail_in);
        }
    }

    // ---- the stream's matrices, read only now (the tile's loads depend on kernel arguments alone and are on their
    // way; the barrier keeps the scheduler from moving these reads back up).  One or two dwords at FIXED offsets
    // from an address that is computed in full: no scalar load with a register and an immediate offset.
    __builtin_amdgcn_sched_barrier(0);
    constexpr u32 NW = (u32)CO;                      // CP == 1: one dword per output channel
    u32 wk[2] = {0, 0}, w0k[2] = {0, 0}, w1k[2] = {0, 0}, inc = 0;
    if constexpr (RAMP) {
        inc = uniform(rec[MIXR_INC]);
        w0k[0] = uniform(rec[MIXR_HDR]);
        w1k[0] = uniform(rec[MIXR_HDR + NW]);
        if constexpr (NW > 1) {
            w0k[1] = uniform(rec[MIXR_HDR + NW - 1u]);
            w1k[1] = uniform(rec[MIXR_HDR + 2u * NW - 1u]);
        }
    } else {
        const u32 *wrow = a.wk + (u64)s * NW;
        wk[0] = uniform(wrow[0]);
        wk[1] = NW > 1 ? uniform(wrow[NW - 1u]) : 0u;
    }
    u32 wlo[2], whi[2];                              // the plain path, mono in: the weight in the low / the high half
#pragma unroll
    for (u32 o = 0; o < 2; o++) {
        wlo[o] = wk[o] & 0xffffu;
        whi[o] = wk[o] << 16;
    }

    // ---- arithmetic and stores
    u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
    u32 wf[UF][2];                                   // RAMP: per frame of the unit, the dword its dot meets, per row
    // (output vector i of unit j.  Called once or twice per unit, not from a loop over i: around a loop of one
    // iteration the optimiser promotes the store out of it and the copy it makes is an ordinary store, not "nt")
    auto out_vec = [&](u32 j, auto ic) {
        constexpr u32 i = decltype(ic)::value;
        u32x4 ov;
#pragma unroll
        for (u32 d = 0; d < 4; d++) {
            int acc[2];
#pragma unroll
            for (u32 h = 0; h < 2; h++) {
                const u32 e = (i * 4u + d) * 2u + h;                 // output sample of the unit
                const u32 f = e / (u32)CO, oc = e % (u32)CO;
                const u32 dw = (f * (u32)CI) >> 1;                   // the input dword that holds frame f
                const u32 xin = x[j][dw >> 2][dw & 3u];
                const u32 w = RAMP ? wf[f][oc] : CI == 2 ? wk[oc] : ((f & 1u) ? whi[oc] : wlo[oc]);
                acc[h] = mix_dot2(xin, w, 8192);
            }
            ov[d] = mix_pack(acc[0], acc[1]);
        }
        const u32 v = (n0 + 64u * j + lane) * VO + i;
        if (FULL || v < nfull_out) {
            __builtin_nontemporal_store(ov, dst + v);
        } else if (ntail_out && v == nfull_out) {
            const u32 o[4] = {ov.x, ov.y, ov.z, ov.w};
            store_tail(outs, v, o, ntail_out);
        }
    };
#pragma unroll
    for (u32 j = 0; j < NU; j++) {
        if constexpr (RAMP) {
            const u32 nb = done + (n0 + 64u * j + lane) * UF + 1u;   // the ramp's frame number of the unit's frame 0
#pragma unroll
            for (u32 f = 0; f < UF; f++) {
                const u32 p = mixr_pos(nb + f, R, inc);
#pragma unroll
                for (u32 oc = 0; oc < (u32)CO; oc++) {
                    if constexpr (CI == 2) {
                        wf[f][oc] = mixr_wk(w0k[oc], w1k[oc], p);
                    } else {
                        const u32 w = (u32)mixr_w((int)(short)w0k[oc], (int)(short)w1k[oc], p);
                        wf[f][oc] = (f & 1u) ? w << 16 : w & 0xffffu;
                    }
                }
            }
        }
        out_vec(j, std::integral_constant<u32, 0>{});
        if constexpr (VO == 2)
            out_vec(j, std::integral_constant<u32, 1>{});
    }
}

// ---------------------------------------------------------------------------
// Form 2: any pair of channel counts (k_mix.hip, "Form 2", explains the planes).

// Step 1 for one vector, in all four any-channel-count kernels: the eight samples x of vector w of the tile's input go
// into the planes, as far as they belong to the slot's nt frames in the tile.  (No loop in here, and none of the
// kernels' own loops moved into a function: a function with a loop is optimised on its own before it is inlined, and
// the kernel's code then comes out in another order.)
__device__ __forceinline__ void mix_scatter_vec(u32 *plane, const u32 (&x)[4], u32 w, u32 nt, u32 CI, u32 CP, u32 tile)
{
    int16_t *plane16 = reinterpret_cast<int16_t *>(plane);
    if ((CI & 1u) == 0) {
#pragma unroll
        for (u32 i = 0; i < 4; i++) {
            const u32 e = w * 4u + i;                                // dword of the tile
            const u32 f = e / CP, kk = e - f * CP;
            if (f < nt)
                plane[kk * tile + f] = x[i];
        }
    } else {
#pragma unroll
        for (u32 i = 0; i < 8; i++) {
            const u32 e = w * 8u + i;                                // sample of the tile
            const u32 f = e / CI, ch = e - f * CI;
            if (f < nt)
                plane16[((ch >> 1) * tile + f) * 2u + (ch & 1u)] = (int16_t)(x[i >> 1] >> (16u * (i & 1u)));
        }
    }
}

// ---------------------------------------------------------------------------
// The plan of a run over `rows` streams or buses (Plan: MixPlan, BusPlan): MixFast's tile for the mono / stereo forms,
// otherwise the largest power-of-two tile whose LDS, lds(tile) bytes, fits; refused where tiles x rows would be a grid
// of 2^31 workgroups (as plan_run)
template <class Plan, class L>
inline Plan mix_plan_tiles(u32 rows, u32 CI, u32 CO, u32 frames, L lds)
{
    Plan p{};
    p.err = hipSuccess;
    if (rows == 0 || frames == 0 || CI == 0 || CI > MAX_CH || CO == 0 || CO > MAX_CH)
        return p;
    u32 tile;
    const bool fast = CI <= 2 && CO <= 2;
    if (fast) {
        tile = CI == 1 && CO == 1 ? MixFast<1, 1>::TILE_FRAMES : MixFast<2, 2>::TILE_FRAMES;     // (2048 : 1024)
    } else {
        for (tile = MIX_TILE_MAX; lds(tile) > MIX_LDS_LIMIT; tile >>= 1)
            ;
    }
    const u64 tiles = ((u64)frames + tile - 1u) / tile;
    if (tiles * rows >= (1ull << 31)) {
        p.err = hipErrorInvalidValue;
        return p;
    }
    p.fast = fast ? 1u : 0u;
    p.block = fast ? 64u : MIX_BLOCK;
    p.tile_frames = tile;
    p.lds_bytes = fast ? 0u : lds(tile);
    p.chunks = (u32)tiles;
    p.grid = rows * p.chunks;
    return p;
}

}  // namespace cmhip
#endif
