// k_bus.h -- what the mix bus's kernel files share (k_bus.hip, k_busramp.hip): the LDS geometry of the any-channel-count
// form, the ONE tile body of the mono / stereo form with the plain and the ramp path (RAMP), and the dispatch of its
// eight instances.  The units, the dot and pack steps, the loads and the ramp's arithmetic are the mixer's (k_mix.h).
#ifndef CMHIP_K_BUS_H
#define CMHIP_K_BUS_H

#include "k_mix.h"

#include "bus_ramp.h"

namespace cmhip {

constexpr u32 BUS_FLAG = 0x80000000u;            // bit 31 of a word of first[] / send[]

// LDS of k_bus_any: the int64 accumulators of the tile, CP planes of tile dwords, one send's matrix (rounded up to
// whole 16-byte vectors), the output tile -- in this order, so that each part is aligned for its widest access.
// k_busr_any has three matrices where k_bus_any has one: the send's target, W0 and W1
__host__ __device__ constexpr u32 bus_lds_bytes(u32 ci, u32 co, u32 tile)
{
    return 8u * co * tile + 4u * mix_cp(ci) * tile + 4u * mix_wk_lds(ci, co) + 2u * co * tile;
}
__host__ __device__ constexpr u32 busr_lds_bytes(u32 ci, u32 co, u32 tile)
{
    return 8u * co * tile + 4u * mix_cp(ci) * tile + 12u * mix_wk_lds(ci, co) + 2u * co * tile;
}

// ---------------------------------------------------------------------------
// Form 1: mono / stereo on both sides, in MixFast's units and tile (k_mix.h): unit u of a lane is unit n0 + 64 u + lane
// of the slot.

// one send of the tile in flight: its vectors, its weight dwords, its flags -- and, RAMP, its ramp.  (Two layouts
// written out, not one with optional members: the order of the fields reaches the register allocator.)
template <int CI, int CO, bool RAMP>
struct BusSend;
template <int CI, int CO>
struct BusSend<CI, CO, false> {
    u32 x[MixFast<CI, CO>::NU][MixFast<CI, CO>::VI][4];
    u32 wk[2];
    u32 start;                                       // the send starts a group
    u32 live;                                        // its stream reaches into this tile
};
template <int CI, int CO>
struct BusSend<CI, CO, true> {
    u32 x[MixFast<CI, CO>::NU][MixFast<CI, CO>::VI][4];
    u32 wk[2];
    u32 w0k[2], w1k[2], inc, R, done;                // read only when the tile begins inside the ramp
    u32 start;
    u32 live;
    u32 ramp;                                        // the tile begins inside its ramp
};

// Everything of send j is wave-uniform and read as scalars at FIXED offsets from addresses computed in full -- no
// scalar load with a register and an immediate offset (tests/test_abi.py tells why).  A send whose stream ends at or
// before the tile's first frame is skipped: neither its slot nor its record is read (its position moves on all the
// same, in k_busr_advance).  The vectors zero-fill past the SEND's own count, which may be below the bus's.
template <int CI, int CO, bool NT, bool RAMP>
__device__ __forceinline__ void bus_fetch(const BusArgs &a, const u32 *ramp, u32 j, u32 k, u32 f0,
                                          BusSend<CI, CO, RAMP> &t)
{
    using G = MixFast<CI, CO>;
    constexpr u32 VI = G::VI, NU = G::NU, NW = (u32)CO;      // CP == 1: one dword per output channel
    const u32 lane = threadIdx.x & 63u;
    const u32 *sp = a.send + j;
    const u32 word = uniform(sp[0]);
    const u32 s = word & ~BUS_FLAG;
    t.start = word >> 31;
    if constexpr (RAMP)
        t.ramp = 0;
    const u32 *wrow = a.wk + (u64)j * NW;
    t.wk[0] = uniform(wrow[0]);
    t.wk[1] = NW > 1 ? uniform(wrow[NW - 1u]) : 0u;
    u32 c = a.frames;
    if (a.nframes) {                                 // (uniform: a kernel argument)
        const u32 *cs = a.nframes + s;
        c = uniform(cs[0]);
    }
    t.live = c > f0 ? 1u : 0u;
    if (!t.live)                                     // (uniform)
        return;
    if constexpr (RAMP) {
        const u32 *rec = ramp + (u64)j * (BUSR_HDR + 2u * NW);
        t.R = uniform(rec[BUSR_R]);
        t.done = uniform(rec[BUSR_DONE]);
        t.ramp = t.done + f0 < t.R ? 1u : 0u;        // (done <= 2^20 and f0 < 2^31: no wrap)
        if (t.ramp) {                                // (uniform)
            t.inc = uniform(rec[BUSR_INC]);
            t.w0k[0] = uniform(rec[BUSR_HDR]);
            t.w1k[0] = uniform(rec[BUSR_HDR + NW]);
            t.w0k[1] = NW > 1 ? uniform(rec[BUSR_HDR + NW - 1u]) : 0u;
            t.w1k[1] = NW > 1 ? uniform(rec[BUSR_HDR + 2u * NW - 1u]) : 0u;
        }
    }
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    const u32 ns = c * (u32)CI, nfull = ns >> 3, ntail = ns & 7u;
    const u32 n0 = k * 64u * NU;
    if (f0 + G::TILE_FRAMES <= c) {                  // (uniform) the send covers the tile
#pragma unroll
        for (u32 u = 0; u < NU; u++)
#pragma unroll
            for (u32 i = 0; i < VI; i++)
                mix_load_vec<NT>(t.x[u][i], ins, (n0 + 64u * u + lane) * VI + i, true, false, 0);
    } else {
#pragma unroll
        for (u32 u = 0; u < NU; u++)
#pragma unroll
            for (u32 i = 0; i < VI; i++) {
                const u32 v = (n0 + 64u * u + lane) * VI + i;
                mix_load_vec<NT>(t.x[u][i], ins, v, v < nfull, ntail && v == nfull, ntail);
            }
    }
}

// One dot instruction per output sample and send, on the input dword that holds the frame (k_mix_fast's scheme: with
// mono input the weight sits in the half of the dword its frame is in), chained in int32 inside a group.  At a group's
// first send the int32 accumulators are added into the int64 ones (WIDE; a bus of one group has none).  RAMP, inside
// the ramp: a lane first makes, per frame of the unit, the position (k_mixr_fast's steps) and per row the dword its
// dot meets; with mono input the two halves of an input dword then meet different weights.
template <int CI, int CO, bool WIDE, bool RAMP>
__device__ __forceinline__ void bus_consume(const BusSend<CI, CO, RAMP> &t, u32 f0, int (&acc)[MixFast<CI, CO>::NOUT],
                                            long long (&tot)[WIDE ? MixFast<CI, CO>::NOUT : 1u])
{
    using G = MixFast<CI, CO>;
    constexpr u32 NOUT = G::NOUT, UF = G::UF;
    if constexpr (WIDE) {
        if (t.start) {                               // (uniform)
#pragma unroll
            for (u32 e = 0; e < NOUT; e++) {
                tot[e] += acc[e];
                acc[e] = 0;
            }
        }
    }
    if (!t.live)                                     // (uniform)
        return;
    if constexpr (RAMP) {
        if (t.ramp) {                                // (uniform)
            const u32 lane = threadIdx.x & 63u;
#pragma unroll
            for (u32 u = 0; u < G::NU; u++) {
                const u32 nb = t.done + f0 + (64u * u + lane) * UF + 1u;     // the ramp's frame number of the unit's frame 0
                u32 wf[UF][2];
#pragma unroll
                for (u32 f = 0; f < UF; f++) {
                    const u32 p = mixr_pos(nb + f, t.R, t.inc);
#pragma unroll
                    for (u32 oc = 0; oc < (u32)CO; oc++) {
                        if constexpr (CI == 2) {
                            wf[f][oc] = mixr_wk(t.w0k[oc], t.w1k[oc], p);
                        } else {
                            const u32 w = (u32)mixr_w((int)(short)t.w0k[oc], (int)(short)t.w1k[oc], p);
                            wf[f][oc] = (f & 1u) ? w << 16 : w & 0xffffu;
                        }
                    }
                }
#pragma unroll
                for (u32 e = 0; e < G::VO * 8u; e++) {                       // output sample of the unit
                    const u32 f = e / (u32)CO, oc = e % (u32)CO;
                    const u32 dw = (f * (u32)CI) >> 1;                       // the input dword that holds frame f
                    acc[u * G::VO * 8u + e] = mix_dot2(t.x[u][dw >> 2][dw & 3u], wf[f][oc], acc[u * G::VO * 8u + e]);
                }
            }
            return;
        }
    }
    u32 wlo[2], whi[2];                              // mono in: the weight in the low / the high half
#pragma unroll
    for (u32 o = 0; o < 2; o++) {
        wlo[o] = t.wk[o] & 0xffffu;
        whi[o] = t.wk[o] << 16;
    }
#pragma unroll
    for (u32 u = 0; u < G::NU; u++) {
#pragma unroll
        for (u32 e = 0; e < G::VO * 8u; e++) {       // output sample of the unit
            const u32 f = e / (u32)CO, oc = e % (u32)CO;
            const u32 dw = (f * (u32)CI) >> 1;       // the input dword that holds frame f
            const u32 w = CI == 2 ? t.wk[oc] : ((f & 1u) ? whi[oc] : wlo[oc]);
            acc[u * G::VO * 8u + e] = mix_dot2(t.x[u][dw >> 2][dw & 3u], w, acc[u * G::VO * 8u + e]);
        }
    }
}

template <int CI, int CO, bool NT, bool FULL, bool WIDE, bool RAMP>
__device__ __forceinline__ void bus_fast_tile(const BusArgs &a, const u32 *ramp, u32 b, u32 k, u32 F, u32 j0, u32 j1)
{
    using G = MixFast<CI, CO>;
    constexpr u32 VO = G::VO, NU = G::NU, NOUT = G::NOUT;
    const u32 lane = threadIdx.x & 63u;
    const u32 f0 = k * G::TILE_FRAMES;
    int acc[NOUT];
    long long tot[WIDE ? NOUT : 1u];
#pragma unroll
    for (u32 e = 0; e < NOUT; e++)
        acc[e] = WIDE ? 0 : 8192;                    // (one group: the rounding costs no instruction)
#pragma unroll
    for (u32 e = 0; e < (WIDE ? NOUT : 1u); e++)
        tot[e] = 0;

    // ---- the sends, two in flight: the loads of send j + 1 are issued before the arithmetic of send j
    BusSend<CI, CO, RAMP> ta, tb;
    bus_fetch<CI, CO, NT, RAMP>(a, ramp, j0, k, f0, ta);
    for (u32 j = j0; j < j1; j += 2) {
        if (j + 1u < j1)
            bus_fetch<CI, CO, NT, RAMP>(a, ramp, j + 1u, k, f0, tb);
        __builtin_amdgcn_sched_barrier(0);
        bus_consume<CI, CO, WIDE, RAMP>(ta, f0, acc, tot);
        if (j + 1u >= j1)
            break;
        if (j + 2u < j1)
            bus_fetch<CI, CO, NT, RAMP>(a, ramp, j + 2u, k, f0, ta);
        __builtin_amdgcn_sched_barrier(0);
        bus_consume<CI, CO, WIDE, RAMP>(tb, f0, acc, tot);
    }

    // ---- the tail and the stores
    int16_t *outs = a.out + (u64)b * a.out_stride;
    const u32 ns_out = F * (u32)CO, nfull_out = ns_out >> 3, ntail_out = ns_out & 7u;
    const u32 n0 = k * 64u * NU;
    u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
    // (output vector i of unit u.  Called once or twice per unit, not from a loop over i: k_mix.h, mixr_fast_tile)
    auto out_vec = [&](u32 u, auto ic) {
        constexpr u32 i = decltype(ic)::value;
        u32x4 ov;
#pragma unroll
        for (u32 d = 0; d < 4; d++) {
            int r[2];
#pragma unroll
            for (u32 h = 0; h < 2; h++) {
                const u32 e = (u * VO + i) * 8u + d * 2u + h;
                if constexpr (WIDE)
                    r[h] = mix_sat16((tot[e] + acc[e] + 8192) >> 14);
                else
                    r[h] = acc[e] >> 14;
            }
            ov[d] = __builtin_bit_cast(u32, __builtin_amdgcn_cvt_pk_i16(r[0], r[1]));   // (clamps and packs)
        }
        const u32 v = (n0 + 64u * u + lane) * VO + i;
        if (FULL || v < nfull_out) {
            __builtin_nontemporal_store(ov, dst + v);
        } else if (ntail_out && v == nfull_out) {
            const u32 o[4] = {ov.x, ov.y, ov.z, ov.w};
            store_tail(outs, v, o, ntail_out);
        }
    };
#pragma unroll
    for (u32 u = 0; u < NU; u++) {
        out_vec(u, std::integral_constant<u32, 0>{});
        if constexpr (VO == 2)
            out_vec(u, std::integral_constant<u32, 1>{});
    }
}

// The eight instances of the mono / stereo form: launch(CI, CO, NT) as integral constants
template <class L>
inline void bus_fast_dispatch(u32 ci, u32 co, bool nt, L &&launch)
{
    using std::integral_constant;
    using I1 = integral_constant<int, 1>;
    using I2 = integral_constant<int, 2>;
    switch ((ci * 2u + co) * 2u + (nt ? 1u : 0u)) {
    case 6: launch(I1{}, I1{}, std::false_type{}); break;
    case 7: launch(I1{}, I1{}, std::true_type{}); break;
    case 8: launch(I1{}, I2{}, std::false_type{}); break;
    case 9: launch(I1{}, I2{}, std::true_type{}); break;
    case 10: launch(I2{}, I1{}, std::false_type{}); break;
    case 11: launch(I2{}, I1{}, std::true_type{}); break;
    case 12: launch(I2{}, I2{}, std::false_type{}); break;
    default: launch(I2{}, I2{}, std::true_type{}); break;
    }
}

}  // namespace cmhip
#endif
