// k_busramp.hip -- gfx950 (MI355X, wave64) kernels of the mix bus's send ramps: a send's matrix moves from W0 to W1
// over R output frames of its bus, every frame with a matrix of its own, in exact integers (include/coolmic_hip.h,
// "send ramps"; the ramp's arithmetic is the mixer's, k_mix.h / csrc/mix_ramp.h, the sum and its one rounding are
// k_bus.hip's):
//     p(n) = min(32768, (min(n, R) * inc) >> 17)     N = w0 * (32768 - p) + w1 * p     w = N / 32768 towards zero
//     p_j  = sum_c w_j[o][c] * x[stream_j][f][c]     acc = sum_j p_j (int64)           y = saturate((acc + 8192) >> 14)
//
//   k_busr_fast<CI, CO, NT>  CI, CO in {1, 2}: k_bus_fast's tile (MixFast's geometry), one wave per (bus, tile), two
//                            sends in flight; a send inside its ramp makes its frames' weight dwords in VGPRs
//   k_busr_any               every other pair up to 16 -> 16: k_bus_any's staging, W0 and W1 beside the send's matrix
//   k_busr_advance           moves every ramping send's position on by its bus's count of the run before
//
// Per send, in the table's compiled order, a record (BusRampArgs::ramp; csrc/bus_ramp.h has the layout): inc, R, done,
// bus, W0[n], W1[n].  The send ramps while done < R, and frame f of its bus is the ramp's frame n = done + f + 1.  Per
// (tile, send) "done + f0 < R" is uniform: a send outside its ramp -- one that never ramped included -- takes
// k_bus.hip's path with the target's dwords from BusArgs::wk.  The group flags are compiled from BOTH ends of every
// running ramp (csrc/bus_ramp.h), so the int32 chain over a group is exact at every position of every ramp.  These
// kernels run only while some send ramps; at every other time the bus launches k_bus.hip's.  k_bus.hip is left as it
// is, so what the two files have in common -- the vector load with a cache policy, the tail -- is written out here.
#include "k_mix.h"

#include "bus_ramp.h"

namespace cmhip {

constexpr u32 BUSR_BLOCK = 256;
constexpr u32 BUSR_LDS_LIMIT = 64u * 1024u;      // what a workgroup may take without raising the device's limit
constexpr u32 BUSR_TILE_MAX = 1024;              // frames of a k_busr_any tile at most: four per thread
constexpr u32 BUSR_FLAG = 0x80000000u;           // bit 31 of a word of first[] / send[]

// LDS of k_busr_any: k_bus_any's parts with three matrices where it has one -- the int64 accumulators of the tile, CP
// planes of tile dwords, the send's target, W0 and W1 (each rounded up to whole 16-byte vectors), the output tile
__host__ __device__ constexpr u32 busr_lds_bytes(u32 ci, u32 co, u32 tile)
{
    return 8u * co * tile + 4u * mix_cp(ci) * tile + 12u * mix_wk_lds(ci, co) + 2u * co * tile;
}

__device__ __forceinline__ int busr_sat16(long long v)
{
    return (int)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
}

// (k_bus.hip's bus_load_vec: load_vec with the cache policy a parameter)
template <bool NT>
__device__ __forceinline__ void busr_load_vec(u32 (&x)[4], const int16_t *ins, u32 v, bool full, bool tail, u32 ntail)
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

// ---------------------------------------------------------------------------
// Form 1: mono / stereo on both sides, k_bus_fast's units and tile (k_mix.hip explains them).

// one send of the tile in flight: its vectors, its target's dwords and flags as k_bus_fast has them, and its ramp
template <int CI, int CO>
struct BusrSend {
    u32 x[MixFast<CI, CO>::NU][MixFast<CI, CO>::VI][4];
    u32 wk[2];
    u32 w0k[2], w1k[2], inc, R, done;                // read only when the tile begins inside the ramp
    u32 start;                                       // the send starts a group
    u32 live;                                        // its stream reaches into this tile
    u32 ramp;                                        // the tile begins inside its ramp
};

// Everything of send j is wave-uniform and read as scalars at FIXED offsets from addresses computed in full (tests/
// test_abi.py tells why).  A send whose stream ends at or before the tile's first frame is skipped: neither its slot
// nor its record is read (its position moves on all the same, in k_busr_advance).
template <int CI, int CO, bool NT>
__device__ __forceinline__ void busr_fetch(const BusRampArgs &ra, u32 j, u32 k, u32 f0, BusrSend<CI, CO> &t)
{
    using G = MixFast<CI, CO>;
    constexpr u32 VI = G::VI, NU = G::NU, NW = (u32)CO;      // CP == 1: one dword per output channel
    const BusArgs &a = ra.b;
    const u32 lane = threadIdx.x & 63u;
    const u32 *sp = a.send + j;
    const u32 word = uniform(sp[0]);
    const u32 s = word & ~BUSR_FLAG;
    t.start = word >> 31;
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
    const u32 *rec = ra.ramp + (u64)j * (BUSR_HDR + 2u * NW);
    t.R = uniform(rec[BUSR_R]);
    t.done = uniform(rec[BUSR_DONE]);
    t.ramp = t.done + f0 < t.R ? 1u : 0u;            // (done <= 2^20 and f0 < 2^31: no wrap)
    if (t.ramp) {                                    // (uniform)
        t.inc = uniform(rec[BUSR_INC]);
        t.w0k[0] = uniform(rec[BUSR_HDR]);
        t.w1k[0] = uniform(rec[BUSR_HDR + NW]);
        t.w0k[1] = NW > 1 ? uniform(rec[BUSR_HDR + NW - 1u]) : 0u;
        t.w1k[1] = NW > 1 ? uniform(rec[BUSR_HDR + 2u * NW - 1u]) : 0u;
    }
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    const u32 ns = c * (u32)CI, nfull = ns >> 3, ntail = ns & 7u;
    const u32 n0 = k * 64u * NU;
    if (f0 + G::TILE_FRAMES <= c) {                  // (uniform) the send covers the tile
#pragma unroll
        for (u32 u = 0; u < NU; u++)
#pragma unroll
            for (u32 i = 0; i < VI; i++)
                busr_load_vec<NT>(t.x[u][i], ins, (n0 + 64u * u + lane) * VI + i, true, false, 0);
    } else {
#pragma unroll
        for (u32 u = 0; u < NU; u++)
#pragma unroll
            for (u32 i = 0; i < VI; i++) {
                const u32 v = (n0 + 64u * u + lane) * VI + i;
                busr_load_vec<NT>(t.x[u][i], ins, v, v < nfull, ntail && v == nfull, ntail);
            }
    }
}

// k_bus_fast's consume: one dot per output sample and send on the input dword that holds the frame, chained in int32
// inside a group.  Inside the ramp a lane first makes, per frame of the unit, the position (k_mixr_fast's steps: a 32 x
// 32 -> 64 multiply, a shift, two mins) and per row the dword its dot meets; with mono input the weight goes into the
// half of the dword its frame sits in, so the two halves of an input dword meet different weights.
template <int CI, int CO, bool WIDE>
__device__ __forceinline__ void busr_consume(const BusrSend<CI, CO> &t, u32 f0, int (&acc)[MixFast<CI, CO>::NU * MixFast<CI, CO>::VO * 8u],
                                             long long (&tot)[WIDE ? MixFast<CI, CO>::NU * MixFast<CI, CO>::VO * 8u : 1u])
{
    using G = MixFast<CI, CO>;
    constexpr u32 NOUT = G::NU * G::VO * 8u, UF = G::UF;
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
    if (t.ramp) {                                    // (uniform)
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
            for (u32 e = 0; e < G::VO * 8u; e++) {   // output sample of the unit
                const u32 f = e / (u32)CO, oc = e % (u32)CO;
                const u32 dw = (f * (u32)CI) >> 1;   // the input dword that holds frame f
                acc[u * G::VO * 8u + e] = mix_dot2(t.x[u][dw >> 2][dw & 3u], wf[f][oc], acc[u * G::VO * 8u + e]);
            }
        }
        return;
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
        for (u32 e = 0; e < G::VO * 8u; e++) {
            const u32 f = e / (u32)CO, oc = e % (u32)CO;
            const u32 dw = (f * (u32)CI) >> 1;
            const u32 w = CI == 2 ? t.wk[oc] : ((f & 1u) ? whi[oc] : wlo[oc]);
            acc[u * G::VO * 8u + e] = mix_dot2(t.x[u][dw >> 2][dw & 3u], w, acc[u * G::VO * 8u + e]);
        }
    }
}

template <int CI, int CO, bool NT, bool FULL, bool WIDE>
__device__ __forceinline__ void busr_fast_tile(const BusRampArgs &ra, u32 b, u32 k, u32 F, u32 j0, u32 j1)
{
    using G = MixFast<CI, CO>;
    constexpr u32 VO = G::VO, NU = G::NU, NOUT = NU * VO * 8u;
    const BusArgs &a = ra.b;
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
    BusrSend<CI, CO> ta, tb;
    busr_fetch<CI, CO, NT>(ra, j0, k, f0, ta);
    for (u32 j = j0; j < j1; j += 2) {
        if (j + 1u < j1)
            busr_fetch<CI, CO, NT>(ra, j + 1u, k, f0, tb);
        __builtin_amdgcn_sched_barrier(0);
        busr_consume<CI, CO, WIDE>(ta, f0, acc, tot);
        if (j + 1u >= j1)
            break;
        if (j + 2u < j1)
            busr_fetch<CI, CO, NT>(ra, j + 2u, k, f0, ta);
        __builtin_amdgcn_sched_barrier(0);
        busr_consume<CI, CO, WIDE>(tb, f0, acc, tot);
    }

    // ---- the tail and the stores (k_bus_fast's)
    int16_t *outs = a.out + (u64)b * a.out_stride;
    const u32 ns_out = F * (u32)CO, nfull_out = ns_out >> 3, ntail_out = ns_out & 7u;
    const u32 n0 = k * 64u * NU;
    u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
    // (called once or twice per unit, not from a loop over i: a store promoted out of a loop of one iteration would be
    // an ordinary store, not "nt" -- DESIGN 4.8)
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
                    r[h] = busr_sat16((tot[e] + acc[e] + 8192) >> 14);
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

template <int CI, int CO, bool NT>
__global__ __launch_bounds__(64) void k_busr_fast(BusRampArgs ra)
{
    using G = MixFast<CI, CO>;
    const BusArgs &a = ra.b;
    const u32 b = blockIdx.x / a.chunks;             // bus
    const u32 k = blockIdx.x - b * a.chunks;         // tile inside the bus
    const u32 *fp = a.first + b;
    const u32 w0 = uniform(fp[0]), w1 = uniform(fp[1]);
    const u32 j0 = w0 & ~BUSR_FLAG, j1 = w1 & ~BUSR_FLAG;
    if (j0 == j1)                                    // (uniform) a bus without sends touches nothing
        return;
    u32 F = a.frames;
    if (a.nframes) {
        const u32 *bf = a.bus_frames + b;
        F = uniform(bf[0]);
    }
    const u32 f0 = k * G::TILE_FRAMES;
    if (f0 >= F)                                     // (uniform)
        return;
    const bool full = f0 + G::TILE_FRAMES <= F, wide = (w0 & BUSR_FLAG) != 0;
    if (!wide) {
        if (full)
            busr_fast_tile<CI, CO, NT, true, false>(ra, b, k, F, j0, j1);
        else
            busr_fast_tile<CI, CO, NT, false, false>(ra, b, k, F, j0, j1);
    } else {
        if (full)
            busr_fast_tile<CI, CO, NT, true, true>(ra, b, k, F, j0, j1);
        else
            busr_fast_tile<CI, CO, NT, false, true>(ra, b, k, F, j0, j1);
    }
}

// ---------------------------------------------------------------------------
// Form 2: any pair of channel counts, k_bus_any's tile and staging (k_bus.hip explains the planes and the int64
// accumulators in LDS).  Beside a send's matrix the workgroup copies W0 and W1 of a send whose ramp the tile begins
// in; the thread that owns a frame computes the frame's position once per send and every weight dword right before
// its dot.  An odd C_in's padding half is zero in W0 and in W1, so it is zero at every position.
__global__ __launch_bounds__(BUSR_BLOCK) void k_busr_any(BusRampArgs ra)
{
    extern __shared__ u32x4 busr_lds[];
    const BusArgs &a = ra.b;
    const u32 CI = a.channels_in, CO = a.channels_out, CP = mix_cp(CI), tile = a.tile_frames;
    const u32 tid = threadIdx.x;
    const u32 b = blockIdx.x / a.chunks;             // bus
    const u32 k = blockIdx.x - b * a.chunks;         // tile inside the bus
    const u32 j0 = a.first[b] & ~BUSR_FLAG, j1 = a.first[b + 1u] & ~BUSR_FLAG;
    if (j0 == j1)                                    // (uniform)
        return;
    const u32 F = a.nframes ? a.bus_frames[b] : a.frames;
    const u32 f0 = k * tile;
    if (f0 >= F)                                     // (uniform)
        return;
    const u32 nt = min(tile, F - f0);                // the tile's frames
    int16_t *outs = a.out + (u64)b * a.out_stride;
    const u32 n = CO * CP, nl = mix_wk_lds(CI, CO);

    long long *acc = reinterpret_cast<long long *>(busr_lds);
    u32 *plane = reinterpret_cast<u32 *>(acc + CO * tile);
    int16_t *plane16 = reinterpret_cast<int16_t *>(plane);
    u32 *wl = plane + CP * tile;                     // the target, W0, W1: nl dwords each
    u32 *w0l = wl + nl, *w1l = w0l + nl;
    int16_t *ot = reinterpret_cast<int16_t *>(w1l + nl);

    for (u32 f = tid; f < nt; f += BUSR_BLOCK)
        for (u32 o = 0; o < CO; o++)
            acc[f * CO + o] = 0;

    for (u32 j = j0; j < j1; j++) {
        const u32 s = a.send[j] & ~BUSR_FLAG;
        const u32 c = a.nframes ? a.nframes[s] : a.frames;
        if (c <= f0)                                 // (uniform) the send has nothing in this tile: its slot is not read
            continue;
        const u32 ntj = min(tile, c - f0);           // the send's frames in the tile (c <= F: at most nt)
        const int16_t *ins = a.in + (u64)s * a.in_stride;
        const u32 *rec = ra.ramp + (u64)j * (BUSR_HDR + 2u * n);
        const u32 inc = uniform(rec[BUSR_INC]), R = uniform(rec[BUSR_R]), done = uniform(rec[BUSR_DONE]);
        const bool ramp = done + f0 < R;             // (uniform) the tile begins inside the send's ramp
        __syncthreads();                             // the last send's planes and matrices are done with
        for (u32 i = tid; i < n; i += BUSR_BLOCK) {
            wl[i] = a.wk[(u64)j * n + i];
            if (ramp) {
                w0l[i] = rec[BUSR_HDR + i];
                w1l[i] = rec[BUSR_HDR + n + i];
            }
        }
        // ---- stage the input: vectors vb .. vb + nv - 1 of the stream (f0 * CI is a multiple of 8)
        {
            const u32 ns = c * CI, nfull = ns >> 3, ntail = ns & 7u;
            const u32 vb = (f0 * CI) >> 3, nv = (ntj * CI + 7u) >> 3;
            for (u32 w = tid; w < nv; w += BUSR_BLOCK) {
                const u32 v = vb + w;
                u32 x[4];
                busr_load_vec<false>(x, ins, v, v < nfull, v == nfull && ntail != 0, ntail);
                if ((CI & 1u) == 0) {
#pragma unroll
                    for (u32 i = 0; i < 4; i++) {
                        const u32 e = w * 4u + i;                        // dword of the tile
                        const u32 f = e / CP, kk = e - f * CP;
                        if (f < ntj)
                            plane[kk * tile + f] = x[i];
                    }
                } else {
#pragma unroll
                    for (u32 i = 0; i < 8; i++) {
                        const u32 e = w * 8u + i;                        // sample of the tile
                        const u32 f = e / CI, ch = e - f * CI;
                        if (f < ntj)
                            plane16[((ch >> 1) * tile + f) * 2u + (ch & 1u)] = (int16_t)(x[i >> 1] >> (16u * (i & 1u)));
                    }
                }
            }
        }
        __syncthreads();
        // ---- one thread per frame, all outputs of the frame, with the frame's own weights inside the ramp
        for (u32 f = tid; f < ntj; f += BUSR_BLOCK) {
            const u32 p = mixr_pos(done + f0 + f + 1u, R, inc);
            for (u32 o = 0; o < CO; o++) {
                int q = 0;
                for (u32 kk = 0; kk < CP; kk++) {
                    const u32 w = ramp ? mixr_wk(w0l[o * CP + kk], w1l[o * CP + kk], p) : wl[o * CP + kk];
                    q = mix_dot2(plane[kk * tile + f], w, q);
                }
                acc[f * CO + o] += q;
            }
        }
    }

    // ---- ONE rounding, after the sum (a thread reads the accumulators it owns: no barrier before this)
    for (u32 f = tid; f < nt; f += BUSR_BLOCK)
        for (u32 o = 0; o < CO; o++)
            ot[f * CO + o] = (int16_t)busr_sat16((acc[f * CO + o] + 8192) >> 14);
    __syncthreads();

    // ---- the output tile: whole vectors, the bus's ragged end sample by sample (f0 * CO is a multiple of 8)
    {
        const u32 ns = F * CO, nfull = ns >> 3, ntail = ns & 7u;
        const u32 vb = (f0 * CO) >> 3, nv = (nt * CO + 7u) >> 3;
        u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
        const u32x4 *otv = reinterpret_cast<const u32x4 *>(ot);
        for (u32 w = tid; w < nv; w += BUSR_BLOCK) {
            const u32 v = vb + w;
            if (v < nfull) {
                __builtin_nontemporal_store(otv[w], dst + v);
            } else if (v == nfull) {
                for (u32 i = 0; i < ntail; i++)
                    outs[(u64)v * 8 + i] = ot[w * 8u + i];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// One thread per send, so a send's record has one writer.  Behind every ramp run on the stream.
__global__ __launch_bounds__(BUSR_BLOCK) void k_busr_advance(u32 *ramp, const u32 *bus_frames, u32 frames, u32 sends,
                                                             u32 n)
{
    const u32 j = blockIdx.x * BUSR_BLOCK + threadIdx.x;
    if (j >= sends)
        return;
    u32 *rec = ramp + (u64)j * (BUSR_HDR + 2u * n);
    const u32 R = rec[BUSR_R], done = rec[BUSR_DONE];
    if (done >= R)
        return;
    const u32 c = bus_frames ? bus_frames[rec[BUSR_BUS]] : frames;       // (a send's bus has a send: its count is `frames`)
    rec[BUSR_DONE] = c >= R - done ? R : done + c;
}

// ---------------------------------------------------------------------------
// launchers

// plan_bus's plan; the any-channel-count form takes the largest power-of-two tile at which W0 and W1 fit as well (they
// can push a tile that plan_bus left near the limit over it), so its grid may be the finer one
BusPlan plan_busramp(const BusArgs &a)
{
    BusPlan p = plan_bus(a);
    if (p.grid == 0 || p.fast)
        return p;
    const u32 CI = a.channels_in, CO = a.channels_out;
    u32 tile;
    for (tile = BUSR_TILE_MAX; busr_lds_bytes(CI, CO, tile) > BUSR_LDS_LIMIT; tile >>= 1)
        ;
    const u64 tiles = ((u64)a.frames + tile - 1u) / tile;
    if (tiles * a.buses >= (1ull << 31)) {
        BusPlan refused{};
        refused.err = hipErrorInvalidValue;
        return refused;
    }
    p.tile_frames = tile;
    p.lds_bytes = busr_lds_bytes(CI, CO, tile);
    p.chunks = (u32)tiles;
    p.grid = a.buses * p.chunks;
    return p;
}

hipError_t launch_busramp(const BusRampArgs &a, hipStream_t st)
{
    const BusPlan p = plan_busramp(a.b);
    if (p.grid == 0)
        return p.err;
    BusRampArgs r = a;
    r.b.chunks = p.chunks;
    r.b.tile_frames = p.tile_frames;
    const u32 form = p.fast ? (a.b.channels_in * 2u + a.b.channels_out) * 2u + (a.b.nt_loads ? 1u : 0u) : 0u;
    switch (form) {
    case 6: hipLaunchKernelGGL((k_busr_fast<1, 1, false>), dim3(p.grid), dim3(p.block), 0, st, r); break;
    case 7: hipLaunchKernelGGL((k_busr_fast<1, 1, true>), dim3(p.grid), dim3(p.block), 0, st, r); break;
    case 8: hipLaunchKernelGGL((k_busr_fast<1, 2, false>), dim3(p.grid), dim3(p.block), 0, st, r); break;
    case 9: hipLaunchKernelGGL((k_busr_fast<1, 2, true>), dim3(p.grid), dim3(p.block), 0, st, r); break;
    case 10: hipLaunchKernelGGL((k_busr_fast<2, 1, false>), dim3(p.grid), dim3(p.block), 0, st, r); break;
    case 11: hipLaunchKernelGGL((k_busr_fast<2, 1, true>), dim3(p.grid), dim3(p.block), 0, st, r); break;
    case 12: hipLaunchKernelGGL((k_busr_fast<2, 2, false>), dim3(p.grid), dim3(p.block), 0, st, r); break;
    case 13: hipLaunchKernelGGL((k_busr_fast<2, 2, true>), dim3(p.grid), dim3(p.block), 0, st, r); break;
    default: hipLaunchKernelGGL(k_busr_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, r); break;
    }
    return hipGetLastError();
}

hipError_t launch_busramp_advance(uint32_t *ramp, const uint32_t *bus_frames, uint32_t frames, uint32_t sends,
                                  uint32_t channels_in, uint32_t channels_out, hipStream_t st)
{
    if (sends == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_busr_advance, dim3((sends + BUSR_BLOCK - 1u) / BUSR_BLOCK), dim3(BUSR_BLOCK), 0, st, ramp,
                       bus_frames, frames, sends, channels_out * mix_cp(channels_in));
    return hipGetLastError();
}

// test hook: the plan of a bus run with a ramping send whose longest stream has `frames` frames (host logic, no GPU)
extern "C" void cmhip_test_plan_busramp(uint32_t buses, uint32_t channels_in, uint32_t channels_out, uint32_t frames,
                                        BusPlan *plan)
{
    BusArgs a{};
    a.buses = buses;
    a.channels_in = channels_in;
    a.channels_out = channels_out;
    a.frames = frames;
    if (plan)
        *plan = plan_busramp(a);
}

}  // namespace cmhip
