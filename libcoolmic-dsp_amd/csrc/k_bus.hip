// k_bus.hip -- gfx950 (MI355X, wave64) mix-bus kernels: S input slots of C_in interleaved int16 channels are summed
// into B bus slots of C_out by a routing table of sends (bus, stream, W[C_out][C_in] in units of 2^-14); include/
// coolmic_hip.h, "mix bus", has the arithmetic to the bit:
//     p_j = sum_c W_j[o][c] * x[stream_j][f][c]    acc = sum_j p_j (int64)    y[b][f][o] = saturate((acc + 8192) >> 14)
//
//   k_bus_fast<CI, CO, NT>  CI, CO in {1, 2}: one wave per (bus, tile) walks the bus's sends; weights in SGPRs
//   k_bus_any               every other pair up to 16 -> 16: a workgroup stages every send's tile through LDS
//
// The table is what csrc/bus_route.h compiles (BusArgs::first / send / wk): sends sorted by bus, every send's matrix in
// the mixer's packed form, and the sends of a bus split into GROUPS over which an int32 accumulator chained through
// the dot instruction is exact; a group's first send carries a flag, and there the int32 goes into an int64.  A bus of
// one group starts its int32 at 8192, shifts and packs -- the mixer's tail, no 64-bit instruction.  Unlike the mixer's,
// these kernels gather: a tile reads K slots and writes one.  No state, no atomics.
#include "cmhip_device.h"

namespace cmhip {

constexpr u32 BUS_BLOCK = 256;
constexpr u32 BUS_LDS_LIMIT = 64u * 1024u;       // what a workgroup may take without raising the device's limit
constexpr u32 BUS_TILE_MAX = 1024;               // frames of a k_bus_any tile at most: four per thread
constexpr u32 BUS_FLAG = 0x80000000u;            // bit 31 of a word of first[] / send[]

__host__ __device__ constexpr u32 bus_cp(u32 ci) { return (ci + 1u) / 2u; }
// LDS of k_bus_any: the int64 accumulators of the tile, CP planes of tile dwords, one send's matrix (rounded up to
// whole 16-byte vectors), the output tile -- in this order, so that each part is aligned for its widest access
__host__ __device__ constexpr u32 bus_wk_lds(u32 ci, u32 co) { return (co * bus_cp(ci) + 3u) & ~3u; }
__host__ __device__ constexpr u32 bus_lds_bytes(u32 ci, u32 co, u32 tile)
{
    return 8u * co * tile + 4u * bus_cp(ci) * tile + 4u * bus_wk_lds(ci, co) + 2u * co * tile;
}

__device__ __forceinline__ int bus_dot2(u32 x, u32 k, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, k), acc, false);
}
__device__ __forceinline__ int bus_sat16(long long v)
{
    return (int)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
}

// load_vec (cmhip_device.h) with the load's cache policy a parameter: a stream that feeds many buses (mix-minus) is
// read again by other waves, which a non-temporal load does not favour
template <bool NT>
__device__ __forceinline__ void bus_load_vec(u32 (&x)[4], const int16_t *ins, u32 v, bool full, bool tail, u32 ntail)
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
// Form 1: mono / stereo on both sides.  The unit and tile geometry is k_mix_fast's (MixFast, csrc/k_mix.hip): a lane
// works in units of UF frames, the fewest that are whole 16-byte vectors on both sides, and NU units make four vectors
// on the wider side; unit j of a lane is unit n0 + 64 j + lane of the slot.
template <int CI, int CO>
struct BusFast {
    static constexpr u32 UF = 8u / (u32)(CI < CO ? CI : CO);
    static constexpr u32 VI = UF * (u32)CI / 8u, VO = UF * (u32)CO / 8u;
    static constexpr u32 NU = 4u / (VI > VO ? VI : VO);
    static constexpr u32 TILE_FRAMES = 64u * NU * UF;
    static constexpr u32 NOUT = NU * VO * 8u;        // output samples of a lane
};

// one send of the tile in flight: its vectors, its weight dwords, its flag
template <int CI, int CO>
struct BusSend {
    u32 x[BusFast<CI, CO>::NU][BusFast<CI, CO>::VI][4];
    u32 wk[2];
    u32 start;                                       // the send starts a group
    u32 live;                                        // its stream reaches into this tile
};

// Everything of send j is wave-uniform and read as scalars at FIXED offsets from addresses computed in full -- no
// scalar load with a register and an immediate offset (tests/test_abi.py tells why).  A send whose stream ends at or
// before the tile's first frame is skipped: nothing of its slot is read.  The vectors zero-fill past the SEND's own
// count, which may be below the bus's.
template <int CI, int CO, bool NT>
__device__ __forceinline__ void bus_fetch(const BusArgs &a, u32 j, u32 k, u32 f0, BusSend<CI, CO> &t)
{
    using G = BusFast<CI, CO>;
    constexpr u32 VI = G::VI, NU = G::NU, NW = (u32)CO;      // CP == 1: one dword per output channel
    const u32 lane = threadIdx.x & 63u;
    const u32 *sp = a.send + j;
    const u32 word = uniform(sp[0]);
    const u32 s = word & ~BUS_FLAG;
    t.start = word >> 31;
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
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    const u32 ns = c * (u32)CI, nfull = ns >> 3, ntail = ns & 7u;
    const u32 n0 = k * 64u * NU;
    if (f0 + G::TILE_FRAMES <= c) {                  // (uniform) the send covers the tile
#pragma unroll
        for (u32 u = 0; u < NU; u++)
#pragma unroll
            for (u32 i = 0; i < VI; i++)
                bus_load_vec<NT>(t.x[u][i], ins, (n0 + 64u * u + lane) * VI + i, true, false, 0);
    } else {
#pragma unroll
        for (u32 u = 0; u < NU; u++)
#pragma unroll
            for (u32 i = 0; i < VI; i++) {
                const u32 v = (n0 + 64u * u + lane) * VI + i;
                bus_load_vec<NT>(t.x[u][i], ins, v, v < nfull, ntail && v == nfull, ntail);
            }
    }
}

// One dot instruction per output sample and send, on the input dword that holds the frame (k_mix_fast's scheme: with
// mono input the weight sits in the half of the dword its frame is in), chained in int32 inside a group.  At a group's
// first send the int32 accumulators are added into the int64 ones (WIDE; a bus of one group has none).
template <int CI, int CO, bool WIDE>
__device__ __forceinline__ void bus_consume(const BusSend<CI, CO> &t, int (&acc)[BusFast<CI, CO>::NOUT],
                                            long long (&tot)[WIDE ? BusFast<CI, CO>::NOUT : 1u])
{
    using G = BusFast<CI, CO>;
    if constexpr (WIDE) {
        if (t.start) {                               // (uniform)
#pragma unroll
            for (u32 e = 0; e < G::NOUT; e++) {
                tot[e] += acc[e];
                acc[e] = 0;
            }
        }
    }
    if (!t.live)                                     // (uniform)
        return;
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
            acc[u * G::VO * 8u + e] = bus_dot2(t.x[u][dw >> 2][dw & 3u], w, acc[u * G::VO * 8u + e]);
        }
    }
}

template <int CI, int CO, bool NT, bool FULL, bool WIDE>
__device__ __forceinline__ void bus_fast_tile(const BusArgs &a, u32 b, u32 k, u32 F, u32 j0, u32 j1)
{
    using G = BusFast<CI, CO>;
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
    BusSend<CI, CO> ta, tb;
    bus_fetch<CI, CO, NT>(a, j0, k, f0, ta);
    for (u32 j = j0; j < j1; j += 2) {
        if (j + 1u < j1)
            bus_fetch<CI, CO, NT>(a, j + 1u, k, f0, tb);
        __builtin_amdgcn_sched_barrier(0);
        bus_consume<CI, CO, WIDE>(ta, acc, tot);
        if (j + 1u >= j1)
            break;
        if (j + 2u < j1)
            bus_fetch<CI, CO, NT>(a, j + 2u, k, f0, ta);
        __builtin_amdgcn_sched_barrier(0);
        bus_consume<CI, CO, WIDE>(tb, acc, tot);
    }

    // ---- the tail and the stores
    int16_t *outs = a.out + (u64)b * a.out_stride;
    const u32 ns_out = F * (u32)CO, nfull_out = ns_out >> 3, ntail_out = ns_out & 7u;
    const u32 n0 = k * 64u * NU;
    u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
    // (output vector i of unit u.  Called once or twice per unit, not from a loop over i: the optimiser promotes a
    // store out of a loop of one iteration and the copy it makes is an ordinary store, not "nt" -- DESIGN 4.8)
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
                    r[h] = bus_sat16((tot[e] + acc[e] + 8192) >> 14);
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
__global__ __launch_bounds__(64) void k_bus_fast(BusArgs a)
{
    using G = BusFast<CI, CO>;
    const u32 b = blockIdx.x / a.chunks;             // bus
    const u32 k = blockIdx.x - b * a.chunks;         // tile inside the bus
    const u32 *fp = a.first + b;
    const u32 w0 = uniform(fp[0]), w1 = uniform(fp[1]);
    const u32 j0 = w0 & ~BUS_FLAG, j1 = w1 & ~BUS_FLAG;
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
    const bool full = f0 + G::TILE_FRAMES <= F, wide = (w0 & BUS_FLAG) != 0;
    if (!wide) {
        if (full)
            bus_fast_tile<CI, CO, NT, true, false>(a, b, k, F, j0, j1);
        else
            bus_fast_tile<CI, CO, NT, false, false>(a, b, k, F, j0, j1);
    } else {
        if (full)
            bus_fast_tile<CI, CO, NT, true, true>(a, b, k, F, j0, j1);
        else
            bus_fast_tile<CI, CO, NT, false, true>(a, b, k, F, j0, j1);
    }
}

// ---------------------------------------------------------------------------
// Form 2: any pair of channel counts.  A workgroup of 256 threads takes one bus and a tile of tile_frames frames (a
// multiple of 8: tile edges are 16-byte edges on both sides for every channel count).  Thread t owns frames t, t + 256,
// ... of the tile and their C_out int64 accumulators, which live in LDS.  Per send, as k_mix_any does per run:
//   1. the send's matrix and the tile's interleaved input -- as far as the SEND's stream reaches -- are staged, the
//      input in 16-byte vectors scattered into CP planes of dwords, plane[k][f] = x[f][2k] | x[f][2k+1] << 16 (an odd
//      C_in by halves; the unused half of the last plane is never written: it meets a zero weight);
//   2. a thread computes the send's C_out int32 sums of its frames (exact: the mixer's bound holds per send) and adds
//      each into its int64.  Frames past the send's count are left alone: silence.
// Then (acc + 8192) >> 14, clamped, goes into an interleaved output tile that leaves as whole 16-byte vectors, the
// bus's ragged end sample by sample.  (The group flags are not needed here.)
__global__ __launch_bounds__(BUS_BLOCK) void k_bus_any(BusArgs a)
{
    extern __shared__ u32x4 bus_lds[];
    const u32 CI = a.channels_in, CO = a.channels_out, CP = bus_cp(CI), tile = a.tile_frames;
    const u32 tid = threadIdx.x;
    const u32 b = blockIdx.x / a.chunks;             // bus
    const u32 k = blockIdx.x - b * a.chunks;         // tile inside the bus
    const u32 j0 = a.first[b] & ~BUS_FLAG, j1 = a.first[b + 1u] & ~BUS_FLAG;
    if (j0 == j1)                                    // (uniform)
        return;
    const u32 F = a.nframes ? a.bus_frames[b] : a.frames;
    const u32 f0 = k * tile;
    if (f0 >= F)                                     // (uniform)
        return;
    const u32 nt = min(tile, F - f0);                // the tile's frames
    int16_t *outs = a.out + (u64)b * a.out_stride;

    long long *acc = reinterpret_cast<long long *>(bus_lds);
    u32 *plane = reinterpret_cast<u32 *>(acc + CO * tile);
    int16_t *plane16 = reinterpret_cast<int16_t *>(plane);
    u32 *wl = plane + CP * tile;
    int16_t *ot = reinterpret_cast<int16_t *>(wl + bus_wk_lds(CI, CO));

    for (u32 f = tid; f < nt; f += BUS_BLOCK)
        for (u32 o = 0; o < CO; o++)
            acc[f * CO + o] = 0;

    for (u32 j = j0; j < j1; j++) {
        const u32 s = a.send[j] & ~BUS_FLAG;
        const u32 c = a.nframes ? a.nframes[s] : a.frames;
        if (c <= f0)                                 // (uniform) the send has nothing in this tile: its slot is not read
            continue;
        const u32 ntj = min(tile, c - f0);           // the send's frames in the tile (c <= F: at most nt)
        const int16_t *ins = a.in + (u64)s * a.in_stride;
        __syncthreads();                             // the last send's planes and matrix are done with
        for (u32 i = tid; i < CO * CP; i += BUS_BLOCK)
            wl[i] = a.wk[(u64)j * CO * CP + i];
        // ---- stage the input: vectors vb .. vb + nv - 1 of the stream (f0 * CI is a multiple of 8)
        {
            const u32 ns = c * CI, nfull = ns >> 3, ntail = ns & 7u;
            const u32 vb = (f0 * CI) >> 3, nv = (ntj * CI + 7u) >> 3;
            for (u32 w = tid; w < nv; w += BUS_BLOCK) {
                const u32 v = vb + w;
                u32 x[4];
                bus_load_vec<false>(x, ins, v, v < nfull, v == nfull && ntail != 0, ntail);
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
        // ---- one thread per frame, all outputs of the frame
        for (u32 f = tid; f < ntj; f += BUS_BLOCK) {
            for (u32 o = 0; o < CO; o++) {
                int p = 0;
                for (u32 kk = 0; kk < CP; kk++)
                    p = bus_dot2(plane[kk * tile + f], wl[o * CP + kk], p);
                acc[f * CO + o] += p;
            }
        }
    }

    // ---- ONE rounding, after the sum (a thread reads the accumulators it owns: no barrier before this)
    for (u32 f = tid; f < nt; f += BUS_BLOCK)
        for (u32 o = 0; o < CO; o++)
            ot[f * CO + o] = (int16_t)bus_sat16((acc[f * CO + o] + 8192) >> 14);
    __syncthreads();

    // ---- the output tile: whole vectors, the bus's ragged end sample by sample (f0 * CO is a multiple of 8)
    {
        const u32 ns = F * CO, nfull = ns >> 3, ntail = ns & 7u;
        const u32 vb = (f0 * CO) >> 3, nv = (nt * CO + 7u) >> 3;
        u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
        const u32x4 *otv = reinterpret_cast<const u32x4 *>(ot);
        for (u32 w = tid; w < nv; w += BUS_BLOCK) {
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
// launcher

BusPlan plan_bus(const BusArgs &a)
{
    BusPlan p{};
    p.err = hipSuccess;
    const u32 CI = a.channels_in, CO = a.channels_out;
    if (a.buses == 0 || a.frames == 0 || CI == 0 || CI > MAX_CH || CO == 0 || CO > MAX_CH)
        return p;
    BusPlan refused{};
    refused.err = hipErrorInvalidValue;
    u32 tile, lds = 0;
    const bool fast = CI <= 2 && CO <= 2;
    if (fast) {
        tile = CI == 1 && CO == 1 ? BusFast<1, 1>::TILE_FRAMES : BusFast<2, 2>::TILE_FRAMES;     // (2048 : 1024)
    } else {
        // the largest power-of-two tile whose accumulators, planes and output fit beside a matrix
        for (tile = BUS_TILE_MAX; bus_lds_bytes(CI, CO, tile) > BUS_LDS_LIMIT; tile >>= 1)
            ;
        lds = bus_lds_bytes(CI, CO, tile);
    }
    const u64 tiles = ((u64)a.frames + tile - 1u) / tile;
    if (tiles * a.buses >= (1ull << 31))                     // (as plan_mix: no grid of 2^31 workgroups)
        return refused;
    p.fast = fast ? 1u : 0u;
    p.block = fast ? 64u : BUS_BLOCK;
    p.tile_frames = tile;
    p.lds_bytes = lds;
    p.chunks = (u32)tiles;
    p.grid = a.buses * p.chunks;
    return p;
}

hipError_t launch_bus(const BusArgs &a, hipStream_t st)
{
    const BusPlan p = plan_bus(a);
    if (p.grid == 0)
        return p.err;
    BusArgs b = a;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    const u32 form = p.fast ? (a.channels_in * 2u + a.channels_out) * 2u + (a.nt_loads ? 1u : 0u) : 0u;
    switch (form) {
    case 6: hipLaunchKernelGGL((k_bus_fast<1, 1, false>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 7: hipLaunchKernelGGL((k_bus_fast<1, 1, true>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 8: hipLaunchKernelGGL((k_bus_fast<1, 2, false>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 9: hipLaunchKernelGGL((k_bus_fast<1, 2, true>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 10: hipLaunchKernelGGL((k_bus_fast<2, 1, false>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 11: hipLaunchKernelGGL((k_bus_fast<2, 1, true>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 12: hipLaunchKernelGGL((k_bus_fast<2, 2, false>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 13: hipLaunchKernelGGL((k_bus_fast<2, 2, true>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    default: hipLaunchKernelGGL(k_bus_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    }
    return hipGetLastError();
}

// test hook: the plan of a bus run whose longest stream has `frames` frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_bus(uint32_t buses, uint32_t channels_in, uint32_t channels_out, uint32_t frames,
                                    BusPlan *plan)
{
    BusArgs a{};
    a.buses = buses;
    a.channels_in = channels_in;
    a.channels_out = channels_out;
    a.frames = frames;
    if (plan)
        *plan = plan_bus(a);
}

}  // namespace cmhip
