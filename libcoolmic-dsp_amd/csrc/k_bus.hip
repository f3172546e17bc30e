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
#include "k_bus.h"

namespace cmhip {

// ---------------------------------------------------------------------------
// Form 1: mono / stereo on both sides (k_bus.h has the sends and the tile; k_mix.h explains units and vectors)
template <int CI, int CO, bool NT>
__global__ __launch_bounds__(64) void k_bus_fast(BusArgs a)
{
    using G = MixFast<CI, CO>;
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
            bus_fast_tile<CI, CO, NT, true, false, false>(a, nullptr, b, k, F, j0, j1);
        else
            bus_fast_tile<CI, CO, NT, false, false, false>(a, nullptr, b, k, F, j0, j1);
    } else {
        if (full)
            bus_fast_tile<CI, CO, NT, true, true, false>(a, nullptr, b, k, F, j0, j1);
        else
            bus_fast_tile<CI, CO, NT, false, true, false>(a, nullptr, b, k, F, j0, j1);
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
__global__ __launch_bounds__(MIX_BLOCK) void k_bus_any(BusArgs a)
{
    extern __shared__ u32x4 bus_lds[];
    const u32 CI = a.channels_in, CO = a.channels_out, CP = mix_cp(CI), tile = a.tile_frames;
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
    u32 *wl = plane + CP * tile;
    int16_t *ot = reinterpret_cast<int16_t *>(wl + mix_wk_lds(CI, CO));

    for (u32 f = tid; f < nt; f += MIX_BLOCK)
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
        for (u32 i = tid; i < CO * CP; i += MIX_BLOCK)
            wl[i] = a.wk[(u64)j * CO * CP + i];
        // ---- stage the input: vectors vb .. vb + nv - 1 of the stream (f0 * CI is a multiple of 8)
        {
            const u32 ns = c * CI, nfull = ns >> 3, ntail = ns & 7u;
            const u32 vb = (f0 * CI) >> 3, nv = (ntj * CI + 7u) >> 3;
            for (u32 w = tid; w < nv; w += MIX_BLOCK) {
                const u32 v = vb + w;
                u32 x[4];
                mix_load_vec<false>(x, ins, v, v < nfull, v == nfull && ntail != 0, ntail);
                mix_scatter_vec(plane, x, w, ntj, CI, CP, tile);
            }
        }
        __syncthreads();
        // ---- one thread per frame, all outputs of the frame
        for (u32 f = tid; f < ntj; f += MIX_BLOCK) {
            for (u32 o = 0; o < CO; o++) {
                int p = 0;
                for (u32 kk = 0; kk < CP; kk++)
                    p = mix_dot2(plane[kk * tile + f], wl[o * CP + kk], p);
                acc[f * CO + o] += p;
            }
        }
    }

    // ---- ONE rounding, after the sum (a thread reads the accumulators it owns: no barrier before this)
    for (u32 f = tid; f < nt; f += MIX_BLOCK)
        for (u32 o = 0; o < CO; o++)
            ot[f * CO + o] = (int16_t)mix_sat16((acc[f * CO + o] + 8192) >> 14);
    __syncthreads();

    // ---- the output tile: whole vectors, the bus's ragged end sample by sample (f0 * CO is a multiple of 8)
    {
        const u32 ns = F * CO, nfull = ns >> 3, ntail = ns & 7u;
        const u32 vb = (f0 * CO) >> 3, nv = (nt * CO + 7u) >> 3;
        u32x4 *dst = reinterpret_cast<u32x4 *>(outs);
        const u32x4 *otv = reinterpret_cast<const u32x4 *>(ot);
        for (u32 w = tid; w < nv; w += MIX_BLOCK) {
            const u32 v = vb + w;
            if (v < nfull) {
                __builtin_nontemporal_store(otv[w], dst + v);
            } else if (v == nfull) {
                for (u32 j = 0; j < ntail; j++)
                    outs[(u64)v * 8 + j] = ot[w * 8u + j];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// launcher

BusPlan plan_bus(const BusArgs &a)
{
    const u32 CI = a.channels_in, CO = a.channels_out;
    return mix_plan_tiles<BusPlan>(a.buses, CI, CO, a.frames, [=](u32 tile) { return bus_lds_bytes(CI, CO, tile); });
}

hipError_t launch_bus(const BusArgs &a, hipStream_t st)
{
    const BusPlan p = plan_bus(a);
    if (p.grid == 0)
        return p.err;
    BusArgs b = a;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    if (p.fast) {
        bus_fast_dispatch(a.channels_in, a.channels_out, a.nt_loads != 0, [&](auto ci, auto co, auto nt) {
            hipLaunchKernelGGL((k_bus_fast<decltype(ci)::value, decltype(co)::value, decltype(nt)::value>), dim3(p.grid),
                               dim3(p.block), 0, st, b);
        });
    } else {
        hipLaunchKernelGGL(k_bus_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
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
