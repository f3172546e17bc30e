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
// kernels run only while some send ramps; at every other time the bus launches k_bus.hip's.  What the two files have
// in common -- the sends, the tile, the tail -- is k_bus.h's.
#include "k_bus.h"

namespace cmhip {

// ---------------------------------------------------------------------------
// Form 1: k_bus_fast's tile (k_bus.h), with the ramp's path for a send whose ramp the tile begins in
template <int CI, int CO, bool NT>
__global__ __launch_bounds__(64) void k_busr_fast(BusRampArgs ra)
{
    using G = MixFast<CI, CO>;
    const BusArgs &a = ra.b;
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
            bus_fast_tile<CI, CO, NT, true, false, true>(a, ra.ramp, b, k, F, j0, j1);
        else
            bus_fast_tile<CI, CO, NT, false, false, true>(a, ra.ramp, b, k, F, j0, j1);
    } else {
        if (full)
            bus_fast_tile<CI, CO, NT, true, true, true>(a, ra.ramp, b, k, F, j0, j1);
        else
            bus_fast_tile<CI, CO, NT, false, true, true>(a, ra.ramp, b, k, F, j0, j1);
    }
}

// ---------------------------------------------------------------------------
// Form 2: any pair of channel counts, k_bus_any's tile and staging (k_bus.hip explains the planes and the int64
// accumulators in LDS).  Beside a send's matrix the workgroup copies W0 and W1 of a send whose ramp the tile begins
// in; the thread that owns a frame computes the frame's position once per send and every weight dword right before
// its dot.  An odd C_in's padding half is zero in W0 and in W1, so it is zero at every position.
__global__ __launch_bounds__(MIX_BLOCK) void k_busr_any(BusRampArgs ra)
{
    extern __shared__ u32x4 busr_lds[];
    const BusArgs &a = ra.b;
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
    const u32 n = CO * CP, nl = mix_wk_lds(CI, CO);

    long long *acc = reinterpret_cast<long long *>(busr_lds);
    u32 *plane = reinterpret_cast<u32 *>(acc + CO * tile);
    u32 *wl = plane + CP * tile;                     // the target, W0, W1: nl dwords each
    u32 *w0l = wl + nl, *w1l = w0l + nl;
    int16_t *ot = reinterpret_cast<int16_t *>(w1l + nl);

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
        const u32 *rec = ra.ramp + (u64)j * (BUSR_HDR + 2u * n);
        const u32 inc = uniform(rec[BUSR_INC]), R = uniform(rec[BUSR_R]), done = uniform(rec[BUSR_DONE]);
        const bool ramp = done + f0 < R;             // (uniform) the tile begins inside the send's ramp
        __syncthreads();                             // the last send's planes and matrices are done with
        for (u32 i = tid; i < n; i += MIX_BLOCK) {
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
            for (u32 w = tid; w < nv; w += MIX_BLOCK) {
                const u32 v = vb + w;
                u32 x[4];
                mix_load_vec<false>(x, ins, v, v < nfull, v == nfull && ntail != 0, ntail);
                mix_scatter_vec(plane, x, w, ntj, CI, CP, tile);
            }
        }
        __syncthreads();
        // ---- one thread per frame, all outputs of the frame, with the frame's own weights inside the ramp
        for (u32 f = tid; f < ntj; f += MIX_BLOCK) {
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
// One thread per send, so a send's record has one writer.  Behind every ramp run on the stream.
__global__ __launch_bounds__(MIX_BLOCK) void k_busr_advance(u32 *ramp, const u32 *bus_frames, u32 frames, u32 sends,
                                                             u32 n)
{
    const u32 j = blockIdx.x * MIX_BLOCK + threadIdx.x;
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

// plan_bus's plan with W0 and W1 counted in the any-channel-count form's LDS (they can push a tile that plan_bus left
// near the limit over it), so its grid may be the finer one
BusPlan plan_busramp(const BusArgs &a)
{
    const u32 CI = a.channels_in, CO = a.channels_out;
    return mix_plan_tiles<BusPlan>(a.buses, CI, CO, a.frames, [=](u32 tile) { return busr_lds_bytes(CI, CO, tile); });
}

hipError_t launch_busramp(const BusRampArgs &a, hipStream_t st)
{
    const BusPlan p = plan_busramp(a.b);
    if (p.grid == 0)
        return p.err;
    BusRampArgs r = a;
    r.b.chunks = p.chunks;
    r.b.tile_frames = p.tile_frames;
    if (p.fast) {
        bus_fast_dispatch(a.b.channels_in, a.b.channels_out, a.b.nt_loads != 0, [&](auto ci, auto co, auto nt) {
            hipLaunchKernelGGL((k_busr_fast<decltype(ci)::value, decltype(co)::value, decltype(nt)::value>), dim3(p.grid),
                               dim3(p.block), 0, st, r);
        });
    } else {
        hipLaunchKernelGGL(k_busr_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, r);
    }
    return hipGetLastError();
}

hipError_t launch_busramp_advance(uint32_t *ramp, const uint32_t *bus_frames, uint32_t frames, uint32_t sends,
                                  uint32_t channels_in, uint32_t channels_out, hipStream_t st)
{
    if (sends == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_busr_advance, dim3((sends + MIX_BLOCK - 1u) / MIX_BLOCK), dim3(MIX_BLOCK), 0, st, ramp,
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
