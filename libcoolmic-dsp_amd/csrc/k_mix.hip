// k_mix.hip -- gfx950 (MI355X, wave64) channel-mixing kernels: S streams of C_in interleaved int16 channels become
// S streams of C_out, frame by frame, by a matrix W[C_out][C_in] per stream in units of 2^-14 (include/coolmic_hip.h,
// "channel mixing", has the arithmetic to the bit):
//     acc = sum_{c<C_in} W[o][c] * x[f][c]      y[f][o] = saturate((acc + 8192) >> 14)
//
//   k_mix_fast<CI, CO>  CI, CO in {1, 2}: one short-lived wave per contiguous tile of one stream, the matrix in SGPRs
//   k_mix_any           every other pair up to 16 -> 16: a workgroup stages a tile through LDS; no speed goal
//   k_mix_set           writes one matrix, handed over as a kernel argument, into the rows of a range of streams
//
// The kernel form of a matrix (MixArgs::wk): per stream [C_out][CP] dwords, CP = ceil(C_in / 2), dword k of row o is
// W[o][2k] | W[o][2k+1] << 16 (an odd C_in padded with a zero weight) -- the order v_dot2_i32_i16 meets the two
// channels of an input dword in.  The accumulator starts at 8192, so rounding costs no instruction; then one shift,
// and v_cvt_pk_i16_i32 clamps and packs two results.  No state: nothing is carried between runs.
#include "k_mix.h"

namespace cmhip {

// ---------------------------------------------------------------------------
// Form 1: mono / stereo on both sides (k_mix.h has the units and the tile)
template <int CI, int CO>
__global__ __launch_bounds__(64) void k_mix_fast(MixArgs a)
{
    using G = MixFast<CI, CO>;
    // every kernel argument the tile's loads need is read here, with the first batch of scalar loads (k_run_fast)
    const int16_t *a_in = a.in;
    int16_t *a_out = a.out;
    const u64 in_stride = a.in_stride, out_stride = a.out_stride;
    const u32 a_frames = a.frames;
    const u32 s = blockIdx.x / a.chunks;             // stream
    const u32 k = blockIdx.x - s * a.chunks;         // tile inside the stream
    const u32 F = a.nframes ? a.nframes[s] : a_frames;
    const u32 f0 = k * G::TILE_FRAMES;
    if (f0 >= F)                                     // (uniform)
        return;
    if (f0 + G::TILE_FRAMES <= F)
        mixr_fast_tile<CI, CO, true, false>(a, nullptr, 0, 0, s, k, F, a_in, a_out, in_stride, out_stride);
    else
        mixr_fast_tile<CI, CO, false, false>(a, nullptr, 0, 0, s, k, F, a_in, a_out, in_stride, out_stride);
}

// ---------------------------------------------------------------------------
// Form 2: any pair of channel counts.  A workgroup of 256 threads takes one stream and a tile of tile_frames frames
// (a multiple of 8: tile edges are 16-byte edges on both sides for every channel count).
//   1. the tile's interleaved input is loaded in 16-byte vectors and scattered into CP planes of dwords,
//      plane[k][f] = x[f][2k] | x[f][2k+1] << 16: for an even C_in every loaded dword is such a pair, for an odd one
//      the samples go in by halves (the unused half of the last plane is never written: it meets a zero weight, and
//      in integers anything times zero is zero);
//   2. a thread computes all C_out samples of its frames: lanes with consecutive frames read consecutive dwords of a
//      plane (conflict-free, and exactly the operand of the dot instruction), the matrix is read from LDS at a
//      wave-uniform address (a broadcast);
//   3. the results go into an interleaved output tile in LDS and leave as whole 16-byte vectors, the ragged end of
//      the stream sample by sample.
__global__ __launch_bounds__(MIX_BLOCK) void k_mix_any(MixArgs a)
{
    extern __shared__ u32x4 mix_lds[];
    const u32 CI = a.channels_in, CO = a.channels_out, CP = mix_cp(CI), tile = a.tile_frames;
    const u32 tid = threadIdx.x;
    const u32 s = blockIdx.x / a.chunks;             // stream
    const u32 k = blockIdx.x - s * a.chunks;         // tile inside the stream
    const u32 F = a.nframes ? a.nframes[s] : a.frames;
    const u32 f0 = k * tile;
    if (f0 >= F)                                     // (uniform)
        return;
    const u32 nt = min(tile, F - f0);                // the tile's frames
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    int16_t *outs = a.out + (u64)s * a.out_stride;

    u32 *wl = reinterpret_cast<u32 *>(mix_lds);
    u32 *plane = wl + mix_wk_lds(CI, CO);
    int16_t *ot = reinterpret_cast<int16_t *>(plane + CP * tile);

    for (u32 i = tid; i < CO * CP; i += MIX_BLOCK)
        wl[i] = a.wk[(u64)s * CO * CP + i];

    // ---- stage the input: vectors vb .. vb + nv - 1 of the stream (f0 * CI is a multiple of 8)
    {
        const u32 ns = F * CI, nfull = ns >> 3, ntail = ns & 7u;
        const u32 vb = (f0 * CI) >> 3, nv = (nt * CI + 7u) >> 3;
        for (u32 w = tid; w < nv; w += MIX_BLOCK) {
            const u32 v = vb + w;
            u32 x[4];
            load_vec(x, ins, v, v < nfull, v == nfull && ntail != 0, ntail);
            mix_scatter_vec(plane, x, w, nt, CI, CP, tile);
        }
    }
    __syncthreads();

    // ---- one thread per frame, all outputs of the frame
    for (u32 f = tid; f < nt; f += MIX_BLOCK) {
        for (u32 o = 0; o < CO; o++) {
            int acc = 8192;
            for (u32 kk = 0; kk < CP; kk++)
                acc = mix_dot2(plane[kk * tile + f], wl[o * CP + kk], acc);
            ot[f * CO + o] = (int16_t)min(max(acc >> 14, -32768), 32767);
        }
    }
    __syncthreads();

    // ---- the output tile: whole vectors, the stream's ragged end sample by sample (f0 * CO is a multiple of 8)
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

// one matrix in the kernel form (at most 16 x 8 dwords, a kernel argument: it travels with the launch, so nothing
// the host owns is read later) into the rows of streams first .. first + count - 1
struct MixSetArgs {
    u32 *wk;
    u32 first, count, n;                             // n = C_out * CP dwords per stream
    u32 w[MAX_CH * (MAX_CH / 2u)];
};
__global__ __launch_bounds__(MIX_BLOCK) void k_mix_set(MixSetArgs a)
{
    const u64 i = (u64)blockIdx.x * MIX_BLOCK + threadIdx.x;
    if (i >= (u64)a.count * a.n)
        return;
    const u32 e = (u32)(i % a.n);
    u32 val = 0;
    for (u32 j = 0; j < MAX_CH * (MAX_CH / 2u); j++)     // (selects: the argument stays in SGPRs)
        if (j == e)
            val = a.w[j];
    a.wk[(u64)a.first * a.n + i] = val;
}

// ---------------------------------------------------------------------------
// launcher

MixPlan plan_mix(const MixArgs &a)
{
    const u32 CI = a.channels_in, CO = a.channels_out;
    return mix_plan_tiles<MixPlan>(a.streams, CI, CO, a.frames, [=](u32 tile) { return mix_lds_bytes(CI, CO, tile); });
}

hipError_t launch_mix(const MixArgs &a, hipStream_t st)
{
    const MixPlan p = plan_mix(a);
    if (p.grid == 0)
        return p.err;
    MixArgs b = a;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    const u32 form = p.fast ? a.channels_in * 2u + a.channels_out : 0u;
    switch (form) {
    case 3: hipLaunchKernelGGL((k_mix_fast<1, 1>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 4: hipLaunchKernelGGL((k_mix_fast<1, 2>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 5: hipLaunchKernelGGL((k_mix_fast<2, 1>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 6: hipLaunchKernelGGL((k_mix_fast<2, 2>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    default: hipLaunchKernelGGL(k_mix_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b); break;
    }
    return hipGetLastError();
}

hipError_t launch_mix_set(uint32_t *wk, uint32_t first, uint32_t count, uint32_t channels_in, uint32_t channels_out,
                          const int16_t *W, hipStream_t st)
{
    MixSetArgs a{};
    const u32 CP = mix_cp(channels_in);
    a.wk = wk;
    a.first = first;
    a.count = count;
    a.n = channels_out * CP;
    for (u32 o = 0; o < channels_out; o++)
        for (u32 c = 0; c < channels_in; c++)
            a.w[o * CP + (c >> 1)] |= (u32)(uint16_t)W[o * channels_in + c] << (16u * (c & 1u));
    const u64 total = (u64)count * a.n;
    if (total == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_mix_set, dim3((u32)((total + MIX_BLOCK - 1u) / MIX_BLOCK)), dim3(MIX_BLOCK), 0, st, a);
    return hipGetLastError();
}

// test hook: the plan of a mixer run whose longest stream has `frames` frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_mix(uint32_t streams, uint32_t channels_in, uint32_t channels_out, uint32_t frames,
                                    MixPlan *plan)
{
    MixArgs a{};
    a.streams = streams;
    a.channels_in = channels_in;
    a.channels_out = channels_out;
    a.frames = frames;
    if (plan)
        *plan = plan_mix(a);
}

}  // namespace cmhip
