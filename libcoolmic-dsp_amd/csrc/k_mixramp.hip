// k_mixramp.hip -- gfx950 (MI355X, wave64) kernels of the mixer's matrix ramps: a stream's matrix moves from W0 to W1
// over R of its frames, every frame with a matrix of its own, in exact integers (include/coolmic_hip.h, "matrix
// ramps", has the arithmetic to the bit; csrc/mix_ramp.h is the same on the host):
//     p(n) = min(32768, (min(n, R) * inc) >> 17)     N = w0 * (32768 - p) + w1 * p     w = N / 32768 towards zero
//     acc  = sum_c w[o][c] * x[f][c]                 y = saturate((acc + 8192) >> 14)   (k_mix.hip's tail)
//
//   k_mixr_fast<CI, CO>  CI, CO in {1, 2}: MixFast's tile, one wave per tile; the weights of a frame are made in VGPRs
//   k_mixr_any           every other pair up to 16 -> 16, staged through LDS as k_mix_any; no speed goal
//   k_mixr_start         starts or retargets the ramps of a range of streams, each from its own matrix in force
//   k_mixr_advance       moves every stream's position on by its count of the run before
//   k_mixr_cancel        ends the ramps of a range of streams (cmhip_mix_set_matrix steps)
//
// Per stream a record (MixRampArgs::ramp): inc, R, done, 0, W0[n], W1[n], the matrices in the kernel's form.  The
// stream ramps while done < R, and frame f of a run is the ramp's frame n = done + f + 1.  A tile whose first frame
// lies behind the ramp (done + f0 >= R, a stream that does not ramp included) is a uniform condition: it takes
// k_mix.hip's path with the target's dwords from MixArgs::wk, which k_mixr_start wrote too.  These kernels run only
// while some stream ramps; at every other time the mixer launches k_mix.hip's.
#include "k_mix.h"

namespace cmhip {

// ---------------------------------------------------------------------------
// Form 1: k_mix_fast's tile (k_mix.h), with the ramp's path where the tile begins inside the ramp
template <int CI, int CO>
__global__ __launch_bounds__(64) void k_mixr_fast(MixRampArgs ra)
{
    using G = MixFast<CI, CO>;
    const MixArgs &a = ra.m;
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
    const u32 *rec = ra.ramp + (u64)s * (MIXR_HDR + 2u * (u32)CO);
    const u32 R = uniform(rec[MIXR_R]), done = uniform(rec[MIXR_DONE]);
    const bool full = f0 + G::TILE_FRAMES <= F;
    if (done + f0 < R) {                             // (uniform) the tile begins inside the ramp
        if (full)
            mixr_fast_tile<CI, CO, true, true>(a, rec, R, done, s, k, F, a_in, a_out, in_stride, out_stride);
        else
            mixr_fast_tile<CI, CO, false, true>(a, rec, R, done, s, k, F, a_in, a_out, in_stride, out_stride);
    } else {
        if (full)
            mixr_fast_tile<CI, CO, true, false>(a, rec, R, done, s, k, F, a_in, a_out, in_stride, out_stride);
        else
            mixr_fast_tile<CI, CO, false, false>(a, rec, R, done, s, k, F, a_in, a_out, in_stride, out_stride);
    }
}

// ---------------------------------------------------------------------------
// Form 2: k_mix_any's tile and staging (k_mix.hip explains the planes).  Beside the target's matrix the workgroup
// copies W0 and W1 into LDS (mixr_lds_bytes, k_mix.h); the thread that owns a frame computes the frame's position once
// and every weight dword right before its dot.  An odd C_in's padding half is zero in W0 and in W1, so it is zero at
// every position.
__global__ __launch_bounds__(MIX_BLOCK) void k_mixr_any(MixRampArgs ra)
{
    extern __shared__ u32x4 mixr_lds[];
    const MixArgs &a = ra.m;
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
    const u32 n = CO * CP, nl = mix_wk_lds(CI, CO);
    const u32 *rec = ra.ramp + (u64)s * (MIXR_HDR + 2u * n);
    const u32 inc = uniform(rec[MIXR_INC]), R = uniform(rec[MIXR_R]), done = uniform(rec[MIXR_DONE]);
    const bool ramp = done + f0 < R;                 // (uniform) the tile begins inside the ramp

    u32 *wl = reinterpret_cast<u32 *>(mixr_lds);     // the target, W0, W1: nl dwords each
    u32 *w0l = wl + nl, *w1l = w0l + nl;
    u32 *plane = w1l + nl;
    int16_t *ot = reinterpret_cast<int16_t *>(plane + CP * tile);

    for (u32 i = tid; i < n; i += MIX_BLOCK) {
        wl[i] = a.wk[(u64)s * n + i];
        if (ramp) {
            w0l[i] = rec[MIXR_HDR + i];
            w1l[i] = rec[MIXR_HDR + n + i];
        }
    }

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

    // ---- one thread per frame, all outputs of the frame, with the frame's own weights inside the ramp
    for (u32 f = tid; f < nt; f += MIX_BLOCK) {
        const u32 p = mixr_pos(done + f0 + f + 1u, R, inc);
        for (u32 o = 0; o < CO; o++) {
            int acc = 8192;
            for (u32 kk = 0; kk < CP; kk++) {
                const u32 w = ramp ? mixr_wk(w0l[o * CP + kk], w1l[o * CP + kk], p) : wl[o * CP + kk];
                acc = mix_dot2(plane[kk * tile + f], w, acc);
            }
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

// ---------------------------------------------------------------------------
// The small kernels: one thread per stream, so a stream's record has one writer.

constexpr u32 MIXR_NMAX = MAX_CH * (MAX_CH / 2u);    // dwords of a matrix in the kernel's form at most

// the target in the kernel's form travels as a kernel argument (k_mix_set): nothing the host owns is read later
struct MixRampStartArgs {
    u32 *ramp, *wk;
    u32 first, count, n;                             // n = C_out * CP dwords per matrix
    u32 R, inc;
    u32 w[MIXR_NMAX];
};
__global__ __launch_bounds__(MIX_BLOCK) void k_mixr_start(MixRampStartArgs a)
{
    const u32 i = blockIdx.x * MIX_BLOCK + threadIdx.x;
    if (i >= a.count)
        return;
    const u32 s = a.first + i;
    u32 *rec = a.ramp + (u64)s * (MIXR_HDR + 2u * a.n);
    u32 *wks = a.wk + (u64)s * a.n;
    const u32 R = rec[MIXR_R], done = rec[MIXR_DONE];
    const bool ramping = done < R;
    const u32 p = mixr_pos(done, R, rec[MIXR_INC]);  // (done = 0: p = 0, W0 itself)
    // the matrix in force becomes W0: w(p(done)) of the running ramp, the stream's plain matrix otherwise.  (Unrolled
    // with constant e: the argument stays in SGPRs and is read at fixed offsets.)
#pragma unroll
    for (u32 e = 0; e < MIXR_NMAX; e++) {
        if (e < a.n) {
            const u32 cur = ramping ? mixr_wk(rec[MIXR_HDR + e], rec[MIXR_HDR + a.n + e], p) : wks[e];
            rec[MIXR_HDR + e] = cur;
            rec[MIXR_HDR + a.n + e] = a.w[e];
            wks[e] = a.w[e];                         // the plain kernels are right the moment all ramps have ended
        }
    }
    rec[MIXR_INC] = a.inc;
    rec[MIXR_R] = a.R;
    rec[MIXR_DONE] = 0;
}

__global__ __launch_bounds__(MIX_BLOCK) void k_mixr_advance(u32 *ramp, const u32 *nframes, u32 frames, u32 streams,
                                                            u32 n)
{
    const u32 s = blockIdx.x * MIX_BLOCK + threadIdx.x;
    if (s >= streams)
        return;
    u32 *rec = ramp + (u64)s * (MIXR_HDR + 2u * n);
    const u32 R = rec[MIXR_R], done = rec[MIXR_DONE];
    if (done >= R)
        return;
    const u32 c = nframes ? nframes[s] : frames;
    rec[MIXR_DONE] = c >= R - done ? R : done + c;
}

__global__ __launch_bounds__(MIX_BLOCK) void k_mixr_cancel(u32 *ramp, u32 first, u32 count, u32 n)
{
    const u32 i = blockIdx.x * MIX_BLOCK + threadIdx.x;
    if (i >= count)
        return;
    u32 *rec = ramp + (u64)(first + i) * (MIXR_HDR + 2u * n);
    rec[MIXR_INC] = 0;
    rec[MIXR_R] = 0;
    rec[MIXR_DONE] = 0;
}

// ---------------------------------------------------------------------------
// launchers

uint32_t mixramp_record_dwords(uint32_t channels_in, uint32_t channels_out)
{
    return MIXR_HDR + 2u * channels_out * mix_cp(channels_in);
}

uint32_t mixramp_lds_bytes(uint32_t channels_in, uint32_t channels_out, uint32_t tile_frames)
{
    return mixr_lds_bytes(channels_in, channels_out, tile_frames);
}

// plan_mix's grid, block and tile.  The two extra matrices are at most 1 KiB, and no pair whose tile plan_mix left at
// MIX_TILE_MAX comes nearer to the limit than 15 -> 16 (63968 bytes), so the limit holds; it is checked all the same.
hipError_t launch_mixramp(const MixRampArgs &a, hipStream_t st)
{
    const MixPlan p = plan_mix(a.m);
    if (p.grid == 0)
        return p.err;
    MixRampArgs b = a;
    b.m.chunks = p.chunks;
    b.m.tile_frames = p.tile_frames;
    const u32 CI = a.m.channels_in, CO = a.m.channels_out;
    const u32 lds = p.fast ? 0u : mixr_lds_bytes(CI, CO, p.tile_frames);
    if (lds > MIX_LDS_LIMIT)
        return hipErrorInvalidValue;
    const u32 form = p.fast ? CI * 2u + CO : 0u;
    switch (form) {
    case 3: hipLaunchKernelGGL((k_mixr_fast<1, 1>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 4: hipLaunchKernelGGL((k_mixr_fast<1, 2>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 5: hipLaunchKernelGGL((k_mixr_fast<2, 1>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 6: hipLaunchKernelGGL((k_mixr_fast<2, 2>), dim3(p.grid), dim3(p.block), 0, st, b); break;
    default: hipLaunchKernelGGL(k_mixr_any, dim3(p.grid), dim3(p.block), lds, st, b); break;
    }
    return hipGetLastError();
}

hipError_t launch_mixramp_start(uint32_t *ramp, uint32_t *wk, uint32_t first, uint32_t count, uint32_t channels_in,
                                uint32_t channels_out, const int16_t *W, uint32_t R, hipStream_t st)
{
    if (count == 0)
        return hipSuccess;
    MixRampStartArgs a{};
    const u32 CP = mix_cp(channels_in);
    a.ramp = ramp;
    a.wk = wk;
    a.first = first;
    a.count = count;
    a.n = channels_out * CP;
    a.R = R;
    a.inc = (u32)(((1ull << 32) + R - 1u) / R);
    for (u32 o = 0; o < channels_out; o++)
        for (u32 c = 0; c < channels_in; c++)
            a.w[o * CP + (c >> 1)] |= (u32)(uint16_t)W[o * channels_in + c] << (16u * (c & 1u));
    hipLaunchKernelGGL(k_mixr_start, dim3((count + MIX_BLOCK - 1u) / MIX_BLOCK), dim3(MIX_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mixramp_advance(uint32_t *ramp, const uint32_t *nframes, uint32_t frames, uint32_t streams,
                                  uint32_t channels_in, uint32_t channels_out, hipStream_t st)
{
    if (streams == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_mixr_advance, dim3((streams + MIX_BLOCK - 1u) / MIX_BLOCK), dim3(MIX_BLOCK), 0, st, ramp,
                       nframes, frames, streams, channels_out * mix_cp(channels_in));
    return hipGetLastError();
}

hipError_t launch_mixramp_cancel(uint32_t *ramp, uint32_t first, uint32_t count, uint32_t channels_in,
                                 uint32_t channels_out, hipStream_t st)
{
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_mixr_cancel, dim3((count + MIX_BLOCK - 1u) / MIX_BLOCK), dim3(MIX_BLOCK), 0, st, ramp, first,
                       count, channels_out * mix_cp(channels_in));
    return hipGetLastError();
}

}  // namespace cmhip
