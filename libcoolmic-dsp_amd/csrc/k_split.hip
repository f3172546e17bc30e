// k_split.hip -- gfx950 (MI355X, wave64) band-split kernels: B - 1 linear-phase FIR filters of T taps in exact integers
// over interleaved int16 and the residual band (include/coolmic_hip.h, "band split", has the arithmetic to the bit):
//     acc_b = sum_{k<T} g_b[k] * x[n-k]      r_b = (acc_b + 2^(q_b-1)) >> q_b      y_b = saturate(r_b)
//     y_{B-1} = saturate(x[n-D] - sum_b r_b)
//
//   k_split_fast<C>  mono, stereo: a lane owns eight consecutive frames of one channel
//   k_split_any      any channel count (3..16 in practice): one channel after the other; no speed goal
//
// No recurrence, so the work is cut along time like the resampler's: one workgroup of 256 threads per stream and tile
// (csrc/split_plan.h has the plan, the table's form and why the sums are exact).
//
// LDS (dynamic): the table, then the tile's input frames j_lo = q0 - (Tp-1) .. as channel planes, TWICE: copy A as it
// is and copy B delayed by one sample (k_src.hip's two copies).  The sample x[n] of output q = n - q0 sits at plane
// index a0 = q + Tp - 1, and the pair (x[n-k-1], x[n-k]) of an even k is dword (a0 >> 1) - k/2 of A for an odd a0, of B
// for an even one.  Tp is a multiple of 8, so output i of lane j (q = 8j + i) has a0 odd for an even i: with
// base = 4j + Tp/2 - 1, pair kk of output i is dword base + i/2 - kk of A (even i), base + (i+1)/2 - kk of B (odd i).
// What differs from k_src.hip: the taps are the same in every lane, so a lane keeps a WINDOW of eight dwords of each
// copy in registers, takes four pairs of taps in one 16-byte read that every lane shares, and every dword it reads from
// the planes feeds up to eight dot instructions: per block of four pairs two 16-byte reads (base - kk0 - 3 is a
// multiple of 4) for 32 dot instructions.  j_lo may be negative in ANY tile: negative frames come from the stream's
// history, frames before the history are zero (they only meet zero taps).
#include "cmhip_device.h"

namespace cmhip {

__device__ __forceinline__ int split_dot2(u32 x, u32 k, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, k), acc, false);
}

// a finished group's sum: -2^31 can only be the wrapped +2^31 of two -32768 taps against two -32768 samples
__device__ __forceinline__ long long split_wide(int acc)
{
    return acc == (int)0x80000000u ? 2147483648ll : (long long)acc;
}

// The stream's new history: the last T-1 frames of (old history, this run's frames), into the slot the next run reads.
// Done by the workgroup of the stream's last tile (its first when the stream has no frame: it copies the slot over).
__device__ __forceinline__ void split_history(const SplitArgs &a, u32 s, u32 F, u32 C, const int16_t *ins)
{
    const u32 HT = a.taps - 1u;
    const int16_t *hrd = a.hist + ((u64)a.parity * a.streams + s) * C * HT;
    int16_t *hwr = a.hist + ((u64)(a.parity ^ 1u) * a.streams + s) * C * HT;
    for (u32 idx = threadIdx.x; idx < C * HT; idx += blockDim.x) {
        const u32 c = idx / HT, i = idx - c * HT;
        int16_t val;
        if (F + i < HT)                              // frame F - (T-1) + i lies before this run
            val = hrd[c * HT + i + F];
        else
            val = ins[(u64)(F - HT + i) * C + c];
        hwr[c * HT + i] = val;
    }
}

// the planes of CT channels (mono, stereo): frames j_lo .. jh, the run's from whole 16-byte vectors of the slot
template <int CT>
__device__ __forceinline__ void split_stage_fast(const SplitArgs &a, int16_t *pl, u32 s, int j_lo, u32 jh, u32 F,
                                                 const int16_t *ins)
{
    constexpr u32 C = (u32)CT;
    const u32 tid = threadIdx.x, row = a.row, HT = a.taps - 1u;
    const u32 staged = (u32)((int)jh - j_lo + 1);
    const u32 npre = j_lo < 0 ? min(staged, (u32)-j_lo) : 0u;
    if (npre) {
        const int16_t *hrd = a.hist + ((u64)a.parity * a.streams + s) * C * HT;
        for (u32 idx = tid; idx < npre * C; idx += SPLIT_BLOCK) {
            const u32 i = idx / C, c = idx - i * C;
            const int j = j_lo + (int)i;
            const int16_t val = j >= -(int)HT ? hrd[c * HT + (u32)((int)HT + j)] : (int16_t)0;
            pl[c * row + i] = val;
            pl[(C + c) * row + i + 1u] = val;
        }
    }
    if (staged > npre) {
        const u32 jb = j_lo < 0 ? 0u : (u32)j_lo;
        const u32 nsamp = F * C, nfull = nsamp >> 3, ntail = nsamp & 7u;
        const u32 v_hi = ((jh + 1u) * C + 7u) >> 3;
        for (u32 v = ((jb * C) >> 3) + tid; v < v_hi; v += SPLIT_BLOCK) {
            u32 x[4];
            load_vec(x, ins, v, v < nfull, v == nfull && ntail != 0, ntail);
#pragma unroll
            for (u32 i = 0; i < 8; i++) {
                const u32 e = v * 8u + i;
                const u32 j = e / C, c = e - j * C;
                if (j >= jb && j <= jh) {
                    const int16_t val = (int16_t)(x[i >> 1] >> (16u * (i & 1u)));
                    const u32 pos = (u32)((int)j - j_lo);
                    pl[c * row + pos] = val;
                    pl[(C + c) * row + pos + 1u] = val;
                }
            }
        }
    }
}

// the plane of channel c of C, sample by sample
__device__ __forceinline__ void split_stage_plane(const SplitArgs &a, int16_t *pl, u32 s, u32 c, u32 C, int j_lo, u32 jh,
                                                  const int16_t *ins)
{
    const u32 row = a.row, HT = a.taps - 1u;
    const u32 staged = (u32)((int)jh - j_lo + 1);
    const int16_t *hrd = a.hist + ((u64)a.parity * a.streams + s) * C * HT;
    for (u32 i = threadIdx.x; i < staged; i += SPLIT_BLOCK) {
        const int j = j_lo + (int)i;
        int16_t val = 0;
        if (j >= 0)
            val = ins[(u64)(u32)j * C + c];
        else if (j >= -(int)HT)
            val = hrd[c * HT + (u32)((int)HT + j)];
        pl[i] = val;
        pl[row + i + 1u] = val;
    }
}

// Frames 8j .. 8j + 7 of one channel: A4 and B4 are the channel's two plane copies, tab the table in LDS.
// emit(b, r): the eight unsaturated results of band b, bands in order, the residual last.
template <class Emit>
__device__ __forceinline__ void split_lane(const u32x4 *A4, const u32x4 *B4, u32 j, const u32 *tab, u32 nf, u32 T,
                                           Emit &&emit)
{
    const u32 Tp = split_tp(T), nb = Tp / 8u;
    const u32x4 *pairs = reinterpret_cast<const u32x4 *>(tab);
    const u32 *masks = tab + nf * (Tp / 2u), *qs = masks + nf * nb;
    int rsum[8];
#pragma unroll
    for (u32 i = 0; i < 8; i++)
        rsum[i] = 0;
    for (u32 b = 0; b < nf; b++) {
        int acc[8];
        long long tot[8];
#pragma unroll
        for (u32 i = 0; i < 8; i++) {
            acc[i] = 0;
            tot[i] = 0;
        }
        u32x4 pa = A4[j + nb], pb = B4[j + nb];
        // one block of four pairs: ENDS tells whether a group may end inside it (fm: behind which pairs)
        auto block = [&](u32 blk, auto ends, u32 fm) {
            constexpr bool ENDS = decltype(ends)::value;
            const u32x4 na = A4[j + nb - 1u - blk], nv = B4[j + nb - 1u - blk];
            const u32x4 kv = pairs[b * nb + blk];
            const u32 wa[8] = {na.x, na.y, na.z, na.w, pa.x, pa.y, pa.z, pa.w};
            const u32 wb[8] = {nv.x, nv.y, nv.z, nv.w, pb.x, pb.y, pb.z, pb.w};
            const u32 k[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
            for (u32 p = 0; p < 4; p++) {
#pragma unroll
                for (u32 i = 0; i < 8; i++)
                    acc[i] = split_dot2((i & 1u) ? wb[3u + (i + 1u) / 2u - p] : wa[3u + i / 2u - p], k[p], acc[i]);
                if constexpr (ENDS) {
                    if ((fm >> p) & 1u) {            // (uniform)
#pragma unroll
                        for (u32 i = 0; i < 8; i++) {
                            tot[i] += split_wide(acc[i]);
                            acc[i] = 0;
                        }
                    }
                }
            }
            pa = na;
            pb = nv;
        };
        // a mask word's upper half counts the blocks from here on in which no group ends: those run in a loop of
        // nothing but reads and dot instructions
        for (u32 blk = 0; blk < nb;) {
            const u32 w = uniform(masks[b * nb + blk]);
            const u32 n = w >> 16;
            if (n) {
#pragma unroll 2
                for (u32 u = 0; u < n; u++)
                    block(blk + u, std::false_type{}, 0u);
                blk += n;
            } else {
                block(blk, std::true_type{}, w & 15u);
                blk++;
            }
        }
        const u32 q = uniform(qs[b]);
        int r[8];
#pragma unroll
        for (u32 i = 0; i < 8; i++) {
            tot[i] += split_wide(acc[i]);
            r[i] = (int)((tot[i] + (1ll << (q - 1u))) >> q);
            rsum[i] += r[i];
        }
        emit(b, r);
    }
    // the residual: x[n-D] is plane index a0 - D = 8j + i + Tp - 1 - D of copy A
    const int16_t *plane = reinterpret_cast<const int16_t *>(A4);
    const u32 at = 8u * j + Tp - 1u - (T - 1u) / 2u;
    int r[8];
#pragma unroll
    for (u32 i = 0; i < 8; i++)
        r[i] = (int)plane[at + i] - rsum[i];
    emit(nf, r);
}

// saturation of a lane's eight results into four packed dwords; -> how many of the first nvalid saturated
__device__ __forceinline__ u32 split_pack(const int (&r)[8], u32 nvalid, u32 (&pk)[4])
{
    u32 cnt = 0;
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        const int y = min(max(r[i], -32768), 32767);
        cnt += (y != r[i] && i < nvalid) ? 1u : 0u;
        if (i & 1u)
            pk[i >> 1] |= (u32)y << 16;
        else
            pk[i >> 1] = (u32)y & 0xffffu;
    }
    return cnt;
}

// the wave's count of saturated samples into the stream's counter of band b (every lane of the wave calls this)
__device__ __forceinline__ void split_count(const SplitArgs &a, u32 s, u32 b, u32 cnt)
{
    const u32 total = wave_add_u32(cnt);
    if ((threadIdx.x & 63u) == 0u && total)
        atomicAdd(a.clips + (u64)s * a.bands + b, total);
}

template <int CT>
__device__ __forceinline__ void split_body(const SplitArgs &a)
{
    extern __shared__ u32x4 split_lds[];
    const u32 C = CT ? (u32)CT : a.channels;
    const u32 tid = threadIdx.x;
    const u32 s = blockIdx.x / a.chunks;             // stream
    const u32 k = blockIdx.x - s * a.chunks;         // tile inside the stream
    const u32 F = a.nframes ? a.nframes[s] : a.frames;
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    const u32 tile = a.tile_frames, q0 = k * tile;
    if (q0 < F) {                                    // (uniform)
        const u32 T = a.taps, Tp = split_tp(T), nf = a.bands - 1u, row = a.row;
        const u32 *tab = reinterpret_cast<const u32 *>(split_lds);
        int16_t *pl = reinterpret_cast<int16_t *>(split_lds + a.table_words / 4u);
        const u32x4 *src = reinterpret_cast<const u32x4 *>(a.table);
        for (u32 i = tid; i < a.table_words / 4u; i += SPLIT_BLOCK)
            split_lds[i] = src[i];
        const int j_lo = (int)q0 - (int)(Tp - 1u);
        const u32 jh = min(q0 + tile, F) - 1u;
        auto band_out = [&](u32 b) { return a.out + ((u64)b * a.streams + s) * a.out_stride; };
        if constexpr (CT != 0) {
            split_stage_fast<CT>(a, pl, s, j_lo, jh, F, ins);
            __syncthreads();
            const u32 j = CT == 2 ? tid >> 1 : tid, c = CT == 2 ? tid & 1u : 0u;
            const u32 f0 = q0 + 8u * j;              // the lane's first frame
            const u32 nvalid = F > f0 ? min(8u, F - f0) : 0u;
            const u32x4 *A4 = reinterpret_cast<const u32x4 *>(pl + c * row);
            const u32x4 *B4 = reinterpret_cast<const u32x4 *>(pl + ((u32)CT + c) * row);
            split_lane(A4, B4, j, tab, nf, T, [&](u32 b, const int (&r)[8]) {
                u32 pk[4];
                split_count(a, s, b, split_pack(r, nvalid, pk));
                int16_t *outs = band_out(b);
                if constexpr (CT == 1) {
                    if (nvalid == 8u) {
                        const u32x4 v = {pk[0], pk[1], pk[2], pk[3]};
                        *reinterpret_cast<u32x4 *>(outs + f0) = v;
                    } else {
                        for (u32 i = 0; i < nvalid; i++)         // frames past the count are not written
                            outs[f0 + i] = (int16_t)half_at(pk, i);
                    }
                } else {
                    // the neighbour lane has the other channel of the same frames: the left lane writes frames
                    // 0..3, the right lane frames 4..7, each 16 bytes
                    const u32 t0 = (u32)__shfl_xor((int)(c ? pk[0] : pk[2]), 1);
                    const u32 t1 = (u32)__shfl_xor((int)(c ? pk[1] : pk[3]), 1);
                    const u32 l0 = c ? t0 : pk[0], l1 = c ? t1 : pk[1];
                    const u32 r0 = c ? pk[2] : t0, r1 = c ? pk[3] : t1;
                    const u32 o[4] = {(l0 & 0xffffu) | (r0 << 16), (l0 >> 16) | (r0 & 0xffff0000u),
                                      (l1 & 0xffffu) | (r1 << 16), (l1 >> 16) | (r1 & 0xffff0000u)};
                    const u32 fb = f0 + 4u * c;
                    const u32 nv = F > fb ? min(4u, F - fb) : 0u;
                    u32 *dst = reinterpret_cast<u32 *>(outs) + fb;
                    if (nv == 4u) {
                        const u32x4 v = {o[0], o[1], o[2], o[3]};
                        *reinterpret_cast<u32x4 *>(dst) = v;
                    } else {
#pragma unroll
                        for (u32 i = 0; i < 4; i++)
                            if (i < nv)
                                dst[i] = o[i];
                    }
                }
            });
        } else {
            const u32 f0 = q0 + 8u * tid;
            const u32 nvalid = F > f0 ? min(8u, F - f0) : 0u;
            const u32x4 *A4 = reinterpret_cast<const u32x4 *>(pl);
            const u32x4 *B4 = reinterpret_cast<const u32x4 *>(pl + row);
            for (u32 c = 0; c < C; c++) {
                __syncthreads();                     // the plane of the channel before is done with
                split_stage_plane(a, pl, s, c, C, j_lo, jh, ins);
                __syncthreads();
                split_lane(A4, B4, tid, tab, nf, T, [&](u32 b, const int (&r)[8]) {
                    u32 pk[4];
                    split_count(a, s, b, split_pack(r, nvalid, pk));
                    int16_t *outs = band_out(b);
                    for (u32 i = 0; i < nvalid; i++)
                        outs[(u64)(f0 + i) * C + c] = (int16_t)half_at(pk, i);
                });
            }
        }
    }
    if (k == (F ? (F - 1u) / tile : 0u))
        split_history(a, s, F, C, ins);
}

template <int C>
__global__ __launch_bounds__(SPLIT_BLOCK) void k_split_fast(SplitArgs a)
{
    split_body<C>(a);
}

__global__ __launch_bounds__(SPLIT_BLOCK) void k_split_any(SplitArgs a)
{
    split_body<0>(a);
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_split(const SplitArgs &a, hipStream_t st)
{
    const SplitPlan p = plan_split(a.streams, a.channels, a.bands, a.taps, a.frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    SplitArgs b = a;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    b.row = p.row;
    b.table_words = p.table_words;
    if (!p.fast)
        hipLaunchKernelGGL(k_split_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    else if (a.channels == 1)
        hipLaunchKernelGGL(k_split_fast<1>, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    else
        hipLaunchKernelGGL(k_split_fast<2>, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    return hipGetLastError();
}

// test hooks (host logic, need no GPU): the plan of a run whose longest stream has `frames` frames, and the table in
// the kernel's form
extern "C" void cmhip_test_plan_split(uint32_t streams, uint32_t channels, uint32_t bands, uint32_t taps, uint32_t frames,
                                      SplitPlan *plan)
{
    if (plan)
        *plan = plan_split(streams, channels, bands, taps, frames);
}

extern "C" int cmhip_test_split_compile(uint32_t bands, uint32_t taps, const int16_t *g, const uint8_t *q, uint32_t *out,
                                        size_t cap)
{
    if (!split_geometry_ok(bands, taps) || !g || !q || !out || cap < split_table_words(bands, taps))
        return -1;
    split_compile(bands, taps, g, q, out);
    return (int)split_table_words(bands, taps);
}

}  // namespace cmhip
