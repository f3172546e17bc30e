// k_src.hip -- gfx950 (MI355X, wave64) sample-rate conversion kernels: a rational L/M polyphase FIR in exact integers
// over interleaved int16 (include/coolmic_hip.h, "sample-rate conversion", has the arithmetic to the bit).  Output
// frame m of a stream reads input frame n = floor(m*M/L) with phase p = (m*M) mod L:
//     acc = sum_{k<T} H[p][k] * x[n-k]      y[m] = saturate((acc + 8192) >> 14)
//
//   k_src_fast<C>  mono, stereo: a lane owns one dword of output (two mono frames / one stereo frame)
//   k_src_any      any channel count (3..16 in practice): a lane owns one output sample; no speed goal
//
// No recurrence, so the work is cut along time like true peak: one workgroup of 256 threads per stream and tile of
// SrcArgs::tile_out output frames.  Everything is periodic in M inputs / L outputs, so a run is counted from the
// stream's r = (frames so far) mod M instead of from its start: the run's outputs are m = kb .. kb + K - 1 with
// kb = ceil(r*L/M), K = ceil((r+F)*L/M) - kb, and frame j of the run is input n = r + j.
//
// LDS (dynamic, plan_src sizes it): the table, when it fits beside the tile, as [L][krow] with krow = Tp + 8 samples
// (Tp: T rounded up to 8, zero taps behind T; the 16 bytes of padding spread the phase rows over the banks) and each
// tap pair swapped into the order the dot instruction wants; then the tile's input frames j_lo .. j_hi as channel
// planes, TWICE: copy A as it is and copy B delayed by one sample.  The pair (x[n-k-1], x[n-k]) of an even k is then
// an aligned dword of A when its first index is even and of B when it is odd -- one choice per output frame, no
// v_alignbit per pair.  j_lo = n0 - r - (Tp-1) may be negative in ANY tile (a long filter over a short tile):
// negative frames come from the stream's history, frames before the history are zero (they only meet zero taps).
#include "cmhip_device.h"

namespace cmhip {

constexpr u32 SRC_BLOCK = 256;
constexpr u32 SRC_LDS_LIMIT = 64u * 1024u;       // what a workgroup may take without raising the device's limit
constexpr u32 SRC_TABLE_LDS_MAX = 45u * 1024u;   // the largest designed table (320 phases x 64 taps, padded) still fits
constexpr u32 SRC_TILE_MAX = 4096;               // output frames; bounds t = p0 + q*M below 2^22 (src_divmod)

__host__ __device__ constexpr u32 src_tp(u32 T) { return (T + 7u) & ~7u; }
__host__ __device__ constexpr u32 src_krow(u32 T) { return src_tp(T) + 8u; }

// floor(t / L) and t mod L for t < 2^22, L <= 640, inv = ceil(2^32 / L) (0 for L == 1): t * inv / 2^32 lies less
// than t / 2^32 < 2^-10 above t / L, which is at least 1 / L > 2^-10 below the next integer when it is not one.
__device__ __forceinline__ u32 src_divmod(u32 t, u32 L, u32 inv, u32 &rem)
{
    const u32 q = inv ? __umulhi(t, inv) : t;
    rem = t - q * L;
    return q;
}

__device__ __forceinline__ int src_dot2(u32 x, u32 k, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, k), acc, false);
}

__device__ __forceinline__ int src_round(int acc)
{
    return min(max((acc + 8192) >> 14, -32768), 32767);
}

// The stream's new history and position: the last T-1 frames of (old history, this run's frames) and (r + F) mod M,
// into the slots the next run reads.  Done by the workgroup of the stream's last tile (its first when the run gives
// the stream no output); a stream without a frame copies both over.
__device__ __forceinline__ void src_history(const SrcArgs &a, u32 s, u32 F, u32 C, u32 r, const int16_t *ins)
{
    const u32 HT = a.T - 1u;
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
    if (threadIdx.x == 0)
        a.rpos[(a.parity ^ 1u) * a.streams + s] = (r + F) % a.M;
}

// one tile: staging, then the lanes' outputs.  CT: the channel count when it is 1 or 2, 0: a.channels.  TLDS: the
// table sits in LDS.
template <int CT, bool TLDS>
__device__ __forceinline__ void src_tile(const SrcArgs &a, u32x4 *lds, u32 s, u32 q0, u32 K, u32 F, u32 r, u64 kb,
                                         const int16_t *ins)
{
    const u32 C = CT ? (u32)CT : a.channels;
    const u32 L = a.L, M = a.M, T = a.T, Tp = src_tp(T), krow = src_krow(T), row = a.row;
    const u32 tid = threadIdx.x;
    const u32 nq = min(a.tile_out, K - q0);          // the tile's output frames
    const u64 b0 = (kb + q0) * M, bl = (kb + q0 + nq - 1u) * M;
    const u64 n0 = b0 / L;
    const u32 p0 = (u32)(b0 - n0 * L);
    const u32 jf = (u32)(n0 - r);                    // run frame of the tile's first output
    const u32 jh = (u32)(bl / L - r);                // ... of its last: the last frame staged
    const int j_lo = (int)jf - (int)(Tp - 1u);       // the first frame staged (plane index 0)
    const u32 staged = (u32)((int)jh - j_lo + 1);
    int16_t *pl = reinterpret_cast<int16_t *>(lds) + (TLDS ? L * krow : 0u);

    if constexpr (TLDS) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(a.table);
        for (u32 i = tid; i < L * krow / 8u; i += SRC_BLOCK)
            lds[i] = src[i];
    }
    // frames before the run: the history, zeros before it
    const u32 npre = j_lo < 0 ? min(staged, (u32)-j_lo) : 0u;
    if (npre) {
        const u32 HT = T - 1u;
        const int16_t *hrd = a.hist + ((u64)a.parity * a.streams + s) * C * HT;
        for (u32 idx = tid; idx < npre * C; idx += SRC_BLOCK) {
            const u32 i = idx / C, c = idx - i * C;
            const int j = j_lo + (int)i;
            const int16_t val = j >= -(int)HT ? hrd[c * HT + (u32)((int)HT + j)] : (int16_t)0;
            pl[c * row + i] = val;
            pl[(C + c) * row + i + 1u] = val;
        }
    }
    // the run's frames jb .. jh: whole 16-byte vectors of the slot, the ragged last one sample by sample
    if (staged > npre) {
        const u32 jb = j_lo < 0 ? 0u : (u32)j_lo;
        const u32 nsamp = F * C, nfull = nsamp >> 3, ntail = nsamp & 7u;
        const u32 v_hi = ((jh + 1u) * C + 7u) >> 3;
        for (u32 v = ((jb * C) >> 3) + tid; v < v_hi; v += SRC_BLOCK) {
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
    __syncthreads();

    // output frame q of the tile, channels c .. c + NC - 1: t = p0 + q*M, n = n0 + t / L, p = t mod L.  x[n] is plane
    // index a0 = (n - r) - j_lo = t / L + Tp - 1; tap pair (k, k+1) is the dword that holds plane indices a0-k-1 and
    // a0-k: dword (a0 >> 1) - k/2 of copy A for an odd a0, of copy B (one sample later) for an even one.
    const u32 inv = a.inv_l;
    const u32x4 *tab = TLDS ? lds : reinterpret_cast<const u32x4 *>(a.table);
    auto frame = [&](u32 q, u32 c, auto nc, int (&y)[2]) {
        constexpr u32 NC = decltype(nc)::value;
        u32 p;
        const u32 a0 = src_divmod(p0 + q * M, L, inv, p) + Tp - 1u;
        const u32 *xp = reinterpret_cast<const u32 *>(pl + (((a0 & 1u) ? 0u : C) + c) * row) + (a0 >> 1);
        const u32x4 *kp = tab + p * (krow / 8u);
        int acc[2] = {0, 0};
        for (u32 kk = 0; kk < Tp / 2u; kk += 4u) {
            const u32x4 kv = kp[kk >> 2];
#pragma unroll
            for (u32 ch = 0; ch < NC; ch++) {
                const u32 *x = xp + ch * (row / 2u) - kk;
                acc[ch] = src_dot2(x[0], kv.x, acc[ch]);
                acc[ch] = src_dot2(*(x - 1), kv.y, acc[ch]);
                acc[ch] = src_dot2(*(x - 2), kv.z, acc[ch]);
                acc[ch] = src_dot2(*(x - 3), kv.w, acc[ch]);
            }
        }
#pragma unroll
        for (u32 ch = 0; ch < NC; ch++)
            y[ch] = src_round(acc[ch]);
    };

    int16_t *outs = a.out + (u64)s * a.out_stride;
    if constexpr (CT == 2) {
        u32 *dst = reinterpret_cast<u32 *>(outs) + q0;
        for (u32 w = tid; w < nq; w += SRC_BLOCK) {
            int y[2];
            frame(w, 0u, std::integral_constant<u32, 2>{}, y);
            dst[w] = ((u32)y[0] & 0xffffu) | ((u32)y[1] << 16);
        }
    } else if constexpr (CT == 1) {
        u32 *dst = reinterpret_cast<u32 *>(outs) + (q0 >> 1);        // (tile_out is even)
        for (u32 w = tid; 2u * w < nq; w += SRC_BLOCK) {
            int y0[2], y1[2];
            frame(2u * w, 0u, std::integral_constant<u32, 1>{}, y0);
            if (2u * w + 1u < nq) {
                frame(2u * w + 1u, 0u, std::integral_constant<u32, 1>{}, y1);
                dst[w] = ((u32)y0[0] & 0xffffu) | ((u32)y1[0] << 16);
            } else {
                outs[q0 + 2u * w] = (int16_t)y0[0];                  // outputs past the count are not written
            }
        }
    } else {
        for (u32 e = tid; e < nq * C; e += SRC_BLOCK) {
            const u32 q = e / C, c = e - q * C;
            int y[2];
            frame(q, c, std::integral_constant<u32, 1>{}, y);
            outs[(u64)(q0 + q) * C + c] = (int16_t)y[0];
        }
    }
}

template <int CT>
__device__ __forceinline__ void src_body(const SrcArgs &a)
{
    extern __shared__ u32x4 src_lds[];
    const u32 C = CT ? (u32)CT : a.channels;
    const u32 s = blockIdx.x / a.chunks;             // stream
    const u32 k = blockIdx.x - s * a.chunks;         // tile inside the stream
    const u32 F = a.nframes ? a.nframes[s] : a.frames;
    const u32 r = a.rpos[a.parity * a.streams + s];
    const u64 kb = ((u64)r * a.L + a.M - 1u) / a.M;  // outputs before this run, counted from r
    const u32 K = (u32)(((u64)(r + F) * a.L + a.M - 1u) / a.M - kb);
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    const u32 q0 = k * a.tile_out;
    if (q0 < K) {                                    // (uniform)
        if (a.table_lds)
            src_tile<CT, true>(a, src_lds, s, q0, K, F, r, kb, ins);
        else
            src_tile<CT, false>(a, src_lds, s, q0, K, F, r, kb, ins);
    }
    if (k == (K ? (K - 1u) / a.tile_out : 0u))
        src_history(a, s, F, C, r, ins);
}

template <int C>
__global__ __launch_bounds__(SRC_BLOCK) void k_src_fast(SrcArgs a)
{
    src_body<C>(a);
}

__global__ __launch_bounds__(SRC_BLOCK) void k_src_any(SrcArgs a)
{
    src_body<0>(a);
}

// ---------------------------------------------------------------------------
// launcher

// a tile of tile_out output frames stages at most floor((tile_out-1)*M/L) + 1 input frames of its own (floor(x+y) -
// floor(x) <= floor(y) + 1) behind a halo of Tp - 1, and copy B needs one sample more
static u32 src_tile_in(u32 tile_out, u32 L, u32 M, u32 T)
{
    return (u32)(((u64)(tile_out - 1u) * M) / L) + src_tp(T) + 1u;
}

SrcPlan plan_src(const SrcArgs &a, uint32_t out_frames)
{
    SrcPlan p{};
    p.err = hipSuccess;
    if (a.streams == 0 || out_frames == 0 || a.channels == 0 || a.channels > MAX_CH || a.L == 0 || a.M == 0 || a.T == 0)
        return p;
    const u32 C = a.channels;
    const u64 table_bytes = (u64)a.L * src_krow(a.T) * sizeof(int16_t);
    const u32 table_lds = table_bytes <= SRC_TABLE_LDS_MAX ? 1u : 0u;
    const u32 fixed = table_lds ? (u32)table_bytes : 0u;
    // the largest power of two of output frames whose planes (two copies, C channels) fit beside the table
    u32 tile = SRC_TILE_MAX, row = 0;
    u64 lds = 0;
    for (;; tile >>= 1) {
        row = (src_tile_in(tile, a.L, a.M, a.T) + 2u) & ~1u;
        lds = fixed + 2ull * C * row * sizeof(int16_t);
        if (lds <= SRC_LDS_LIMIT || tile == 1u)
            break;
    }
    SrcPlan refused{};
    refused.err = hipErrorInvalidValue;
    if (lds > SRC_LDS_LIMIT || (C <= 2 && tile < 2u))        // (not with L, M <= 640 and T <= 192)
        return refused;
    const u64 tiles = ((u64)out_frames + tile - 1u) / tile;
    if (tiles * a.streams >= (1ull << 31))                   // (as plan_run: no grid of 2^31 workgroups)
        return refused;
    p.fast = C <= 2 ? 1u : 0u;
    p.block = SRC_BLOCK;
    p.tile_out = tile;
    p.tile_in = src_tile_in(tile, a.L, a.M, a.T);
    p.row = row;
    p.table_lds = table_lds;
    p.lds_bytes = (u32)lds;
    p.chunks = (u32)tiles;
    p.grid = a.streams * p.chunks;
    return p;
}

hipError_t launch_src(const SrcArgs &a, uint32_t out_frames, hipStream_t st)
{
    const SrcPlan p = plan_src(a, out_frames);
    if (p.grid == 0)
        return p.err;
    SrcArgs b = a;
    b.chunks = p.chunks;
    b.tile_out = p.tile_out;
    b.row = p.row;
    b.table_lds = p.table_lds;
    b.inv_l = a.L == 1 ? 0u : (u32)(((1ull << 32) + a.L - 1u) / a.L);
    if (!p.fast)
        hipLaunchKernelGGL(k_src_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    else if (a.channels == 1)
        hipLaunchKernelGGL(k_src_fast<1>, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    else
        hipLaunchKernelGGL(k_src_fast<2>, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    return hipGetLastError();
}

// test hook: the plan of a resampler run that gives its longest stream out_frames frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_src(uint32_t streams, uint32_t channels, uint32_t L, uint32_t M, uint32_t T,
                                    uint32_t out_frames, SrcPlan *plan)
{
    SrcArgs a{};
    a.streams = streams;
    a.channels = channels;
    a.L = L;
    a.M = M;
    a.T = T;
    if (plan)
        *plan = plan_src(a, out_frames);
}

}  // namespace cmhip
