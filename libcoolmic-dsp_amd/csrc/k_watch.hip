// k_watch.hip -- gfx950 (MI355X, wave64) kernels of the signal watch: per stream the run-length and sum statistics of
// dead air D, quiet channels Q(c) and samples at the rail R(c) over the TRANSFORMED stream (channel map, gain,
// saturation), in exact integers.  A pass of its own, launched ahead of the block kernel of the same run: it reads the
// run's INPUT slots and transforms them itself with the block kernels' arithmetic (cmhip_device.h).
//
//   k_watch_fast<C>  mono and stereo: one wave per 8 KiB tile of one stream
//   k_watch_any      3..16 channels: one workgroup per 1024 frames, no speed goal
//   k_watch_fold     one lane per stream and predicate: the run's tile summaries, in stream order, into the window
//
// The length of a run of consecutive frames is associative but not commutative, so nothing here merges by atomics in
// arrival order but the channel sums.  The tile pass writes a summary (csrc/watch_plan.h) per stream, tile and
// predicate; the fold, queued behind it on the same stream, walks them in order from the stream's state.  No workgroup
// waits for another.  DESIGN 4.22.
#include "cmhip_device.h"

namespace cmhip {

// ---------------------------------------------------------------------------
// Mono and stereo.
//
// A wave owns a contiguous tile of WATCH_TILE_VEC = 512 16-byte vectors of one stream (2048 stereo or 4096 mono
// frames) and loads it as k_corr_fast does: lane l takes the vectors l, l + 64, ..., so each of the 8 load
// instructions reads 1 KiB in one piece.  That order is wrong for runs (a lane holds 4 frames, then skips 252), so the
// tile goes through 8 KiB of LDS once and comes back a dword per lane: lane l of word n holds frame 64 n + l (stereo),
// or frames 64 n + l and 64 (n + 1) + l in its two halves (mono).  Now a predicate IS its mask: one v_cmp per
// predicate and frame writes the 64-bit word of 64 consecutive frames into a pair of SGPRs, bit l = frame 64 n + l,
// already in stream order, and dead air is one s_and of the two quiet words.  The runs are read off the words on the
// scalar unit (watch_run_push, csrc/watch_plan.h): a word that is all ones is an addition, a word in which no predicate
// holds -- programme -- is found by one s_or over the masks, and a mixed word is summarised with all its bits at once
// (watch_word) and combined, beside the other waves' vector work.  The word loops are not unrolled: twice unrolled,
// the accumulators' scalar registers no longer fit and six v_readlane per frame stood in the loop.
//
// A frame past the stream's count is a zero dword for the sums, and its bit is cleared in every mask: it is neither
// quiet nor at the rail, and does not count in len.
template <int C>
struct WatchAcc {
    WatchRun dead, quiet[C], rail[C];
};

template <int C, bool FULL>
__device__ __forceinline__ void watch_tile(const WatchArgs &a, u32 s, u32 k, u32 nfr, u32 nvec, const int16_t *ins,
                                           u32x4 *tile)
{
    constexpr u32 TILE_FRAMES = WATCH_TILE_VEC * 8u / C;
    constexpr u32 U = WATCH_TILE_VEC / 64u;
    const u32 lane = threadIdx.x & 63u;
    const u32 vl = k * WATCH_TILE_VEC + lane;    // the lane's first vector; its others follow 64 apart
    const u32x4 *src = reinterpret_cast<const u32x4 *>(ins);

    if constexpr (FULL) {                        // all loads in flight, then the writes
        u32x4 v[U];
#pragma unroll
        for (u32 i = 0; i < U; i++)
            v[i] = __builtin_nontemporal_load(src + vl + 64u * i);
#pragma unroll
        for (u32 i = 0; i < U; i++)
            tile[64u * i + lane] = v[i];
    } else {                                     // the stream's last tile: vectors past the count are not loaded
#pragma unroll
        for (u32 i = 0; i < U; i++) {
            u32x4 w = {0, 0, 0, 0};
            if (vl + 64u * i < nvec)
                w = __builtin_nontemporal_load(src + vl + 64u * i);
            tile[64u * i + lane] = w;
        }
    }
    __syncthreads();                             // (one wave: no s_barrier, the wait for the LDS writes)

    const StreamParam *p = a.param + s;
    const u32 perm2 = p->perm2;
    const u32 mi01 = p->mi01;
    const u32 mf0 = p->mf[0], mf1 = p->mf[C - 1];
    const u32 mipk = C == 1 ? (mi01 & 0xffffu) * 0x10001u : mi01;
    const u32 quiet = a.quiet, rail = a.rail, K = a.clip_run;
    const u32 f0 = k * TILE_FRAMES;              // the tile's first frame; f0 < nfr
    const u32 len = min(TILE_FRAMES, nfr - f0);  // (uniform)

    WatchAcc<C> acc{};
    int sum0 = 0, sum1 = 0;                      // per lane at most 64 * 2^15
    const u32 *tw = reinterpret_cast<const u32 *>(tile);
    const uint16_t *th = reinterpret_cast<const uint16_t *>(tile);
    if constexpr (C == 2 || !FULL) {
        // a word per step.  (Mono takes this form for its ragged tile only, a sample per lane in the low half of the
        // dword and nothing in the high one: the tile that counts, below, takes two words per dword.)
#pragma unroll 1
        for (u32 n = 0; n < TILE_FRAMES / 64u; n++) {
            if (!FULL && 64u * n >= len)         // (uniform)
                break;
            const u32 nb = FULL ? 64u : min(64u, len - 64u * n);
            const bool in = FULL || lane < nb;       // a frame past the count holds nothing
            u32 x = C == 2 ? tw[64u * n + lane] : (u32)th[64u * n + lane];
            if constexpr (!FULL)
                x = in ? x : 0u;
            if constexpr (C == 2)
                x = __builtin_amdgcn_perm(x, x, perm2);
            u32 w;
            const u32 mag = gain2<true>(x, mipk, mf0, mf1, w);
            sum0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, w), __builtin_bit_cast(v2s, 0x00000001u), sum0, false);
            const u32 m0 = mag & 0xffffu;
            const u64 q0 = __builtin_amdgcn_ballot_w64(in && m0 <= quiet);
            const u64 r0 = __builtin_amdgcn_ballot_w64(in && m0 >= rail);
            if constexpr (C == 2) {
                sum1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, w), __builtin_bit_cast(v2s, 0x00010000u), sum1,
                                              false);
                const u64 q1 = __builtin_amdgcn_ballot_w64(in && mag <= (quiet << 16 | 0xffffu));
                const u64 r1 = __builtin_amdgcn_ballot_w64(in && mag >= rail << 16);
                if ((q0 | q1 | r0 | r1) == 0) {      // (uniform) nothing in this word, the usual case
                    watch_run_zeros(acc.dead, nb, K);
                    watch_run_zeros(acc.quiet[0], nb, K);
                    watch_run_zeros(acc.quiet[C - 1], nb, K);
                    watch_run_zeros(acc.rail[0], nb, K);
                    watch_run_zeros(acc.rail[C - 1], nb, K);
                } else {
                    watch_run_push(acc.dead, q0 & q1, nb, K);
                    watch_run_push(acc.quiet[0], q0, nb, K);
                    watch_run_push(acc.quiet[C - 1], q1, nb, K);
                    watch_run_push(acc.rail[0], r0, nb, K);
                    watch_run_push(acc.rail[C - 1], r1, nb, K);
                }
            } else {
                watch_run_push(acc.quiet[0], q0, nb, K);
                watch_run_push(acc.rail[0], r0, nb, K);
            }
        }
    } else {
#pragma unroll 1
        for (u32 n = 0; n < TILE_FRAMES / 64u; n += 2) {
            const u32 x = (u32)th[64u * n + lane] | (u32)th[64u * (n + 1u) + lane] << 16;
            u32 w;
            const u32 mag = gain2<true>(x, mipk, mf0, mf1, w);
            sum0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, w), __builtin_bit_cast(v2s, 0x00010001u), sum0, false);
            const u32 m0 = mag & 0xffffu;
            const u64 qa = __builtin_amdgcn_ballot_w64(m0 <= quiet);
            const u64 qb = __builtin_amdgcn_ballot_w64(mag <= (quiet << 16 | 0xffffu));
            const u64 ra = __builtin_amdgcn_ballot_w64(m0 >= rail);
            const u64 rb = __builtin_amdgcn_ballot_w64(mag >= rail << 16);
            if ((qa | qb | ra | rb) == 0) {          // (uniform)
                watch_run_zeros(acc.quiet[0], 128u, K);
                watch_run_zeros(acc.rail[0], 128u, K);
            } else {
                watch_run_push(acc.quiet[0], qa, 64u, K);
                watch_run_push(acc.quiet[0], qb, 64u, K);
                watch_run_push(acc.rail[0], ra, 64u, K);
                watch_run_push(acc.rail[0], rb, 64u, K);
            }
        }
    }
    if constexpr (C == 1)
        acc.dead = acc.quiet[0];                 // mono: dead air is the one channel being quiet

    // the channel sums: |lane sum| <= 2^21, the wave's <= 2^27 -- exact as the low 32 bits of a two's complement sum
    const int t0 = (int)wave_add_u32((u32)sum0);
    const int t1 = C == 2 ? (int)wave_add_u32((u32)sum1) : 0;
    if (lane == 0) {
        unsigned long long *win = a.words + (u64)s * WATCH_WINDOW_WORDS + WATCH_W_SUM;
        if (t0)
            atomicAdd(win, (unsigned long long)(long long)t0);
        if (C == 2 && t1)
            atomicAdd(win + 1, (unsigned long long)(long long)t1);
        WatchSum *out = a.scratch + ((u64)s * a.chunks + k) * watch_preds(C);
        out[0] = watch_run_finish(acc.dead, K);
#pragma unroll
        for (u32 c = 0; c < (u32)C; c++) {
            out[1 + c] = watch_run_finish(acc.quiet[c], K);
            out[1 + C + c] = watch_run_finish(acc.rail[c], K);
        }
    }
}

template <int C>
__global__ __launch_bounds__(64) void k_watch_fast(WatchArgs a)
{
    __shared__ u32x4 tile[WATCH_TILE_VEC];
    const u32 s = blockIdx.x / a.chunks;         // stream
    const u32 k = blockIdx.x - s * a.chunks;     // tile inside the stream
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    const u32 nsamp = nfr * (u32)C;
    const u32 nvec = (nsamp + 7u) >> 3;          // 16-byte vectors that hold a sample of the stream
    const u32 v0 = k * WATCH_TILE_VEC;
    const int16_t *ins = a.in + (u64)s * a.stride;
    if (v0 >= nvec)                              // (the fold reads ceil(nfr / tile) summaries of this stream, no more)
        return;
    if (v0 + WATCH_TILE_VEC <= (nsamp >> 3))
        watch_tile<C, true>(a, s, k, nfr, nvec, ins, tile);
    else
        watch_tile<C, false>(a, s, k, nfr, nvec, ins, tile);
}

// ---------------------------------------------------------------------------
// Any channel count.  A workgroup of 256 threads takes WATCH_ANY_FRAMES = 1024 frames of one stream; thread t takes
// the frames t, t + 256, ... of the tile, so wave w's ballot for round j is the word of frames 256 j + 64 w .. + 63,
// word 4 j + w of the tile.  Channel by channel (gain1, as k_corr_any) the quiet and rail words go to LDS, the lanes
// keep the AND of their quiet bits for dead air; then thread p of the first 2C + 1 reads predicate p's 16 words in
// order.  The sums meet in LDS, one global atomic per channel that is not zero follows.
constexpr u32 WATCH_ANY_PER = WATCH_ANY_FRAMES / 256;        // frames per thread
constexpr u32 WATCH_ANY_WORDS = WATCH_ANY_FRAMES / 64;

__global__ __launch_bounds__(256) void k_watch_any(WatchArgs a)
{
    __shared__ u64 lmask[2 * MAX_CH + 1][WATCH_ANY_WORDS];
    __shared__ unsigned long long lsum[MAX_CH];
    __shared__ u32 lmf[MAX_CH], lmi[MAX_CH], lmap[MAX_CH];
    const u32 C = a.channels;
    const u32 s = blockIdx.x / a.chunks;
    const u32 k = blockIdx.x - s * a.chunks;
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    const u32 f0 = k * WATCH_ANY_FRAMES;         // the tile's first frame
    if (f0 >= nfr)                               // (uniform)
        return;
    const u32 len = min(WATCH_ANY_FRAMES, nfr - f0);
    const int16_t *ins = a.in + (u64)s * a.stride;
    const StreamParam *p = a.param + s;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < C) {
        lsum[threadIdx.x] = 0;
        lmf[threadIdx.x] = p->mf[threadIdx.x];
        lmi[threadIdx.x] = p->mi[threadIdx.x];
        lmap[threadIdx.x] = p->chmap[threadIdx.x];
    }
    __syncthreads();

    bool alive[WATCH_ANY_PER];                   // the frame is inside the count and every channel so far is quiet
#pragma unroll
    for (u32 j = 0; j < WATCH_ANY_PER; j++)
        alive[j] = j * 256u + threadIdx.x < len;
    for (u32 c = 0; c < C; c++) {                // (uniform)
        const u32 ic = lmap[c], mi = lmi[c], mf = lmf[c];
        int sum = 0;                             // per lane at most 4 * 2^15
#pragma unroll
        for (u32 j = 0; j < WATCH_ANY_PER; j++) {
            const u32 t = j * 256u + threadIdx.x;
            const bool in = t < len;
            int x = 0;
            if (in)
                x = gain1(ins[(u64)(f0 + t) * C + ic], mi, mf);
            sum += x;
            const u32 m = (u32)(x < 0 ? -x : x);
            const bool q = in && m <= a.quiet, r = in && m >= a.rail;
            alive[j] = alive[j] && q;
            // (every lane of every wave arrives here: the ballots and the reduction see full waves)
            const u64 qw = __builtin_amdgcn_ballot_w64(q), rw = __builtin_amdgcn_ballot_w64(r);
            if (lane == 0) {
                lmask[1 + c][4u * j + wave] = qw;
                lmask[1 + C + c][4u * j + wave] = rw;
            }
        }
        const int t = (int)wave_add_u32((u32)sum);
        if (lane == 0 && t)
            atomicAdd(&lsum[c], (unsigned long long)(long long)t);
    }
#pragma unroll
    for (u32 j = 0; j < WATCH_ANY_PER; j++) {
        const u64 dw = __builtin_amdgcn_ballot_w64(alive[j]);
        if (lane == 0)
            lmask[0][4u * j + wave] = dw;
    }
    __syncthreads();

    if (threadIdx.x < watch_preds(C)) {
        WatchRun acc{};
        for (u32 n = 0; n < WATCH_ANY_WORDS && 64u * n < len; n++)
            watch_run_push(acc, lmask[threadIdx.x][n], min(64u, len - 64u * n), a.clip_run);     // (q, r: inside len)
        a.scratch[((u64)s * a.chunks + k) * watch_preds(C) + threadIdx.x] = watch_run_finish(acc, a.clip_run);
    }
    if (threadIdx.x < C && lsum[threadIdx.x])
        atomicAdd(&a.words[(u64)s * WATCH_WINDOW_WORDS + WATCH_W_SUM + threadIdx.x], lsum[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// The fold: lane (s, p) takes predicate p of stream s through the run's tile summaries in stream order, from the
// state the stream brought along, and stores the window words and the new state.  Nobody else touches those words:
// no atomics.  A stream with 0 frames in the run keeps its window and state.
__global__ __launch_bounds__(WATCH_FOLD_BLOCK) void k_watch_fold(WatchArgs a, u32 tile_frames)
{
    const u32 np = watch_preds(a.channels);
    const u64 idx = (u64)blockIdx.x * WATCH_FOLD_BLOCK + threadIdx.x;
    if (idx >= (u64)a.streams * np)
        return;
    const u32 s = (u32)(idx / np), p = (u32)(idx - (u64)s * np);
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    if (nfr == 0)
        return;
    const u32 tiles = min((u32)(((u64)nfr + tile_frames - 1) / tile_frames), a.chunks);  // (a count past the run's
                                                                                         // frames reads no further)
    const u32 slot = watch_slot(a.channels, p);
    unsigned long long *w = a.words + (u64)s * WATCH_WINDOW_WORDS + slot;
    unsigned long long *st = a.state + (u64)s * WATCH_SLOTS + slot;
    WatchWords acc = {w[WATCH_W_CNT], w[WATCH_W_LONGEST], w[WATCH_W_EV], *st};
    const WatchSum *t = a.scratch + (u64)s * a.chunks * np + p;
    for (u32 i = 0; i < tiles; i++)
        watch_fold(acc, t[(u64)i * np], a.clip_run);
    w[WATCH_W_CNT] = acc.cnt;
    w[WATCH_W_LONGEST] = acc.longest;
    w[WATCH_W_EV] = acc.ev;
    *st = acc.state;
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_watch(const WatchArgs &a, const WatchPlan &p, hipStream_t st, hipEvent_t *ev)
{
    if (p.grid == 0)
        return p.refused ? hipErrorInvalidValue : hipSuccess;
    WatchArgs b = a;
    b.chunks = p.chunks;
    if (ev)
        (void)hipEventRecord(ev[0], st);
    if (a.channels == 1)
        hipLaunchKernelGGL(k_watch_fast<1>, dim3(p.grid), dim3(p.block), 0, st, b);
    else if (a.channels == 2)
        hipLaunchKernelGGL(k_watch_fast<2>, dim3(p.grid), dim3(p.block), 0, st, b);
    else
        hipLaunchKernelGGL(k_watch_any, dim3(p.grid), dim3(p.block), 0, st, b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (ev)
        (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(k_watch_fold, dim3(p.fold_grid), dim3(p.fold_block), 0, st, b, p.tile_frames);
    e = hipGetLastError();
    if (ev)
        (void)hipEventRecord(ev[2], st);
    return e;
}

// test hook: the plan of a watch pass (host logic, needs no GPU)
extern "C" void cmhip_test_plan_watch(uint32_t streams, uint32_t channels, uint32_t frames, WatchPlan *plan)
{
    if (plan)
        *plan = watch_plan(streams, channels, frames);
}

}  // namespace cmhip
