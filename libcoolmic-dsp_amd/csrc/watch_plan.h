// watch_plan.h -- the signal watch's run-length arithmetic, its launch plan and a plain reference
// (include/coolmic_hip.h, "signal watch").  Plain C++17, no HIP: tests/cpp/watch_plan_test.cpp compiles it with g++
// alone; the kernels (k_watch.hip) build their tile summaries and fold them with the same functions.
//
// A predicate P(n) over a stream's frames has the run length l(n) = P(n) ? l(n - 1) + 1 : 0.  The length of a run is
// associative but not commutative, so a piece of the stream (a tile) is summarised by a record that can be combined
// with its neighbours IN STREAM ORDER and nothing else:
//     len    frames of the piece (inside the stream's count)
//     pre    the leading run: frames from the piece's first that are all P (pre == len: the whole piece)
//     suf    the trailing run
//     best   the longest run inside the piece
//     cnt    frames with P
//     ev     frames whose run length COUNTED FROM THE PIECE'S FIRST FRAME equals K (clip events seen from inside)
// The fold takes a stream's pieces in order from the state l0 = l(first frame - 1) the stream brought along.
#ifndef CMHIP_WATCH_PLAN_H
#define CMHIP_WATCH_PLAN_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CMHIP_WATCH_HD __host__ __device__ inline
#else
#define CMHIP_WATCH_HD inline
#endif

namespace cmhip {

constexpr uint32_t WATCH_MAX_CH = 16;
constexpr uint32_t WATCH_MAX_RUN = 16;                       // the largest K
constexpr uint32_t WATCH_DEFAULT_QUIET = 32, WATCH_DEFAULT_RAIL = 32767, WATCH_DEFAULT_RUN = 3;

// Predicates of a stream of C channels, in the order the tile summaries are stored: dead air, then quiet per
// channel, then at-the-rail per channel.  The windows keep them in fixed slots, whatever C is.
constexpr uint32_t watch_preds(uint32_t C) { return 2 * C + 1; }
constexpr uint32_t WATCH_SLOTS = 2 * WATCH_MAX_CH + 1;       // 0: dead, 1 + c: quiet, 17 + c: rail
constexpr uint32_t watch_slot(uint32_t C, uint32_t p) { return p <= C ? p : WATCH_MAX_CH + 1 + (p - C - 1); }
// One stream's words on the device, 64-bit each: the window [S][WATCH_WINDOW_WORDS] (cnt, longest, ev per slot; the
// channel sums, two's complement) and, in an array of its own behind all windows, the state [S][WATCH_SLOTS], which
// a result leaves alone.
constexpr uint32_t WATCH_W_CNT = 0, WATCH_W_LONGEST = WATCH_SLOTS, WATCH_W_EV = 2 * WATCH_SLOTS,
                   WATCH_W_SUM = 3 * WATCH_SLOTS, WATCH_WINDOW_WORDS = 3 * WATCH_SLOTS + WATCH_MAX_CH,
                   WATCH_WORDS = WATCH_WINDOW_WORDS + WATCH_SLOTS;

struct WatchSum {
    uint32_t len, pre, suf, best, cnt, ev;
};

// ---------------------------------------------------------------------------
// building a summary: `ones` frames with P, then `zeros` frames without, behind what acc holds
CMHIP_WATCH_HD void watch_append(WatchSum &acc, uint32_t ones, uint32_t zeros, uint32_t K)
{
    if (ones) {
        if (acc.suf < K && K - acc.suf <= ones)
            acc.ev++;
        if (acc.pre == acc.len)
            acc.pre += ones;
        acc.suf += ones;
        acc.len += ones;
        acc.cnt += ones;
        if (acc.suf > acc.best)
            acc.best = acc.suf;
    }
    if (zeros) {
        acc.suf = 0;
        acc.len += zeros;
    }
}

// the low nbits (0..64) of mask, bit i the piece's frame i behind what acc holds, run by run
CMHIP_WATCH_HD void watch_push_word(WatchSum &acc, uint64_t mask, uint32_t nbits, uint32_t K)
{
    uint32_t left = nbits;
    while (left) {
        // the ones at the bottom, then the zeros behind them, neither past `left`
        const uint64_t inv = ~mask;
        uint32_t ones = inv ? (uint32_t)__builtin_ctzll(inv) : 64u;
        if (ones > left)
            ones = left;
        mask = ones < 64u ? mask >> ones : 0;
        uint32_t zeros = mask ? (uint32_t)__builtin_ctzll(mask) : 64u;
        if (zeros > left - ones)
            zeros = left - ones;
        mask = zeros < 64u ? mask >> zeros : 0;
        watch_append(acc, ones, zeros, K);
        left -= ones + zeros;
    }
}

// The same, made cheap for what a meter mostly sees -- words that are all zeros (programme) or all ones (silence, a
// stuck converter): ones are held back in `pend` while whole words of them keep coming and appended in one step when
// something else arrives, so a word of either kind costs a compare and an addition.  watch_run_finish gives the
// summary.  (On the GPU these run on the scalar unit, where an instruction costs a wave as much as a vector one.)
struct WatchRun {
    WatchSum sum;
    uint32_t pend;                  // ones seen and not yet appended to sum
};

CMHIP_WATCH_HD void watch_run_flush(WatchRun &r, uint32_t K)
{
    if (r.pend) {
        watch_append(r.sum, r.pend, 0, K);
        r.pend = 0;
    }
}
// nbits frames without P
CMHIP_WATCH_HD void watch_run_zeros(WatchRun &r, uint32_t nbits, uint32_t K)
{
    watch_run_flush(r, K);
    watch_append(r.sum, 0, nbits, K);
}
// The summary of one word by itself, all bits at once: nbits in 1..64, no bit of mask at or above nbits, mask neither
// 0 nor all ones.  What a signal that flips a predicate every few frames needs: the cost is the longest run of the
// word (one AND per frame of it), not the number of its runs.
CMHIP_WATCH_HD WatchSum watch_word(uint64_t mask, uint32_t nbits, uint32_t K)
{
    WatchSum w;
    w.len = nbits;
    w.cnt = (uint32_t)__builtin_popcountll(mask);
    w.pre = (uint32_t)__builtin_ctzll(~mask);                        // (mask is not all ones)
    // the trailing run: ones below bit nbits, counted down from there
    const uint64_t top = ~(mask << (64u - nbits));                   // (nbits >= 1) not 0: the bits below are ones
    w.suf = (uint32_t)__builtin_clzll(top);
    // runs of K: bit n of a is set where the frames n - K + 1 .. n all hold; the shifts bring zeros in below
    uint64_t a = mask;
    uint32_t have = 1;
    while (have < K && a) {                                          // doubling: K <= 16 takes four steps
        const uint32_t step = have < K - have ? have : K - have;
        a &= a << step;
        have += step;
    }
    w.ev = (uint32_t)__builtin_popcountll(a & ~(mask << K));         // ... and frame n - K does not (or lies before)
    uint32_t best = 0;
    for (uint64_t x = mask; x; x &= x << 1)
        best++;
    w.best = best;
    return w;
}

// a word whose bits at and above nbits are ZERO (so a word of all ones is a whole word)
CMHIP_WATCH_HD WatchSum watch_combine(const WatchSum &a, const WatchSum &b, uint32_t K);
CMHIP_WATCH_HD void watch_run_push(WatchRun &r, uint64_t mask, uint32_t nbits, uint32_t K)
{
    if (mask == ~0ull) {
        r.pend += 64u;
        return;
    }
    watch_run_flush(r, K);
    if (mask == 0)
        watch_append(r.sum, 0, nbits, K);
    else
        r.sum = watch_combine(r.sum, watch_word(mask, nbits, K), K);
}
CMHIP_WATCH_HD WatchSum watch_run_finish(WatchRun &r, uint32_t K)
{
    watch_run_flush(r, K);
    return r.sum;
}

// a || b: the summary of piece a followed by piece b
CMHIP_WATCH_HD WatchSum watch_combine(const WatchSum &a, const WatchSum &b, uint32_t K)
{
    WatchSum r;
    r.len = a.len + b.len;
    r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
    r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
    const uint32_t mid = a.suf + b.pre;
    r.best = a.best > b.best ? a.best : b.best;
    if (mid > r.best)
        r.best = mid;
    r.cnt = a.cnt + b.cnt;
    r.ev = a.ev + b.ev - (b.pre >= K ? 1u : 0u) + (a.suf < K && K <= mid ? 1u : 0u);
    return r;
}

// ---------------------------------------------------------------------------
// the fold: one predicate's window words and state, taken through one piece
struct WatchWords {
    uint64_t cnt, longest, ev;      // the window since its last result
    uint64_t state;                 // l at the last frame accounted; the window's `current` while it holds a frame
};

CMHIP_WATCH_HD void watch_fold(WatchWords &w, const WatchSum &t, uint32_t K)
{
    const uint64_t l0 = w.state;
    const uint64_t lead = t.pre ? l0 + t.pre : 0;            // a run from before counts only if it continues
    if (t.best > w.longest)
        w.longest = t.best;
    if (lead > w.longest)
        w.longest = lead;
    w.cnt += t.cnt;
    w.ev += t.ev;
    if (t.pre >= K)                                          // counted from the piece's first frame: not where l is K
        w.ev -= 1;
    if (l0 < K && K - l0 <= t.pre)
        w.ev += 1;
    w.state = t.suf == t.len ? l0 + t.suf : t.suf;
}

// ---------------------------------------------------------------------------
// the plain reference: the definition, frame by frame
inline void watch_online(WatchWords &w, const unsigned char *P, size_t n, uint32_t K)
{
    for (size_t i = 0; i < n; i++) {
        w.state = P[i] ? w.state + 1 : 0;
        w.cnt += P[i] ? 1 : 0;
        if (w.state > w.longest)
            w.longest = w.state;
        if (w.state == K)
            w.ev++;
    }
}

// ---------------------------------------------------------------------------
// the launch plan.  fast (mono, stereo): one wave per tile of 512 16-byte vectors, 4096 / C frames.  Otherwise one
// workgroup of 256 threads per 1024 frames.  The tile pass writes one summary per stream, tile and predicate into a
// scratch array [S][tiles][2C + 1]; the fold runs one lane per stream and predicate.
constexpr uint32_t WATCH_TILE_VEC = 512;                     // 8 KiB of PCM
constexpr uint32_t WATCH_ANY_FRAMES = 1024;
constexpr uint32_t WATCH_FOLD_BLOCK = 256;

struct WatchPlan {
    int32_t  refused;               // 1: the grid would reach 2^31 workgroups
    uint32_t fast;
    uint32_t tile_frames;
    uint32_t chunks;                // tiles per stream
    uint32_t grid, block;           // the tile pass; grid 0: nothing to launch (or refused)
    uint32_t fold_grid, fold_block;
    uint64_t scratch;               // summaries the scratch array holds: streams * chunks * (2C + 1)
};

inline WatchPlan watch_plan(uint32_t streams, uint32_t channels, uint32_t frames)
{
    WatchPlan p{};
    if (streams == 0 || frames == 0 || channels == 0 || channels > WATCH_MAX_CH)
        return p;
    p.fast = channels <= 2 ? 1u : 0u;
    p.tile_frames = p.fast ? WATCH_TILE_VEC * 8u / channels : WATCH_ANY_FRAMES;
    const uint64_t tiles = ((uint64_t)frames + p.tile_frames - 1) / p.tile_frames;
    if (tiles * streams >= (1ull << 31)) {                   // (as the block kernels' plan: no grid of 2^31 workgroups)
        WatchPlan refused{};
        refused.refused = 1;
        return refused;
    }
    p.chunks = (uint32_t)tiles;
    p.grid = streams * p.chunks;
    p.block = p.fast ? 64u : 256u;
    p.fold_block = WATCH_FOLD_BLOCK;
    p.fold_grid = (uint32_t)(((uint64_t)streams * watch_preds(channels) + WATCH_FOLD_BLOCK - 1) / WATCH_FOLD_BLOCK);
    p.scratch = (uint64_t)p.grid * watch_preds(channels);
    return p;
}

}  // namespace cmhip
#endif
