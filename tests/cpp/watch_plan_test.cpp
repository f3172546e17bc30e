// watch_plan_test.cpp -- csrc/watch_plan.h's run-length arithmetic against its own online reference, compiled by g++
// alone (no HIP).  A random bit sequence P (density 0.03 / 0.5 / 0.97 / 1.0, up to 600 frames) is cut at random places
// into windows, the windows into runs, the runs into tiles -- empty pieces, one-frame pieces and pieces that are all P
// included -- and taken through the text the kernels run:
//   - a tile's summary is built word by word (watch_push_word run by run, and watch_run_push / _zeros / _finish, which
//     hold whole words of ones back and summarise a mixed word with all its bits at once, watch_word; ragged last
//     word) and must equal the summary built frame by frame (watch_append), and the left-to-right watch_combine of its
//     two halves cut anywhere;
//   - a run's tiles are folded in order (watch_fold) from the incoming state; at every window's end count, longest,
//     events and state must equal watch_online over the same frames from the same state;
//   - every K from 1 to 16, incoming states 0, small, K - 1, K and 2^32 - 2 (why the state is 64 bits wide);
//   - the launch plan: tiles, grid, scratch size and the refusal at 2^31 workgroups.
// It counts what it drew and fails if a named edge case never came up.
//   usage: watch_plan_test [cases]      (default 20000)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "watch_plan.h"

using namespace cmhip;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static unsigned long iteration;

#define CHECK(c)                                                                                                      \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "%s:%d: %s failed (iteration %lu)\n", __FILE__, __LINE__, #c, iteration);                 \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

static bool same(const WatchSum &a, const WatchSum &b)
{
    return a.len == b.len && a.pre == b.pre && a.suf == b.suf && a.best == b.best && a.cnt == b.cnt && a.ev == b.ev;
}

// the summary of P[0..n), frame by frame
static WatchSum by_frames(const unsigned char *P, size_t n, uint32_t K)
{
    WatchSum s{};
    for (size_t i = 0; i < n; i++)
        watch_append(s, P[i] ? 1 : 0, P[i] ? 0 : 1, K);
    return s;
}

// ... and word by word, as the kernels build it; the bits past the piece are noise
static unsigned long words_all_ones, words_all_zeros, words_mixed;
static WatchSum by_words(const unsigned char *P, size_t n, uint32_t K)
{
    WatchSum s{};
    WatchRun r{};
    for (size_t at = 0; at < n; at += 64) {
        const uint32_t nb = (uint32_t)(n - at < 64 ? n - at : 64);
        uint64_t m = ((uint64_t)rnd() << 32) | rnd();
        for (uint32_t i = 0; i < nb; i++)
            m = (m & ~(1ull << i)) | ((uint64_t)(P[at + i] ? 1 : 0) << i);
        watch_push_word(s, m, nb, K);
        const uint64_t low = nb == 64 ? m : m & ((1ull << nb) - 1);
        if (low == 0 && rnd() % 2) {                 // (the kernels' shortcut for a word in which nothing holds)
            watch_run_zeros(r, nb, K);
        } else {
            watch_run_push(r, low, nb, K);           // (its contract: no bit at or above nb)
        }
        if (nb == 64)
            (m == ~0ull ? words_all_ones : m == 0 ? words_all_zeros : words_mixed)++;
    }
    const WatchSum held = watch_run_finish(r, K);    // the form that holds whole words of ones back: the same summary
    CHECK(same(held, s) && r.pend == 0);
    return s;
}

struct Seen {
    unsigned long empty_tile, all_p_tile, all_p_between_partial, one_frame_tile, big_state, event_on_cut, carried_in,
        not_carried_in, ragged_word, window_cut_in_run;
};

static void plan_checks()
{
    WatchPlan p = watch_plan(4096, 2, 65536);
    CHECK(!p.refused && p.fast == 1 && p.tile_frames == 2048 && p.chunks == 32 && p.grid == 4096u * 32u && p.block == 64);
    CHECK(p.scratch == (uint64_t)p.grid * 5 && p.fold_grid == (4096u * 5u + 255u) / 256u && p.fold_block == 256);
    p = watch_plan(8192, 1, 65536);
    CHECK(p.fast == 1 && p.tile_frames == 4096 && p.chunks == 16 && p.scratch == 8192ull * 16 * 3);
    p = watch_plan(3, 6, 1025);
    CHECK(p.fast == 0 && p.tile_frames == 1024 && p.chunks == 2 && p.grid == 6 && p.block == 256 && p.scratch == 6 * 13);
    p = watch_plan(1, 2, 1);
    CHECK(p.chunks == 1 && p.grid == 1);
    p = watch_plan(1, 2, 2049);
    CHECK(p.chunks == 2);
    CHECK(watch_plan(0, 2, 100).grid == 0 && watch_plan(4, 2, 0).grid == 0 && watch_plan(4, 17, 100).grid == 0);
    CHECK(!watch_plan(0, 2, 100).refused);
    // the limit: streams * tiles == 2^31 is refused, one tile less is not
    p = watch_plan(1u << 20, 2, 2048u << 11);
    CHECK(p.refused == 1 && p.grid == 0);
    p = watch_plan(1u << 20, 2, (2048u << 11) - 2048u);
    CHECK(!p.refused && p.grid == (1u << 20) * 2047u);
    p = watch_plan(1u << 19, 1, 4096u << 12);
    CHECK(p.refused == 1);
    p = watch_plan((1u << 19) - 1u, 1, 4096u << 12);
    CHECK(!p.refused && p.chunks == 4096);
    p = watch_plan(1u << 21, 5, 1024u << 10);
    CHECK(p.refused == 1);
    p = watch_plan(1u << 21, 5, (1024u << 10) - 1024u);
    CHECK(!p.refused && p.chunks == 1023);
    for (uint32_t C = 1; C <= 16; C++) {
        bool used[WATCH_SLOTS] = {};
        for (uint32_t q = 0; q < watch_preds(C); q++) {
            const uint32_t slot = watch_slot(C, q);
            CHECK(slot < WATCH_SLOTS && !used[slot]);
            used[slot] = true;
            CHECK(slot == (q == 0 ? 0 : q <= C ? q : 17 + (q - C - 1)));
        }
    }
}

int main(int argc, char **argv)
{
    const unsigned long cases = argc > 1 ? strtoul(argv[1], nullptr, 10) : 20000ul;
    static const double density[4] = {0.03, 0.5, 0.97, 1.0};
    Seen seen{};
    plan_checks();

    std::vector<unsigned char> P;
    for (iteration = 0; iteration < cases; iteration++) {
        const uint32_t K = 1 + (uint32_t)(iteration % 16);
        const double d = density[(iteration / 16) % 4];
        const size_t n = 1 + rnd() % 600;
        P.resize(n);
        for (size_t i = 0; i < n; i++)
            P[i] = d >= 1.0 || (rnd() & 0xffffff) < d * 16777216.0 ? 1 : 0;

        uint64_t l0;
        switch (rnd() % 6) {
        case 0: l0 = 0; break;
        case 1: l0 = 1 + rnd() % 20; break;
        case 2: l0 = K - 1; break;
        case 3: l0 = K; break;
        case 4: l0 = 0xfffffffeull; seen.big_state++; break;
        default: l0 = ((uint64_t)rnd() << 8) + rnd() % 7; break;
        }

        WatchWords dev{0, 0, 0, l0}, ref{0, 0, 0, l0};
        size_t at = 0;
        bool window_open = false;
        while (at < n) {
            // a run: 0 .. 600 frames, cut into tiles of 0 .. 299 frames
            size_t run = rnd() % 8 == 0 ? 0 : rnd() % 8 == 0 ? 1 : rnd() % 601;
            if (run > n - at)
                run = n - at;
            size_t done = 0;
            int last_kind = 0;                       // 1: a partial tile (not all P), 2: an all-P tile after one
            while (done < run || (run == 0 && rnd() % 2)) {
                size_t t = rnd() % 6 == 0 ? 0 : rnd() % 6 == 0 ? 1 : rnd() % 300;
                if (t > run - done)
                    t = run - done;
                const unsigned char *q = P.data() + at + done;
                const WatchSum a = by_words(q, t, K), b = by_frames(q, t, K);
                CHECK(same(a, b));
                CHECK(a.len == t && a.pre <= a.len && a.suf <= a.len && a.best <= a.len && a.cnt <= a.len);
                CHECK((a.pre == a.len) == (a.cnt == a.len) && (a.suf == a.len) == (a.cnt == a.len));
                if (t) {                             // the same tile from two halves, cut anywhere
                    const size_t h = rnd() % (t + 1);
                    CHECK(same(watch_combine(by_words(q, h, K), by_words(q + h, t - h, K), K), a));
                }
                if (t == 0)
                    seen.empty_tile++;
                if (t == 1)
                    seen.one_frame_tile++;
                if (t % 64)
                    seen.ragged_word++;
                if (t && a.cnt == a.len) {
                    seen.all_p_tile++;
                    if (last_kind == 1)
                        last_kind = 2;
                } else if (t) {
                    if (last_kind == 2 && a.pre)
                        seen.all_p_between_partial++;
                    last_kind = a.suf ? 1 : 0;
                }
                if (t && a.pre && dev.state)
                    seen.carried_in++;
                if (t && !a.pre && dev.state)
                    seen.not_carried_in++;
                if (t && dev.state && dev.state < K && dev.state + a.pre >= K)
                    seen.event_on_cut++;
                watch_fold(dev, a, K);
                done += t;
                if (run == 0)
                    break;
            }
            watch_online(ref, P.data() + at, run, K);
            at += run;
            window_open = window_open || run;
            CHECK(dev.state == ref.state);
            // a window's end: sometimes in the middle, always at the end
            if (window_open && (at == n || rnd() % 3 == 0)) {
                CHECK(dev.cnt == ref.cnt && dev.longest == ref.longest && dev.ev == ref.ev);
                if (dev.state && at < n)
                    seen.window_cut_in_run++;
                dev.cnt = dev.longest = dev.ev = 0;  // a result keeps the state
                ref.cnt = ref.longest = ref.ev = 0;
                window_open = false;
            }
        }
    }

    if (cases >= 20000) {
        CHECK(seen.empty_tile && seen.all_p_tile && seen.all_p_between_partial && seen.one_frame_tile && seen.big_state);
        CHECK(seen.event_on_cut && seen.carried_in && seen.not_carried_in && seen.ragged_word && seen.window_cut_in_run);
        CHECK(words_all_ones && words_all_zeros && words_mixed);
    }
    printf("watch plan ok: %lu cases (empty tiles %lu, all-P tiles %lu, all-P between partial %lu, states of 2^32 - 2 %lu, "
           "events completed across a cut %lu, windows cut inside a run %lu)\n",
           cases, seen.empty_tile, seen.all_p_tile, seen.all_p_between_partial, seen.big_state, seen.event_on_cut,
           seen.window_cut_in_run);
    return 0;
}
