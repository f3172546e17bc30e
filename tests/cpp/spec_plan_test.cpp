// spec_plan_test.cpp -- csrc/spec_plan.h's bookkeeping over cuts of a stream, compiled by g++ alone (no HIP).  A stream
// of 3000 frames (more at n = 11 and 12) whose samples are their own indices is cut into runs of 0..700 frames --
// constant run lengths, then random cuts -- and walked the way the kernel walks it (k_spec.hip): blocks gathered from
// the state and the run, the state rewritten from the state and the run.
//   - every block a cut completes is block j of the stream, frames [j H, j H + N), each once and in order, and the cut
//     completes exactly the blocks of the single run;
//   - every index formed stays inside the run (below its count) or inside the state (0 .. N - 2): the state ranges
//     never reach past N - 1;
//   - after every run the state is the stream's last N - 1 frames and back is below N.
//   - the tables' exact entries and symmetries, the default and designed band tables, and one block of the reference
//     (under the sanitizers: its indices).
//   usage: spec_plan_test [random cuts per size]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "spec_plan.h"

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

constexpr uint32_t MAX_RUN = 700;
// 3000 frames, and for the sizes at which that is hardly a block three blocks more
static uint32_t total(uint32_t n) { return n <= 10 ? 3000u : 3000u + (3u << n); }

struct Stream {
    uint32_t n, back = 0;
    uint64_t pos = 0, blocks = 0;
    std::vector<long> state;                         // entry j: the stream frame it holds, -1 before the stream
    explicit Stream(uint32_t n_) : n(n_), state((1u << n_) - 1u, -1) {}

    void run(uint32_t f)
    {
        const uint32_t N = 1u << n, H = N / 2;
        CHECK(back < N);
        const uint32_t nb = spec_run_blocks(n, back, f);
        for (uint32_t i = 0; i < nb; i++, blocks++)
            for (uint32_t t = 0; t < N; t++) {
                const int64_t rel = spec_block_frame(n, back, i, t);
                long frame;
                if (rel >= 0) {
                    CHECK(rel < (int64_t)f);
                    frame = (long)(pos + (uint64_t)rel);
                } else {
                    const int64_t j = (int64_t)N - 1 + rel;
                    CHECK(j >= 0 && j <= (int64_t)N - 2);
                    frame = state[(size_t)j];
                }
                CHECK(frame == (long)(blocks * H + t));
            }
        // no further block was complete
        CHECK((pos + f < N && blocks == 0) || (pos + f >= N && blocks == (pos + f - N) / H + 1));
        std::vector<long> next(N - 1);
        for (uint32_t j = 0; j + 1 < N; j++) {
            const int64_t rel = spec_state_frame(n, f, j);
            if (rel >= 0) {
                CHECK(rel < (int64_t)f);
                next[j] = (long)(pos + (uint64_t)rel);
            } else {
                CHECK((uint64_t)j + f <= N - 2);
                next[j] = state[j + f];
            }
        }
        state.swap(next);
        back = spec_next_back(n, back, f);
        pos += f;
        CHECK(back < N && back == pos - blocks * H);
        for (uint32_t j = 0; j + 1 < N; j++)
            CHECK(state[j] == (long)pos - (long)(N - 1) + (long)j || (state[j] == -1 && pos + j < N - 1));
    }
};

static void cut(uint32_t n, uint32_t fixed)
{
    Stream whole(n), parts(n);
    whole.run(total(n));
    uint32_t left = total(n);
    while (left) {
        uint32_t f = fixed ? fixed : rnd() % (MAX_RUN + 1u);
        if (f > left)
            f = left;
        parts.run(f);
        if (!fixed && rnd() % 4u == 0)
            parts.run(0);                            // a run that gives the stream nothing keeps everything
        left -= f;
    }
    CHECK(parts.blocks == whole.blocks && parts.back == whole.back && parts.state == whole.state);
}

static void tables(uint32_t n)
{
    const uint32_t N = 1u << n, Q = N / 4;
    std::vector<int16_t> win(N);
    std::vector<int32_t> wr(N / 2), wi(N / 2);
    spec_window(n, win.data());
    spec_twiddles(n, wr.data(), wi.data());
    CHECK(win[0] == 0 && win[N / 2] == 32767);
    for (uint32_t i = 1; i < N; i++)
        CHECK(win[i] == win[N - i] && win[i] >= 0);
    CHECK(wr[0] == SPEC_ONE && wi[0] == 0 && wr[Q] == 0 && wi[Q] == -SPEC_ONE);
    for (uint32_t k = 0; k <= Q; k++)
        CHECK(wr[Q - k] == -wi[k]);
    for (uint32_t k = 0; k < Q; k++)
        CHECK(wr[k + Q] == wi[k] && wi[k + Q] == -wr[k]);

    uint16_t e[SPEC_MAX_BANDS + 1];
    CHECK(spec_default_bands(n, e) == n && spec_bands_ok(n, n, e) && e[0] == 1 && e[n] == N / 2 + 1);
    for (uint32_t rate : {8000u, 44100u, 48000u, 192000u})
        for (uint32_t per = 1; per <= 3; per++) {
            const int nb = spec_design_bands(rate, n, per, e);
            CHECK(nb == -1 || (nb >= 1 && nb <= 32 && spec_bands_ok(n, (uint32_t)nb, e) && e[0] == 1 && e[nb] == N / 2 + 1));
        }
    CHECK(spec_design_bands(0, n, 1, e) == -1 && spec_design_bands(48000, n, 0, e) == -1 &&
          spec_design_bands(48000, n, 4, e) == -1);
    e[0] = 5, e[1] = 5;
    CHECK(!spec_bands_ok(n, 1, e) && !spec_bands_ok(n, 0, e) && !spec_bands_ok(n, 33, e));
    e[0] = 0, e[1] = (uint16_t)(N / 2 + 2);
    CHECK(!spec_bands_ok(n, 1, e));
    e[1] = (uint16_t)(N / 2 + 1);
    CHECK(spec_bands_ok(n, 1, e));

    // one block of the reference: full-scale noise, then DC at -32768, whose power lies in bins 0 and 1 alone
    std::vector<int16_t> x(N);
    std::vector<int32_t> z(2 * N);
    std::vector<uint64_t> p(N / 2 + 1);
    for (auto &v : x)
        v = (int16_t)(rnd() & 0xffffu);
    spec_block_ref(n, x.data(), win.data(), wr.data(), wi.data(), z.data(), z.data() + N, p.data());
    for (auto &v : x)
        v = -32768;
    spec_block_ref(n, x.data(), win.data(), wr.data(), wi.data(), z.data(), z.data() + N, p.data());
    uint64_t rest = 0;
    for (uint32_t k = 2; k <= N / 2; k++)
        rest += p[k];
    // (the window's own rounding to int16 is what the other bins hold: 60 dB and more below)
    CHECK(p[0] > (1ull << 41) && p[1] > (1ull << 39) && rest < (p[0] >> 20));
    CHECK(spec_db(0, 0) == 0.0 && spec_db(1649267441664ull, 1) == 0.0 && spec_db(0, 3) < -1e300);
}

int main(int argc, char **argv)
{
    const unsigned long random_cuts = argc > 1 ? strtoul(argv[1], nullptr, 10) : 200;
    unsigned long cuts = 0;
    for (uint32_t n = SPEC_MIN_LOG2; n <= SPEC_MAX_LOG2; n++) {
        tables(n);
        for (uint32_t f = 1; f <= MAX_RUN; f += n == SPEC_MIN_LOG2 || f < 8 ? 1 : 7, cuts++) {
            iteration = f;
            cut(n, f);
        }
        for (iteration = 0; iteration < random_cuts; iteration++, cuts++)
            cut(n, 0);
    }
    printf("spec plan ok: %lu cuts of %u to %u frames, n = %u..%u\n", cuts, total(SPEC_MIN_LOG2), total(SPEC_MAX_LOG2),
           SPEC_MIN_LOG2, SPEC_MAX_LOG2);
    return 0;
}
