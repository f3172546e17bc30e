// agc_plan_test.cpp -- csrc/agc_plan.h, compiled by g++ alone (no HIP):
//   - agc_step against a restatement of the header's step in 64-bit integers over a grid of A, L and parameters: L = 0
//     and 32768, rise / fall of 0, 1 and 65535, D clamped at both ends, max(1, ...) making the last approach;
//   - the run plan (first window, window count, completed windows, head and tail) for every start position mod W and
//     every run length 0..3W+1 at w = 6, against a frame-by-frame count; NW is never exceeded;
//   - the tiles of such runs: every frame of the run lies in exactly one tile, a tile lies inside one window and says
//     which, its span covers its samples once -- whole vectors inside, at most 7 samples in front and behind -- and the
//     plan's tiles per stream and vectors per thread suffice, for every channel count;
//   - the interpolation's and the product's int32 bounds at the extremes, and the level's bound at E = 2^44;
//   - a stream walked window by window as k_agc_step walks it equals a stream walked frame by frame, whatever the cuts.
//   usage: agc_plan_test [iterations]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "agc_plan.h"

using namespace cmhip;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static uint32_t pick(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1u); }

static unsigned long iteration;

#define CHECK(c)                                                                                                      \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "%s:%d: %s failed (iteration %lu)\n", __FILE__, __LINE__, #c, iteration);                 \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

// the header's step, restated in int64 with min and max as it writes them
static int64_t step_model(int64_t A, int64_t L, const AgcParams &p)
{
    if (L == 0 || L < p.gate)
        return A;
    int64_t D = ((int64_t)p.target << 12) / L;
    D = D < p.gain_min ? p.gain_min : D > p.gain_max ? p.gain_max : D;
    if (D > A && p.rise) {
        int64_t d = (A * p.rise) >> 16;
        d = d > 1 ? d : 1;
        return D < A + d ? D : A + d;
    }
    if (D < A && p.fall) {
        int64_t d = (A * p.fall) >> 16;
        d = d > 1 ? d : 1;
        return D > A - d ? D : A - d;
    }
    return A;
}

static unsigned long test_step()
{
    static const uint16_t rates[] = {0, 1, 2, 655, 6132, 32768, 65535};
    static const uint32_t levels[] = {0, 1, 2, 3, 29, 30, 31, 299, 300, 3277, 3278, 20000, 32767, 32768};
    static const uint16_t targets[] = {1, 300, 3277, 32767};
    static const uint16_t gates[] = {0, 1, 30, 300, 32767};
    static const uint16_t bounds[][2] = {{1, 65535}, {4096, 4096}, {1024, 16384}, {1, 1}, {65535, 65535}, {4095, 4097}};
    unsigned long n = 0, taken[6] = {0, 0, 0, 0, 0, 0};
    for (uint16_t T : targets)
        for (uint16_t Q : gates)
            for (auto &b : bounds)
                for (uint16_t rise : rates)
                    for (uint16_t fall : rates) {
                        const AgcParams p = {T, Q, b[0], b[1], rise, fall, b[0]};
                        CHECK(agc_params_ok(p));
                        for (uint32_t L : levels) {
                            // A over the whole range, densely around the desired gain: the last approach
                            const int64_t D0 = L ? ((int64_t)T << 12) / L : 0;
                            const int64_t D = D0 < b[0] ? b[0] : D0 > b[1] ? b[1] : D0;
                            std::vector<int64_t> gains;
                            for (int64_t A = b[0]; A <= b[1]; A += 997)
                                gains.push_back(A);
                            for (int64_t A = D - 3; A <= D + 3; A++)
                                gains.push_back(A);
                            for (int64_t A = (int64_t)b[1] - 3; A <= b[1]; A++)
                                gains.push_back(A);
                            for (int64_t A : gains) {
                                if (A < b[0] || A > b[1])
                                    continue;
                                const uint32_t got = agc_step((uint32_t)A, L, p);
                                const int64_t want = step_model(A, (int64_t)L, p);
                                CHECK((int64_t)got == want);
                                CHECK(got >= b[0] && got <= b[1]);
                                if (L == 0 || L < Q)
                                    taken[0]++;
                                else if (got > A)
                                    taken[got == D ? 1 : 2]++;
                                else if (got < A)
                                    taken[got == D ? 3 : 4]++;
                                else
                                    taken[5]++;
                                n++;
                            }
                        }
                    }
    for (unsigned long t : taken)
        CHECK(t > 0);
    // the figures of the header: 3277 at level 300 wants 44741; full scale at the largest gain falls to 4095 at once;
    // one unit below the wanted gain with the smallest rise, max(1, ...) makes the last approach
    const AgcParams q = {3277, 0, 1, 65535, 1, 1, 4096};
    CHECK(agc_step(44740, 300, q) == 44741 && agc_step(44741, 300, q) == 44741 && agc_step(44742, 300, q) == 44741);
    const AgcParams low = {16, 0, 1, 65535, 1, 1, 4096};                 // (16 << 12) / 32768 = 2
    CHECK(agc_step(1, 32768, low) == 2 && agc_step(2, 32768, low) == 2 && agc_step(3, 32768, low) == 2);
    const AgcParams f = {32767, 0, 1, 65535, 65535, 65535, 65535};
    CHECK(agc_step(65535, 32768, f) == 4095 && agc_step(1, 1, f) == 2 && agc_step(40000, 1, f) == 65535);
    return n;
}

// a run's plan against a frame-by-frame count
static unsigned long test_run_plan(uint32_t w)
{
    const uint32_t W = 1u << w;
    unsigned long n = 0;
    for (uint32_t j0 = 0; j0 < W; j0++)
        for (uint32_t count = 0; count <= 3u * W + 1u; count++) {
            const uint64_t pos = (uint64_t)pick(0, 5) * W + j0 + ((uint64_t)(rnd() & 1u) << 33);
            const AgcRun r = agc_run(pos, count, w);
            uint32_t nwin = 0, complete = 0, head = 0, tail = 0;
            uint64_t last = ~0ull;
            for (uint32_t f = 0; f < count; f++) {
                const uint64_t k = (pos + f) >> w;
                if (k != last) {
                    nwin++;
                    last = k;
                }
                if (((pos + f + 1u) & (W - 1u)) == 0)
                    complete++;
                if (k == (pos >> w) && j0 != 0)
                    head++;
                if (k == ((pos + count) >> w) && !(k == (pos >> w) && j0 != 0))
                    tail++;
            }
            CHECK(r.first == (pos >> w) && r.nwin == nwin && r.complete == complete && r.head == head && r.tail == tail);
            CHECK(r.nwin == r.complete || r.nwin == r.complete + 1u);
            // NW: the rows of a stream in the tables, for every max_frames that admits the run
            CHECK(r.nwin <= agc_table_windows(count ? count : 1u, w));
            n++;
        }
    return n;
}

// the tiles of a run, for one channel count
static void check_tiles(uint32_t C, uint32_t w, uint64_t pos, uint32_t count, uint32_t max_frames)
{
    const AgcPlan p = plan_agc(3, C, w, max_frames, count);
    CHECK(p.err == 0 && p.grid == 3u * p.chunks && p.nw == agc_table_windows(max_frames, w) && p.tile_log2 <= w);
    if (count == 0) {                                                    // nothing is launched
        CHECK(p.grid == 0 && p.chunks == 0 && agc_run(pos, 0, w).nwin == 0);
        return;
    }
    CHECK(p.block == (C <= 2 ? AGC_FAST_BLOCK : AGC_ANY_BLOCK) && p.step_grid == 1);
    const uint32_t per_thread = C <= 2 ? AGC_FAST_VECS / AGC_FAST_BLOCK : AGC_ANY_VECS;
    std::vector<int> frames(count, 0), samples((size_t)count * C, 0);
    const AgcRun r = agc_run(pos, count, w);
    for (uint32_t t = 0; t < p.chunks + 2u; t++) {
        const AgcTile tl = agc_tile((uint32_t)pos, count, w, p.tile_log2, t);
        CHECK(tl.fa <= count && tl.fb <= count);
        if (tl.fa >= tl.fb)
            continue;
        CHECK(t < p.chunks);                                             // the grid has a workgroup for it
        CHECK(tl.fb - tl.fa <= (1u << p.tile_log2));
        CHECK(tl.win < r.nwin && tl.win < p.nw);
        for (uint32_t f = tl.fa; f < tl.fb; f++) {
            frames[f]++;
            CHECK(((pos + f) >> w) - r.first == tl.win);                 // one window, and the one it names
            CHECK(((pos + f) & ((1u << w) - 1u)) == tl.j + (f - tl.fa));
        }
        const AgcSpan s = agc_tile_span(tl.fa, tl.fb, C);
        CHECK(s.sa == tl.fa * C && s.sb == tl.fb * C && s.sa <= s.hend && s.hend <= s.tb && s.tb <= s.sb);
        CHECK(s.hend - s.sa <= 7u && s.sb - s.tb <= 7u);
        CHECK(s.ve - s.vb <= p.block * per_thread);
        for (uint32_t e = s.sa; e < s.hend; e++)
            samples[e]++;
        for (uint32_t v = s.vb; v < s.ve; v++)
            for (uint32_t i = 0; i < 8; i++) {
                CHECK(v * 8u + i >= s.hend && v * 8u + i < s.tb);
                samples[v * 8u + i]++;
            }
        for (uint32_t e = s.tb; e < s.sb; e++)
            samples[e]++;
    }
    for (int v : frames)
        CHECK(v == 1);
    for (int v : samples)
        CHECK(v == 1);
}

// the bounds the header states
static void test_bounds()
{
    for (uint32_t w = AGC_W_MIN; w <= AGC_W_MAX; w++) {
        const uint32_t W = 1u << w;
        const uint32_t ends[][2] = {{1, 65535}, {65535, 1}, {65535, 65535}, {1, 1}, {4096, 4095}};
        for (auto &e : ends)
            for (uint32_t j : {0u, 1u, W / 2u, W - 1u}) {
                const int64_t prod = ((int64_t)e[1] - (int64_t)e[0]) * (int64_t)j;
                CHECK(prod < (1ll << 30) && prod > -(1ll << 30));
                const int64_t want = (int64_t)e[0] + (prod >> w);         // (arithmetic: floor)
                const int32_t g = agc_gain(e[0], e[1], j, w);
                CHECK((int64_t)g == want && g >= 1 && g <= 65535);
                CHECK((e[0] <= e[1] ? g >= (int32_t)e[0] && g <= (int32_t)e[1] : g <= (int32_t)e[0] && g >= (int32_t)e[1]));
            }
        // the loudest window there is: every frame -32768
        const uint64_t E = (uint64_t)W << 30;
        CHECK(E <= (1ull << 44) && agc_level(E, w) == 32768u && agc_level(E - 1u, w) == 32767u && agc_level(0, w) == 0u);
        CHECK(agc_level(((uint64_t)W * 300u * 300u), w) == 300u);
    }
    for (int32_t x : {-32768, -32767, -1, 0, 1, 32767})
        for (int32_t g : {1, 4095, 4096, 4097, 65535}) {
            const int64_t wide = (int64_t)x * g + 2048;
            CHECK(wide < (1ll << 31) && wide >= -(1ll << 31));
            const int64_t v = wide >> 12, y = v < -32768 ? -32768 : v > 32767 ? 32767 : v;
            uint32_t clip = 7;
            CHECK(agc_sample(x, g, &clip) == y && clip == (y != v ? 1u : 0u));
            if (g == 4096)
                CHECK(y == x && clip == 0);
        }
}

// ---- a stream, frame by frame: the header's statement
struct ByFrame {
    uint32_t C = 0, w = 0;
    uint64_t n = 0;
    std::vector<uint64_t> sum;
    uint32_t a_lo = 0, a_hi = 0, level = 0;
    uint64_t clips = 0;
    void frame(const int16_t *x, int16_t *y, const AgcParams &p)
    {
        const uint32_t W = 1u << w, j = (uint32_t)n & (W - 1u);
        if (n == 0) {
            a_lo = a_hi = p.initial;
            level = 0;
            sum.assign(C, 0);
        } else if (j == 0) {                                             // frame k W, k >= 1
            const uint32_t next = agc_step(a_hi, level, p);
            a_lo = a_hi;
            a_hi = next;
        }
        const int32_t g = agc_gain(a_lo, a_hi, j, w);
        for (uint32_t c = 0; c < C; c++) {
            uint32_t clip;
            y[c] = (int16_t)agc_sample(x[c], g, &clip);
            clips += clip;
            sum[c] += (uint64_t)((int64_t)x[c] * x[c]);
        }
        n++;
        if ((n & (W - 1u)) == 0) {
            uint64_t E = 0;
            for (uint32_t c = 0; c < C; c++) {
                E = sum[c] > E ? sum[c] : E;
                sum[c] = 0;
            }
            level = agc_level(E, w);
        }
    }
};

// ---- the same stream, run by run as the three kernels cut it
struct ByRun {
    uint32_t C = 0, w = 0, max_frames = 0;
    uint64_t pos = 0;
    std::vector<uint64_t> psum;
    uint32_t a_lo = 0, a_hi = 0, level = 0;
    uint64_t clips = 0;
    void run(const int16_t *x, int16_t *y, uint32_t count, const AgcParams &p)
    {
        if (count == 0)
            return;
        const AgcPlan pl = plan_agc(1, C, w, max_frames, count);
        std::vector<uint64_t> table((size_t)pl.nw * C, 0);
        std::vector<uint32_t> nodes(pl.nw + 1u, 0);
        // energy: tile by tile, in a shuffled order
        std::vector<uint32_t> order(pl.chunks);
        for (uint32_t t = 0; t < pl.chunks; t++)
            order[t] = t;
        for (uint32_t t = pl.chunks; t > 1; t--) {
            const uint32_t o = rnd() % t, tmp = order[o];
            order[o] = order[t - 1];
            order[t - 1] = tmp;
        }
        for (uint32_t t : order) {
            const AgcTile tl = agc_tile((uint32_t)pos, count, w, pl.tile_log2, t);
            for (uint32_t f = tl.fa; f < tl.fb; f++)
                for (uint32_t c = 0; c < C; c++)
                    table[(size_t)tl.win * C + c] += (uint64_t)((int64_t)x[f * C + c] * x[f * C + c]);
        }
        // step
        psum.resize(C, 0);
        const bool fresh = pos == 0, carried = (pos & ((1u << w) - 1u)) != 0;
        if (fresh) {
            a_lo = a_hi = p.initial;
            level = 0;
        }
        const AgcRun r = agc_run(pos, count, w);
        CHECK(r.nwin <= pl.nw);
        for (uint32_t i = 0; i < r.nwin; i++) {
            if ((i > 0 || !carried) && r.first + i >= 1u) {
                const uint32_t next = agc_step(a_hi, level, p);
                a_lo = a_hi;
                a_hi = next;
            }
            nodes[i] = a_lo;
            nodes[i + 1u] = a_hi;
            uint64_t E = 0;
            for (uint32_t c = 0; c < C; c++) {
                const uint64_t e = table[(size_t)i * C + c] + (i == 0 && carried ? psum[c] : 0u);
                if (i >= r.complete)
                    psum[c] = e;
                E = e > E ? e : E;
            }
            if (i < r.complete)
                level = agc_level(E, w);
        }
        // apply
        for (uint32_t t : order) {
            const AgcTile tl = agc_tile((uint32_t)pos, count, w, pl.tile_log2, t);
            for (uint32_t f = tl.fa; f < tl.fb; f++) {
                const int32_t g = agc_gain(nodes[tl.win], nodes[tl.win + 1u], tl.j + (f - tl.fa), w);
                for (uint32_t c = 0; c < C; c++) {
                    uint32_t clip;
                    y[f * C + c] = (int16_t)agc_sample(x[f * C + c], g, &clip);
                    clips += clip;
                }
            }
        }
        pos += count;
    }
};

static void test_walk(uint32_t C, uint32_t w)
{
    const uint32_t W = 1u << w, max_frames = 5u * W + 3u, total = 40u * W + pick(0, W);
    std::vector<int16_t> x((size_t)total * C), ya(x.size()), yb(x.size());
    for (uint32_t f = 0; f < total; f++) {
        const int amp = (f / (3u * W)) % 3u == 0 ? 30 : (f / (3u * W)) % 3u == 1 ? 30000 : 3000;
        for (uint32_t c = 0; c < C; c++)
            x[(size_t)f * C + c] = (int16_t)((int)(rnd() % (2u * (uint32_t)amp + 1u)) - amp);
    }
    AgcParams p = {3277, 100, 1024, 40000, 9000, 20000, 4096};
    ByFrame a;
    a.C = C;
    a.w = w;
    ByRun b;
    b.C = C;
    b.w = w;
    b.max_frames = max_frames;
    uint32_t at = 0;
    while (at < total) {
        static const uint32_t lens[] = {0, 1, 63, 64, 65, 323, 7, 8, 9, 200};
        uint32_t len = lens[rnd() % 10u] * (W / 64u) + rnd() % 3u;
        len = len > max_frames ? max_frames : len;
        len = len > total - at ? total - at : len;
        if (rnd() % 4u == 0) {
            p.rise = (uint16_t)pick(0, 65535);
            p.fall = (uint16_t)pick(0, 65535);
            p.gate = (uint16_t)pick(0, 400);
        }
        for (uint32_t f = 0; f < len; f++)
            a.frame(&x[(size_t)(at + f) * C], &ya[(size_t)(at + f) * C], p);
        b.run(&x[(size_t)at * C], &yb[(size_t)at * C], len, p);
        at += len;
        CHECK(a.n == b.pos && a.clips == b.clips && a.a_lo == b.a_lo && a.a_hi == b.a_hi && a.level == b.level);
    }
    CHECK(ya == yb);
}

int main(int argc, char **argv)
{
    const unsigned long iterations = argc > 1 ? strtoul(argv[1], nullptr, 10) : 200;
    const unsigned long steps = test_step();
    const unsigned long plans = test_run_plan(6);
    test_bounds();
    // tiles: every start position mod W and the run lengths around the tile and the window, at w = 6, every channel count
    unsigned long tiles = 0;
    for (uint32_t C = 1; C <= AGC_MAX_CH; C++)
        for (uint32_t j0 = 0; j0 < 64; j0++)
            for (uint32_t count : {0u, 1u, 2u, 7u, 8u, 9u, 63u, 64u, 65u, 127u, 128u, 129u, 193u, 323u}) {
                check_tiles(C, 6, (uint64_t)pick(0, 9) * 64u + j0, count, 323);
                tiles++;
            }
    for (iteration = 0; iteration < iterations; iteration++) {
        const uint32_t C = pick(1, AGC_MAX_CH), w = pick(AGC_W_MIN, AGC_W_MAX);
        const uint32_t max_frames = pick(1, 40000), count = pick(0, max_frames);
        check_tiles(C, w, ((uint64_t)rnd() << 20) ^ rnd(), count, max_frames);
        tiles++;
    }
    for (uint32_t C : {1u, 2u, 3u, 6u, 16u})
        for (uint32_t w : {6u, 8u})
            test_walk(C, w);
    // refused geometries and the grid's limit
    CHECK(plan_agc(0, 2, 6, 64, 8).grid == 0 && plan_agc(3, 0, 6, 64, 8).grid == 0 && plan_agc(3, 17, 6, 64, 8).grid == 0);
    CHECK(plan_agc(3, 2, 5, 64, 8).grid == 0 && plan_agc(3, 2, 15, 64, 8).grid == 0 && plan_agc(3, 2, 6, 0, 0).grid == 0);
    CHECK(plan_agc(3, 2, 6, 1ull << 30, 8).grid == 0 && plan_agc(3, 2, 6, 64, 0).grid == 0 && plan_agc(3, 2, 6, 64, 0).nw == 3);
    CHECK(plan_agc(1u << 20, 1, 6, 1u << 21, 1u << 21).err == 1 && plan_agc(1u << 20, 1, 14, 1u << 21, 1u << 21).err == 0);
    printf("agc plan ok: %lu steps, %lu run plans, %lu tilings\n", steps, plans, tiles);
    return 0;
}
