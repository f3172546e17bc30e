// denoise_plan_test.cpp -- csrc/denoise_plan.h compiled by g++ alone (no HIP).
//   - the target rule on its edges (p = 0, p = t, p = t + 1, p at 2^34 +- 1 and at 2^45, beta = 0 and 255, the largest
//     profile) against a second statement in 128-bit integers with a root found by bisection;
//   - the smoothing: from every distance and with every shift a gain reaches its target exactly, never passes it, and a
//     shift of 0 is instant;
//   - sat32 and the rounding of an inverse butterfly at the int32 rails;
//   - the block reference (denoise_block_ref) against a second statement that walks a block the way k_denoise.hip does:
//     butterflies numbered 0 .. H - 1 over padded planes, the mirrored write of the removed spectrum in place, the
//     pairwise bit-reversal swap -- every index under the sanitizers;
//   - rows walked the way the kernel walks them (outputs in front of the first block from the tail, blocks, the
//     history rewritten) over random cuts, against the whole stream in one piece stated by absolute frames, with the
//     mirror's back, fresh, learn and cnt doing the bookkeeping: sets, learning on and off and resets at the same frames.
//   usage: denoise_plan_test [random cuts per size]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "denoise_plan.h"

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

// ---------------------------------------------------------------------------
// the target rule, stated again

static uint32_t root_by_bisection(uint64_t v)
{
    uint64_t lo = 0, hi = 1ull << 16;                // v <= 2^30
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        if (mid * mid <= v)
            lo = mid;
        else
            hi = mid - 1;
    }
    return (uint32_t)lo;
}

static uint32_t target_again(uint64_t p, uint64_t np, uint32_t over, uint32_t floor)
{
    const unsigned __int128 t = ((unsigned __int128)np * over) >> 4;
    if ((unsigned __int128)p <= t)
        return floor;
    uint32_t bits = 0;
    while (bits < 64 && (p >> bits))
        bits++;
    const uint32_t sh = bits > 34 ? bits - 34 : 0;
    const unsigned __int128 ps = p >> sh, ts = t >> sh;
    const uint32_t r = root_by_bisection((uint64_t)(((ps - ts) << 30) / ps));
    return r > floor ? r : floor;
}

static void target_edges()
{
    const uint64_t nps[] = {0, 1, 15, 16, 17, 1000, (1ull << 34) - 1, 1ull << 34, (1ull << 34) + 1, 1ull << 45,
                            (1ull << 52) - 1, 1ull << 52};
    const uint32_t overs[] = {0, 1, 15, 16, 17, 64, 255}, floors[] = {0, 1, 4125, 32767, 32768};
    unsigned long n = 0;
    for (uint64_t np : nps)
        for (uint32_t over : overs)
            for (uint32_t floor : floors) {
                const uint64_t t = (np * over) >> 4;
                const uint64_t ps[] = {0, 1, t, t + 1, t + 2, 2 * t, 2 * t + 1, (1ull << 34) - 1, 1ull << 34, (1ull << 34) + 1,
                                       1ull << 45, (1ull << 45) + 12345, (1ull << 46) - 1, t > 0 ? t - 1 : 0};
                for (uint64_t p : ps) {
                    const uint32_t g = denoise_target(p, np, over, floor);
                    CHECK(g == target_again(p, np, over, floor));
                    CHECK(g >= floor && g <= DENOISE_UNITY);
                    if (p <= t)
                        CHECK(g == floor);
                    if (over == 0 && p > 0)
                        CHECK(g == DENOISE_UNITY);  // nothing to subtract: (p << 30) / p is 2^30
                    n++;
                }
            }
    for (iteration = 0; iteration < 200000; iteration++) {
        const uint64_t p = (((uint64_t)rnd() << 32) | rnd()) >> (18 + rnd() % 46);
        const uint64_t np = (((uint64_t)rnd() << 32) | rnd()) >> (12 + rnd() % 52);
        const uint32_t over = rnd() % 256, floor = rnd() % 32769;
        CHECK(np <= DENOISE_NP_MAX && denoise_target(p, np, over, floor) == target_again(p, np, over, floor));
    }
    CHECK(denoise_bitlength(0) == 0 && denoise_bitlength(1) == 1 && denoise_bitlength(1ull << 34) == 35 &&
          denoise_bitlength(~0ull) == 64);
    printf("  target: %lu edge cases and 200000 random ones\n", n);
}

static void smoothing()
{
    for (uint32_t shift = 0; shift <= DENOISE_SHIFT_MAX; shift++)
        for (uint32_t from : {0u, 1u, 4125u, 32767u, 32768u})
            for (uint32_t to : {0u, 1u, 4124u, 4125u, 4126u, 32768u}) {
                uint32_t g = from, steps = 0;
                while (g != to) {
                    const uint32_t next = denoise_smooth(g, to, shift, shift);
                    CHECK(next != g && (from <= to ? next > g && next <= to : next < g && next >= to));   // no dead band
                    g = next;
                    CHECK(++steps <= 32768u);
                }
                CHECK(denoise_smooth(g, to, shift, shift) == to);
                if (shift == 0)
                    CHECK(steps <= 1);
            }
    // the two directions take their own shift
    CHECK(denoise_smooth(0, 32768, 3, 0) == 4096 && denoise_smooth(32768, 0, 3, 0) == 0);
    CHECK(denoise_smooth(0, 32768, 0, 3) == 32768 && denoise_smooth(32768, 0, 0, 3) == 28672);
    CHECK(denoise_smooth(100, 103, 8, 8) == 101 && denoise_smooth(103, 100, 8, 8) == 102);
}

static void rails()
{
    uint32_t sat = 0;
    CHECK(denoise_sat32(2147483647ll, &sat) == 2147483647 && sat == 0);
    CHECK(denoise_sat32(2147483648ll, &sat) == 2147483647 && sat == 1);
    CHECK(denoise_sat32(-2147483648ll, &sat) == (int32_t)(-2147483648ll) && sat == 1);
    CHECK(denoise_sat32(-2147483649ll, &sat) == (int32_t)(-2147483648ll) && sat == 2);
    CHECK(denoise_sat32((int64_t)1 << 62, &sat) == 2147483647 && sat == 3);
    // an inverse butterfly at the rails: a = 2^31 - 1, P = +-(2^31 - 1) 2^30
    const int64_t a30 = (int64_t)2147483647 * SPEC_ONE + (SPEC_ONE >> 1), P = (int64_t)2147483647 * SPEC_ONE;
    sat = 0;
    CHECK(denoise_inv_round(a30, P, &sat) == 2147483647 && sat == 1);
    CHECK(denoise_inv_round(a30, -P, &sat) == 0 && sat == 1);
    CHECK(denoise_inv_round(-a30, -P, &sat) == (int32_t)(-2147483648ll) && sat == 2);     // about -2^32: the lower rail
    // rounding: (a 2^30 + 2^29) >> 30 = a, halves go up
    CHECK(denoise_inv_round((int64_t)5 * SPEC_ONE + (SPEC_ONE >> 1), (SPEC_ONE >> 1), &sat) == 6);
    CHECK(denoise_inv_round((int64_t)5 * SPEC_ONE + (SPEC_ONE >> 1), -(SPEC_ONE >> 1) - 1, &sat) == 4);
    CHECK(denoise_inv_round((int64_t)-5 * SPEC_ONE + (SPEC_ONE >> 1), -(SPEC_ONE >> 1), &sat) == -5);
    CHECK(denoise_removed(1 << 30, 0) == 1 << 28 && denoise_removed(-(1 << 30), 0) == -(1 << 28) &&
          denoise_removed(12345678, DENOISE_UNITY) == 0 && denoise_removed(-3, 0) == -1 && denoise_removed(-2, 0) == 0);
    uint32_t clip = 0;
    CHECK(denoise_out(32767, -1, &clip) == 32767 && clip == 1 && denoise_out(-32768, 1, &clip) == -32768 && clip == 2 &&
          denoise_out(100, 30, &clip) == 70 && clip == 2);
    CHECK(denoise_r(4095) == 0 && denoise_r(4096) == 1 && denoise_r(-4097) == -1 && denoise_r(-4096) == 0);
    CHECK(denoise_synth(1 << 15, 1) == 1 && denoise_synth(-(1 << 14) - 1, 1) == -1 && denoise_synth(-(1 << 14), 1) == 0);
    const DenoiseParams p = {4125, 64, 1, 2};
    const DenoiseParams q = denoise_unpack(denoise_pack(p));
    CHECK(q.floor == 4125 && q.over == 64 && q.rise_shift == 1 && q.fall_shift == 2);
    const DenoiseParams top = {32768, 255, 8, 8};
    const DenoiseParams back = denoise_unpack(denoise_pack(top));
    CHECK(back.floor == 32768 && back.over == 255 && back.rise_shift == 8 && back.fall_shift == 8 && denoise_params_ok(back));
    const DenoiseParams bad = {32768, 0, 9, 0};
    CHECK(!denoise_params_ok(bad));
}

// ---------------------------------------------------------------------------
// a block the way the kernel walks it

struct Tables {
    uint32_t n, N, H;
    std::vector<int16_t> sw;
    std::vector<int32_t> wr, wi;
    explicit Tables(uint32_t n_) : n(n_), N(1u << n_), H(N / 2), sw(N), wr(H), wi(H)
    {
        denoise_window(n, sw.data());
        spec_twiddles(n, wr.data(), wi.data());
        CHECK(sw[0] == 0 && sw[H] == 32767);
        for (uint32_t i = 1; i < N; i++)
            CHECK(sw[i] == sw[N - i] && sw[i] > 0);
    }
};

static uint32_t pad(uint32_t i) { return i + (i >> 5); }
static uint32_t brev(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t b = 0; b < n; b++)
        r |= ((v >> b) & 1u) << (n - 1 - b);
    return r;
}

// x[N] -> c[N]; g, np, acc updated; returns the clamps.  Planes of N + N / 32 words exactly, as the kernel's.
static uint32_t block_as_kernel(const Tables &T, const int16_t *x, const DenoiseParams &par, bool learn, uint32_t *cnt,
                                uint32_t *g, uint64_t *np, uint64_t *acc, int32_t *c)
{
    const uint32_t n = T.n, N = T.N, H = T.H;
    std::vector<int32_t> zr(N + N / 32), zi(N + N / 32);
    for (uint32_t t = 0; t < N; t++) {
        zr[pad(brev(t, n))] = (int32_t)x[t] * T.sw[t];
        zi[pad(brev(t, n))] = 0;
    }
    for (uint32_t st = 1; st <= n; st++) {
        const uint32_t h = 1u << (st - 1);
        for (uint32_t b = 0; b < H; b++) {
            const uint32_t j = b & (h - 1u), ia = pad(((b >> (st - 1)) << st) + j), ib = pad(((b >> (st - 1)) << st) + j + h);
            const uint32_t kw = j << (n - st);
            const int64_t cr = T.wr[kw], cw = T.wi[kw], br = zr[ib], bi = zi[ib];
            const int64_t pr = br * cr - bi * cw, pi = br * cw + bi * cr;
            const int64_t ar = (int64_t)zr[ia] * SPEC_ONE + SPEC_ONE, ai = (int64_t)zi[ia] * SPEC_ONE + SPEC_ONE;
            zr[ia] = spec_round(ar, pr);
            zr[ib] = spec_round(ar, -pr);
            zi[ia] = spec_round(ai, pi);
            zi[ib] = spec_round(ai, -pi);
        }
    }
    const bool learns = learn && *cnt < DENOISE_CNT_MAX;
    for (uint32_t k = 0; k <= H; k++) {
        const int32_t re = zr[pad(k)], ig = zi[pad(k)];
        const uint64_t p = (uint64_t)((int64_t)re * re + (int64_t)ig * ig) >> 16;
        const uint32_t gk = denoise_smooth(g[k], denoise_target(p, np[k], par.over, par.floor), par.rise_shift, par.fall_shift);
        g[k] = gk;
        if (learns) {
            const uint64_t sum = *cnt ? acc[k] + p : p;
            acc[k] = sum;
            np[k] = sum / (*cnt + 1u);
        }
        const int32_t ur = denoise_removed(re, gk), ui = k == 0 || k == H ? 0 : denoise_removed(ig, gk);
        const uint32_t km = pad((N - k) & (N - 1u));
        zr[pad(k)] = ur;
        zi[pad(k)] = ui;
        zr[km] = ur;
        zi[km] = k == 0 ? 0 : -ui;
    }
    if (learns)
        ++*cnt;
    for (uint32_t t = 0; t < N; t++) {
        const uint32_t r = brev(t, n);
        if (t < r) {
            std::swap(zr[pad(t)], zr[pad(r)]);
            std::swap(zi[pad(t)], zi[pad(r)]);
        }
    }
    uint32_t sat = 0;
    for (uint32_t st = 1; st <= n; st++) {
        const uint32_t h = 1u << (st - 1);
        for (uint32_t b = 0; b < H; b++) {
            const uint32_t j = b & (h - 1u), ia = pad(((b >> (st - 1)) << st) + j), ib = pad(((b >> (st - 1)) << st) + j + h);
            const uint32_t kw = j << (n - st);
            const int64_t cr = T.wr[kw], cw = -(int64_t)T.wi[kw], br = zr[ib], bi = zi[ib];
            const int64_t pr = br * cr - bi * cw, pi = br * cw + bi * cr;
            const int64_t ar = (int64_t)zr[ia] * SPEC_ONE + (SPEC_ONE >> 1), ai = (int64_t)zi[ia] * SPEC_ONE + (SPEC_ONE >> 1);
            zr[ia] = denoise_inv_round(ar, pr, &sat);
            zr[ib] = denoise_inv_round(ar, -pr, &sat);
            zi[ia] = denoise_inv_round(ai, pi, &sat);
            zi[ib] = denoise_inv_round(ai, -pi, &sat);
        }
    }
    for (uint32_t t = 0; t < N; t++)
        c[t] = denoise_synth(zr[pad(t)], T.sw[t]);
    return sat;
}

static void fill_block(std::vector<int16_t> &x, uint32_t kind)
{
    for (size_t i = 0; i < x.size(); i++) {
        const int32_t v = (int32_t)(rnd() & 0xffffu) - 32768;
        x[i] = (int16_t)(kind == 0 ? v : kind == 1 ? v / 64 : (rnd() & 1u) ? 32767 : -32768);
    }
}

static void blocks(uint32_t n)
{
    const Tables T(n);
    const uint32_t N = T.N, H = T.H;
    std::vector<int16_t> x(N);
    std::vector<int32_t> z(2 * N), c1(N), c2(N);
    std::vector<uint64_t> p(H + 1);
    for (iteration = 0; iteration < 6; iteration++) {
        std::vector<uint32_t> g1(H + 1), g2;
        std::vector<uint64_t> np1(H + 1), np2, acc1(H + 1, 7), acc2;
        for (uint32_t k = 0; k <= H; k++) {
            g1[k] = rnd() % 32769;
            np1[k] = iteration & 1 ? ((uint64_t)rnd() << (rnd() % 21)) : (rnd() & 1u) ? DENOISE_NP_MAX : 0;
        }
        g2 = g1, np2 = np1, acc2 = acc1;
        const DenoiseParams par = {(uint16_t)(iteration == 0 ? 32768 : rnd() % 32769), (uint8_t)(rnd() % 256),
                                   (uint8_t)(rnd() % 9), (uint8_t)(rnd() % 9)};
        if (iteration == 0)
            for (auto &v : g1)
                v = DENOISE_UNITY;                  // property 1: unity gains remove nothing
        g2 = g1;
        uint32_t cnt1 = iteration == 2 ? 0 : iteration == 3 ? DENOISE_CNT_MAX : 5, cnt2 = cnt1;
        const bool learn = iteration >= 2;
        fill_block(x, (uint32_t)iteration % 3);
        const uint32_t s1 = denoise_block_ref(n, x.data(), T.sw.data(), T.wr.data(), T.wi.data(), par, learn, &cnt1, g1.data(),
                                              np1.data(), acc1.data(), z.data(), z.data() + N, p.data(), c1.data());
        const uint32_t s2 = block_as_kernel(T, x.data(), par, learn, &cnt2, g2.data(), np2.data(), acc2.data(), c2.data());
        CHECK(s1 == s2 && cnt1 == cnt2 && c1 == c2 && g1 == g2 && np1 == np2 && acc1 == acc2);
        if (iteration == 0)
            for (uint32_t i = 0; i < N; i++)
                CHECK(c1[i] == 0);
        if (iteration == 2)
            for (uint32_t k = 0; k <= H; k++)
                CHECK(acc1[k] == p[k] && np1[k] == p[k] && cnt1 == 1);
        if (iteration == 3)
            CHECK(cnt1 == DENOISE_CNT_MAX && acc1[0] == 7);
    }
}

// ---------------------------------------------------------------------------
// rows under cuts

struct Event {                                       // in front of the run that begins at frame `at`
    uint32_t at;
    int kind;                                        // 0 set, 1 learn on, 2 learn off, 3 reset
    DenoiseParams par;
};

struct RowState {
    std::vector<int16_t> hist;
    std::vector<int32_t> tail;
    std::vector<uint32_t> g;
    std::vector<uint64_t> np, acc;
    explicit RowState(const Tables &T) : hist(T.N, 99), tail(T.N, 99), g(T.H + 1, 99), np(T.H + 1, 0), acc(T.H + 1, 0) {}
};

// one run of a row, as k_denoise.hip: rec is the stream's record
static void row_run(const Tables &T, RowState &R, const uint32_t *rec, const int16_t *in, int16_t *out, uint32_t *sat, uint32_t *clip)
{
    const uint32_t n = T.n, N = T.N, H = T.H;
    const uint32_t count = rec[NREC_COUNT], back = rec[NREC_BACK];
    uint32_t cnt = rec[NREC_CNT];
    const DenoiseParams par = denoise_unpack(rec[NREC_PAR]);
    const bool fresh = rec[NREC_FLAGS] & DENOISE_FRESH, learn = rec[NREC_FLAGS] & DENOISE_LEARN;
    if (count == 0)
        return;
    CHECK(back < N);
    if (fresh) {
        std::fill(R.tail.begin(), R.tail.end(), 0);
        std::fill(R.g.begin(), R.g.end(), DENOISE_UNITY);
    }
    const uint32_t nblk = spec_run_blocks(n, back, count), e0 = N - 1 - back, lim = count < e0 ? count : e0;
    for (uint32_t q = 0; q < lim; q++) {
        const int64_t u = denoise_tail_entry(n, back, q);
        CHECK(u < (int64_t)H && q < N - 1);
        out[q] = denoise_out(fresh ? 0 : R.hist[q], u >= 0 ? R.tail[(size_t)u] : 0, clip);
    }
    std::vector<int16_t> x(N);
    std::vector<int32_t> c(N);
    for (uint32_t i = 0; i < nblk; i++) {
        for (uint32_t t = 0; t < N; t++) {
            const int64_t rel = spec_block_frame(n, back, i, t);
            CHECK(rel < (int64_t)count && rel >= -(int64_t)(N - 1));
            x[t] = rel >= 0 ? in[rel] : fresh ? (int16_t)0 : R.hist[(size_t)((int64_t)N - 1 + rel)];
        }
        *sat += block_as_kernel(T, x.data(), par, learn, &cnt, R.g.data(), R.np.data(), R.acc.data(), c.data());
        const uint32_t ei = e0 + i * H;
        for (uint32_t t = 0; t < H; t++) {
            const int32_t r = denoise_r((int64_t)R.tail[H + t] + c[t]);
            R.tail[H + t] = c[t + H];
            const uint32_t q = ei + t;
            if (q < count) {
                const int64_t rel = (int64_t)q - (int64_t)(N - 1);
                CHECK(rel >= 0 || q < N - 1);
                out[q] = denoise_out(rel >= 0 ? in[rel] : fresh ? 0 : R.hist[q], r, clip);
            } else {
                CHECK(i == nblk - 1);
                R.tail[t] = r;
            }
        }
    }
    std::vector<int16_t> next(N, 99);
    for (uint32_t j = 0; j + 1 < N; j++) {
        const int64_t rel = spec_state_frame(n, count, j);
        CHECK(rel < (int64_t)count && (rel >= 0 || j + count <= N - 2));
        next[j] = rel >= 0 ? in[rel] : fresh ? (int16_t)0 : R.hist[j + count];
    }
    R.hist.swap(next);
}

struct Result {
    std::vector<int16_t> y;
    std::vector<uint32_t> g;
    std::vector<uint64_t> np;
    uint32_t sat = 0, clip = 0, cnt = 0;
    bool operator==(const Result &o) const
    {
        return y == o.y && g == o.g && np == o.np && sat == o.sat && clip == o.clip && cnt == o.cnt;
    }
};

// the stream in runs that end at `ends` (ascending, the last one its length), through the mirror and row_run
static Result walk(const Tables &T, const std::vector<int16_t> &x, const std::vector<uint32_t> &ends, const std::vector<Event> &ev,
                   const std::vector<uint64_t> &profile)
{
    DenoiseMirror M;
    const DenoiseParams def = {32768, 16, 0, 0};
    M.init(1, T.n, def);
    RowState R(T);
    R.np = profile;
    Result res;
    res.y.assign(x.size(), 77);
    uint32_t at = 0;
    size_t e = 0;
    for (uint32_t end : ends) {
        for (; e < ev.size() && ev[e].at <= at; e++) {
            CHECK(ev[e].at == at);                   // every cut list holds the events' frames
            if (ev[e].kind == 0)
                M.par[0] = ev[e].par;
            else if (ev[e].kind == 3)
                M.reset(0);
            else
                M.set_learn(0, ev[e].kind == 1);
        }
        uint32_t rec[DENOISE_REC];
        M.record(0, end - at, rec);
        row_run(T, R, rec, x.data() + at, res.y.data() + at, &res.sat, &res.clip);
        M.advance(0, end - at);
        at = end;
    }
    res.g = M.fresh[0] ? std::vector<uint32_t>(T.H + 1, DENOISE_UNITY) : R.g;
    res.np = R.np;
    res.cnt = M.cnt[0];
    return res;
}

// the same stream in one piece, by absolute frames: every block of a segment between resets on the whole signal
static Result whole(const Tables &T, const std::vector<int16_t> &x, const std::vector<Event> &ev, const std::vector<uint64_t> &profile)
{
    const uint32_t n = T.n, N = T.N, H = T.H, D = N - 1;
    Result res;
    res.y.assign(x.size(), 77);
    res.np = profile;
    std::vector<uint64_t> acc(H + 1, 0), p(H + 1);
    std::vector<int32_t> z(2 * N), c(N);
    DenoiseParams par = {32768, 16, 0, 0};
    bool learn = false;
    size_t e = 0;
    uint32_t seg = 0;                                // the frame the current segment began at
    std::vector<uint32_t> g(H + 1, DENOISE_UNITY);
    std::vector<int64_t> ola;
    auto finish = [&](uint32_t end) {                // outputs of the segment [seg, end)
        for (uint32_t f = seg; f < end; f++) {
            const int64_t m = (int64_t)(f - seg) - D;
            const int32_t xd = m >= 0 ? x[seg + (size_t)m] : 0;
            const int32_t r = m >= 0 ? denoise_r(ola[(size_t)m]) : 0;
            res.y[f] = denoise_out(xd, r, &res.clip);
        }
    };
    uint32_t blocks_done = 0;
    for (uint32_t f = 0; f <= x.size(); f++) {
        // events in front of frame f take effect for every block completed at frame f or later
        for (; e < ev.size() && ev[e].at == f; e++) {
            if (ev[e].kind == 0) {
                par = ev[e].par;
            } else if (ev[e].kind == 3) {
                finish(f);
                seg = f;
                blocks_done = 0;
                ola.clear();
                std::fill(g.begin(), g.end(), DENOISE_UNITY);
                learn = false;
            } else {
                if (ev[e].kind == 1 && !learn)
                    res.cnt = 0;
                learn = ev[e].kind == 1;
            }
        }
        if (f == x.size())
            break;
        // frame f arrives: it may complete block blocks_done of the segment -- but a block uses the parameters in force
        // in the RUN that completes it, and the cut lists hold every event's frame, so "in force at frame f" is that
        const uint32_t len = f + 1 - seg;
        if (len >= N && (len - N) % H == 0) {
            const uint32_t j = (len - N) / H;
            CHECK(j == blocks_done);
            res.sat += denoise_block_ref(n, x.data() + seg + (size_t)j * H, T.sw.data(), T.wr.data(), T.wi.data(), par, learn,
                                         &res.cnt, g.data(), res.np.data(), acc.data(), z.data(), z.data() + N, p.data(), c.data());
            ola.resize((size_t)j * H + N, 0);
            for (uint32_t i = 0; i < N; i++)
                ola[(size_t)j * H + i] += c[i];
            blocks_done++;
        }
    }
    finish((uint32_t)x.size());
    res.g = g;
    return res;
}

static void cuts(uint32_t n, unsigned long random_cuts)
{
    const Tables T(n);
    const uint32_t N = T.N, H = T.H, total = 7 * N + 37;
    std::vector<int16_t> x(total);
    for (uint32_t i = 0; i < total; i++) {
        const int32_t v = (int32_t)(rnd() & 0xffffu) - 32768;
        x[i] = (int16_t)(i < 3 * N ? v / 32 : v);    // quiet while the profile is learned, then loud
    }
    std::vector<uint64_t> profile(H + 1);
    for (auto &v : profile)
        v = (rnd() & 3u) ? (uint64_t)rnd() << 10 : 0;
    const DenoiseParams a = {4125, 64, 1, 2}, b = {0, 255, 0, 0};
    const std::vector<Event> ev = {{0, 0, a}, {H + 3, 1, a}, {3 * N - 1, 2, a}, {4 * N + 1, 0, b}, {5 * N + 5, 3, a}, {5 * N + 5, 1, a}};
    const Result want = whole(T, x, ev, profile);
    CHECK(want.cnt > 0);
    for (iteration = 0; iteration < random_cuts; iteration++) {
        std::vector<uint32_t> ends;
        size_t e = 0;
        uint32_t at = 0;
        while (at < total) {
            uint32_t f = iteration == 0 ? total : iteration == 1 ? 1 + rnd() % 3 : rnd() % (2 * N + 2);
            if (iteration % 5 == 2 && rnd() % 3 == 0)
                f = 0;                               // a run that gives the stream nothing
            uint32_t end = at + f > total ? total : at + f;
            while (e < ev.size() && ev[e].at <= at)
                e++;
            if (e < ev.size() && ev[e].at < end)
                end = ev[e].at;                      // the calls fall between runs
            ends.push_back(end);
            at = end;
        }
        const Result got = walk(T, x, ends, ev, profile);
        CHECK(got == want);
    }
}

int main(int argc, char **argv)
{
    const unsigned long random_cuts = argc > 1 ? strtoul(argv[1], nullptr, 10) : 40;
    target_edges();
    smoothing();
    rails();
    for (uint32_t n = SPEC_MIN_LOG2; n <= SPEC_MAX_LOG2; n++) {
        blocks(n);
        cuts(n, n <= 9 ? random_cuts : n == 10 ? random_cuts / 4 + 3 : 3);
    }
    printf("denoise plan ok: n = %u..%u, %lu random cuts at the small sizes\n", SPEC_MIN_LOG2, SPEC_MAX_LOG2, random_cuts);
    return 0;
}
