// automix_plan_test.cpp -- csrc/automix_plan.h, compiled by g++ alone (no HIP):
//   - automix_power and automix_share against a restatement in 128-bit integers (the root by bisection) over a grid that
//     takes every branch: V above, below and equal to P; shifts 0 and 8; m = 0, 1 and 2^30; u = 0, 1, 4095 and 4096; a sum
//     of 0; a single member; a floor above the share; 0 <= P <= 2^38, the quotient <= 2^24, and with floors 0 the squares
//     of a group's D sum to at most 2^24;
//   - the record: pack and unpack, the count and the position in the leveller's places;
//   - the mirror: through any sequence of set_group, reset and run a group stays on one clock, unequal counts are refused
//     and name two members of one group, a refused run changes nothing;
//   - a group walked run by run as k_automix_level and k_automix_share walk it (the table's sums taken per run's window,
//     the carried partial window, the groups' sums cleared per run, the nodes table) equals the group walked window by
//     window, whatever the cuts.
//   usage: automix_plan_test [iterations]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "automix_plan.h"

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

typedef __int128 i128;

// floor(a / 2^sh) of a signed value, without a shift of a negative number
static i128 floor_shift(i128 a, unsigned sh)
{
    const i128 d = (i128)1 << sh;
    i128 q = a / d;
    if (a % d != 0 && a < 0)
        q -= 1;
    return q;
}

static i128 power_model(i128 P, i128 m, const AutomixParams &p)
{
    const i128 v = (m * p.weight) / 4096, V = v * 256;
    const unsigned sh = V > P ? p.attack : p.release;
    return P + floor_shift(V - P, sh);
}

static i128 root_model(i128 q)                        // the largest r with r r <= q
{
    i128 lo = 0, hi = 1 << 13;
    while (lo < hi) {
        const i128 mid = (lo + hi + 1) / 2;
        if (mid * mid <= q)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

static i128 share_model(i128 P, i128 sum, i128 floor, i128 before)
{
    if (sum == 0)
        return before;
    const i128 q = (P * ((i128)1 << 24)) / sum;
    CHECK(q <= ((i128)1 << 24));
    const i128 D = root_model(q);
    return D > floor ? D : floor;
}

static void test_arithmetic(unsigned long iterations)
{
    const uint32_t ms[] = {0, 1, 2, 4095, 4096, 4097, 1u << 20, (1u << 30) - 1u, 1u << 30};
    const uint16_t us[] = {0, 1, 4095, 4096, 2048, 77};
    const uint16_t shs[] = {0, 1, 8, 3};
    unsigned long above = 0, below = 0, equal = 0;
    for (uint32_t m : ms)
        for (uint16_t u : us)
            for (uint16_t at : shs)
                for (uint16_t re : shs) {
                    const AutomixParams p = {u, 0, at, re, 4096};
                    CHECK(automix_params_ok(p));
                    const uint64_t V = (((uint64_t)m * u) >> 12) << 8;
                    const uint64_t Ps[] = {0, 1, V, V ? V - 1 : 0, V + 1, V / 2, 1ull << 38, (1ull << 38) - 1, 255, 256, 257};
                    for (uint64_t P : Ps) {
                        if (P > (1ull << 38))
                            continue;
                        const uint64_t got = automix_power(P, m, p);
                        CHECK((i128)got == power_model(P, m, p));
                        CHECK(got <= (1ull << 38));
                        above += V > P;
                        below += V < P;
                        equal += V == P;
                        if (V > P)
                            CHECK(got >= P && got <= V);                 // towards V, never past it
                        if (V < P)
                            CHECK(got < P && got >= V);
                        if (V == P)
                            CHECK(got == P);
                        if ((V > P ? at : re) == 0)
                            CHECK(got == V);
                    }
                }
    CHECK(above && below && equal);
    CHECK(automix_power(0, 1u << 30, AutomixParams{4096, 0, 0, 0, 0}) == 1ull << 38);
    CHECK(automix_mean((uint64_t)16384 << 30, 14) == 1u << 30 && automix_mean(63, 6) == 0);

    // the share: the figures, the corners, and random groups
    CHECK(automix_share(0, 0, 5, 1234) == 1234 && automix_share(0, 0, 4096, 0) == 0);            // a sum of 0 keeps D
    CHECK(automix_share(1, 1, 0, 7) == 4096 && automix_share(1ull << 38, 1ull << 38, 0, 7) == 4096);   // a single member
    CHECK(automix_share(0, 1, 0, 7) == 0 && automix_share(0, 5, 300, 7) == 300);                 // silent beside a talker
    const uint32_t want[] = {4096, 2896, 2364, 2048};
    for (uint64_t n = 1; n <= 4; n++)
        for (uint64_t P : {1ull, 1000ull, 123456789ull, 1ull << 38})
            CHECK(automix_share(P, n * P, 0, 0) == want[n - 1]);
    CHECK(automix_share(1000, 4000, 3000, 0) == 3000 && automix_share(1000, 4000, 2048, 0) == 2048 &&
          automix_share(1000, 4000, 2049, 0) == 2049);                                           // a floor above the share
    for (iteration = 0; iteration < iterations * 10ul; iteration++) {
        const uint32_t n = pick(1, 8);
        uint64_t P[8], sum = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t kind = pick(0, 5);
            P[i] = kind == 0 ? 0 : kind == 1 ? 1ull << 38 : kind == 2 ? pick(0, 300) : (((uint64_t)rnd() << 7) ^ rnd()) & ((1ull << 38) - 1u);
            CHECK(P[i] <= 1ull << 38);
            sum += P[i];
        }
        uint64_t squares = 0;
        const uint32_t floor = pick(0, 3) ? 0 : pick(0, 4096);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t before = pick(0, 4096), D = automix_share(P[i], sum, floor, before);
            CHECK((i128)D == share_model(P[i], sum, floor, before));
            CHECK(D <= 4096);
            const uint32_t bare = automix_share(P[i], sum, 0, 0);
            squares += (uint64_t)bare * bare;
        }
        CHECK(squares <= 1ull << 24);                                    // with floors 0: never more than one microphone
    }
}

static void test_record()
{
    const AutomixParams p = {4095, 513, 8, 7, 4096};
    AutomixMirror mr;
    mr.init(3, p);
    mr.set_group(1, 2);
    mr.pos[1] = 0x123456789abcull;
    uint32_t rec[AGC_REC];
    mr.record(1, 77, rec);
    CHECK(rec[AREC_COUNT] == 77 && rec[AREC_POS_LO] == 0x56789abcu && rec[AREC_POS_HI] == 0x1234u && rec[XREC_GROUP] == 2);
    const AutomixParams q = automix_unpack(rec);
    CHECK(q.weight == 4095 && q.floor == 513 && q.attack == 8 && q.release == 7 && q.initial == 4096);
    mr.record(0, 0, rec);
    CHECK(rec[XREC_GROUP] == AUTOMIX_NO_GROUP && rec[7] == 0);
    for (const AutomixParams &bad : {AutomixParams{4097, 0, 0, 0, 0}, AutomixParams{0, 4097, 0, 0, 0}, AutomixParams{0, 0, 9, 0, 0},
                                     AutomixParams{0, 0, 0, 9, 0}, AutomixParams{0, 0, 0, 0, 4097}})
        CHECK(!automix_params_ok(bad));
    CHECK(automix_params_ok(AutomixParams{0, 0, 0, 0, 0}) && automix_params_ok(AutomixParams{4096, 4096, 8, 8, 4096}));
}

// the mirror's invariant: the members of a group have one position
static void one_clock(const AutomixMirror &mr)
{
    const size_t S = mr.pos.size();
    for (size_t a = 0; a < S; a++)
        for (size_t b = a + 1; b < S; b++)
            if (mr.group[a] != AUTOMIX_NO_GROUP && mr.group[a] == mr.group[b])
                CHECK(mr.pos[a] == mr.pos[b]);
}

static void test_mirror(unsigned long iterations)
{
    for (iteration = 0; iteration < iterations; iteration++) {
        const size_t S = pick(1, 9);
        AutomixMirror mr;
        mr.init(S, AutomixParams{4096, 0, 0, 0, 4096});
        std::vector<uint32_t> counts(S);
        for (unsigned step = 0; step < 60; step++) {
            const uint32_t what = pick(0, 9);
            const size_t s = pick(0, (uint32_t)S - 1u);
            if (what < 3) {
                const uint32_t g = pick(0, 3) ? pick(0, (uint32_t)S - 1u) : AUTOMIX_NO_GROUP, old = mr.group[s];
                const std::vector<uint64_t> before = mr.pos;
                mr.set_group(s, g);
                CHECK(mr.group[s] == g && mr.pos[s] == 0);
                for (size_t j = 0; j < S; j++) {                         // the group left and the group joined restart,
                    const bool touched = j == s || (old != AUTOMIX_NO_GROUP && mr.group[j] == old) ||
                                         (g != AUTOMIX_NO_GROUP && mr.group[j] == g);
                    CHECK(mr.pos[j] == (touched ? 0 : before[j]));       // nobody else
                }
            } else if (what == 3) {
                const std::vector<uint64_t> before = mr.pos;
                mr.reset(s);
                for (size_t j = 0; j < S; j++) {
                    const bool same = j == s || (mr.group[s] != AUTOMIX_NO_GROUP && mr.group[j] == mr.group[s]);
                    CHECK(mr.pos[j] == (same ? 0 : before[j]));
                }
            } else {
                // a run: counts per group, now and then one member out of step
                for (size_t j = 0; j < S; j++)
                    counts[j] = pick(0, 200);
                for (size_t j = 0; j < S; j++)
                    for (size_t i = 0; i < j; i++)
                        if (mr.group[j] != AUTOMIX_NO_GROUP && mr.group[i] == mr.group[j])
                            counts[j] = counts[i];
                bool spoiled = false;
                if (pick(0, 3) == 0 && mr.group[s] != AUTOMIX_NO_GROUP) {
                    for (size_t j = 0; j < S; j++)
                        spoiled = spoiled || (j != s && mr.group[j] == mr.group[s]);
                    if (spoiled)
                        counts[s] += 1;
                }
                size_t a = S, b = S;
                const bool ok = mr.counts_agree([&](size_t j) { return counts[j]; }, &a, &b);
                CHECK(ok == !spoiled);
                for (size_t j = 0; j < S; j++)
                    CHECK(mr.seen[j] == AUTOMIX_NO_GROUP);               // the check leaves its scratch clean
                if (!ok) {
                    CHECK(a < b && b < S && mr.group[a] == mr.group[b] && mr.group[a] != AUTOMIX_NO_GROUP && counts[a] != counts[b]);
                    CHECK(a == s || b == s);
                } else {
                    for (size_t j = 0; j < S; j++)
                        mr.advance(j, counts[j]);
                }
            }
            one_clock(mr);
        }
    }
}

// ---- a group run by run, as the kernels walk it, against the group window by window
struct Member {
    AutomixParams p;
    std::vector<uint32_t> m;       // per window of the stream: E >> w is all the walk needs
    // window by window
    std::vector<uint32_t> D;       // D[k]
    std::vector<uint64_t> P;
    // run by run (AutomixState)
    uint64_t psum, power;
    uint32_t a_lo, a_hi, pending;
};

static void test_walk(unsigned long iterations)
{
    const uint32_t w = 6, W = 64;
    for (iteration = 0; iteration < iterations; iteration++) {
        const uint32_t n = pick(1, 5), windows = pick(1, 12), max_frames = 5 * W + 3, nw = agc_table_windows(max_frames, w);
        std::vector<Member> g(n);
        for (Member &t : g) {
            t.p = AutomixParams{(uint16_t)(pick(0, 3) ? 4096 : pick(0, 4096)), (uint16_t)(pick(0, 2) ? 0 : pick(0, 4096)),
                                (uint16_t)pick(0, 8), (uint16_t)pick(0, 8), (uint16_t)pick(0, 4096)};
            for (uint32_t k = 0; k < windows; k++)
                t.m.push_back(pick(0, 2) ? pick(0, 1u << 30) : 0);
        }
        // window by window: the header's lines
        std::vector<uint64_t> P(n, 0);
        std::vector<uint32_t> D(n);
        for (uint32_t i = 0; i < n; i++)
            D[i] = g[i].p.initial;
        for (uint32_t k = 0; k < windows; k++) {
            uint64_t sum = 0;
            for (uint32_t i = 0; i < n; i++)
                sum += P[i] = automix_power(P[i], g[i].m[k], g[i].p);
            for (uint32_t i = 0; i < n; i++) {
                D[i] = automix_share(P[i], sum, g[i].p.floor, D[i]);
                g[i].D.push_back(D[i]);
                g[i].P.push_back(P[i]);
            }
        }
        // run by run.  A frame of window k carries E = m[k] << w in its first frame and nothing in the others, so that a
        // window cut anywhere behind its first frame needs the carried sums.
        uint64_t pos = 0;
        const uint64_t total = (uint64_t)windows * W - pick(0, W - 1);
        std::vector<uint64_t> gsum(nw), table(n * nw, 0), power(n * nw);
        while (pos < total) {
            uint32_t count = pick(0, 4) ? pick(0, max_frames) : pick(0, 3);
            if (count > total - pos)
                count = (uint32_t)(total - pos);
            const AgcRun r = agc_run(pos, count, w);
            CHECK(r.nwin <= nw);
            gsum.assign(nw, 0);                                          // cleared in front of every run
            const bool carried = (pos & (W - 1)) != 0;
            for (uint32_t i = 0; i < n; i++)                             // energy: a window's first frame, where the run has it
                for (uint64_t f = pos; f < pos + count; f++)
                    if ((f & (W - 1)) == 0)
                        table[i * nw + (uint32_t)((f >> w) - r.first)] += (uint64_t)g[i].m[f >> w] << w;
            for (uint32_t i = 0; i < n && count; i++) {                  // level
                Member &t = g[i];
                uint64_t Pl = pos == 0 ? 0 : t.power;
                for (uint32_t k = 0; k < r.nwin; k++) {
                    const uint64_t E = table[i * nw + k] + (k == 0 && carried ? t.psum : 0);
                    table[i * nw + k] = 0;
                    if (k < r.complete) {
                        Pl = automix_power(Pl, automix_mean(E, w), t.p);
                        power[i * nw + k] = Pl;
                        gsum[k] += Pl;
                    } else {
                        t.psum = E;
                    }
                }
                t.power = Pl;
            }
            for (uint32_t i = 0; i < n && count; i++) {                  // share
                Member &t = g[i];
                if (pos == 0)
                    t.a_lo = t.a_hi = t.pending = t.p.initial;
                for (uint32_t k = 0; k < r.nwin; k++) {
                    if ((k > 0 || !carried) && r.first + k >= 1) {
                        t.a_lo = t.a_hi;
                        t.a_hi = t.pending;
                    }
                    const uint64_t win = r.first + k;
                    // the nodes of window `win`: A[win] and A[win + 1] of the header
                    const uint32_t want_lo = win < 2 ? t.p.initial : t.D[win - 2], want_hi = win < 1 ? t.p.initial : t.D[win - 1];
                    CHECK(t.a_lo == want_lo && t.a_hi == want_hi);
                    if (k < r.complete)
                        t.pending = automix_share(power[i * nw + k], gsum[k], t.p.floor, t.pending);
                }
            }
            pos += count;
            for (uint32_t i = 0; i < n; i++) {
                const uint64_t done = pos >> w;                          // complete windows so far
                if (pos && done) {
                    CHECK(g[i].power == g[i].P[done - 1] && g[i].pending == g[i].D[done - 1]);
                }
            }
        }
        for (uint64_t v : table)
            CHECK(v == 0);
    }
}

int main(int argc, char **argv)
{
    const unsigned long iterations = argc > 1 ? strtoul(argv[1], nullptr, 10) : 2000ul;
    test_arithmetic(iterations);
    test_record();
    test_mirror(iterations);
    test_walk(iterations);
    printf("automix plan ok: %lu iterations\n", iterations);
    return 0;
}
