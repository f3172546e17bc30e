// split_plan_test.cpp -- csrc/split_plan.h over random and extreme tables, as a stand-alone program: g++ alone compiles
// it (the header includes no HIP), tests/test_split_host.py runs it plainly and under AddressSanitizer + UBSan.
//   split_plan_test [tables]  ->  "groups ok: N tables"
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "split_plan.h"

using namespace cmhip;

#define CHECK(c)                                                                                  \
    do {                                                                                          \
        if (!(c)) {                                                                               \
            fprintf(stderr, "%s:%d: %s (table %lu, T %u, bands %u)\n", __FILE__, __LINE__, #c, n, T, bands); \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

static uint32_t rnd_state = 12345;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

// what the header promises of one table; the groups of filter b are returned in *count
static int check_table(unsigned long n, uint32_t bands, uint32_t T, const std::vector<int16_t> &g, const std::vector<uint8_t> &q,
                       size_t *count)
{
    const uint32_t nf = bands - 1, Tp = split_tp(T);
    CHECK(Tp % 8 == 0 && Tp >= T + 1 && Tp < T + 9);
    std::vector<uint32_t> tab(split_table_words(bands, T), 0xdeadbeefu), ends;
    split_compile(bands, T, g.data(), q.data(), tab.data());
    const uint32_t *pairs = tab.data(), *masks = pairs + nf * (Tp / 2), *qs = masks + nf * (Tp / 8);
    *count = 0;
    for (uint32_t b = 0; b < nf; b++) {
        const int16_t *gb = g.data() + (size_t)b * T;
        split_groups(gb, T, &ends);
        CHECK(!ends.empty() && ends.back() == T);
        uint32_t lo = 0;
        for (size_t i = 0; i < ends.size(); i++) {
            const uint32_t hi = ends[i];
            CHECK(hi > lo && (hi % 2 == 0 || hi == T));                 // covers the taps once, on even boundaries
            uint64_t sum = 0;
            int64_t most = 0, least = 0;                                // the group's extreme sums against any int16 input
            for (uint32_t k = lo; k < hi; k++) {
                sum += split_abs(gb[k]);
                most += gb[k] < 0 ? (int64_t)gb[k] * -32768 : (int64_t)gb[k] * 32767;
                least += gb[k] < 0 ? (int64_t)gb[k] * 32767 : (int64_t)gb[k] * -32768;
            }
            if (sum > SPLIT_GROUP_BOUND) {                              // only the pair of two -32768
                CHECK(hi - lo == 2 && gb[lo] == -32768 && gb[lo + 1] == -32768);
                CHECK(most == 2147483648ll);
            } else {
                CHECK(most < 2147483648ll);
            }
            CHECK(least > -2147483648ll);                               // -2^31 is free to stand for the wrapped +2^31
            // greedy: the next pair would not have fitted
            if (hi < T) {
                const uint64_t next = split_abs(gb[hi]) + (hi + 1 < T ? split_abs(gb[hi + 1]) : 0u);
                CHECK(sum + next > SPLIT_GROUP_BOUND);
            }
            lo = hi;
        }
        *count += ends.size();
        // the table: pairs give the taps back, zero behind T; a mask bit per group end but the last
        for (uint32_t kk = 0; kk < Tp / 2; kk++) {
            const uint32_t w = pairs[b * (Tp / 2) + kk], k = 2 * kk;
            CHECK((int16_t)(w >> 16) == (k < T ? gb[k] : 0) && (int16_t)(w & 0xffffu) == (k + 1 < T ? gb[k + 1] : 0));
        }
        size_t bits = 0, at = 0;
        for (uint32_t kk = 0; kk < Tp / 2; kk++)
            if ((masks[b * (Tp / 8) + kk / 4] >> (kk % 4)) & 1u) {
                CHECK(at + 1 < ends.size() && ends[at] == 2 * (kk + 1));
                at++;
                bits++;
            }
        CHECK(bits + 1 == ends.size());
        // the upper half: the blocks in a row from j on in which no group ends
        for (uint32_t j = 0; j < Tp / 8; j++) {
            const uint32_t w = masks[b * (Tp / 8) + j];
            uint32_t run = 0;
            while (j + run < Tp / 8 && (masks[b * (Tp / 8) + j + run] & 0xffffu) == 0)
                run++;
            CHECK((w & 0xffffu) < 16u && (w >> 16) == run);
        }
        CHECK(qs[b] == q[b]);
    }
    return 0;
}

int main(int argc, char **argv)
{
    const unsigned long tables = argc > 1 ? strtoul(argv[1], nullptr, 10) : 500;
    unsigned long n = 0;
    uint32_t T = 3, bands = 2;
    size_t count = 0;
    CHECK(split_tp(3) == 8 && split_tp(7) == 8 && split_tp(9) == 16 && split_tp(1023) == 1024);
    CHECK(!split_geometry_ok(1, 3) && !split_geometry_ok(9, 3) && !split_geometry_ok(2, 1) && !split_geometry_ok(2, 4));
    CHECK(!split_geometry_ok(2, 1025) && split_geometry_ok(2, 3) && split_geometry_ok(8, 1023));
    // random tables of every magnitude class
    for (n = 0; n < tables; n++) {
        bands = 2 + rnd() % 7;
        T = 3 + 2 * (rnd() % 511);
        const uint32_t cls = rnd() % 5;
        const uint32_t top = cls == 0 ? 4 : cls == 1 ? 64 : cls == 2 ? 1024 : cls == 3 ? 16384 : 65536;
        std::vector<int16_t> g((size_t)(bands - 1) * T);
        std::vector<uint8_t> q(bands - 1);
        for (auto &v : g)
            v = (int16_t)((int)(rnd() % top) - (int)(top / 2));
        if (cls == 4)
            for (uint32_t i = 0; i + 1 < g.size(); i += 2 + rnd() % 9)
                g[i] = g[i + 1] = -32768;                                // pairs, and straddling pairs, of the least tap
        for (auto &v : q)
            v = (uint8_t)(SPLIT_Q_MIN + rnd() % 7);
        if (check_table(n, bands, T, g, q, &count))
            return 1;
    }
    // all taps +-32767: groups of two taps
    for (T = 3; T <= 1023; T += 102) {
        bands = 3;
        std::vector<int16_t> g((size_t)2 * T);
        std::vector<uint8_t> q(2, 20);
        for (uint32_t k = 0; k < T; k++) {
            g[k] = 32767;
            g[T + k] = (int16_t)(k % 2 ? -32767 : 32767);
        }
        if (check_table(n, bands, T, g, q, &count))
            return 1;
        CHECK(count == 2 * (size_t)((T + 1) / 2));
        n++;
    }
    // sum |g| = 65535 exactly: one group; one more: two
    for (T = 3; T <= 1023; T += 20) {
        bands = 2;
        std::vector<int16_t> g(T);
        std::vector<uint8_t> q(1, 14);
        for (uint32_t k = 0; k < T; k++)
            g[k] = (int16_t)((65535 / T + (k < 65535 % T ? 1 : 0)) * (k % 3 ? 1 : -1));
        if (check_table(n, bands, T, g, q, &count))
            return 1;
        CHECK(count == 1);
        g[T - 1] = (int16_t)(g[T - 1] + (g[T - 1] < 0 ? -1 : 1));
        if (check_table(n, bands, T, g, q, &count))
            return 1;
        CHECK(count == 2);
        n++;
    }
    // the plan
    for (uint32_t ch = 1; ch <= SPLIT_MAX_CH; ch++)
        for (bands = 2; bands <= 8; bands++)
            for (T = 3; T <= 1023; T += 4) {
                if (!(T & 1u))
                    continue;
                const uint32_t frames[] = {1, 1023, 1024, 1025, 2048, 2049, 100000};
                for (uint32_t f : frames) {
                    const SplitPlan p = plan_split(3, ch, bands, T, f);
                    const uint32_t t = ch <= 2 ? SPLIT_TILE / ch : SPLIT_TILE, planes = ch <= 2 ? ch : 1;
                    CHECK(p.err == 0 && p.block == SPLIT_BLOCK && p.fast == (ch <= 2 ? 1u : 0u) && p.tile_frames == t);
                    CHECK(p.tp == split_tp(T) && p.row == t + p.tp + 8 && p.row % 8 == 0);
                    CHECK(p.table_words % 4 == 0 && p.table_words >= split_table_words(bands, T));
                    CHECK(p.lds_bytes == p.table_words * 4 + 2 * planes * p.row * 2 && p.lds_bytes <= SPLIT_LDS_LIMIT);
                    CHECK(p.chunks == (f + t - 1) / t && p.grid == 3 * p.chunks);
                    // a lane's reads stay inside its plane: 16-byte vector j + Tp/8 is the highest, lane t/8 - 1
                    CHECK((t / 8 - 1 + p.tp / 8 + 1) * 8 <= p.row);
                }
            }
    T = 255; bands = 3;
    CHECK(plan_split(1u << 20, 2, 3, 255, 1u << 21).err == 1 && plan_split(1u << 20, 2, 3, 255, 1u << 21).grid == 0);
    CHECK(plan_split(1u << 20, 2, 3, 255, (1u << 21) - 1024).err == 0);
    CHECK(plan_split(0, 2, 3, 255, 100).grid == 0 && plan_split(4, 2, 3, 255, 0).grid == 0 && plan_split(4, 17, 3, 255, 100).grid == 0);
    CHECK(plan_split(4, 2, 9, 255, 100).grid == 0 && plan_split(4, 2, 3, 254, 100).grid == 0 && plan_split(4, 2, 3, 254, 100).err == 0);
    printf("groups ok: %lu tables\n", n);
    return 0;
}
