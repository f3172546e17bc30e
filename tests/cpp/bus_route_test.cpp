// bus_route_test.cpp -- drives csrc/bus_route.h (the mix bus's routing compiler; plain C++, no HIP) over random tables
// and checks the CSR invariants of what it compiles.  A stand-alone program: tests/test_bus_host.py builds it with g++
// once plainly and once under AddressSanitizer + UBSan and runs it.   usage: bus_route_test [tables]
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "bus_route.h"

using namespace cmhip;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "table %d: line %d: %s\n", table, __LINE__, #cond);      \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main(int argc, char **argv)
{
    const int tables = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937 rng(20240611u);
    auto upto = [&](uint32_t hi) { return (uint32_t)(rng() % (hi + 1u)); };      // 0 .. hi
    size_t sends_seen = 0, groups_seen = 0;
    for (int table = 0; table < tables; table++) {
        const uint32_t B = 1 + upto(11), S = 1 + upto(11), ci = 1 + upto(15), co = 1 + upto(15), cp = (ci + 1) / 2;
        const size_t n = upto(3) == 0 ? 0 : upto(79);
        // three kinds of weights: light (many sends to a group), heavy (about one each), anything valid
        const uint32_t kind = upto(2), row_max = kind == 0 ? 4000 : 65535, row_min = kind == 1 ? 30000 : 0;
        std::vector<uint32_t> bus(n), stream(n);
        std::vector<int16_t> W(n * co * ci);
        for (size_t j = 0; j < n; j++) {
            bus[j] = upto(B - 1);
            stream[j] = upto(S - 1);
            for (uint32_t o = 0; o < co; o++) {
                uint32_t left = row_min + upto(row_max - row_min);           // this row's sum |w| at most
                for (uint32_t c = 0; c < ci; c++) {
                    const uint32_t cap = std::min(left, 32767u);
                    const uint32_t mag = kind == 1 && c + 1 == ci ? cap : upto(cap);     // (heavy: spend what is left)
                    W[(j * co + o) * ci + c] = (int16_t)(upto(1) ? -(int)mag : (int)mag);
                    left -= mag;
                }
            }
        }
        size_t where = 0;
        CHECK(bus_route_check(B, S, ci, co, n, bus.data(), stream.data(), W.data(), &where) == BUS_ROUTE_OK);
        BusTable t;
        bus_route_compile(B, ci, co, n, bus.data(), stream.data(), W.data(), t);

        // ---- the CSR: first[] rises from 0 to n, every bus's range holds exactly its sends, in the caller's order
        CHECK(t.first.size() == (size_t)B + 1 && t.first[0] == 0 && t.first[B] == n);
        CHECK(t.stream.size() == n && t.flag.size() == n && t.wk.size() == n * co * cp && t.groups.size() == B);
        for (uint32_t b = 0; b < B; b++) {
            CHECK(t.first[b] <= t.first[b + 1]);
            std::vector<size_t> mine;
            for (size_t j = 0; j < n; j++)
                if (bus[j] == b)
                    mine.push_back(j);
            CHECK(mine.size() == t.first[b + 1] - t.first[b]);
            uint32_t run[BUS_MAX_CH] = {0}, groups = 0;
            for (size_t i = 0; i < mine.size(); i++) {
                const size_t p = t.first[b] + i, j = mine[i];                // stable: the i-th of the bus's sends
                CHECK(t.stream[p] == stream[j] && t.flag[p] <= 1);
                // the packed matrix, and the greedy rule restated: a send joins the group iff every row still fits
                bool fits = i != 0;
                uint32_t row[BUS_MAX_CH];
                for (uint32_t o = 0; o < co; o++) {
                    row[o] = 0;
                    for (uint32_t k = 0; k < cp; k++) {
                        const uint32_t d = t.wk[(p * co + o) * cp + k];
                        const int16_t lo = (int16_t)(d & 0xffffu), hi = (int16_t)(d >> 16);
                        CHECK(lo == W[(j * co + o) * ci + 2 * k]);
                        CHECK(hi == (2 * k + 1 < ci ? W[(j * co + o) * ci + 2 * k + 1] : 0));
                        row[o] += bus_abs16(lo) + bus_abs16(hi);
                    }
                    if (run[o] + row[o] > BUS_ROW_MAX)
                        fits = false;
                }
                CHECK(t.flag[p] == (fits ? 0u : 1u));
                for (uint32_t o = 0; o < co; o++) {
                    run[o] = fits ? run[o] + row[o] : row[o];
                    CHECK(run[o] <= BUS_ROW_MAX);                            // int32 is exact over every group
                }
                groups += t.flag[p];
            }
            CHECK(groups == t.groups[b] && (mine.empty() ? groups == 0 : groups >= 1));
            CHECK(bus_first_word(t, b) == (t.first[b] | (groups > 1 ? BUS_BIT : 0u)));
            groups_seen += groups;
        }
        for (size_t p = 0; p < n; p++)
            CHECK(bus_send_word(t, p) == (t.stream[p] | (t.flag[p] ? BUS_BIT : 0u)));
        // ---- a bus's count: the largest among its sends' streams
        std::vector<uint32_t> counts(S);
        for (auto &c : counts)
            c = upto(1000);
        for (uint32_t b = 0; b < B; b++) {
            uint32_t want = 0;
            for (size_t j = 0; j < n; j++)
                if (bus[j] == b)
                    want = std::max(want, counts[stream[j]]);
            CHECK(bus_out_frames(t, b, counts.data(), 1000) == want);
            CHECK(bus_out_frames(t, b, nullptr, 1000) == (t.first[b] == t.first[b + 1] ? 0u : 1000u));
        }
        // ---- refusals: one index or one row out of range
        if (n) {
            const size_t j = upto((uint32_t)n - 1);
            std::vector<uint32_t> bad = bus;
            bad[j] = B;
            CHECK(bus_route_check(B, S, ci, co, n, bad.data(), stream.data(), W.data(), &where) == BUS_ROUTE_BUS && where == j);
            bad = stream;
            bad[j] = S + upto(5);
            CHECK(bus_route_check(B, S, ci, co, n, bus.data(), bad.data(), W.data(), &where) == BUS_ROUTE_STREAM);
            if (ci >= 2) {
                std::vector<int16_t> w2 = W;
                w2[j * co * ci] = -32768;
                w2[j * co * ci + 1] = -32768;
                CHECK(bus_route_check(B, S, ci, co, n, bus.data(), stream.data(), w2.data(), &where) == BUS_ROUTE_ROW);
            }
        }
        sends_seen += n;
    }
    int table = -1;
    CHECK(bus_route_check(0, 1, 1, 1, 0, nullptr, nullptr, nullptr, nullptr) == BUS_ROUTE_GEOMETRY);
    CHECK(bus_route_check(1, 1, 17, 1, 0, nullptr, nullptr, nullptr, nullptr) == BUS_ROUTE_GEOMETRY);
    CHECK(bus_route_check(1, 1, 1, 1, (size_t)1 << 31, nullptr, nullptr, nullptr, nullptr) == BUS_ROUTE_SIZE);
    CHECK(bus_route_check(1, 1, 16, 16, (size_t)1 << 24, nullptr, nullptr, nullptr, nullptr) == BUS_ROUTE_SIZE);
    CHECK(bus_route_check(1, 1, 1, 1, 3, nullptr, nullptr, nullptr, nullptr) == BUS_ROUTE_NULL);
    CHECK(bus_route_check(1, 1, 1, 1, 0, nullptr, nullptr, nullptr, nullptr) == BUS_ROUTE_OK);
    printf("routes ok: %d tables, %zu sends, %zu groups\n", tables, sends_seen, groups_seen);
    return 0;
}
